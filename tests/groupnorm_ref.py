"""numpy restatement of the quantized GroupNorm (include/i8ie_hip.h, i8ie_groupnorm_u8_nhwc), the real-number value it is
bounded against (torch.nn.functional.group_norm in float64) and that bound, the float64 reference of the FP32 form with its
bound, the ctypes side of the three entries and the constants that decide the kernel form.  A row is a group of one image; the
per-row arithmetic, the affine pair and the bounds are layernorm_ref's, with C read as N.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import layernorm_ref as lr

f32, f64 = np.float32, np.float64
MAX_N = 65536
MAX_C = 16384
# csrc/i8ie_groupnorm.hip (I8IE_GROUPNORM_IMAGE_BYTES, I8IE_GROUPNORM_CHUNK_BYTES of include/i8ie_hip.h)
IMAGE_BYTES = 98304     # h * w * C of the image form
CHUNK_BYTES = 32768     # the split form's chunk: max(1, CHUNK_BYTES // C) pixels
FAST_MAX_C = 4096       # beyond it, and where C % 16 != 0, the direct form


def form(Cn, h, w):
    """the kernel form of aligned buffers without forced fallback"""
    if Cn % 16 or Cn > FAST_MAX_C:
        return "direct"
    return "image" if h * w * Cn <= IMAGE_BYTES else "split"


def kernels(Cn, h, w, fallback=False):
    """{kernel name: launches} of one call"""
    f = "direct" if fallback else form(Cn, h, w)
    if f == "split":
        return {"groupnorm_u8_stats": 1, "groupnorm_u8_apply": 1}
    return {"groupnorm_u8_" + f: 1}


def chunks(Cn, h, w):
    px = max(1, CHUNK_BYTES // Cn)
    return -(-(h * w) // px)


def workspace_bytes(n, Cn, G, h, w):
    return n * chunks(Cn, h, w) * 2 * G * 4 if form(Cn, h, w) == "split" else 0


def as4(q):
    q = np.asarray(q)
    return q.reshape(q.shape[0], q.shape[1], 1, 1) if q.ndim == 2 else q


def rows_of(q, G):
    """[n, C, h, w] -> [n, G, N]: a row is contiguous in NCHW (channel-major, then pixels)"""
    n, Cn, h, w = q.shape
    assert Cn % G == 0 and 1 <= (Cn // G) * h * w <= MAX_N
    return q.reshape(n, G, (Cn // G) * h * w)


def per_element(p, G, hw):
    """per-channel values [C] -> [G, N], repeated per pixel in the order of rows_of"""
    p = np.asarray(p)
    return np.repeat(p.reshape(G, -1), hw, axis=1)


def stats(rows):
    """(S1, S2, V) of rows [..., N] of bytes, exact (int64), asserted inside the definition's limits"""
    a = np.asarray(rows, np.uint8).astype(np.int64)
    N = a.shape[-1]
    S1, S2 = a.sum(-1, keepdims=True), (a * a).sum(-1, keepdims=True)
    V = N * S2 - S1 * S1
    assert 1 <= N <= MAX_N and S2.max() < 2 ** 32 and V.min() >= 0 and V.max() < 2 ** 47
    return S1, S2, V


def group_norm_v(q, G, s_in, eps, g, b):
    """the fp32 value v of the definition, before the clamp: [n, C, h, w] (or [n, C]) bytes, g / b per channel"""
    shape = np.asarray(q).shape
    q = as4(np.asarray(q, np.uint8))
    hw = q.shape[2] * q.shape[3]
    a = rows_of(q, G)
    N = a.shape[-1]
    S1, _, V = stats(a)
    r = (f64(1.0) / np.sqrt(V.astype(f64) + lr.big_e(N, s_in, eps))).astype(f32)
    d = N * a.astype(np.int64) - S1
    assert np.abs(d).max() < 2 ** 24
    t = (d.astype(f32) * r).astype(f32)
    u = (t * per_element(np.asarray(g, f32), G, hw)).astype(f32)
    return (u + per_element(np.asarray(b, f32), G, hw)).astype(f32).reshape(shape)


def group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out, relu=False):
    """[n, C, h, w] or [n, C] bytes -> bytes"""
    g, b = lr.affine(gamma, beta, s_out, zp_out)
    out = lr.clamp_trunc(group_norm_v(q, G, s_in, eps, g, b))
    return np.maximum(out, np.uint8(zp_out)) if relu else out


def real_parts(q, G, s_in, zp_in, eps, gamma, beta, s_out, zp_out):
    """float64, by torch.nn.functional.group_norm on the dequantised tensor: (y*, T G, beta / s_out) in output units"""
    import torch

    q = as4(np.asarray(q, np.uint8))
    x = torch.from_numpy((q.astype(f64) - f64(zp_in)) * f64(f32(s_in)))
    T = torch.nn.functional.group_norm(x, G, None, None, float(f64(f32(eps)))).numpy()
    per_c = lambda p: np.asarray(p, f64).reshape(1, -1, 1, 1)  # noqa: E731
    TG = T * per_c(np.asarray(gamma, f32).astype(f64) / f64(f32(s_out)))
    Bs = per_c(np.asarray(beta, f32).astype(f64) / f64(f32(s_out)))
    return TG + Bs + f64(zp_out), TG, np.broadcast_to(Bs, TG.shape)


bound = lr.bound   # B(y*) of include/i8ie_hip.h: its derivation uses the row length in |T| <= sqrt(N) alone


# ---- FP32 form -------------------------------------------------------------------------------------------------------------
def group_norm_f64(x, G, gamma, beta, eps):
    x = as4(np.asarray(x, f64))
    hw = x.shape[2] * x.shape[3]
    return lr.layer_norm_f64(rows_of(x, G), per_element(gamma, G, hw), per_element(beta, G, hw), eps).reshape(x.shape)


def group_norm_f32_bound(x, G, gamma, beta, eps):
    """The FP32 form is i8ie_layernorm_f32's sequence on the N contiguous floats of a row in ascending address order, so the
    bound is layernorm_ref.layer_norm_f32_bound with C = N and gamma / beta of each element's channel.  Its factor 1.01 for the
    second-order terms was stated for C u <= 2^-10; here N u <= 2^-8 and the largest second-order term, gam(N + 2)^2 against
    gam(N + 2), is below 0.4 %."""
    x = as4(np.asarray(x, f64))
    hw = x.shape[2] * x.shape[3]
    return lr.layer_norm_f32_bound(rows_of(x, G), per_element(gamma, G, hw), per_element(beta, G, hw), eps).reshape(x.shape)


def tracer(layers, into):
    """a trace callback for spec_ref.forward: into[attr] = the output bytes of every ("gn", groups, channels) layer"""
    def trace(op, out, operands):
        if op[0] == "layer" and layers[op[1]][0] == "gn":
            into[op[1]] = out[0]

    return trace


# ---- ctypes ------------------------------------------------------------------------------------------------------------------
def bind(lib):
    vp, i = C.c_void_p, C.c_int
    lr.bind(lib)
    lib.i8ie_groupnorm_u8_nhwc.argtypes = [vp, vp, i, i, vp, i, i, i, i, i, i, i, vp, vp, C.c_float, C.c_float, i, C.c_uint8, vp]
    lib.i8ie_groupnorm_workspace_bytes.argtypes = [i, i, i, i, i]
    lib.i8ie_groupnorm_workspace_bytes.restype = C.c_int64
    lib.i8ie_groupnorm_f32.argtypes = [vp, vp, vp, i, i, i, C.c_int64, vp, vp, C.c_float]
    return lib


# the statistics extremes of the definition at the longest row: (name, images [n, C, h, w]) with N = (C / G) h w
def extreme_images(Cn=16, G=1, h=64, w=64):
    cg = Cn // G
    assert cg * h * w == MAX_N
    out = [("all255", np.full((1, Cn, h, w), 255, np.uint8))]          # the largest S1 and S2
    half = np.zeros((2, Cn, h, w), np.uint8)
    half[0, :, :h // 2] = 255                                          # half the pixels of every channel
    half[1, :, :, 1::2] = 255
    out.append(("half", half))                                         # the largest V
    const = np.empty((3, Cn, h, w), np.uint8)
    const[0], const[1], const[2] = 0, 128, 255
    out.append(("const", const))                                       # V = 0
    one = np.full((3, Cn, h, w), 200, np.uint8)
    one[0, 0, 0, 0], one[1, Cn - 1, h - 1, w - 1], one[2, Cn // 2, h // 2, 3] = 201, 0, 255
    out.append(("one_differs", one))
    return out
