"""numpy restatement of the quantized LayerNorm (include/i8ie_hip.h, i8ie_layernorm_u8), the real-number value it is bounded
against and that bound, the float64 reference of the FP32 form with its bound, the ctypes side of the four entries, and the trace adapter of the
ConvNeXt networks.  A helper, not a conftest."""
import ctypes as C

import numpy as np

f32, f64 = np.float32, np.float64
MAX_C = 16384
U = 2.0 ** -24   # unit roundoff of fp32
# csrc/i8ie_layernorm.hip: lanes per row double where ceil(C / 16) passes 4 G, and rows beyond GROUP_MAX_C take one block each
GROUP_WIDTHS = [64, 128, 256, 512, 1024, 2048]
GROUP_MAX_C = 4096
DIRECT_ROWS_PER_PASS = 2048 * 256   # the direct kernel's grid: at most 2048 blocks of 256 one-row lanes


def affine(gamma, beta, s_out, zp_out):
    """g = gamma / s_out, b = (beta / s_out) + zp_out: fp32, one rounding per operation"""
    gamma, beta, s_out = np.asarray(gamma, f32), np.asarray(beta, f32), f32(s_out)
    return (gamma / s_out).astype(f32), ((beta / s_out).astype(f32) + f32(zp_out)).astype(f32)


def stats(a):
    """(S1, S2, V) of rows [..., C] of bytes, exact (int64), asserted inside the definition's limits"""
    a = np.asarray(a, np.uint8).astype(np.int64)
    Cn = a.shape[-1]
    S1, S2 = a.sum(-1, keepdims=True), (a * a).sum(-1, keepdims=True)
    V = Cn * S2 - S1 * S1
    assert 1 <= Cn <= MAX_C and S2.max() < 2 ** 31 and V.min() >= 0 and V.max() < 2 ** 53
    return S1, S2, V


def big_e(Cn, s_in, eps):
    return f64(Cn) * f64(Cn) * f64(f32(eps)) / (f64(f32(s_in)) * f64(f32(s_in)))


def layer_norm_v(a, s_in, eps, g, b):
    """the fp32 value v of the definition, before the clamp: rows [..., C]"""
    a = np.asarray(a, np.uint8)
    Cn = a.shape[-1]
    S1, _, V = stats(a)
    r = (f64(1.0) / np.sqrt(V.astype(f64) + big_e(Cn, s_in, eps))).astype(f32)
    d = Cn * a.astype(np.int64) - S1
    assert np.abs(d).max() < 2 ** 22
    t = (d.astype(f32) * r).astype(f32)
    u = (t * np.asarray(g, f32)).astype(f32)
    return (u + np.asarray(b, f32)).astype(f32)


def clamp_trunc(v):
    """down_scale's clamp + truncation (src/quantize_utils.cc:27-36) on float values"""
    v = np.asarray(v)
    return np.where(v >= 255, 255, np.where(v < 0, 0, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)


def layer_norm_u8(a, s_in, eps, gamma, beta, s_out, zp_out, relu=False):
    """rows [..., C] of bytes -> bytes"""
    g, b = affine(gamma, beta, s_out, zp_out)
    q = clamp_trunc(layer_norm_v(a, s_in, eps, g, b))
    return np.maximum(q, np.uint8(zp_out)) if relu else q


def layer_norm_u8_nchw(q, s_in, eps, gamma, beta, s_out, zp_out, relu=False):
    """[n, c, h, w] normalised over c per pixel"""
    out = layer_norm_u8(np.ascontiguousarray(q.transpose(0, 2, 3, 1)), s_in, eps, gamma, beta, s_out, zp_out, relu)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def layer_norm_any(q, *args, **kw):
    """the Python surface's shape rule: rank 4 over axis 1, ranks 2 and 3 over the last axis"""
    return layer_norm_u8_nchw(q, *args, **kw) if q.ndim == 4 else layer_norm_u8(q, *args, **kw)


def real_parts(a, s_in, zp_in, eps, gamma, beta, s_out, zp_out):
    """float64, by torch.nn.functional.layer_norm on the dequantised rows: (y*, T G, beta / s_out) in output units, where
    y* = T G + beta / s_out + zp_out and T = (x - mean) / sqrt(var + eps)"""
    import torch

    a = np.asarray(a, np.uint8)
    Cn = a.shape[-1]
    x = torch.from_numpy((a.astype(f64) - f64(zp_in)) * f64(f32(s_in)))
    T = torch.nn.functional.layer_norm(x, (Cn,), None, None, float(f64(f32(eps)))).numpy()
    TG = T * (np.asarray(gamma, f32).astype(f64) / f64(f32(s_out)))
    Bs = np.asarray(beta, f32).astype(f64) / f64(f32(s_out))
    return TG + Bs + f64(zp_out), TG, np.broadcast_to(Bs, TG.shape)


def bound(y, TG, Bs):
    """B(y*) of include/i8ie_hip.h: |v - y*| <= 1.01 * 2^-24 * (5 |T G| + 2 |beta / s_out| + 255 + |y*|); + 1e-12 |y*| + 1e-40
    for the float64 reference's own roundings and a product that underflows"""
    return 1.01 * U * (5 * np.abs(TG) + 2 * np.abs(Bs) + 255 + np.abs(y)) + 1e-12 * (np.abs(y) + np.abs(TG)) + 1e-40


# ---- FP32 form -------------------------------------------------------------------------------------------------------------
def layer_norm_f64(x, gamma, beta, eps):
    """float64 over the last axis"""
    x = np.asarray(x, f64)
    dx = x - x.mean(-1, keepdims=True)
    return dx / np.sqrt((dx * dx).mean(-1, keepdims=True) + f64(f32(eps))) * np.asarray(gamma, f64) + np.asarray(beta, f64)


def layer_norm_f32_bound(x, gamma, beta, eps):
    """Bound on |fp32 sequence - float64| per element, from C and the number of roundings (u = 2^-24, gam(k) = k u / (1 - k u)):
      mean: C - 1 additions and one division           |dmean| <= gam(C) mean|x|
      dx = x - mean: one rounding                       e = u |dx| + (1 + u) |dmean|
      var: square, C - 1 additions, one division        dvar <= gam(C + 2) var + 2 mean(|dx| e) + mean(e^2)
      sd = sqrtf(var + eps): two roundings              rel_sd <= (dvar + u (var + eps)) / (var + eps) + 2 u
                                                        (sqrt halves a relative error; the full one is kept as slack)
      n = dx / sd: one rounding                         dn <= e / sd + |n| (rel_sd + u)
      out = n * gamma + beta: two roundings             dout <= (dn |gamma| + u |n gamma|) + u |out|
    all times 1.01 for the second-order terms (C u <= 2^-10 here)."""
    x, gamma, beta = np.asarray(x, f64), np.asarray(gamma, f64), np.asarray(beta, f64)
    Cn = x.shape[-1]
    gam = lambda k: k * U / (1 - k * U)  # noqa: E731
    mean = x.mean(-1, keepdims=True)
    dx = x - mean
    var = (dx * dx).mean(-1, keepdims=True)
    z = var + f64(f32(eps))
    sd = np.sqrt(z)
    dmean = gam(Cn) * np.abs(x).mean(-1, keepdims=True)
    e = U * np.abs(dx) + (1 + U) * dmean
    dvar = gam(Cn + 2) * var + 2 * (np.abs(dx) * e).mean(-1, keepdims=True) + (e * e).mean(-1, keepdims=True)
    rel_sd = (dvar + U * z) / z + 2 * U
    n = dx / sd
    dn = e / sd + np.abs(n) * (rel_sd + U)
    out = n * gamma + beta
    return 1.01 * (dn * np.abs(gamma) + U * np.abs(n * gamma) + U * np.abs(out))


# ---- ctypes ------------------------------------------------------------------------------------------------------------------
def bind(lib):
    vp = C.c_void_p
    lib.i8ie_layernorm_affine.argtypes = [vp, vp, C.c_int, C.c_float, C.c_uint8, vp, vp]
    lib.i8ie_layernorm_u8.argtypes = [vp, vp, vp, C.c_int64, C.c_int, vp, vp, C.c_float, C.c_float, C.c_int, C.c_uint8]
    lib.i8ie_layernorm_u8_nhwc.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp,
                                           C.c_float, C.c_float, C.c_int, C.c_uint8]
    lib.i8ie_layernorm_f32.argtypes = [vp, vp, vp, C.c_int64, C.c_int, vp, vp, C.c_float, C.c_int64]
    return lib


def affine_entry(lib, gamma, beta, s_out, zp_out):
    """(rc, g, b) of i8ie_layernorm_affine"""
    gamma, beta = np.ascontiguousarray(gamma, f32), np.ascontiguousarray(beta, f32)
    g, b = np.zeros_like(gamma), np.zeros_like(gamma)
    rc = lib.i8ie_layernorm_affine(gamma.ctypes.data, beta.ctypes.data, gamma.size, float(s_out), int(zp_out), g.ctypes.data, b.ctypes.data)
    return rc, g, b


# the statistics extremes of the definition: (name, rows [r, C])
def extreme_rows():
    out = [("const%d_C%d" % (v, c), np.full((2, c), v, np.uint8)) for v in (0, 128, 255) for c in (1, 17, 96, 5000)]
    for c in (2, 96, 1024, MAX_C):
        one = np.full((3, c), 200, np.uint8)
        one[0, 0], one[1, c - 1], one[2, c // 2] = 201, 0, 255
        out.append(("one_differs_C%d" % c, one))
    half = np.zeros((2, MAX_C), np.uint8)
    half[0, :MAX_C // 2] = 255
    half[1, 1::2] = 255
    out.append(("half_C16384", half))                                 # the largest V
    out.append(("all255_C16384", np.full((1, MAX_C), 255, np.uint8)))  # the largest S2 and S1^2
    return out


def tracer(layers, into):
    """a trace callback for spec_ref.forward: into[attr] = the output bytes of every ("ln", channels) layer"""
    def trace(op, out, operands):
        if op[0] == "layer" and layers[op[1]][0] == "ln":
            into[op[1]] = out[0]

    return trace
