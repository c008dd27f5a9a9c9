"""numpy restatement of the quantized inference BatchNorm (include/i8ie_hip.h, i8ie_batchnorm_u8_nhwc): the affine in double with
one rounding to float, the u8 sequence in np.float32, the real-number value it is bounded against and that bound, the FP32
sequence with its float64 reference and bound, the fold into a neighbouring layer, the case lists, the kernel's tiling constants
and the ctypes side of the four entries.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import f64_ref

f32, f64 = np.float32, np.float64
MAX_C = 16384
U = 2.0 ** -24   # unit roundoff of fp32
# csrc/i8ie_batchnorm.hip: a lane of batchnorm_u8_nhwc owns one channel item of 16 / 4 / 1 bytes (C % 16, C % 4) and walks WALK
# pixels; a block of 256 lanes holds 256 // min(C // item, 256) pixels, so a block covers pixel_run(C) pixels of one image
WALK = 8
ITEM_WIDTHS = (16, 4, 1)
MAX_BLOCKS = 2048   # the grid cap: more (image, channel chunk, pixel tile) units than this and a block takes a second unit


def item_width(Cn):
    return 16 if Cn % 16 == 0 else (4 if Cn % 4 == 0 else 1)


def pixel_run(Cn):
    """pixels of one image a block covers: its rows times WALK"""
    return (256 // min(Cn // item_width(Cn), 256)) * WALK


# ---- the definition ------------------------------------------------------------------------------------------------------------
def k_of(gamma, var, eps):
    return np.asarray(gamma, f32).astype(f64) / np.sqrt(np.asarray(var, f32).astype(f64) + f64(f32(eps)))


def affine(gamma, beta, mean, var, eps, s_out, zp_out):
    """(g, b): double arithmetic in the order of the definition, one rounding to float each"""
    k = k_of(gamma, var, eps)
    s = f64(f32(s_out))
    g = (k / s).astype(f32)
    b = ((np.asarray(beta, f32).astype(f64) - np.asarray(mean, f32).astype(f64) * k) / s + f64(zp_out)).astype(f32)
    return g, b


def _per_channel(v, ndim):
    """[C] -> broadcastable against [n, C, ...] of rank ndim"""
    return np.asarray(v).reshape((1, -1) + (1,) * (ndim - 2))


def batch_norm_v(q, s_in, zp_in, g, b):
    """the fp32 value v of the definition, before the clamp: q is [n, C] or [n, C, h, w]"""
    q = np.asarray(q, np.uint8)
    x = ((q.astype(np.int32) - int(zp_in)).astype(f32) * f32(s_in)).astype(f32)
    t = (x * _per_channel(np.asarray(g, f32), q.ndim)).astype(f32)
    return (t + _per_channel(np.asarray(b, f32), q.ndim)).astype(f32)


def clamp_trunc(v):
    """down_scale's clamp + truncation (src/quantize_utils.cc:27-36) on float values"""
    v = np.asarray(v)
    return np.where(v >= 255, 255, np.where(v < 0, 0, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)


def bytes_of(q, s_in, zp_in, g, b, zp_out, relu=False):
    """the bytes of the definition from a given (g, b)"""
    out = clamp_trunc(batch_norm_v(q, s_in, zp_in, g, b))
    return np.maximum(out, np.uint8(zp_out)) if relu else out


def batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, relu=False):
    g, b = affine(gamma, beta, mean, var, eps, s_out, zp_out)
    return bytes_of(q, s_in, zp_in, g, b, zp_out, relu)


def real_parts(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out):
    """float64, by torch's CPU batch_norm(training=False) on the dequantised input, mapped to output units: (y*, T, Bt) with
    T = (a - zp_in) s_in k / s_out, Bt = (beta - mean k) / s_out + zp_out, y* = T + Bt = bn(x) / s_out + zp_out"""
    import torch

    q = np.asarray(q, np.uint8)
    t64 = lambda v: torch.from_numpy(np.asarray(v, f32).astype(f64))  # noqa: E731
    x = torch.from_numpy((q.astype(f64) - f64(zp_in)) * f64(f32(s_in)))
    y = torch.nn.functional.batch_norm(x, t64(mean), t64(var), t64(gamma), t64(beta), False, 0.0, float(f64(f32(eps)))).numpy()
    s = f64(f32(s_out))
    k = k_of(gamma, var, eps)
    Bt = _per_channel((np.asarray(beta, f32).astype(f64) - np.asarray(mean, f32).astype(f64) * k) / s + f64(zp_out), q.ndim)
    ystar = y / s + f64(zp_out)
    return ystar, ystar - Bt, np.broadcast_to(Bt, ystar.shape)


def bound(y, T, Bt):
    """B of include/i8ie_hip.h: |v - y*| <= 1.01 * 2^-24 * (4 |T| + |Bt| + |y*|)"""
    return 1.01 * U * (4 * np.abs(T) + np.abs(Bt) + np.abs(y))


# ---- FP32 form -----------------------------------------------------------------------------------------------------------------
def batch_norm_f32(x, gamma, beta, mean, var, eps):
    """the fp32 sequence: out = (x - mean) / sqrtf(var + eps) * gamma + beta, one rounding per operation"""
    x = np.asarray(x, f32)
    p = lambda v: _per_channel(np.asarray(v, f32), x.ndim)  # noqa: E731
    dx = (x - p(mean)).astype(f32)
    sd = np.sqrt((p(var) + f32(eps)).astype(f32)).astype(f32)
    nrm = (dx / sd).astype(f32)
    return ((nrm * p(gamma)).astype(f32) + p(beta)).astype(f32)


def batch_norm_f64(x, gamma, beta, mean, var, eps):
    x = np.asarray(x, f64)
    p = lambda v: _per_channel(np.asarray(v, f32).astype(f64), x.ndim)  # noqa: E731
    return (x - p(mean)) / np.sqrt(p(var) + f64(f32(eps))) * p(gamma) + p(beta)


def batch_norm_f32_bound(x, gamma, beta, mean, var, eps):
    """|fp32 sequence - float64| per element, with f64_ref.gamma as for LayerNorm's FP32 entry: the product term
    P = (x - mean) / sqrt(var + eps) * gamma carries five roundings (the difference, the sum under the root -- a relative error
    the root halves, kept whole --, the root, the quotient, the product) and is then added once: gamma(6) |P| + u |out|, and
    2^-126 per operation for a result that underflows"""
    x = np.asarray(x, f64)
    p = lambda v: _per_channel(np.asarray(v, f32).astype(f64), x.ndim)  # noqa: E731
    P = (x - p(mean)) / np.sqrt(p(var) + f64(f32(eps))) * p(gamma)
    return f64_ref.gamma(6) * np.abs(P) + f64_ref.U * np.abs(P + p(beta)) + 6 * 2.0 ** -126


# ---- the fold ----------------------------------------------------------------------------------------------------------------
def fold(w, b, gamma, beta, mean, var, eps, axis=0):
    """(W', b') of i8ie.fold_batchnorm: W'[o, ...] = (float)((double)W k[o]), b'[o] = (float)(((double)b - mean) k + beta);
    axis: the weight's output-feature axis (1 for ConvTranspose2d's [in, out, k, k])"""
    w, b = np.asarray(w, f32), np.asarray(b, f32)
    k = k_of(gamma, var, eps)
    shape = [1] * w.ndim
    shape[axis] = -1
    w2 = (w.astype(f64) * k.reshape(shape)).astype(f32)
    b2 = ((b.astype(f64) - np.asarray(mean, f32).astype(f64)) * k + np.asarray(beta, f32).astype(f64)).astype(f32)
    return w2, b2


# ---- case lists --------------------------------------------------------------------------------------------------------------
def random_params(rng, Cn):
    """the ranges of the definition's check: gamma ~ N(1, 0.5), beta ~ N(0, 0.5), mean ~ N(0, 1), var in [0.01, 4]"""
    return (rng.normal(1.0, 0.5, Cn).astype(f32), rng.normal(0.0, 0.5, Cn).astype(f32), rng.normal(0.0, 1.0, Cn).astype(f32),
            rng.uniform(0.01, 4.0, Cn).astype(f32))


def random_qparams(rng):
    """(s_in, zp_in, s_out, zp_out): scales in [0.005, 0.1]"""
    return f32(rng.uniform(0.005, 0.1)), int(rng.integers(0, 256)), f32(rng.uniform(0.005, 0.1)), int(rng.integers(0, 256))


EXHAUSTIVE_C = [1, 3, 4, 15, 16, 17, 20, 32, 48]
# (s_in, zp_in, s_out, zp_out, eps, what): the parameter sets of the exhaustive test
PARAM_SETS = [(f32(0.025), 127, f32(0.02), 128, f32(1e-5), "plain"),
              (f32(0.1), 0, f32(0.05), 255, f32(1e-5), "zero_gamma"),
              (f32(0.004), 255, f32(0.011), 0, f32(1e-3), "negative_gamma"),
              (f32(0.05), 13, f32(0.03), 100, f32(1e-5), "zero_var"),
              (f32(0.09), 200, f32(0.006), 31, f32(1e-6), "plain")]


def case_params(Cn, seed, what):
    gamma, beta, mean, var = random_params(np.random.default_rng(seed), Cn)
    if what == "zero_gamma":
        gamma[0] = 0.0
    if what == "negative_gamma":
        gamma[::2] = -np.abs(gamma[::2]) - f32(0.25)
    if what == "zero_var":
        var[Cn // 2] = 0.0
        gamma[Cn // 2] = f32(0.002)   # (k = gamma / sqrt(eps) stays inside the byte range)
    return gamma, beta, mean, var


# ---- ctypes --------------------------------------------------------------------------------------------------------------------
def bind(lib):
    vp = C.c_void_p
    lib.i8ie_batchnorm_affine.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_uint8, vp, vp]
    lib.i8ie_batchnorm_u8_nhwc.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp,
                                           C.c_float, C.c_uint8, C.c_int, C.c_uint8]
    lib.i8ie_batchnorm_u8.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_int64, vp, vp, C.c_float, C.c_uint8, C.c_int, C.c_uint8]
    lib.i8ie_batchnorm_f32.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_int64, vp, vp, vp, vp, C.c_float]
    return lib


def affine_entry(lib, gamma, beta, mean, var, eps, s_out, zp_out, Cn=None):
    """(rc, g, b) of i8ie_batchnorm_affine"""
    arrs = [np.ascontiguousarray(v, f32) for v in (gamma, beta, mean, var)]
    g, b = np.full(arrs[0].shape, np.nan, f32), np.full(arrs[0].shape, np.nan, f32)
    rc = lib.i8ie_batchnorm_affine(*[a.ctypes.data for a in arrs], arrs[0].size if Cn is None else Cn, float(eps), float(s_out), int(zp_out),
                                   g.ctypes.data, b.ctypes.data)
    return rc, g, b
