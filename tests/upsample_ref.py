"""Quantized upsampling restated for the tests.  A helper module, not a conftest.

The reference has no resize op.  The definition is the one of include/i8ie_hip.h: integer factors fh, fw in 1..8 on an NCHW
tensor, the input's (scale, zero_point) carried through; nearest is out[y, x] = in[y // fh, x // fw]; bilinear is torch's
align_corners=False written in integers -- per axis the taps (i0, i1) and weights (w0, w1) of 2 f, S the doubly weighted sum
of the four taps, D = 4 fh fw, out = (S + D // 2) // D.  taps() is that rule as arrays over the output index, bilinear_sd the
exact (S, D) in int64, upsample_u8 the bytes, bilinear_f64 the float64 value S / D of any real input (with the largest
magnitude among each output's four taps), upsample_f32 the FP32 sequence in order (row blends first, one float32 rounding
per operation).  tracer() keeps the upsamples' bytes of a spec_ref.forward, and the three new C symbols get their ctypes
signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32
NEAREST, BILINEAR = 0, 1
MODES = {"nearest": NEAREST, "bilinear": BILINEAR}
MAX_FACTOR = 8


def factors(factor):
    """(fh, fw) of a spec op's factor: an int or a pair"""
    return tuple(factor) if isinstance(factor, (tuple, list)) else (factor, factor)


def taps(L, f):
    """(i0, i1, w0, w1), each an int64 array over the L * f output indices of one axis"""
    assert L > 0 and 1 <= f <= MAX_FACTOR
    o = np.arange(L * f, dtype=np.int64)
    i, r = o // f, o % f
    t = 2 * r + 1 - f
    i0 = np.where(t >= 0, i, i - 1)
    w1 = np.where(t >= 0, t, 2 * f + t)
    w1 = np.where(i0 < 0, 0, w1)
    i0 = np.maximum(i0, 0)
    i1 = np.minimum(i0 + 1, L - 1)
    return i0, i1, 2 * f - w1, w1


def nearest(x, fh, fw):
    x = np.asarray(x)
    assert x.ndim == 4 and 1 <= fh <= MAX_FACTOR and 1 <= fw <= MAX_FACTOR
    return np.ascontiguousarray(x[:, :, np.arange(x.shape[2] * fh) // fh][:, :, :, np.arange(x.shape[3] * fw) // fw])


def _four(x, fh, fw):
    """the four taps of every output and the weights, broadcastable: (q00, q10, q01, q11, wy0, wy1, wx0, wx1)"""
    y0, y1, wy0, wy1 = taps(x.shape[2], fh)
    x0, x1, wx0, wx1 = taps(x.shape[3], fw)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    return (r0[:, :, :, x0], r1[:, :, :, x0], r0[:, :, :, x1], r1[:, :, :, x1], wy0[:, None], wy1[:, None], wx0[None, :], wx1[None, :])


def bilinear_sd(q, fh, fw):
    """u8 [n, c, h, w] -> (S int64 [n, c, h fh, w fw], D)"""
    q00, q10, q01, q11, wy0, wy1, wx0, wx1 = _four(np.asarray(q, np.uint8).astype(np.int64), fh, fw)
    return wx0 * (wy0 * q00 + wy1 * q10) + wx1 * (wy0 * q01 + wy1 * q11), 4 * fh * fw


def upsample_u8(q, fh, fw, mode, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, h fh, w fw]; mode "nearest" / "bilinear" (or NEAREST / BILINEAR)"""
    mode = MODES.get(mode, mode)
    assert mode in (NEAREST, BILINEAR)
    q = np.asarray(q, np.uint8)
    if mode == NEAREST:
        out = nearest(q, fh, fw).astype(np.int64)
    else:
        S, D = bilinear_sd(q, fh, fw)
        out = (S + D // 2) // D
        assert out.min() >= 0 and out.max() <= 255
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def bilinear_f64(x, fh, fw):
    """(S / D in float64, the largest |tap| of every output's window)"""
    x = np.asarray(x, np.float64)
    q00, q10, q01, q11, wy0, wy1, wx0, wx1 = _four(x, fh, fw)
    val = (wx0 * (wy0 * q00 + wy1 * q10) + wx1 * (wy0 * q01 + wy1 * q11)) / float(4 * fh * fw)
    mag = np.maximum(np.maximum(np.abs(q00), np.abs(q10)), np.maximum(np.abs(q01), np.abs(q11)))
    return val, mag


def upsample_f32(x, fh, fw, mode):
    """float32 in, float32 out, the FP32 sequence of include/i8ie_hip.h: every step one fp32 operation"""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, f32)
    if mode == NEAREST:
        return nearest(x, fh, fw)
    q00, q10, q01, q11, _, wy1, _, wx1 = _four(x, fh, fw)
    ly = (wy1.astype(f32) / f32(2 * fh)).astype(f32)
    lx = (wx1.astype(f32) / f32(2 * fw)).astype(f32)
    my, mx = (f32(1) - ly).astype(f32), (f32(1) - lx).astype(f32)
    with np.errstate(all="ignore"):
        top = ((q00 * mx).astype(f32) + (q01 * lx).astype(f32)).astype(f32)
        bot = ((q10 * mx).astype(f32) + (q11 * lx).astype(f32)).astype(f32)
        return ((top * my).astype(f32) + (bot * ly).astype(f32)).astype(f32)


# ---- spec networks -----------------------------------------------------------------------------------------------------
def tracer(into):
    """a trace callback for spec_ref.forward: (op, output bytes) of every upsample, appended to the list `into`"""
    def trace(op, out, operands):
        if op[0] == "upsample":
            into.append((op, out[0]))

    return trace


# ---- ctypes signatures of the upsample entry points -----------------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8


def bind(lib):
    lib.i8ie_upsample2d_u8.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_upsample2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_B]
    lib.i8ie_upsample2d_f32.argtypes = [_P, _P, _P] + [_I] * 7
    for f in (lib.i8ie_upsample2d_u8, lib.i8ie_upsample2d_u8_nhwc, lib.i8ie_upsample2d_f32):
        f.restype = _I
    return lib
