"""Quantized average pooling restated for the tests.  A helper module, not a conftest.

The reference has no average pool.  Everything but the reduction follows its max_pool2d<u8_t> (src/functional.cc:36-64):
NCHW, window kh x kw, one stride, floor output size, no padding, the input's (scale, zero_point) carried through.
avg_pool2d_u8 is the integer definition q = (S + n // 2) // n in int64, avg_pool2d_f32 the FP32 one (fp32 sum in window
order, rows outer and columns inner, then one fp32 division), avg_pool2d_f64 the float64 mean the FP32 kernel is bounded
against.  The three new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32


def out_hw(h, w, kh, kw, s):
    assert 0 < kh <= h and 0 < kw <= w and s > 0
    return (h - kh) // s + 1, (w - kw) // s + 1


def _windows(x, kh, kw, s):
    """the kh * kw strided views of x [n, c, h, w], window rows outer and columns inner"""
    oh, ow = out_hw(x.shape[2], x.shape[3], kh, kw, s)
    for m in range(kh):
        for l in range(kw):
            yield x[:, :, m:m + (oh - 1) * s + 1:s, l:l + (ow - 1) * s + 1:s]


def avg_pool2d_u8(q, kh, kw, s, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, oh, ow]: (S + n // 2) // n with S the exact window sum, then max(q, zp) if relu."""
    q = np.asarray(q, np.uint8)
    n = kh * kw
    assert n <= 65536
    S = None
    for v in _windows(q.astype(np.int64), kh, kw, s):
        S = v.copy() if S is None else S + v
    out = (S + n // 2) // n
    assert out.min() >= 0 and out.max() <= 255
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def global_avg_pool2d_u8(q, relu=False, zp=0):
    return avg_pool2d_u8(q, q.shape[2], q.shape[3], 1, relu, zp)


def avg_pool2d_f32(x, kh, kw, s):
    """float32 in, float32 out: every step one fp32 operation"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        acc = None
        for v in _windows(x, kh, kw, s):
            acc = (f32(0) + v).astype(f32) if acc is None else (acc + v).astype(f32)
        return (acc / f32(kh * kw)).astype(f32)


def avg_pool2d_f64(x, kh, kw, s):
    """(mean, mean of |x|) of every window in float64"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        tot = sum(_windows(x, kh, kw, s))
        mag = sum(_windows(np.abs(x), kh, kw, s))
    return tot / (kh * kw), mag / (kh * kw)


# ---- ctypes signatures of the average-pool entry points ------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8


def bind(lib):
    lib.i8ie_avgpool2d_u8.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_avgpool2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_B]
    lib.i8ie_avgpool2d_f32.argtypes = [_P, _P, _P] + [_I] * 7
    for f in (lib.i8ie_avgpool2d_u8, lib.i8ie_avgpool2d_u8_nhwc, lib.i8ie_avgpool2d_f32):
        f.restype = _I
    return lib
