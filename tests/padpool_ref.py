"""Max and average pooling with torch's padding and ceil_mode, restated for the tests (include/i8ie_hip.h,
i8ie_pool_output_size).  A helper module, not a conftest.

One square window k, one stride s, one padding p with 0 <= p <= k // 2, k <= in + 2 p.  out_size is the output size with
the ceil-mode drop rule; cuts() gives, per output index of one axis, the window [y0, y1) = [o s - p, min(o s - p + k, in + p))
and its valid part [ys, ye) inside [0, in).  max_pool2d_u8 / avg_pool2d_u8 are the integer definitions in int64,
max_pool2d_f64 / avg_pool2d_f64 the float64 references the FP32 kernels are held against.  The new C symbols get their ctypes
signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32


def legal(size, k, s, p):
    return size > 0 and k > 0 and s > 0 and 0 <= p <= k // 2 and k <= size + 2 * p


def out_size(size, k, s, p, ceil_mode):
    assert legal(size, k, s, p), (size, k, s, p)
    o = (size + 2 * p - k + (s - 1 if ceil_mode else 0)) // s + 1
    if ceil_mode and (o - 1) * s >= size + p:
        o -= 1
    return o


def cuts(size, k, s, p, ceil_mode):
    """[(y0, y1, ys, ye)] per output index: the window with its padding, and its valid part"""
    out = []
    for o in range(out_size(size, k, s, p, ceil_mode)):
        y0 = o * s - p
        y1 = min(y0 + k, size + p)
        ys, ye = max(y0, 0), min(y1, size)
        assert 0 <= ys < ye <= size, "every window has a valid tap"
        out.append((y0, y1, ys, ye))
    return out


def divisors(h, w, k, s, p, ceil_mode, count_include_pad):
    """[oh, ow] int64: the divisor D of every output"""
    rows, cols = cuts(h, k, s, p, ceil_mode), cuts(w, k, s, p, ceil_mode)
    if count_include_pad:
        return np.array([[(r[1] - r[0]) * (c[1] - c[0]) for c in cols] for r in rows], np.int64)
    return np.array([[(r[3] - r[2]) * (c[3] - c[2]) for c in cols] for r in rows], np.int64)


def max_pool2d_u8(q, k, s, p=0, ceil_mode=False, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, oh, ow]: the maximum of the valid taps, then max(q, zp) if relu"""
    q = np.asarray(q, np.uint8)
    rows, cols = cuts(q.shape[2], k, s, p, ceil_mode), cuts(q.shape[3], k, s, p, ceil_mode)
    out = np.empty(q.shape[:2] + (len(rows), len(cols)), np.uint8)
    for y, r in enumerate(rows):
        for x, c in enumerate(cols):
            out[:, :, y, x] = q[:, :, r[2]:r[3], c[2]:c[3]].max(axis=(2, 3))
    return np.maximum(out, np.uint8(zp)) if relu else out


def avg_pool2d_u8(q, k, s, p=0, ceil_mode=False, count_include_pad=True, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, oh, ow]: S' = S + (D - n_valid) zp, q = (S' + D // 2) // D, then max(q, zp) if relu"""
    q = np.asarray(q, np.uint8).astype(np.int64)
    assert k * k <= 65536
    rows, cols = cuts(q.shape[2], k, s, p, ceil_mode), cuts(q.shape[3], k, s, p, ceil_mode)
    out = np.empty(q.shape[:2] + (len(rows), len(cols)), np.int64)
    for y, r in enumerate(rows):
        for x, c in enumerate(cols):
            nv = (r[3] - r[2]) * (c[3] - c[2])
            D = (r[1] - r[0]) * (c[1] - c[0]) if count_include_pad else nv
            S = q[:, :, r[2]:r[3], c[2]:c[3]].sum(axis=(2, 3)) + (D - nv) * int(zp)
            out[:, :, y, x] = (S + D // 2) // D
    assert out.min() >= 0 and out.max() <= 255
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def max_pool2d_f64(x, k, s, p=0, ceil_mode=False):
    """the maximum of the valid taps in float64 (exact for float32 input)"""
    x = np.asarray(x, np.float64)
    rows, cols = cuts(x.shape[2], k, s, p, ceil_mode), cuts(x.shape[3], k, s, p, ceil_mode)
    out = np.empty(x.shape[:2] + (len(rows), len(cols)), np.float64)
    for y, r in enumerate(rows):
        for xx, c in enumerate(cols):
            out[:, :, y, xx] = x[:, :, r[2]:r[3], c[2]:c[3]].max(axis=(2, 3))
    return out


def avg_pool2d_f64(x, k, s, p=0, ceil_mode=False, count_include_pad=True):
    """(sum of the valid taps / D, sum of their magnitudes / D, the number of valid taps) of every window in float64"""
    x = np.asarray(x, np.float64)
    rows, cols = cuts(x.shape[2], k, s, p, ceil_mode), cuts(x.shape[3], k, s, p, ceil_mode)
    shape = x.shape[:2] + (len(rows), len(cols))
    mean, mag, taps = np.empty(shape), np.empty(shape), np.empty(shape[2:], np.int64)
    for y, r in enumerate(rows):
        for xx, c in enumerate(cols):
            nv = (r[3] - r[2]) * (c[3] - c[2])
            D = (r[1] - r[0]) * (c[1] - c[0]) if count_include_pad else nv
            v = x[:, :, r[2]:r[3], c[2]:c[3]]
            mean[:, :, y, xx], mag[:, :, y, xx], taps[y, xx] = v.sum(axis=(2, 3)) / D, np.abs(v).sum(axis=(2, 3)) / D, nv
    return mean, mag, taps


# ---- ctypes signatures of the padded-pool entry points ---------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8
SYMBOLS = ["i8ie_pool_output_size", "i8ie_maxpool2d_u8_pad", "i8ie_maxpool2d_u8_nhwc_pad", "i8ie_maxpool2d_f32_pad",
           "i8ie_avgpool2d_u8_pad", "i8ie_avgpool2d_u8_nhwc_pad", "i8ie_avgpool2d_f32_pad"]


def bind(lib):
    lib.i8ie_pool_output_size.argtypes = [_I] * 5
    lib.i8ie_maxpool2d_u8_pad.argtypes = [_P, _P, _P] + [_I] * 8                    # n c h w k s p ceil
    lib.i8ie_maxpool2d_f32_pad.argtypes = [_P, _P, _P] + [_I] * 8
    lib.i8ie_avgpool2d_u8_pad.argtypes = [_P, _P, _P] + [_I] * 9 + [_B]             # ... count_include_pad, zp
    lib.i8ie_avgpool2d_f32_pad.argtypes = [_P, _P, _P] + [_I] * 9
    lib.i8ie_maxpool2d_u8_nhwc_pad.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 9 + [_B]   # n c h w k s p ceil relu, zp
    lib.i8ie_avgpool2d_u8_nhwc_pad.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 10 + [_B]  # ... ceil include relu, zp
    for n in SYMBOLS:
        getattr(lib, n).restype = _I
    return lib
