"""Resize to any size and adaptive average pooling restated for the tests.  A helper module, not a
conftest.

The definitions are the ones of include/i8ie_hip.h.  Resize: per axis (input length L, output length O) axis() gives the taps
(i0, i1) and weights (w0, w1) of `den` as int64 arrays over the output index -- BILINEAR is torch's align_corners=False,
num = max((2 o + 1) L - O, 0) over den = 2 O; ALIGNED is align_corners=True, num = o (L - 1) over den = max(O - 1, 1); NEAREST
is i0 = i1 = o L // O with den = 1.  bilinear_sd is the exact (S, D) in int64, resize_u8 the bytes (S + D // 2) // D,
bilinear_f64 the float64 value S / D of any real input, resize_f32 the FP32 sequence in order (row blends first, one float32
rounding per operation).  Adaptive pool: windows() gives (start, length) per output index, [floor(i L / O), ceil((i + 1) L / O));
adaptive_sn the exact window sums and counts, adaptive_u8 the bytes (S + n // 2) // n, adaptive_f32 the fp32 sum in window
order (rows outer, columns inner) divided by float32(n).  The new C symbols get their ctypes signatures in bind()."""
import ctypes as C

import numpy as np

f32 = np.float32
NEAREST, BILINEAR, ALIGNED = 0, 1, 2
MODES = {"nearest": NEAREST, "bilinear": BILINEAR, "aligned": ALIGNED}
MAX_D = 1 << 22


def axis(L, O, mode):
    """(i0, i1, w0, w1, den): four int64 arrays over the O output indices of one axis and the common denominator"""
    mode = MODES.get(mode, mode)
    assert L > 0 and O > 0 and mode in (NEAREST, BILINEAR, ALIGNED)
    o = np.arange(O, dtype=np.int64)
    if mode == NEAREST:
        i0 = (o * L) // O
        return i0, i0.copy(), np.ones(O, np.int64), np.zeros(O, np.int64), 1
    if mode == BILINEAR:
        den = 2 * O
        num = np.maximum((2 * o + 1) * L - O, 0)
    else:
        den = max(O - 1, 1)
        num = o * (L - 1) if O > 1 else np.zeros(O, np.int64)
    i0, w1 = num // den, num % den
    return i0, np.minimum(i0 + 1, L - 1), den - w1, w1, den


def _four(x, oh, ow, mode):
    """the four taps of every output and the weights, broadcastable: (q00, q10, q01, q11, wy0, wy1, wx0, wx1, den_y, den_x)"""
    y0, y1, wy0, wy1, dy = axis(x.shape[2], oh, mode)
    x0, x1, wx0, wx1, dx = axis(x.shape[3], ow, mode)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    return (r0[:, :, :, x0], r1[:, :, :, x0], r0[:, :, :, x1], r1[:, :, :, x1], wy0[:, None], wy1[:, None], wx0[None, :], wx1[None, :], dy, dx)


def bilinear_sd(q, oh, ow, mode):
    """u8 [n, c, h, w] -> (S int64 [n, c, oh, ow], D)"""
    q00, q10, q01, q11, wy0, wy1, wx0, wx1, dy, dx = _four(np.asarray(q, np.uint8).astype(np.int64), oh, ow, mode)
    return wx0 * (wy0 * q00 + wy1 * q10) + wx1 * (wy0 * q01 + wy1 * q11), dy * dx


def nearest(x, oh, ow):
    x = np.asarray(x)
    y0, x0 = axis(x.shape[2], oh, NEAREST)[0], axis(x.shape[3], ow, NEAREST)[0]
    return np.ascontiguousarray(x[:, :, y0][:, :, :, x0])


def resize_u8(q, oh, ow, mode, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, oh, ow]; mode "nearest" / "bilinear" / "aligned" (or the codes)"""
    mode = MODES.get(mode, mode)
    q = np.asarray(q, np.uint8)
    if mode == NEAREST:
        out = nearest(q, oh, ow).astype(np.int64)
    else:
        S, D = bilinear_sd(q, oh, ow, mode)
        assert D <= MAX_D
        out = (S + D // 2) // D
        assert out.min() >= 0 and out.max() <= 255
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def bilinear_f64(x, oh, ow, mode):
    """S / D in float64 of any real input"""
    q00, q10, q01, q11, wy0, wy1, wx0, wx1, dy, dx = _four(np.asarray(x, np.float64), oh, ow, mode)
    return (wx0 * (wy0 * q00 + wy1 * q10) + wx1 * (wy0 * q01 + wy1 * q11)) / float(dy * dx)


def resize_f32(x, oh, ow, mode):
    """float32 in, float32 out, the FP32 sequence of include/i8ie_hip.h: every step one fp32 operation"""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, f32)
    if mode == NEAREST:
        return nearest(x, oh, ow)
    q00, q10, q01, q11, _, wy1, _, wx1, dy, dx = _four(x, oh, ow, mode)
    ly = (wy1.astype(f32) / f32(dy)).astype(f32)
    lx = (wx1.astype(f32) / f32(dx)).astype(f32)
    my, mx = (f32(1) - ly).astype(f32), (f32(1) - lx).astype(f32)
    with np.errstate(all="ignore"):
        top = ((q00 * mx).astype(f32) + (q01 * lx).astype(f32)).astype(f32)
        bot = ((q10 * mx).astype(f32) + (q11 * lx).astype(f32)).astype(f32)
        return ((top * my).astype(f32) + (bot * ly).astype(f32)).astype(f32)


# ---- adaptive average pool ----------------------------------------------------------------------------------------------
def windows(L, O):
    """(start, length) int64 arrays over the O outputs of one axis"""
    assert L > 0 and O > 0
    i = np.arange(O, dtype=np.int64)
    start = (i * L) // O
    return start, -((-(i + 1) * L) // O) - start


def adaptive_sn(q, oh, ow):
    """[n, c, h, w] (any integer or real dtype) -> (window sums in int64 / float64 [n, c, oh, ow], counts int64 [oh, ow])"""
    q = np.asarray(q)
    acc = np.float64 if q.dtype.kind == "f" else np.int64
    ys, yl = windows(q.shape[2], oh)
    xs, xl = windows(q.shape[3], ow)
    S = np.zeros(q.shape[:2] + (oh, ow), acc)
    for i in range(oh):
        for j in range(ow):
            S[:, :, i, j] = q[:, :, ys[i]:ys[i] + yl[i], xs[j]:xs[j] + xl[j]].astype(acc).sum(axis=(2, 3))
    return S, yl[:, None] * xl[None, :]


def adaptive_u8(q, oh, ow, relu=False, zp=0):
    S, n = adaptive_sn(np.asarray(q, np.uint8), oh, ow)
    out = (S + n // 2) // n
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def adaptive_f32(x, oh, ow):
    """the fp32 sum of each window, rows outer, columns inner, one rounding per addition, divided by float32(n)"""
    x = np.asarray(x, f32)
    ys, yl = windows(x.shape[2], oh)
    xs, xl = windows(x.shape[3], ow)
    out = np.zeros(x.shape[:2] + (oh, ow), f32)
    with np.errstate(all="ignore"):
        for i in range(oh):
            for j in range(ow):
                s = np.zeros(x.shape[:2], f32)
                for m in range(yl[i]):
                    for l in range(xl[j]):
                        s = (s + x[:, :, ys[i] + m, xs[j] + l]).astype(f32)
                out[:, :, i, j] = (s / f32(yl[i] * xl[j])).astype(f32)
    return out


# ---- ctypes signatures of the new entry points ----------------------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8
_IP = C.POINTER(C.c_int)


def bind(lib):
    lib.i8ie_resize_axis.argtypes = [_I] * 4 + [_IP] * 5
    lib.i8ie_resize2d_u8.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_resize2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_B]
    lib.i8ie_resize2d_f32.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_adaptive_avgpool2d_u8.argtypes = [_P, _P, _P] + [_I] * 6
    lib.i8ie_adaptive_avgpool2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 7 + [_B]
    lib.i8ie_adaptive_avgpool2d_f32.argtypes = [_P, _P, _P] + [_I] * 6
    for f in (lib.i8ie_resize_axis, lib.i8ie_resize2d_u8, lib.i8ie_resize2d_u8_nhwc, lib.i8ie_resize2d_f32,
              lib.i8ie_adaptive_avgpool2d_u8, lib.i8ie_adaptive_avgpool2d_u8_nhwc, lib.i8ie_adaptive_avgpool2d_f32):
        f.restype = _I
    return lib


def c_axis(lib, L, O, mode, o):
    """i8ie_resize_axis as (i0, i1, w0, w1, den)"""
    v = [C.c_int(-7) for _ in range(5)]
    rc = lib.i8ie_resize_axis(L, O, mode, o, *[C.byref(x) for x in v])
    assert rc == 0, rc
    return tuple(x.value for x in v)
