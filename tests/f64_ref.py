"""A plain float64 numpy reference of the FP32 ops (Conv2d, Linear, relu, max_pool2d), used to pin
csrc/i8ie_fp32.hip (test_gpu_fp32.py) and itself checked against torch in float64 on the CPU
(test_f64_ref.py).  A helper module, not a conftest.

conv2d / linear accumulate in float64; the *magnitude* mag = sum_k |x_k||w_k| + |b| that the
rounding bound scales with is the same function called on absolute values (conv2d_mag / linear_mag).

relu / max_pool2d restate the reference's definitions (src/functional.cc:5-13, 36-64), which fix what
happens to the special values:
  relu      v > 0 ? v : 0                       -0.0 and NaN give +0.0
  max_pool  mx = -FLT_MAX; mx = mx >= v ? mx : v   a NaN element replaces the running maximum (mx >= NaN is
                                                false), a later non-NaN element replaces a NaN (NaN >= v is
                                                false), -inf never beats -FLT_MAX
They are written with np.where on the comparison itself: np.maximum differs on NaN.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

FLT_MAX = np.float32(3.402823466e+38)


def conv_out_hw(h, w, kh, kw, stride, pad):
    return (h - kh + 2 * pad) // stride + 1, (w - kw + 2 * pad) // stride + 1


def conv2d(x, w, b, stride, pad):
    """x [n, c, h, w], w [kc, c, kh, kw], b [kc] -> float64 [n, kc, oh, ow]; zero padding on all four sides."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    n, c, h, wd = x.shape
    kc, c2, kh, kw = w.shape
    assert c == c2 and b.shape == (kc,) and stride > 0 and pad >= 0
    assert h + 2 * pad >= kh and wd + 2 * pad >= kw
    xp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad), np.float64)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    win = sliding_window_view(xp, (kh, kw), axis=(2, 3))[:, :, ::stride, ::stride]  # [n, c, oh, ow, kh, kw]
    oh, ow = win.shape[2], win.shape[3]
    cols = win.transpose(0, 2, 3, 1, 4, 5).reshape(n * oh * ow, c * kh * kw)  # im2col, K in (c, kh, kw) order
    out = cols @ w.reshape(kc, c * kh * kw).T + b
    return np.ascontiguousarray(out.reshape(n, oh, ow, kc).transpose(0, 3, 1, 2))


def linear(x, w, b):
    """x [m, k], w [n, k], b [n] -> float64 [m, n]."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    assert x.shape[1] == w.shape[1] and b.shape == (w.shape[0],)
    return x @ w.T + b


def conv2d_mag(x, w, b, stride, pad):
    return conv2d(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                  np.abs(np.asarray(b, np.float64)), stride, pad)


def linear_mag(x, w, b):
    return linear(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                  np.abs(np.asarray(b, np.float64)))


def relu(x):
    """v > 0 ? v : 0 in x's own dtype (the comparison is exact in any format)."""
    x = np.asarray(x)
    return np.where(x > 0, x, x.dtype.type(0))


def max_pool2d(x, k, s):
    """x [n, c, h, w] -> [n, c, (h-k)//s+1, (w-k)//s+1], no padding; the running a >= b ? a : b from -FLT_MAX,
    window rows outer, columns inner (the order matters once a NaN is in the window)."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    assert 0 < k <= h and k <= w and s > 0
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    mx = np.full((n, c, oh, ow), -FLT_MAX, x.dtype)
    with np.errstate(invalid="ignore"):
        for m in range(k):
            for l in range(k):
                v = x[:, :, m:m + (oh - 1) * s + 1:s, l:l + (ow - 1) * s + 1:s]
                mx = np.where(mx >= v, mx, v)
    return mx


# ---- the rounding bound of an fp32 dot product --------------------------------------------------------------
U = 2.0 ** -24  # unit roundoff of binary32


def gamma(n):
    nu = n * U
    assert nu < 1
    return nu / (1 - nu)


def dot_bound(mag, K):
    """Bound on |fl(sum_k x_k w_k + b) - exact| for ANY order of K fp32 fmas (or multiplies and adds) and one
    bias add: gamma(K+1) * mag, the standard dot-product bound (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., section 3.1), plus 2^-126 per operation for partial results that underflow, plus
    2^-50 * mag for the float64 reference's own rounding (its error relative to the first term is 2^-29)."""
    mag = np.asarray(mag, np.float64)
    return gamma(K + 1) * mag + 2.0 ** -126 * (K + 1) + 2.0 ** -50 * mag
