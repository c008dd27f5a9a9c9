"""tests/f64_ref.py, the float64 reference behind test_gpu_fp32.py, checked on the CPU: conv2d / linear against
torch in float64 (both sides are double, only the summation order differs: rtol 1e-12), relu / max_pool2d
against torch on finite data and against hand-written arrays for the special values, whose treatment the
reference's definitions fix (src/functional.cc:5-13, 36-64) and torch's do not share."""
import numpy as np
import pytest

import f64_ref

# (n, c, h, w, kc, kh, kw, stride, pad)
CONV_GEOMETRIES = [
    (2, 3, 9, 9, 4, 3, 3, 1, 0),
    (2, 3, 9, 9, 4, 3, 3, 1, 1),
    (1, 2, 8, 8, 5, 3, 3, 1, 2),      # pad > kernel / 2
    (1, 2, 3, 3, 3, 5, 5, 1, 4),      # pad > kernel / 2, whole windows in the padding
    (3, 1, 7, 7, 2, 1, 1, 1, 0),
    (3, 4, 7, 7, 2, 1, 1, 2, 0),
    (2, 2, 11, 11, 3, 2, 2, 3, 0),    # stride > kernel
    (1, 3, 19, 23, 6, 1, 7, 1, 3),    # rectangular kernel and image
    (1, 3, 23, 19, 6, 7, 1, 2, 3),
    (2, 2, 19, 23, 3, 3, 5, 2, 1),
    (1, 2, 5, 5, 7, 5, 5, 1, 0),      # kernel = input: one output pixel
    (1, 2, 4, 6, 7, 6, 8, 1, 1),      # kernel = padded input, rectangular
    (2, 10, 50, 50, 20, 3, 3, 7, 3),  # the reference tests' 7/3 case
    (1, 3, 35, 35, 8, 11, 11, 4, 2),  # AlexNet's stem geometry
]


def _check_double(got, want, mag, K, signed):
    """Both sides are double dot products of K terms plus a bias that differ in summation order only, so each is
    within gamma(K+1) * mag of the exact value, gamma taken at u = 2^-53: they differ by at most twice that
    (1.8e-13 * mag at K = 800, the largest here).  On data of one sign mag = |want| and this is rtol 1e-12 with
    room, asserted as such.  On signed data a sum that cancels to 1e-3 of its magnitude cannot be held to 1e-12
    of its own value by any correct summation (seen: 2 of 2500 outputs of the 800 -> 500 Linear off by 3e-12 of
    their value, 9e-15 absolute), so there the same figure is taken of the magnitude."""
    assert np.all(np.abs(got - want) <= 2 * (K + 1) * 2.0 ** -53 * mag)
    if not signed:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("g", CONV_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_conv2d_vs_torch_float64(g):
    import torch

    n, c, h, w, kc, kh, kw, stride, pad = g
    rng = np.random.default_rng(sum(g))
    K = c * kh * kw
    for lo in (-1.0, 0.0):
        x, wt, b = rng.uniform(lo, 1, (n, c, h, w)), rng.uniform(lo, 1, (kc, c, kh, kw)), rng.uniform(lo, 1, kc)
        want = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=stride,
                                          padding=pad).numpy()
        got = f64_ref.conv2d(x, wt, b, stride, pad)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert got.shape[2:] == f64_ref.conv_out_hw(h, w, kh, kw, stride, pad)
        mag = f64_ref.conv2d_mag(x, wt, b, stride, pad)
        _check_double(got, want, mag, K, signed=lo < 0)
        # mag is the same function on absolute values
        want_mag = torch.nn.functional.conv2d(torch.from_numpy(np.abs(x)), torch.from_numpy(np.abs(wt)),
                                              torch.from_numpy(np.abs(b)), stride=stride, padding=pad).numpy()
        np.testing.assert_allclose(mag, want_mag, rtol=1e-12, atol=0)
        assert np.all(mag >= np.abs(got))


def test_conv2d_accepts_float32_and_widens():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (1, 2, 5, 5)).astype(np.float32)
    w = rng.uniform(-1, 1, (3, 2, 3, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, 3).astype(np.float32)
    got = f64_ref.conv2d(x, w, b, 1, 1)
    assert got.dtype == np.float64
    assert np.array_equal(got, f64_ref.conv2d(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), 1, 1))


def test_conv2d_exact_on_small_integers():
    """the exact data class of test_gpu_fp32.py: integer data gives the integer result, in a hand-checkable case"""
    x = np.arange(1, 10, dtype=np.float32).reshape(1, 1, 3, 3)
    w = np.ones((1, 1, 3, 3), np.float32)
    got = f64_ref.conv2d(x, w, np.array([10.0]), 1, 1)
    want = np.array([[12, 21, 16], [27, 45, 33], [24, 39, 28]], np.float64) + 10
    assert np.array_equal(got[0, 0], want)
    # a 5x5 window at pad 4 on the 3x3 image: the corner windows see one input value, whole windows none
    got = f64_ref.conv2d(x, np.ones((1, 1, 5, 5)), np.array([0.5]), 1, 4)
    assert got.shape == (1, 1, 7, 7) and got[0, 0, 0, 0] == 1.5 and got[0, 0, 6, 6] == 9.5 and got[0, 0, 3, 3] == 45.5
    got = f64_ref.conv2d(x, np.ones((1, 1, 2, 2)), np.array([0.5]), 3, 3)  # windows wholly in the padding
    assert got.shape == (1, 1, 3, 3) and got[0, 0, 0, 0] == 0.5 and got[0, 0, 1, 1] == 12.5 and got[0, 0, 2, 2] == 0.5


@pytest.mark.parametrize("mkn", [(1, 1, 1), (2, 15, 10), (127, 16, 3), (129, 17, 130), (5, 800, 500), (200, 63, 7)])
def test_linear_vs_torch_float64(mkn):
    import torch

    m, k, n = mkn
    rng = np.random.default_rng(m * 1000 + k)
    for lo in (-1.0, 0.0):
        x, w, b = rng.uniform(lo, 1, (m, k)), rng.uniform(lo, 1, (n, k)), rng.uniform(lo, 1, n)
        want = torch.nn.functional.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)).numpy()
        got = f64_ref.linear(x, w, b)
        assert got.dtype == np.float64
        mag = f64_ref.linear_mag(x, w, b)
        _check_double(got, want, mag, k, signed=lo < 0)
        np.testing.assert_allclose(mag, np.abs(x) @ np.abs(w).T + np.abs(b), rtol=1e-12, atol=0)
        assert np.all(mag >= np.abs(got))


@pytest.mark.parametrize("ks", [(3, 2), (2, 2), (3, 1), (2, 1), (1, 2), (9, 1)])
@pytest.mark.parametrize("shape", [(1, 1, 9, 9), (2, 3, 17, 9), (1, 2, 13, 27)])
def test_max_pool_and_relu_vs_torch_on_finite_data(shape, ks):
    import torch

    k, s = ks
    x = np.random.default_rng(k * 10 + s).uniform(-100, 100, shape).astype(np.float32)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x), k, s).numpy()
    got = f64_ref.max_pool2d(x, k, s)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    r = f64_ref.relu(x)
    assert r.dtype == np.float32 and np.array_equal(r.view(np.uint32), torch.relu(torch.from_numpy(x)).numpy().view(np.uint32))


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_relu_special_values():
    nan, inf, fmax = np.float32(np.nan), np.float32(np.inf), f64_ref.FLT_MAX
    den = np.float32(1e-45)
    x = np.array([-0.0, 0.0, nan, -nan, inf, -inf, fmax, -fmax, den, -den, 1.5, -1.5], np.float32)
    want = np.array([0.0, 0.0, 0.0, 0.0, inf, 0.0, fmax, 0.0, den, 0.0, 1.5, 0.0], np.float32)
    got = f64_ref.relu(x)
    assert np.array_equal(_bits(got), _bits(want))  # every zero is +0.0: the sign bit would show here
    assert not np.signbit(got).any()


def test_max_pool_special_values():
    nan, inf, fmax = np.float32(np.nan), np.float32(np.inf), f64_ref.FLT_MAX
    # one row of 2x2 windows (k = 2, s = 2) on a 2 x 14 plane; window order: (0,0) (0,1) (1,0) (1,1)
    wins = [
        ((nan, 1, 2, 3), 3.0),           # NaN first: replaced by the next element, then a plain maximum
        ((1, 2, 3, nan), nan),           # NaN last: replaces the running maximum and stays
        ((5, nan, 1, 2), 2.0),           # NaN in the middle: the element after it restarts the maximum (not 5)
        ((-inf, -inf, -inf, -inf), -fmax),  # -inf never beats the start value
        ((-inf, -fmax, -inf, -inf), -fmax),
        ((-0.0, 0.0, -0.0, -0.0), -0.0),  # a >= b keeps the first of equal values: -0.0 >= +0.0
        ((0.0, -0.0, 0.0, 0.0), 0.0),
    ]
    x = np.zeros((1, 1, 2, 2 * len(wins)), np.float32)
    for i, (v, _) in enumerate(wins):
        x[0, 0, 0, 2 * i:2 * i + 2] = v[:2]
        x[0, 0, 1, 2 * i:2 * i + 2] = v[2:]
    got = f64_ref.max_pool2d(x, 2, 2)
    want = np.array([w for _, w in wins], np.float32).reshape(1, 1, 1, -1)
    assert got.shape == want.shape
    nanmask = np.isnan(want)
    assert np.array_equal(np.isnan(got), nanmask)
    assert np.array_equal(_bits(got)[~nanmask], _bits(want)[~nanmask])
    # +inf and +-FLT_MAX are ordinary ordered values
    y = np.array([[-fmax, 1], [inf, fmax]], np.float32).reshape(1, 1, 2, 2)
    assert f64_ref.max_pool2d(y, 2, 2)[0, 0, 0, 0] == inf
    assert f64_ref.max_pool2d(y, 1, 1).tobytes() == y.tobytes()


def test_dot_bound_holds_for_numpy_fp32_and_sees_bf16():
    """the real-class bound on the CPU, with numpy's fp32 matmul in place of the kernel: inside the bound; the
    same operands cut to bf16 precision: outside it"""
    rng = np.random.default_rng(3)
    for k in (5, 363):
        x = rng.uniform(-1, 1, (64, k)).astype(np.float32)
        w = rng.uniform(-1, 1, (48, k)).astype(np.float32)
        b = rng.uniform(-1, 1, 48).astype(np.float32)
        want, bound = f64_ref.linear(x, w, b), f64_ref.dot_bound(f64_ref.linear_mag(x, w, b), k)
        got = x @ w.T + b
        assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
        xc = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        cut = xc @ w.T + b
        assert np.any(np.abs(cut.astype(np.float64) - want) > bound)
