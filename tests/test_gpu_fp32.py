"""The FP32 path (csrc/i8ie_fp32.hip: gemm_f32_kernel<CONV>, relu_f32_kernel, maxpool_f32_kernel) pinned to the plain
float64 reference of tests/f64_ref.py.  prepare() -> one FP32 batch -> convert() runs this path, so every calibrated
(scale, zero_point) comes out of it, and it is the FP32 teacher of the benchmark line.

Conv2d and Linear are checked on two data classes; neither needs a measured tolerance.

EXACT.  x, w integers in [-8, 8], b integers in [-64, 64], stored as float32.  Every partial sum, in any order, is an
integer of magnitude at most 64 K + 64 < 2^24 for K <= 9216, so it is representable and an fp32 fma (or multiply-add)
chain is exact whatever its order: the output must EQUAL the float64 result, bit for bit.  One dropped, doubled or
misplaced tap, a wrong padding decision, a wrong bias index or a wrong store address cannot pass it.

REAL.  x, w, b ~ U(-1, 1) float32.  The kernel computes fl(sum_k x_k w_k + b) as a chain of K fp32 fmas and one bias
add.  Each of these K + 1 operations rounds once (a product inside an fma is not rounded on its own), with relative
error at most u = 2^-24; for any order of the operations the standard dot-product bound follows (Higham, Accuracy
and Stability of Numerical Algorithms, 2nd ed., section 3.1):
    |got - exact| <= gamma(K+1) * mag,   gamma(n) = n u / (1 - n u),   mag = sum_k |x_k||w_k| + |b|
(a kernel that rounds the products too stays inside it: that is gamma(K) on the products and adds, K >= 1).  Added
to it: 2^-126 (K+1) absolute for partial results that underflow, and 2^-50 mag for the float64 reference's own
rounding.  It is asserted element by element.  Operands cut to bf16 give errors near 2^-9 sqrt(K) 0.3, far outside
it.  The bound grows like K^2 and by K ~ 2400 no longer sees one small tap, which is what the exact class is for:
the real class runs at K <= 400 plus one large-K case.

Every contraction output lies inside a larger device buffer whose guard floats before and after it must come back
untouched, and is pre-filled with a pattern that no element may still hold (abi.GuardedOut).

relu and max_pool2d are compared bit for bit (uint32 views) with f64_ref's restatement of the reference's
definitions, special values included."""
import ctypes as C
import zlib

import numpy as np
import pytest

import abi
import f64_ref
import support
import synth

pytestmark = pytest.mark.gpu


gpu = support.ctx_fixture()


# ---- the shapes: (reason, n, c, h, w, kc, kh, kw, stride, pad);  M = n*oh*ow rows, N = kc, K = c*kh*kw -------------
CONV_CASES = [
    # M edges around the 128-row tile
    ("M1", 1, 3, 3, 3, 20, 3, 3, 1, 0),
    ("M127", 1, 3, 1, 127, 20, 1, 1, 1, 0),
    ("M128", 2, 3, 8, 8, 20, 3, 3, 1, 1),
    ("M129", 1, 3, 3, 43, 20, 3, 3, 1, 1),
    ("M256", 4, 3, 8, 8, 20, 3, 3, 1, 1),
    ("P25-images-share-a-tile", 11, 3, 5, 5, 20, 3, 3, 1, 1),
    ("P25-N130", 11, 3, 5, 5, 130, 3, 3, 1, 1),
    ("P144", 1, 3, 12, 12, 20, 3, 3, 1, 1),
    ("P144-three-images", 3, 3, 12, 12, 33, 3, 3, 1, 1),
    ("M128-N128-K16-all-exact-tiles", 2, 16, 8, 8, 128, 1, 1, 1, 0),
    ("M256-N257", 4, 4, 8, 8, 257, 3, 3, 1, 1),
    # N edges around the 32-wide MFMA tile, the 64-wide wave slice and the 128-feature block (M = 162, K = 36)
    ("N1", 2, 4, 9, 9, 1, 3, 3, 1, 1),
    ("N31", 2, 4, 9, 9, 31, 3, 3, 1, 1),
    ("N32", 2, 4, 9, 9, 32, 3, 3, 1, 1),
    ("N33", 2, 4, 9, 9, 33, 3, 3, 1, 1),
    ("N63", 2, 4, 9, 9, 63, 3, 3, 1, 1),
    ("N65", 2, 4, 9, 9, 65, 3, 3, 1, 1),
    ("N127", 2, 4, 9, 9, 127, 3, 3, 1, 1),
    ("N128", 2, 4, 9, 9, 128, 3, 3, 1, 1),
    ("N129", 2, 4, 9, 9, 129, 3, 3, 1, 1),
    ("N130", 2, 4, 9, 9, 130, 3, 3, 1, 1),
    ("N257", 2, 4, 9, 9, 257, 3, 3, 1, 1),
    # K edges around the 16-deep K block (M = 200, N = 40)
    ("K1", 2, 1, 10, 10, 40, 1, 1, 1, 0),
    ("K2", 2, 2, 10, 10, 40, 1, 1, 1, 0),
    ("K5", 2, 5, 10, 10, 40, 1, 1, 1, 0),
    ("K5-one-channel-1x5", 2, 1, 10, 14, 40, 1, 5, 1, 0),
    ("K9", 2, 1, 10, 10, 40, 3, 3, 1, 1),
    ("K15", 2, 15, 10, 10, 40, 1, 1, 1, 0),
    ("K16", 2, 16, 10, 10, 40, 1, 1, 1, 0),
    ("K16-2x2", 2, 4, 11, 11, 40, 2, 2, 1, 0),
    ("K17", 2, 17, 10, 10, 40, 1, 1, 1, 0),
    ("K31", 2, 31, 10, 10, 40, 1, 1, 1, 0),
    ("K32", 2, 2, 13, 13, 40, 4, 4, 1, 0),
    ("K33", 2, 11, 10, 10, 40, 1, 3, 1, 1),
    ("K144-no-tail", 2, 16, 10, 10, 40, 3, 3, 1, 1),
    ("K363", 1, 3, 35, 35, 40, 11, 11, 4, 2),
    ("K363-N130", 2, 3, 35, 35, 130, 11, 11, 4, 2),
    # geometry
    ("1x1-stride1", 3, 7, 9, 11, 24, 1, 1, 1, 0),
    ("1x1-stride2", 3, 7, 9, 11, 24, 1, 1, 2, 0),
    ("1x1-stride2-N129", 3, 7, 9, 11, 129, 1, 1, 2, 0),
    ("3x3-pad0", 2, 6, 12, 12, 24, 3, 3, 1, 0),
    ("3x3-pad1", 2, 6, 12, 12, 24, 3, 3, 1, 1),
    ("3x3-pad2", 2, 6, 12, 12, 24, 3, 3, 1, 2),
    ("3x3-pad1-stride2", 2, 6, 13, 13, 24, 3, 3, 2, 1),
    ("5x5-pad2", 2, 3, 11, 11, 24, 5, 5, 1, 2),
    ("5x5-pad4-windows-in-padding", 2, 3, 3, 3, 24, 5, 5, 1, 4),
    ("2x2-stride3-pad3-windows-in-padding", 5, 4, 3, 3, 24, 2, 2, 3, 3),
    ("stride-larger-than-kernel", 2, 5, 14, 14, 24, 2, 2, 3, 0),
    ("kernel-is-padded-input", 3, 4, 4, 4, 24, 6, 6, 1, 1),
    ("kernel-is-input-N130", 130, 4, 5, 5, 130, 5, 5, 1, 0),
    ("1x7-on-19x23", 2, 3, 19, 23, 24, 1, 7, 1, 0),
    ("1x7-on-23x19-pad3", 2, 3, 23, 19, 24, 1, 7, 1, 3),
    ("7x1-on-19x23", 2, 3, 19, 23, 24, 7, 1, 1, 0),
    ("7x1-on-23x19-pad3-stride2", 2, 3, 23, 19, 24, 7, 1, 2, 3),
    ("3x5-on-19x23-pad1", 2, 3, 19, 23, 24, 3, 5, 1, 1),
    ("3x5-on-23x19-pad2-N129", 1, 3, 23, 19, 129, 3, 5, 1, 2),
    ("5x3-on-19x23-stride2", 2, 3, 19, 23, 24, 5, 3, 2, 1),
    ("reference-test-stride7-pad3", 30, 10, 50, 50, 20, 3, 3, 7, 3),
    ("reference-test-pad1", 30, 10, 22, 22, 20, 3, 3, 1, 1),
    ("two_conv-conv1", 16, 1, 28, 28, 20, 5, 5, 1, 0),
    ("two_conv-conv2", 16, 20, 12, 12, 50, 5, 5, 1, 0),
    # AlexNet at 2 images (conv4: N = 384 is a multiple of 128; conv1: M = 2 * 55 * 55 is not)
    ("alexnet-conv1", 2, 3, 224, 224, 96, 11, 11, 4, 2),
    ("alexnet-conv2", 2, 96, 27, 27, 256, 5, 5, 1, 2),
    ("alexnet-conv3", 2, 256, 13, 13, 384, 3, 3, 1, 1),
    ("alexnet-conv4", 2, 384, 13, 13, 384, 3, 3, 1, 1),
    ("alexnet-conv5", 2, 384, 13, 13, 256, 3, 3, 1, 1),
]

# (reason, m, k, n)
LINEAR_CASES = [
    ("M1", 1, 40, 24),
    ("M2", 2, 40, 24),
    ("M127", 127, 40, 24),
    ("M128", 128, 40, 24),
    ("M129", 129, 40, 24),
    ("M200", 200, 40, 24),
    ("M300", 300, 40, 24),
    ("N1", 50, 40, 1),
    ("N10", 50, 40, 10),
    ("N31", 50, 40, 31),
    ("N33", 50, 40, 33),
    ("N127", 50, 40, 127),
    ("N128", 50, 40, 128),
    ("N129", 50, 40, 129),
    ("N500", 50, 40, 500),
    ("K1", 50, 1, 24),
    ("K15", 50, 15, 24),
    ("K16", 50, 16, 24),
    ("K17", 50, 17, 24),
    ("K32", 50, 32, 24),
    ("K363", 50, 363, 24),
    ("K800", 50, 800, 24),
    ("M1-N1-K1", 1, 1, 1),
    ("M128-N128-K16-all-exact-tiles", 128, 16, 128),
    ("M129-N129-K17", 129, 17, 129),
    ("M300-N500-K33", 300, 33, 500),
    ("reference-test", 200, 800, 500),
    ("two_conv-fc1", 16, 800, 500),
    ("two_conv-fc2", 16, 500, 10),
    ("mnist-fc", 16, 784, 10),
    ("alexnet-fc1", 5, 9216, 4096),
    ("alexnet-fc3-large-K-real", 129, 4096, 10),
]

REAL_K_MAX = 400  # the real class: K <= 400, plus the cases named here
REAL_LARGE_K = {"alexnet-fc3-large-K-real"}


def _conv_K(cs):
    return cs[2] * cs[6] * cs[7]


def _classes(cases, K_of):
    out = []
    for cs in cases:
        out.append(pytest.param(cs, "exact", id=cs[0] + "-exact"))
        if K_of(cs) <= REAL_K_MAX or cs[0] in REAL_LARGE_K:
            out.append(pytest.param(cs, "real", id=cs[0] + "-real"))
    return out


def _data(rng, cls, xshape, wshape):
    if cls == "exact":
        return (rng.integers(-8, 9, xshape).astype(np.float32), rng.integers(-8, 9, wshape).astype(np.float32),
                rng.integers(-64, 65, wshape[0]).astype(np.float32))
    return (rng.uniform(-1, 1, xshape).astype(np.float32), rng.uniform(-1, 1, wshape).astype(np.float32),
            rng.uniform(-1, 1, wshape[0]).astype(np.float32))


def _check(cls, got, ok, want, mag, K, what):
    """got: the kernel's float32 output; want / mag: float64 reference and magnitude"""
    assert ok, "%s: a guard float outside the output was overwritten" % what
    assert got.shape == want.shape
    assert abi.GuardedOut.unwritten(got) == 0, "%s: %d output elements were never stored" % (
        what, abi.GuardedOut.unwritten(got))
    if cls == "exact":
        assert K <= 9216 and np.abs(want).max() < 2.0 ** 24 and np.array_equal(want, np.rint(want))
        want32 = (want + 0.0).astype(np.float32)  # exact: integers below 2^24
        bad = got.view(np.uint32) != want32.view(np.uint32)
        assert not bad.any(), "%s: %d of %d outputs differ from the exact result, first at %s: got %r, exact %r" % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want32[bad][0])
    else:
        err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, K)
        bad = ~(err <= bound)  # (a NaN is bad)
        assert not bad.any(), "%s: %d of %d outputs outside gamma(K+1) * mag, worst err / bound = %.3g" % (
            what, int(bad.sum()), bad.size, float(np.nanmax(err / bound)))


@pytest.mark.parametrize("cs,cls", _classes(CONV_CASES, _conv_K))
def test_conv2d_f32(gpu, cs, cls):
    reason, n, c, h, w, kc, kh, kw, stride, pad = cs
    rng = np.random.default_rng(zlib.crc32((reason + cls).encode()))
    x, wt, b = _data(rng, cls, (n, c, h, w), (kc, c, kh, kw))
    got, ok = gpu.conv2d_f32(x, wt, b, stride, pad)
    want = f64_ref.conv2d(x, wt, b, stride, pad)
    mag = f64_ref.conv2d_mag(x, wt, b, stride, pad) if cls == "real" else None
    _check(cls, got, ok, want, mag, c * kh * kw, "conv2d_f32 " + reason)


@pytest.mark.parametrize("cs,cls", _classes(LINEAR_CASES, lambda cs: cs[2]))
def test_linear_f32(gpu, cs, cls):
    reason, m, k, n = cs
    rng = np.random.default_rng(zlib.crc32((reason + cls).encode()))
    x, wt, b = _data(rng, cls, (m, k), (n, k))
    got, ok = gpu.linear_f32(x, wt, b)
    want = f64_ref.linear(x, wt, b)
    mag = f64_ref.linear_mag(x, wt, b) if cls == "real" else None
    _check(cls, got, ok, want, mag, k, "linear_f32 " + reason)


def test_case_lists_cover_the_edges():
    """the parameter lists above are data: hold the edges they were chosen for in place"""
    geo = [(n * f64_ref.conv_out_hw(h, w, kh, kw, s, p)[0] * f64_ref.conv_out_hw(h, w, kh, kw, s, p)[1],
            f64_ref.conv_out_hw(h, w, kh, kw, s, p)[0] * f64_ref.conv_out_hw(h, w, kh, kw, s, p)[1], kc, c * kh * kw)
           for _, n, c, h, w, kc, kh, kw, s, p in CONV_CASES]
    assert {1, 127, 128, 129, 256} <= {g[0] for g in geo}
    assert 25 in {g[1] for g in geo} and any(g[1] > 128 for g in geo)
    assert {1, 31, 32, 33, 127, 128, 129, 130, 257} <= {g[2] for g in geo}
    assert {1, 5, 15, 16, 17, 32, 33, 363} <= {g[3] for g in geo}
    assert {1, 2, 127, 128, 129, 200, 300} <= {c[1] for c in LINEAR_CASES}
    assert {1, 10, 127, 128, 129, 500} <= {c[3] for c in LINEAR_CASES}
    assert {1, 15, 16, 17, 800} <= {c[2] for c in LINEAR_CASES}
    assert len({c[0] for c in CONV_CASES}) == len(CONV_CASES) and len({c[0] for c in LINEAR_CASES}) == len(LINEAR_CASES)


# ---- max-pool and ReLU: bit for bit ------------------------------------------------------------------------------
def _bits_equal_f32(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(
        got.view(np.uint32), want.view(np.uint32))


POOL_KS = [(3, 2), (2, 2), (3, 1), (2, 1), (1, 2)]
# (reason, shape, (k, s) list)
POOL_CASES = [
    ("alexnet-pool1", (2, 96, 55, 55), [(3, 2)]),
    ("alexnet-pool2", (2, 256, 27, 27), [(3, 2), (2, 2)]),
    ("alexnet-pool3", (2, 256, 13, 13), [(3, 2), (3, 1)]),
    ("reference-test", (1, 1, 4, 4), POOL_KS + [(4, 1)]),          # k = h: a single output
    ("non-square", (5, 3, 17, 9), POOL_KS + [(9, 1), (9, 4)]),     # k = w: a single output column
    ("non-square-wide", (3, 2, 9, 17), POOL_KS + [(9, 2)]),
    ("two_conv-pool", (16, 20, 24, 24), [(2, 2)]),
]


@pytest.mark.parametrize("cs", POOL_CASES, ids=lambda cs: cs[0])
def test_maxpool2d_f32(gpu, cs):
    _, shape, kss = cs
    x = np.random.default_rng(sum(shape)).uniform(-100, 100, shape).astype(np.float32)
    for k, s in kss:
        assert _bits_equal_f32(gpu.maxpool2d_f32(x, k, s), f64_ref.max_pool2d(x, k, s)), (k, s)


RELU_SIZES = [1, 255, 256, 257, 256 * 32 * 256 + 3]  # the last is past cap_grid's 8192 blocks: the grid-stride loop wraps


@pytest.mark.parametrize("n", RELU_SIZES)
def test_relu_f32(gpu, n):
    x = np.random.default_rng(n).uniform(-100, 100, n).astype(np.float32)
    x[-1] = 7.25  # the very last element is stored, with its own value
    got = gpu.relu_f32(x)
    assert _bits_equal_f32(got, f64_ref.relu(x)) and got[-1] == np.float32(7.25)


def _specials():
    nan = np.float32(np.nan)
    return [np.float32(-0.0), np.float32(0.0), nan, -nan, np.float32(np.inf), np.float32(-np.inf), f64_ref.FLT_MAX,
            -f64_ref.FLT_MAX, np.float32(1e-45), np.float32(-1e-45), np.float32(1e-39), np.float32(-1e-39)]


def test_relu_f32_special_values(gpu):
    x = np.random.default_rng(11).uniform(-2, 2, 1000).astype(np.float32)
    sp = _specials()
    for i, v in enumerate(sp):  # at fixed positions, the first and last element among them
        x[(i * 83) % 1000] = v
    x[0], x[-1] = np.float32(-0.0), -np.float32(np.nan)
    got, want = gpu.relu_f32(x), f64_ref.relu(x)
    assert _bits_equal_f32(got, want)
    assert not np.isnan(got).any() and not np.signbit(got).any()  # NaN and -0.0 give +0.0


def test_maxpool2d_f32_special_values(gpu):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.random.default_rng(12).uniform(-2, 2, (2, 3, 12, 12)).astype(np.float32)
    sp = _specials()
    for i, v in enumerate(sp):
        x[1, i % 3, (5 * i) % 12, (7 * i) % 12] = v
    x[0, 0, 0, 0] = nan          # the first element of the first window of every (k, s)
    x[0, 0, 1, 1] = -nan         # the last element of that window for k = 2
    x[0, 0, 2, 8] = nan          # the last element of the (k = 3) window at (0, 6)
    x[0, 0, 11, 11] = nan        # the last element of the last window
    x[0, 1, 4:8, 4:8] = -inf     # whole windows of -inf for every k <= 3: the result is -FLT_MAX
    x[0, 2, :, :] = -inf         # a whole plane of it
    x[0, 2, 6, 6] = -f64_ref.FLT_MAX
    x[1, 0, 3, 3:6] = (inf, f64_ref.FLT_MAX, -0.0)
    x[1, 1, 8:10, 8:10] = ((-0.0, 0.0), (0.0, -0.0))  # a >= b keeps the first of equal values
    for k, s in POOL_KS + [(12, 1), (4, 4)]:
        got, want = gpu.maxpool2d_f32(x, k, s), f64_ref.max_pool2d(x, k, s)
        assert _bits_equal_f32(got, want), (k, s, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
    w = f64_ref.max_pool2d(x, 2, 2)
    assert w[0, 1, 2, 2] == -f64_ref.FLT_MAX and np.isnan(w[0, 0, 0, 0]) and np.isnan(w[0, 0, 5, 5])


# ---- the K table lives in the ctx workspace, which the INT8 path also reserves and may reallocate -------------
def test_workspace_shared_with_int8_path(orc):
    """conv2d_f32 (K = 363), linear_f32 (K = 5), an INT8 layer_forward through the im2col fallback whose scratch
    forces the workspace to grow (i8ie_ws_reserve synchronises the stream before it frees the old one), conv2d_f32
    (K = 17): queued on one ctx with no sync in between, each must give what it gives alone on a fresh ctx."""
    L = abi.lib()
    rng = np.random.default_rng(77)
    xa, wa, ba = _data(rng, "exact", (2, 3, 35, 35), (40, 3, 11, 11))
    xb, wb, bb = _data(rng, "exact", (130, 5), (33, 5))
    xd, wd, bd = _data(rng, "exact", (2, 17, 10, 10), (40, 17, 1, 1))
    cs = synth.conv_case(orc, 78, 16, 32, 32, 32, 32, 3, 1, 1)  # im2col scratch 16 * 1024 * 384 bytes = 6 MiB > 1 MiB

    def alone(f):
        c = abi.Ctx(0)
        try:
            return f(c)
        finally:
            c.close()

    def int8_alone(c):
        c.set_force_fallback(True)
        return c.layer_forward("conv", cs["q_in"], cs["qw"], cs["qb"], cs["s_in"], cs["zp_in"], cs["s_w"], cs["s_out"],
                               cs["zp_out"], stride=1, pad=1)

    (wa_out, ok_a) = alone(lambda c: c.conv2d_f32(xa, wa, ba, 4, 2))
    (wb_out, ok_b) = alone(lambda c: c.linear_f32(xb, wb, bb))
    (wc_out, wc_acc) = alone(int8_alone)
    (wd_out, ok_d) = alone(lambda c: c.conv2d_f32(xd, wd, bd, 1, 0))
    assert ok_a and ok_b and ok_d
    assert np.array_equal(wa_out, f64_ref.conv2d(xa, wa, ba, 4, 2)) and np.array_equal(wb_out, f64_ref.linear(xb, wb, bb))
    assert np.array_equal(wd_out, f64_ref.conv2d(xd, wd, bd, 1, 0))
    assert np.array_equal(wc_out, cs["out"]) and np.array_equal(wc_acc, cs["acc"])

    ctx = abi.Ctx(0)
    bufs = []
    layer = C.c_void_p()
    try:
        ctx.set_force_fallback(True)  # (an INT8 dispatch option: the FP32 calls do not read it)
        put = lambda a: bufs.append(ctx.put(a)) or bufs[-1]
        dxa, dwa, dba, dxb, dwb, dbb, dxd, dwd, dbd = (put(a) for a in (xa, wa, ba, xb, wb, bb, xd, wd, bd))
        dq = put(cs["q_in"])
        qw, qb = np.ascontiguousarray(cs["qw"], np.int8), np.ascontiguousarray(cs["qb"], np.int8)
        abi.ck(L.i8ie_conv2d_create(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), 32, 32, 3, 3, 1,
                                    1, C.c_float(cs["s_w"]), C.byref(layer)))
        abi.ck(L.i8ie_layer_set_output_qparams(layer, C.c_float(cs["s_out"]), C.c_uint8(cs["zp_out"])))
        oa, ob, od = ctx.guarded(wa_out.shape), ctx.guarded(wb_out.shape), ctx.guarded(wd_out.shape)
        oc_out, oc_acc = ctx.empty(wc_out.shape, np.uint8), ctx.empty(wc_acc.shape, np.int32)
        bufs += [oa, ob, od, oc_out, oc_acc]
        ctx.sync()
        # ---- the four calls, back to back
        abi.ck(L.i8ie_conv2d_f32(ctx.h, dxa.ptr, 2, 3, 35, 35, dwa.ptr, dba.ptr, 40, 11, 11, 4, 2, oa.ptr))
        abi.ck(L.i8ie_linear_f32(ctx.h, dxb.ptr, 130, 5, dwb.ptr, dbb.ptr, 33, ob.ptr))
        abi.ck(L.i8ie_layer_forward(layer, dq.ptr, 16, 32, 32, C.c_float(cs["s_in"]), C.c_uint8(cs["zp_in"]), oc_out.ptr,
                                    oc_acc.ptr))
        abi.ck(L.i8ie_conv2d_f32(ctx.h, dxd.ptr, 2, 17, 10, 10, dwd.ptr, dbd.ptr, 40, 1, 1, 1, 0, od.ptr))
        ctx.sync()
        (ga, ok_a), (gb, ok_b), (gd, ok_d) = oa.read(), ob.read(), od.read()
        assert ok_a and ok_b and ok_d
        assert _bits_equal_f32(ga, wa_out) and _bits_equal_f32(gb, wb_out) and _bits_equal_f32(gd, wd_out)
        assert np.array_equal(oc_out.get(), wc_out) and np.array_equal(oc_acc.get(), wc_acc)
    finally:
        if layer:
            L.i8ie_layer_destroy(layer)
        for d in bufs:
            d.free()
        ctx.close()


# ---- argument guards: return codes only (host side; nothing here runs the contraction kernel) -----------------
def test_linear_f32_refuses_more_rows_than_one_launch_covers(gpu):
    m = 65535 * 128 + 1
    x, w, b = gpu.empty((m, 1), np.float32), gpu.put(np.ones((1, 1), np.float32)), gpu.put(np.ones(1, np.float32))
    o = gpu.guarded((m, 1))  # (full-size buffers: the arguments are valid but for the row count)
    try:
        rc = abi.lib().i8ie_linear_f32(gpu.h, x.ptr, m, 1, w.ptr, b.ptr, 1, o.ptr)
        assert rc == -1 and b"more than 8.4 M output rows" in abi.lib().i8ie_last_error()
        gpu.sync()
        out, ok = o.read()
        assert ok and abi.GuardedOut.unwritten(out) == m  # the output is untouched
    finally:
        for d in (x, w, b, o):
            d.free()


@pytest.mark.parametrize("bad", [dict(kh=8), dict(kw=8), dict(kh=7, kw=7, pad=0), dict(stride=0), dict(stride=-1),
                                 dict(pad=-1)], ids=lambda d: "-".join("%s%d" % kv for kv in d.items()))
def test_conv2d_f32_refuses_bad_geometry(gpu, bad):
    g = dict(kh=3, kw=3, stride=1, pad=1)
    g.update(bad)  # on a 5x5 image: padded 7x7 (5x5 at pad 0)
    x, w = gpu.put(np.ones((1, 2, 5, 5), np.float32)), gpu.put(np.ones((4, 2, g["kh"], g["kw"]), np.float32))
    b, o = gpu.put(np.ones(4, np.float32)), gpu.guarded((1, 4, 7, 7))
    try:
        rc = abi.lib().i8ie_conv2d_f32(gpu.h, x.ptr, 1, 2, 5, 5, w.ptr, b.ptr, 4, g["kh"], g["kw"], g["stride"],
                                       g["pad"], o.ptr)
        assert rc == -1
        gpu.sync()
        out, ok = o.read()
        assert ok and abi.GuardedOut.unwritten(out) == out.size
    finally:
        for d in (x, w, b, o):
            d.free()


# ---- the Python surface, layer by layer -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", [("alexnet", 2), ("simple_conv", 16), ("two_conv", 16), ("mnist_fc", 16)])
def test_networks_layer_by_layer(name, batch):
    """Walk workloads.NETWORKS[name] by hand with the FP32 i8ie ops, every op fed the product's own previous output:
    conv / fc outputs within the real-class bound of f64_ref on that same input, relu / pool / flatten bit-identical;
    then net(x) in one call must equal the walked result bit for bit.  (The pybind11 callers of the four FP32 entry
    points, the reshape views between conv and fc, and the networks' own weight distributions.)"""
    import int8inferenceengine_amd  # noqa: F401
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    layers, spec, _ = wl.NETWORKS[name]
    sd = wl.synthetic_state_dict(name)
    net = wl.build(name)
    net.load(sd)
    x = wl.synthetic_input(name, batch, seed=5)
    t = i8ie.tensor(x)
    assert _bits_equal_f32(t.numpy(), x)
    for op in spec:
        prev = t.numpy()
        if op[0] == "layer":
            L, w, b = layers[op[1]], sd[op[1] + ".weight"], sd[op[1] + ".bias"]
            t = getattr(net, op[1])(t)
            got = t.numpy()
            if L[0] == "conv":
                want, mag = f64_ref.conv2d(prev, w, b, L[4], L[5]), f64_ref.conv2d_mag(prev, w, b, L[4], L[5])
                K = L[1] * L[3] * L[3]
            else:
                want, mag, K = f64_ref.linear(prev, w, b), f64_ref.linear_mag(prev, w, b), L[1]
            assert got.dtype == np.float32 and got.shape == want.shape
            err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, K)
            assert np.all(err <= bound), "%s %s: worst err / bound = %.3g" % (name, op[1], float(np.nanmax(err / bound)))
        elif op[0] == "relu":
            t = i8ie.relu(t)
            assert _bits_equal_f32(t.numpy(), f64_ref.relu(prev)), (name, op)
        elif op[0] == "pool":
            t = i8ie.max_pool2d(t, op[1], op[2])
            assert _bits_equal_f32(t.numpy(), f64_ref.max_pool2d(prev, op[1], op[2])), (name, op)
        else:
            t = t.reshape(-1, op[1])
            assert _bits_equal_f32(t.numpy(), prev.reshape(-1, op[1])), (name, op)
    walked = t.numpy()
    assert walked.shape == (batch, 10)
    assert _bits_equal_f32(net(i8ie.tensor(x)).numpy(), walked)
