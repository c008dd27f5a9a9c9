"""Resize to any size and adaptive average pooling on the GPU (csrc/i8ie_resize.hip).  Every comparison
is for equality of every byte with the numpy restatement of the definition (tests/resize_ref.py), never with the code under
test: the size pairs in every item width through both kernels of each op (the kernel that ran checked by name), the rounding
cases, the D limit, agreement with the upsample and average-pool kernels where the ops coincide, every divisor of the pool at
its rounding boundaries, the bordered / re-biased layout matrix with guard bytes and poisoned borders, a grid that wraps, the
FP32 entries, and the Python surface with routing, launch counts, a replayed graph and a pyramid pooling module."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import avgpool_ref as ar
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import pointwise_util as pu
import resize_ref as rr
import support
from support import i8ie  # noqa: F401
import upsample_ref as ur

pytestmark = pytest.mark.gpu
f32 = np.float32
CHANNELS = [3, 20, 16, 48]  # item widths 1, 4, 16 and a pixel of several items
MODES = [rr.NEAREST, rr.BILINEAR, rr.ALIGNED]
POOL = -1  # the adaptive pool, where a mode is asked for
SIZES = [((1, 1), (5, 3)), ((5, 3), (1, 1)), ((3, 5), (8, 7)), ((8, 7), (3, 5)), ((7, 6), (7, 6)), ((6, 4), (4, 6)), ((5, 2), (13, 16)),
         ((13, 16), (5, 2))]
POOL_SIZES = [((8, 8), (3, 3)), ((8, 8), (6, 6)), ((8, 8), (5, 5)), ((7, 5), (3, 4)), ((3, 4), (7, 5)), ((6, 6), (2, 3)), ((13, 13), (6, 6))]
FAST = {True: "resize_u8_nhwc", False: "adaptive_avgpool_u8_nhwc"}
DIRECT = {True: "resize_u8_direct", False: "adaptive_avgpool_u8_direct"}

ctx = support.ctx_fixture(rr, ur, ar)


def _assert_same(got, want, tag):
    """bit equality, with the first few places that differ in the message"""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, "%d of %d differ" % (len(bad), want.size),
                           [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
    return True


def _want(q, oh, ow, mode, relu=False, zp=0):
    return rr.adaptive_u8(q, oh, ow, relu, zp) if mode == POOL else rr.resize_u8(q, oh, ow, mode, relu, zp)


def _nchw(ctx, q, oh, ow, mode):
    """the flat NCHW entry -> (bytes, the names of the kernels that ran)"""
    n, c, h, w = q.shape
    di, do = ctx.put(q), abi.GuardedU8(ctx, (n, c, oh, ow), fill=0xEE)
    try:
        if mode == POOL:
            _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_adaptive_avgpool2d_u8(ctx.h, di.ptr, do.ptr, n, c, h, w, oh, ow)))
        else:
            _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_resize2d_u8(ctx.h, di.ptr, do.ptr, n, c, h, w, oh, ow, mode)))
        got = do.get()
        assert do.guards_ok(), "a byte outside the NCHW result was written"
        return got, names
    finally:
        di.free()
        do.free()


def _nhwc(ctx, q, oh, ow, mode, relu=False, zp=0, ib=0, ob=0, in_s8=0, out_s8=0, skew=0, in_fill=0xC7, out_fill=0x3C):
    """q NCHW logical -> (the NHWC entry's result, NCHW logical again; the names of the kernels that ran).  The input's border
    holds in_fill (not the zero point, not the edge pixel: a kernel that read it would blend it in); the output's border holds
    out_fill and, like the guard bytes around both buffers, must come back untouched (pointwise_util.interior asserts it).
    skew: both buffers start that many bytes off their allocation's alignment."""
    n, c, h, w = q.shape
    x = np.ascontiguousarray(q.transpose(0, 2, 3, 1))
    fi, _ = pu.phys(x, ib, in_fill, in_s8, skew)
    fo, oshape = pu.phys(np.full((n, oh, ow, c), 0xEE, np.uint8), ob, out_fill, out_s8, skew)
    di, do = ctx.put(fi), ctx.put(fo)
    pi, po = C.c_void_p(di.ptr.value + pu.GUARD + skew), C.c_void_p(do.ptr.value + pu.GUARD + skew)
    try:
        if mode == POOL:
            call = lambda: abi.ck(abi.lib().i8ie_adaptive_avgpool2d_u8_nhwc(ctx.h, pi, ib, in_s8, po, ob, out_s8, n, c, h, w, oh, ow, 1 if relu else 0, zp))
        else:
            call = lambda: abi.ck(abi.lib().i8ie_resize2d_u8_nhwc(ctx.h, pi, ib, in_s8, po, ob, out_s8, n, c, h, w, oh, ow, mode, 1 if relu else 0, zp))
        _, names = ctx.kernels_run(call)
        gi, go = di.get(), do.get()
    finally:
        di.free()
        do.free()
    assert np.array_equal(gi, fi), "the input (and its guards) must be untouched"
    return np.ascontiguousarray(pu.interior(go, oshape, ob, out_fill, out_s8, skew).transpose(0, 3, 1, 2)), names


def _both_kernels(ctx, q, oh, ow, mode, tag, relu=False, zp=0):
    """the fast NHWC kernel, and the direct kernel by its three ways in: the flat entry, buffers one byte off, the option"""
    is_resize = mode != POOL
    want = _want(q, oh, ow, mode, relu, zp)
    got, names = _nhwc(ctx, q, oh, ow, mode, relu, zp)
    assert names == [FAST[is_resize]], names
    assert _assert_same(got, want, tag + ("nhwc",))
    got, names = _nhwc(ctx, q, oh, ow, mode, relu, zp, skew=1)
    assert names == [(DIRECT if q.shape[1] % 4 == 0 else FAST)[is_resize]], names  # (byte items have no alignment to miss)
    assert _assert_same(got, want, tag + ("off by one",))
    ctx.set_force_fallback(True)
    try:
        got, names = _nhwc(ctx, q, oh, ow, mode, relu, zp, ib=1, ob=1, in_s8=1)
    finally:
        ctx.set_force_fallback(False)
    assert names == [DIRECT[is_resize]], names
    assert _assert_same(got, want, tag + ("forced",))
    got, names = _nchw(ctx, q, oh, ow, mode)
    assert names == [DIRECT[is_resize]], names
    assert _assert_same(got, _want(q, oh, ow, mode), tag + ("flat",))


# ---- 1. the size pairs, every item width, both kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
def test_resize_size_pairs(ctx, c):
    rng = np.random.default_rng(c)
    for ((h, w), (oh, ow)), mode in itertools.product(SIZES, MODES):
        q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
        _both_kernels(ctx, q, oh, ow, mode, (c, h, w, oh, ow, mode))


@pytest.mark.parametrize("c", CHANNELS)
def test_adaptive_pool_size_pairs(ctx, c):
    rng = np.random.default_rng(50 + c)
    for (h, w), (oh, ow) in POOL_SIZES:
        q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
        _both_kernels(ctx, q, oh, ow, POOL, (c, h, w, oh, ow))


# ---- 2. rounding -----------------------------------------------------------------------------------------------------------
def _reachable(L, O, mode):
    """the residues S mod D that bytes can reach with an axis (L -> O) on both sides: the multiples of
    g = gcd(the four weight products, D), united over the output positions"""
    import math

    _, _, w0, w1, den = rr.axis(L, O, mode)
    D, out = den * den, set()
    for a0, a1 in zip(w0, w1):
        for b0, b1 in zip(w0, w1):
            g = D
            for p in (a0 * b0, a1 * b0, a0 * b1, a1 * b1):
                g = math.gcd(g, int(p))
            out |= set(range(0, D, g))
    return out


def test_rounding(ctx):
    """the tie goes up; every residue of S mod D that (3 -> 8), not aligned, can reach on a one-channel ramp; all 0, all 255"""
    for lo in (0, 254):
        q = np.array([lo, lo + 1], np.uint8).reshape(1, 1, 1, 2)
        S, D = rr.bilinear_sd(q, 1, 3, rr.ALIGNED)
        assert D == 2 and S.ravel().tolist() == [2 * lo, 2 * lo + 1, 2 * lo + 2]
        for got in (_nhwc(ctx, q, 1, 3, rr.ALIGNED)[0], _nchw(ctx, q, 1, 3, rr.ALIGNED)[0]):
            assert got.ravel().tolist() == [lo, lo + 1, lo + 1]
    ramp = np.arange(256, dtype=np.uint8)
    q = np.stack([np.stack([ramp[(17 * i + 31 * j + 7 * k) % 256] for j in range(3)]) for k in range(64) for i in range(3)]).reshape(64, 1, 3, 3)
    q = np.concatenate([q, np.random.default_rng(2).integers(0, 256, (64, 1, 3, 3), dtype=np.uint8)])
    S, D = rr.bilinear_sd(q, 8, 8, rr.BILINEAR)
    reached, reachable = set(np.unique(S % D).tolist()), _reachable(3, 8, rr.BILINEAR)
    print("3 -> 8: D = %d, %d of %d reachable residues, ties %s" % (D, len(reached), len(reachable), D // 2 in reached))
    assert D == 256 and reached == reachable and D // 2 in reached
    _both_kernels(ctx, q, 8, 8, rr.BILINEAR, ("ramp",))
    for v in (0, 255):
        q = np.full((1, 20, 5, 3), v, np.uint8)
        for mode in MODES:
            _both_kernels(ctx, q, 7, 11, mode, ("all", v, mode))
        _both_kernels(ctx, q, 2, 2, POOL, ("all", v, "pool"))


# ---- 3. the D limit --------------------------------------------------------------------------------------------------------
def test_d_limit(ctx):
    """2 x 2 -> 1024 x 1024, not aligned: D = 2^22, S + D / 2 up to 255.5 * 2^22 < 2^31; every byte.  1024 x 1025 is refused."""
    q = np.array([255, 0, 255, 254], np.uint8).reshape(1, 1, 2, 2)
    S, D = rr.bilinear_sd(q, 1024, 1024, rr.BILINEAR)
    assert D == 1 << 22 and int(S.max()) + D // 2 == 255 * D + D // 2 < 2 ** 31
    want = rr.resize_u8(q, 1024, 1024, rr.BILINEAR)
    got, names = _nhwc(ctx, q, 1024, 1024, rr.BILINEAR)
    assert names == ["resize_u8_nhwc"] and _assert_same(got, want, ("nhwc",))
    got, names = _nchw(ctx, q, 1024, 1024, rr.BILINEAR)
    assert names == ["resize_u8_direct"] and _assert_same(got, want, ("flat",))
    # D just below the limit and no power of two: the multiplier at its largest x
    q3 = np.array([255, 255, 255, 254], np.uint8).reshape(1, 1, 2, 2)
    want = rr.resize_u8(q3, 1023, 1025, rr.BILINEAR)
    assert _assert_same(_nhwc(ctx, q3, 1023, 1025, rr.BILINEAR)[0], want, ("1023 x 1025",))
    buf = ctx.put(np.zeros(64, np.uint8))
    try:
        lib = abi.lib()
        assert lib.i8ie_resize2d_u8_nhwc(ctx.h, buf.ptr, 0, 0, buf.ptr, 0, 0, 1, 1, 2, 2, 1024, 1025, rr.BILINEAR, 0, 0) == -1
        assert lib.i8ie_resize2d_u8(ctx.h, buf.ptr, buf.ptr, 1, 1, 2, 2, 1024, 1025, rr.BILINEAR) == -1
        assert (buf.get() == 0).all()
    finally:
        buf.free()


# ---- 4. agreement with the existing kernels --------------------------------------------------------------------------------
def test_agrees_with_the_upsample_and_avg_pool_kernels(ctx):
    lib = abi.lib()
    q = np.random.default_rng(3).integers(0, 256, (2, 20, 5, 7), dtype=np.uint8)
    x = np.ascontiguousarray(q.transpose(0, 2, 3, 1))
    for fh, fw in [(2, 2), (2, 3)]:
        for mode in (rr.NEAREST, rr.BILINEAR):
            di, do = ctx.put(x), ctx.put(np.zeros((2, 5 * fh, 7 * fw, 20), np.uint8))
            try:
                abi.ck(lib.i8ie_upsample2d_u8_nhwc(ctx.h, di.ptr, 0, 0, do.ptr, 0, 0, 2, 20, 5, 7, fh, fw, mode, 0, 0))
                old = do.get()
                abi.ck(lib.i8ie_resize2d_u8_nhwc(ctx.h, di.ptr, 0, 0, do.ptr, 0, 0, 2, 20, 5, 7, 5 * fh, 7 * fw, mode, 0, 0))
                assert _assert_same(do.get(), old, (fh, fw, mode))
            finally:
                di.free()
                do.free()
    xf = (np.random.default_rng(4).standard_normal((2, 5, 3, 4)) * 7).astype(f32)
    di, d1, d2 = ctx.put(xf), ctx.put(np.zeros((2, 5, 6, 8), f32)), ctx.put(np.zeros((2, 5, 6, 8), f32))
    try:
        for mode in (rr.NEAREST, rr.BILINEAR):
            abi.ck(lib.i8ie_upsample2d_f32(ctx.h, di.ptr, d1.ptr, 2, 5, 3, 4, 2, 2, mode))
            abi.ck(lib.i8ie_resize2d_f32(ctx.h, di.ptr, d2.ptr, 2, 5, 3, 4, 6, 8, mode))
            assert support.same_bits(d2.get(), d1.get())
    finally:
        for d in (di, d1, d2):
            d.free()
    q = np.random.default_rng(5).integers(0, 256, (2, 16, 8, 8), dtype=np.uint8)
    di, do = ctx.put(support.nhwc(q)), ctx.put(np.zeros((2, 4, 4, 16), np.uint8))
    try:
        abi.ck(lib.i8ie_avgpool2d_u8_nhwc(ctx.h, di.ptr, 0, 0, do.ptr, 0, 0, 2, 16, 8, 8, 2, 2, 2, 0, 0))
        old = do.get()
        abi.ck(lib.i8ie_adaptive_avgpool2d_u8_nhwc(ctx.h, di.ptr, 0, 0, do.ptr, 0, 0, 2, 16, 8, 8, 4, 4, 0, 0))
        assert _assert_same(do.get(), old, "pool 8 -> 4")
    finally:
        di.free()
        do.free()


# ---- 5. every divisor of the pool at its rounding boundaries ---------------------------------------------------------------
def _boundary_planes(h, w, oh, ow, rng):
    """[planes, h, w] u8 and the list of (plane, i, j, T): per distinct window size n one output position whose window sums
    to T, for T on k n + n / 2 - 1 and k n + n / 2 (k = 0, 1, 100, 254) and on 255 n; everything else random"""
    ys, yl = rr.windows(h, oh)
    xs, xl = rr.windows(w, ow)
    first = {}
    for i, j in itertools.product(range(oh), range(ow)):
        first.setdefault(int(yl[i] * xl[j]), (i, j))
    planes, marks = [], []
    for n, (i, j) in sorted(first.items()):
        targets = [k * n + n // 2 - d for k in (0, 1, 100, 254) for d in (1, 0)] + [255 * n]
        for T in targets:
            if T < 0:
                continue
            p = rng.integers(0, 256, (h, w), dtype=np.uint8)
            cells = np.full(n, T // n, np.int64)
            cells[:T % n] += 1
            p[ys[i]:ys[i] + yl[i], xs[j]:xs[j] + xl[j]] = cells.reshape(yl[i], xl[j])
            marks.append((len(planes), i, j, T))
            planes.append(p)
    return np.stack(planes), marks


@pytest.mark.parametrize("c", CHANNELS)
def test_adaptive_pool_divisors_at_their_boundaries(ctx, c):
    rng = np.random.default_rng(70 + c)
    for (h, w), (oh, ow) in POOL_SIZES:
        planes, marks = _boundary_planes(h, w, oh, ow, rng)
        images = -(-len(planes) // c)
        q = rng.integers(0, 256, (images * c, h, w), dtype=np.uint8)
        q[:len(planes)] = planes
        q = q.reshape(images, c, h, w)
        S, n = rr.adaptive_sn(q, oh, ow)
        assert sorted(set(n.ravel().tolist())) == sorted({int(n[i, j]) for _, i, j, _ in marks})
        for p, i, j, T in marks:
            assert S[p // c, p % c, i, j] == T
        _both_kernels(ctx, q, oh, ow, POOL, (c, h, w, oh, ow, "boundaries"))


# ---- 6. the layout matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
def test_layout_matrix(ctx, c):
    rng = np.random.default_rng(100 + c)
    q = rng.integers(0, 256, (2, c, 5, 4), dtype=np.uint8)
    q[0, :, 0, :], q[1, :, :, 0] = 255, 0
    for (oh, ow), mode in [((7, 9), rr.BILINEAR), ((7, 9), rr.ALIGNED), ((3, 2), rr.BILINEAR), ((7, 9), rr.NEAREST), ((3, 3), POOL), ((7, 6), POOL)]:
        for relu, zp in [(False, 0), (True, 128)]:
            want = _want(q, oh, ow, mode, relu, zp)
            assert not relu or ((want == zp).any() and (want > zp).any())  # (zp lies in the middle of the data)
            for ib, ob, in_s8, out_s8 in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1)):
                got, names = _nhwc(ctx, q, oh, ow, mode, relu, zp, ib, ob, in_s8, out_s8)
                assert names == [FAST[mode != POOL]]
                assert _assert_same(got, want, (c, oh, ow, mode, relu, zp, ib, ob, in_s8, out_s8))


# ---- 7. a grid that wraps, and FP32 ----------------------------------------------------------------------------------------
def test_grid_wraps(ctx):
    """[3, 20, 20, 30] -> 700 x 53: 51 five-item pixels per block, two runs per row, 4200 units for the 2048 blocks of the
    largest grid, and 2.2 M output bytes for the 2048 x 256 lanes of the direct kernels: both grid-stride loops go round"""
    q = np.random.default_rng(7).integers(0, 256, (3, 20, 20, 30), dtype=np.uint8)
    assert 3 * 700 * -(-53 // (256 // 5)) > 2048 and q.shape[0] * q.shape[1] * 700 * 53 > 2048 * 256
    for mode in (rr.BILINEAR, rr.NEAREST):
        want = rr.resize_u8(q, 700, 53, mode, True, 100)
        got, names = _nhwc(ctx, q, 700, 53, mode, True, 100, ib=1, ob=1, out_s8=1)
        assert names == ["resize_u8_nhwc"] and _assert_same(got, want, (mode, "nhwc"))
    assert _assert_same(_nchw(ctx, q, 700, 53, rr.BILINEAR)[0], rr.resize_u8(q, 700, 53, rr.BILINEAR), "flat")
    q = np.random.default_rng(8).integers(0, 256, (3, 20, 90, 61), dtype=np.uint8)
    base = rr.adaptive_u8(q, 700, 53)
    got, names = _nhwc(ctx, q, 700, 53, POOL, True, 100, ib=1, ob=1, out_s8=1)
    assert names == ["adaptive_avgpool_u8_nhwc"] and _assert_same(got, np.maximum(base, 100), "pool nhwc")
    assert _assert_same(_nchw(ctx, q, 700, 53, POOL)[0], base, "pool flat")


def _f32(ctx, x, oh, ow, mode):
    n, c, h, w = x.shape
    di, do = ctx.put(x), ctx.guarded((n, c, oh, ow))
    try:
        if mode == POOL:
            abi.ck(abi.lib().i8ie_adaptive_avgpool2d_f32(ctx.h, di.ptr, do.ptr, n, c, h, w, oh, ow))
        else:
            abi.ck(abi.lib().i8ie_resize2d_f32(ctx.h, di.ptr, do.ptr, n, c, h, w, oh, ow, mode))
        got, ok = do.read()
    finally:
        di.free()
        do.free()
    assert ok
    return got


def _same_f32(got, want):
    """the same bits wherever the restatement has a number, and a NaN exactly where it has a NaN (a NaN's sign and payload
    are the machine's: the host's and the GPU's differ for one made from inf * 0)"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_fp32_bit_for_bit(ctx):
    """the FP32 sequences of include/i8ie_hip.h bit for bit, a NaN and an inf among the inputs"""
    rng, seen_nan = np.random.default_rng(11), 0
    for (h, w), (oh, ow) in SIZES + POOL_SIZES:
        x = (rng.standard_normal((2, 5, h, w)) * np.exp(rng.uniform(-3, 3, (2, 5, h, w)))).astype(f32)
        x[0, 0, 0, 0], x[1, 2, h - 1, w - 1] = np.nan, np.inf
        for mode in MODES:
            got = _f32(ctx, x, oh, ow, mode)
            want = rr.resize_f32(x, oh, ow, mode)
            seen_nan += int(np.isnan(want).any())
            assert got.dtype == f32 and _same_f32(got, want), (h, w, oh, ow, mode)
        assert _same_f32(_f32(ctx, x, oh, ow, POOL), rr.adaptive_f32(x, oh, ow)), (h, w, oh, ow)
    assert seen_nan >= 30  # (a downscale may pass the two special values by; most cases blend them in)
    x = rng.standard_normal((2, 3, 5, 4)).astype(f32)
    val = rr.bilinear_f64(x, 9, 7, rr.ALIGNED)  # (and close to the exact value: 16 * 2^-24 * max|x|, as the upsample's FP32 test)
    assert np.all(np.abs(_f32(ctx, x, 9, 7, rr.ALIGNED).astype(np.float64) - val) <= 16 * 2.0 ** -24 * np.abs(x).max())


# ---- 8. the Python surface ---------------------------------------------------------------------------------------------------
def test_surface_routing_by_kernel_name(i8ie):
    """(a tensor whose bytes were observed lies in the reference's order from then on, so every run below takes a fresh conv
    result, NHWC as the engine keeps it, and the expected bytes come from another one)"""
    q = support.activation(i8ie)  # [2, 16, 8, 8], recorded
    conv0 = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110))
    src = lambda: conv0(q)
    qv = src().numpy()

    def ran(fn):
        return {k for k, v in support.counted(lambda: [fn()]).items() if v}

    assert "upsample_bilinear_u8_nhwc" in ran(lambda: i8ie.interpolate(src(), size=(16, 24), mode="bilinear"))
    assert "upsample_nearest_u8_nhwc" in ran(lambda: i8ie.interpolate(src(), scale_factor=2))
    names = ran(lambda: i8ie.interpolate(i8ie.adaptive_avg_pool2d(src(), 3), size=(8, 8), mode="bilinear"))
    assert {"resize_u8_nhwc", "adaptive_avgpool_u8_nhwc"} <= names and not any(k.startswith("upsample") for k in names), names
    assert "resize_u8_nhwc" in ran(lambda: i8ie.interpolate(src(), scale_factor=2, mode="bilinear", align_corners=True))
    assert "resize_u8_nhwc" in ran(lambda: i8ie.interpolate(src(), size=(4, 5)))
    assert any(k.startswith("avgpool_u8_nhwc") for k in ran(lambda: i8ie.adaptive_avg_pool2d(src(), 4)))
    assert any(k.startswith("avgpool_u8_nhwc") for k in ran(lambda: i8ie.adaptive_avg_pool2d(src(), 1)))
    got = i8ie.interpolate(i8ie.adaptive_avg_pool2d(src(), 3), size=(8, 8), mode="bilinear")
    assert got.shape == (2, 16, 8, 8) and got.scale == pytest.approx(0.04) and got.zero_point == 110
    assert np.array_equal(got.numpy(), rr.resize_u8(rr.adaptive_u8(qv, 3, 3), 8, 8, rr.BILINEAR))
    assert np.array_equal(i8ie.interpolate(src(), size=(16, 24), mode="bilinear").numpy(), rr.resize_u8(qv, 16, 24, rr.BILINEAR))
    assert np.array_equal(i8ie.interpolate(src(), size=(4, 5)).numpy(), rr.resize_u8(qv, 4, 5, rr.NEAREST))
    assert np.array_equal(i8ie.adaptive_avg_pool2d(src(), 4).numpy(), rr.adaptive_u8(qv, 4, 4))
    assert np.array_equal(i8ie.adaptive_avg_pool2d(src(), 1).numpy(), rr.adaptive_u8(qv, 1, 1))


@pytest.mark.parametrize("op", ["interpolate", "adaptive_avg_pool2d"])
def test_three_launches(i8ie, op):
    """conv -> interpolate -> relu -> conv(3x3 pad 1) and conv -> adaptive_avg_pool2d -> conv: one launch each; the relu folds
    into the resize, whose kernel writes the border and the bytes the second conv asks for"""
    q = support.activation(i8ie)
    conv0, conv_c = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    if op == "interpolate":
        mid_of = lambda: i8ie.relu(i8ie.interpolate(conv0(q), size=(11, 13), mode="bilinear"))
        ref = lambda v: rr.resize_u8(v, 11, 13, rr.BILINEAR, True, 110)
    else:
        mid_of = lambda: i8ie.adaptive_avg_pool2d(conv0(q), (5, 3))
        ref = lambda v: rr.adaptive_u8(v, 5, 3)
    first, got, launches = support.counted_forward(lambda: conv_c(mid_of()))
    mid = mid_of()
    assert mid.scale == pytest.approx(0.04) and mid.zero_point == 110
    assert np.array_equal(mid.numpy(), ref(conv0(q).numpy()))
    assert np.array_equal(got, conv_c(mid).numpy()) and np.array_equal(first, got)
    own, others, _ = support.split_launches(launches, FAST[op == "interpolate"])
    assert own == 1 and others == 2, launches


def test_user_tensors_s8_and_graph_replay(i8ie):
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(12)
    x = rng.uniform(-3, 3, (2, 5, 6, 7)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)  # a user-made tensor: NCHW bytes, the flat entries
    qv = q.numpy()
    for size, mode, ac, code in [((9, 4), "bilinear", None, rr.BILINEAR), ((9, 4), "bilinear", True, rr.ALIGNED), ((4, 11), "nearest", None, rr.NEAREST)]:
        r = i8ie.interpolate(q, size=size, mode=mode, align_corners=ac)
        assert r.shape == (2, 5) + size and r.scale == pytest.approx(0.025) and r.zero_point == 127
        assert np.array_equal(r.numpy(), rr.resize_u8(qv, size[0], size[1], code))
        r = i8ie.relu(i8ie.interpolate(q, size=size, mode=mode, align_corners=ac))
        assert np.array_equal(r.numpy(), rr.resize_u8(qv, size[0], size[1], code, True, 127))
        t = i8ie.interpolate(i8ie.tensor(x), size=size, mode=mode, align_corners=ac)
        assert support.same_bits(t.numpy(), rr.resize_f32(x, size[0], size[1], code))
    assert np.array_equal(i8ie.relu(i8ie.adaptive_avg_pool2d(q, (4, None))).numpy(), rr.adaptive_u8(qv, 4, 7, True, 127))
    assert support.same_bits(i8ie.adaptive_avg_pool2d(i8ie.tensor(x), (4, 3)).numpy(), rr.adaptive_f32(x, 4, 3))
    s8 = i8ie.Tensor(cx.tensor_s8(np.zeros((1, 4, 2, 2), np.int8), 0.5, 0))
    for bad in (lambda: i8ie.interpolate(s8, size=3), lambda: i8ie.adaptive_avg_pool2d(s8, 1), lambda: cx._interpolate(s8.data, 3, 3, 1),
                lambda: cx._adaptive_avg_pool2d(s8.data, 3, 3)):
        with pytest.raises(RuntimeError, match="int8"):
            bad()

    conv0 = support.conv(i8ie, 5, 16, 3, 1, 1, (0.04, 110))

    def forward(t):
        y = conv0(i8ie.quantize(t, 0.025, 127))
        return i8ie.dequantize(i8ie.relu(i8ie.interpolate(i8ie.adaptive_avg_pool2d(y, 3), size=(6, 7), mode="bilinear", align_corners=True)))

    want = forward(i8ie.tensor(x)).numpy()
    cx.force_fallback(True)
    try:
        assert np.array_equal(forward(i8ie.tensor(x)).numpy(), want)
    finally:
        cx.force_fallback(False)
    g = GraphedForward(forward, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy(), want)


def test_pyramid_pooling_module_step_by_step(i8ie):
    """adaptive_avg_pool2d to 1 / 2 / 3 / 6 bins, a 1x1 conv each, bilinear back to 8 x 8, at 16 channels: every step against
    support.conv_ref + tests/resize_ref.py.  Bins 1 and 2 go back up through `upsample`, 3 and 6 through the new kernel."""
    s_in, zp_in, qp = 0.025, 127, (0.04, 110)
    stem, body = support.conv(i8ie, 3, 16, 3, 1, 1, qp), support.conv(i8ie, 16, 16, 3, 1, 5, qp)
    heads = {b: support.conv(i8ie, 16, 16, 1, 0, 10 + b, (0.03, 100 + b)) for b in (1, 2, 3, 6)}
    x = np.random.default_rng(21).uniform(-3, 3, (2, 3, 8, 8)).astype(f32)

    def forward():
        f = i8ie.relu(body(i8ie.relu(stem(i8ie.quantize(i8ie.tensor(x), s_in, zp_in)))))
        return [f] + [i8ie.interpolate(i8ie.relu(heads[b](i8ie.adaptive_avg_pool2d(f, b))), size=(8, 8), mode="bilinear") for b in (1, 2, 3, 6)]

    outs = forward()
    vals = [o.numpy() for o in outs[1:]]  # (before the feature map itself: observing a tensor puts it into the reference's order)
    qx = i8ie.quantize(i8ie.tensor(x), s_in, zp_in).numpy()
    fv = np.maximum(support.conv_ref(body, np.maximum(support.conv_ref(stem, qx, s_in, zp_in, pad=1), 110), 0.04, 110, pad=1), 110)
    assert np.array_equal(outs[0].numpy(), fv)
    for b, got, val in zip((1, 2, 3, 6), outs[1:], vals):
        pooled = rr.adaptive_u8(fv, b, b)
        hv = np.maximum(support.conv_ref(heads[b], pooled, 0.04, 110), 100 + b)
        assert got.shape == (2, 16, 8, 8) and got.zero_point == 100 + b
        assert _assert_same(val, rr.resize_u8(hv, 8, 8, rr.BILINEAR), ("bin", b))
    launches = support.counted(forward)
    print(launches)
    assert launches.get("resize_u8_nhwc", 0) == 2 and launches.get("upsample_bilinear_u8_nhwc", 0) == 2, launches
    assert launches.get("adaptive_avgpool_u8_nhwc", 0) == 2, launches  # bins 3 and 6 (1 is the global pool, 2 is avg_pool2d(4))
    assert not any(k.endswith("_direct") for k in launches), launches


def test_pspnet_example_runs(i8ie):
    """examples/pspnet_cifar10.py's network at 2 images: FP32, prepare / convert, INT8; per-pixel argmax [2, 32, 32]; bins 3 and
    6 and the aligned head resize run the new kernels, bins 1 and 2 the upsample kernel"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("pspnet_cifar10", os.path.join(abi.ROOT, "examples", "pspnet_cifar10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.make_model(i8ie)
    model.load(mod.synthetic_state_dict(model))
    x = i8ie.tensor(np.random.default_rng(1234).standard_normal((2, 3, 32, 32)).astype(f32))
    fp = model(x).numpy()
    assert fp.shape == (2, 10, 32, 32) and np.isfinite(fp).all()
    model.prepare()
    model(x)
    model.convert()
    out = model(x).numpy()
    assert out.shape == (2, 10, 32, 32) and i8ie.argmax(model(x), axis=1).numpy().shape == (2, 32, 32)
    assert np.isfinite(out).all()
    launches = support.counted(lambda: [model(x)])
    print(launches)
    count = lambda prefix: sum(v for k, v in launches.items() if k.startswith(prefix))
    assert count("resize_u8") == 3 and count("adaptive_avgpool_u8") == 2 and count("upsample_bilinear_u8") == 2, launches
