"""Quantized average pooling on the GPU (csrc/i8ie_avgpool.hip).  Every comparison is against the
numpy restatement of the definition (tests/avgpool_ref.py) or the closed form (j + n // 2) // n, never against the code
under test: every reachable window sum through both u8 entries and both NHWC regimes, the bordered / re-biased layout
matrix with sentinel borders, the FP32 entry against the float64 mean, the Python surface with launch counts, and the two
pooled residual networks end to end.

Every sum, the one departure from "every j in 0 ... 255 n": the 255 x 257 window has n = 65 535 and 16.7 million reachable
sums, each of which needs its own 65 535-byte window -- a terabyte of input.  For that window alone the sums are a subset
chosen by reasoning about where a division can go wrong: the three sums around every one of the 255 rounding boundaries
(j = q n + (n - n // 2) + {-1, 0, 1}: there S + n // 2 is a multiple of n or next to one), both ends, and 200 seeded random
ones.  All other windows run every j."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import add_ref as ar
import avgpool_ref as apr
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32

# the regime rule of csrc/i8ie_avgpool.hip: the reduce kernel when n >= 16 and there are fewer than 65536 lane items
# (or 255 n >= 65536), the windowed kernel otherwise
REDUCE_MIN_WINDOW, REDUCE_MAX_ITEMS, PACKED_MAX = 16, 65536, 257


ctx = support.ctx_fixture(apr)


# ---- 1. every sum ------------------------------------------------------------------------------------------------------
def _sum_windows(js, n, rng):
    """[len(js), n] u8: row i sums to js[i] exactly -- js[i] // n everywhere, +1 on js[i] % n elements at shuffled
    positions (one seeded permutation of the n positions, rotated by a random amount per row)"""
    js = np.asarray(js, np.int64)
    assert js.min() >= 0 and js.max() <= 255 * n
    rank = rng.permutation(n).astype(np.int32)[None, :]
    out = np.empty((js.size, n), np.uint8)
    step = max(1, (1 << 22) // n)  # a few MB of temporaries at a time
    for a in range(0, js.size, step):
        j = js[a:a + step]
        t = rank + rng.integers(0, n, (j.size, 1), dtype=np.int32)
        t -= n * (t >= n)
        out[a:a + step] = (j // n).astype(np.uint8)[:, None] + (t < (j % n).astype(np.int32)[:, None])
    return out


def _every_sum_case(kh, kw, c, min_outputs, rng):
    """logical NHWC input [ni, h, w, c] whose outputs, in NHWC order, have the window sums js (every j in 0 ... 255 n,
    repeated from the start to fill whole images and at least min_outputs).  Two by two windows per image with stride
    max(kh, kw) (the bytes between windows are random), or one window per image (a global pool) for the 255 x 257 window."""
    n = kh * kw
    if n > 65025:
        per_img, s, h, w = 1, 1, kh, kw
        bound = np.arange(255, dtype=np.int64) * n + (n - n // 2)
        js = np.unique(np.concatenate([bound - 1, bound, bound + 1, [0, 1, 255 * n - 1, 255 * n], rng.integers(0, 255 * n + 1, 200)]))
    else:
        s = max(kh, kw)
        per_img, h, w = 4, kh + s, kw + s
        js = np.arange(255 * n + 1, dtype=np.int64)
    unit = per_img * c
    total = max(js.size, min_outputs)
    total = (total + unit - 1) // unit * unit
    js = np.resize(js, total)
    ni = total // unit
    vals = _sum_windows(js, n, rng)
    if per_img == 1:
        x = np.ascontiguousarray(vals.reshape(ni, c, kh, kw).transpose(0, 2, 3, 1))
    else:
        x = rng.integers(0, 256, (ni, h, w, c), dtype=np.uint8)
        v = vals.reshape(ni, 2, 2, c, kh, kw)
        for oy in range(2):
            for ox in range(2):
                x[:, oy * s:oy * s + kh, ox * s:ox * s + kw, :] = v[:, oy, ox].transpose(0, 2, 3, 1)
    want = ((js + n // 2) // n).astype(np.uint8).reshape(ni, 2 if per_img == 4 else 1, 2 if per_img == 4 else 1, c)
    return x, want, s


def _run_nhwc(ctx, dx, do, shape, kh, kw, s, relu, zp, in_border=0, in_s8=0, out_border=0, out_s8=0):
    ni, h, w, c = shape
    abi.ck(abi.lib().i8ie_avgpool2d_u8_nhwc(ctx.h, dx, in_border, in_s8, do, out_border, out_s8, ni, c, h, w, kh, kw, s,
                                            1 if relu else 0, zp))


WINDOWS = [(1, 1), (2, 2), (3, 3), (4, 4), (3, 4), (7, 7), (8, 8), (13, 13), (16, 16), (255, 257)]
RELUS = [(False, 0), (True, 0), (True, 128), (True, 255)]


def _check_every_sum(ctx, x, want, kh, kw, s, regime, nchw):
    ni, h, w, c = x.shape
    dx, do = ctx.put(x), ctx.put(np.full(want.shape, 0xEE, np.uint8))
    try:
        for relu, zp in RELUS:
            names = sorted(ctx.kernels_run(lambda: _run_nhwc(ctx, dx.ptr, do.ptr, x.shape, kh, kw, s, relu, zp))[1])
            assert names == [regime], (names, regime)
            got = do.get()
            exp = np.maximum(want, zp) if relu else want
            bad = np.flatnonzero(got.ravel() != exp.ravel())
            print("window %dx%d c=%d %s relu=%s zp=%d: %d outputs, %d wrong" % (kh, kw, c, regime, relu, zp, exp.size, bad.size))
            assert bad.size == 0, (kh, kw, c, regime, relu, zp, bad[:8], got.ravel()[bad[:8]], exp.ravel()[bad[:8]])
    finally:
        dx.free()
        do.free()
    if nchw:
        dx, do = ctx.put(x.transpose(0, 3, 1, 2)), ctx.put(np.full(want.size, 0xEE, np.uint8))
        try:
            abi.ck(abi.lib().i8ie_avgpool2d_u8(ctx.h, dx.ptr, do.ptr, ni, c, h, w, kh, kw, s))
            got = do.get().reshape(ni, c, want.shape[1], want.shape[2])
        finally:
            dx.free()
            do.free()
        assert np.array_equal(got, want.transpose(0, 3, 1, 2)), (kh, kw, "nchw")


@pytest.mark.parametrize("kh,kw", WINDOWS, ids=["%dx%d" % k for k in WINDOWS])
def test_every_sum(ctx, kh, kw):
    """Output j has window sum exactly j, for every reachable j (module docstring for 255 x 257): both u8 entries must give
    (j + n // 2) // n, the NHWC one with and without ReLU at zp 0 / 128 / 255 -- in each regime that accepts the window, in
    16-channel items (packed sums, dwordx4) and, for the windowed kernel at n >= 16, 4-channel items (the same packed sums),
    whose shapes are the smallest that the rule sends there."""
    n = kh * kw
    rng = np.random.default_rng(1000 * kh + kw)
    x, want, s = _every_sum_case(kh, kw, 16, 0, rng)
    items = want.size // 16
    assert items < REDUCE_MAX_ITEMS
    small_regime = "avgpool_u8_nhwc_reduce" if n >= REDUCE_MIN_WINDOW else "avgpool_u8_nhwc"
    _check_every_sum(ctx, x, want, kh, kw, s, small_regime, nchw=True)
    if REDUCE_MIN_WINDOW <= n <= PACKED_MAX:  # the windowed kernel takes it from 65536 items on
        x, want, s = _every_sum_case(kh, kw, 4, 4 * REDUCE_MAX_ITEMS, rng)
        _check_every_sum(ctx, x, want, kh, kw, s, "avgpool_u8_nhwc", nchw=False)
    if n <= PACKED_MAX:  # byte items too (c % 4 != 0), in the regime the small shape gets
        x, want, s = _every_sum_case(kh, kw, 3, 0, rng)
        _check_every_sum(ctx, x, want, kh, kw, s, small_regime, nchw=False)


# ---- 2. the layout matrix ----------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = 0xC7


def _guarded_phys(x_nhwc, border, s8):
    """[n, h, w, c] u8 -> guarded flat buffer holding [n, h+2b, w+2b, c] with SENTINEL in the border (interior re-biased if s8)"""
    n, h, w, c = x_nhwc.shape
    p = np.full((n, h + 2 * border, w + 2 * border, c), SENTINEL, np.uint8)
    p[:, border:border + h, border:border + w, :] = x_nhwc ^ np.uint8(0x80 if s8 else 0)
    return np.concatenate([np.full(GUARD, 0x5A, np.uint8), p.ravel(), np.full(GUARD, 0x5A, np.uint8)]), p.shape


@pytest.mark.parametrize("c", [3, 20, 16, 48])
def test_layout_matrix(ctx, c):
    n, h, w = 3, 9, 11
    rng = np.random.default_rng(c)
    x = rng.integers(0, 256, (n, c, h, w), dtype=np.uint8)
    x[0, :, :3, :3] = 255
    x[1, :, :4, :4] = 0
    x_nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    i = 0
    for (kh, kw, s) in [(2, 2, 2), (3, 3, 2), (3, 3, 1), (h, w, 1)]:
        for ib, ob in itertools.product((0, 1, 2), repeat=2):
            for in_s8, out_s8 in itertools.product((0, 1), repeat=2):
                i += 1
                relu, zp = bool(i % 2), 100 + (i % 7) * 10
                want = apr.avg_pool2d_u8(x, kh, kw, s, relu, zp).transpose(0, 2, 3, 1)
                oh, ow = want.shape[1:3]
                fi, _ = _guarded_phys(x_nhwc, ib, in_s8)
                fo, oshape = _guarded_phys(np.full(want.shape, 0xEE, np.uint8), ob, 0)
                di, do = ctx.put(fi), ctx.put(fo)
                try:
                    _run_nhwc(ctx, C.c_void_p(di.ptr.value + GUARD), C.c_void_p(do.ptr.value + GUARD), (n, h, w, c), kh, kw, s, relu, zp,
                              ib, in_s8, ob, out_s8)
                    gi, go = di.get(), do.get()
                finally:
                    di.free()
                    do.free()
                tag = (c, kh, kw, s, ib, ob, in_s8, out_s8, relu, zp)
                assert np.array_equal(gi, fi), ("the input (and its guards) must be untouched", tag)
                assert (go[:GUARD] == 0x5A).all() and (go[-GUARD:] == 0x5A).all(), ("guard bytes around the result", tag)
                out = go[GUARD:-GUARD].reshape(oshape)
                inner = out[:, ob:ob + oh, ob:ob + ow, :] ^ np.uint8(0x80 if out_s8 else 0)
                assert np.array_equal(inner, want), tag
                ring = out.copy()
                ring[:, ob:ob + oh, ob:ob + ow, :] = SENTINEL
                assert (ring == SENTINEL).all(), ("a border byte of the result was written", tag)
    # the NCHW entry on the same data
    for (kh, kw, s) in [(2, 2, 2), (3, 3, 2), (3, 4, 1), (h, w, 1)]:
        want = apr.avg_pool2d_u8(x, kh, kw, s)
        di, do = ctx.put(x), ctx.put(np.full(want.shape, 0xEE, np.uint8))
        try:
            abi.ck(abi.lib().i8ie_avgpool2d_u8(ctx.h, di.ptr, do.ptr, n, c, h, w, kh, kw, s))
            assert np.array_equal(do.get(), want), (c, kh, kw, s)
        finally:
            di.free()
            do.free()


# ---- 3. FP32 -----------------------------------------------------------------------------------------------------------
def _avg_f32(ctx, x, kh, kw, s):
    n, c, h, w = x.shape
    oh, ow = apr.out_hw(h, w, kh, kw, s)
    di, do = ctx.put(x), ctx.guarded((n, c, oh, ow))
    try:
        abi.ck(abi.lib().i8ie_avgpool2d_f32(ctx.h, di.ptr, do.ptr, n, c, h, w, kh, kw, s))
        got, ok = do.read()
    finally:
        di.free()
        do.free()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    return got


FP32_WINDOWS = [(2, 2, 2), (3, 3, 2), (3, 4, 1), (7, 7, 1), (9, 11, 1)]


@pytest.mark.parametrize("kh,kw,s", FP32_WINDOWS)
def test_fp32_against_float64_mean(ctx, kh, kw, s):
    """|got - mean64| <= gamma(n + 1) * mean|x|: n - 1 roundings of the running sum and one of the division, each
    relative to a partial result no larger than sum|x| (f64_ref.gamma; Higham section 3.1, 4.2).  Ordinary values of mixed
    sign and magnitude with one element in ten replaced by a denormal."""
    rng = np.random.default_rng(kh * 10 + kw)
    x = (rng.standard_normal((2, 5, 9, 11)) * np.exp(rng.uniform(-3, 3, (2, 5, 9, 11)))).astype(f32)
    den = rng.random(x.shape) < 0.1
    x[den] = (rng.integers(1, 1 << 22, int(den.sum())).astype(np.uint32)).view(f32) * rng.choice([f32(-1), f32(1)], int(den.sum()))
    assert (np.abs(x[den]) < 2.0 ** -126).all() and (x[den] != 0).all()
    got = _avg_f32(ctx, x, kh, kw, s)
    mean, mag = apr.avg_pool2d_f64(x, kh, kw, s)
    err, bound = np.abs(got.astype(np.float64) - mean), f64_ref.gamma(kh * kw + 1) * mag
    print("fp32 %dx%d/%d: worst err / bound = %.3g" % (kh, kw, s, float((err / bound).max())))
    assert got.dtype == f32 and np.all(err <= bound), float((err / bound).max())


def test_fp32_special_values_by_class(ctx):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 6, 4, 4)).astype(f32)
    inf, nan = f32(np.inf), f32(np.nan)
    x[0, 0, 1, 1] = nan
    x[0, 1, 0, 0] = inf
    x[0, 2, 3, 3] = -inf
    x[0, 3, 0, 1], x[0, 3, 2, 2] = inf, -inf  # inf - inf inside a 4 x 4 window; apart in 2 x 2 windows
    x[0, 4, 0, 0], x[0, 4, 0, 1] = inf, nan
    for kh, kw, s in [(2, 2, 2), (4, 4, 1)]:
        got = _avg_f32(ctx, x, kh, kw, s)
        with np.errstate(all="ignore"):
            mean, _ = apr.avg_pool2d_f64(x, kh, kw, s)
        for cls in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(cls(got), cls(mean)), (kh, kw, cls.__name__)
        fin = np.isfinite(mean)
        assert fin.any() and np.allclose(got[fin], mean[fin], rtol=1e-5, atol=1e-6)


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------
def test_relu_avg_pool_conv_launch_counts(i8ie):
    """relu(avg_pool2d(conv(x))): one conv launch and ONE pool launch with the relu folded in; nothing converts."""
    q = support.activation(i8ie)
    conv = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110))
    first, got, launches = support.counted_forward(lambda: i8ie.relu(i8ie.avg_pool2d(conv(q), 2)))
    want = apr.avg_pool2d_u8(conv(q).numpy(), 2, 2, 2, True, 110)
    assert got.shape == (2, 16, 4, 4) and np.array_equal(got, want) and np.array_equal(first, want)
    pools = sum(v for k, v in launches.items() if k.startswith("avgpool_u8_nhwc"))
    assert pools == 1, launches
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_", "avgpool_u8_nchw")), launches
    # a conv behind the pool gets its zero-point border (and what it reads) from the pool kernel
    conv2 = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    first, got, launches = support.counted_forward(lambda: conv2(i8ie.relu(i8ie.avg_pool2d(conv(q), 3, 1))))
    pooled = i8ie.relu(i8ie.avg_pool2d(conv(q), 3, 1))
    assert np.array_equal(pooled.numpy(), apr.avg_pool2d_u8(conv(q).numpy(), 3, 3, 1, True, 110))
    assert np.array_equal(got, conv2(pooled).numpy()) and np.array_equal(first, got)  # (pooled: observed, NCHW, border-free)
    assert sum(v for k, v in launches.items() if k.startswith("avgpool_u8_nhwc")) == 1, launches
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "reborder", "layout_")), launches
    # (asked last: observing q launches it once more without a border, and a conv would then re-border it on every call)
    assert q.data.layout() == 1  # NHWC


def test_head_launch_counts(i8ie):
    """fc(global_avg_pool2d(relu(add(a, b))).reshape(-1, c)): two convs, one add (relu folded), one pool, one Linear -- and
    no layout conversion in front of the Linear: [n, c, 1, 1] is the same bytes in both orders."""
    q = support.activation(i8ie)
    conv_a, conv_b = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120)), support.conv(i8ie, 16, 16, 3, 1, 3, (0.06, 130))
    add = i8ie.Add()
    add.set_output_qparams(0.07, 100)
    add.convert()
    rng = np.random.default_rng(6)
    fc = i8ie.Linear(16, 10)
    fc.load_weight(rng.uniform(-0.5, 0.5, (10, 16)).astype(f32))
    fc.load_bias(rng.uniform(-0.1, 0.1, 10).astype(f32))
    fc.set_output_qparams(0.1, 128)
    fc.convert()

    def head():
        return fc(i8ie.global_avg_pool2d(i8ie.relu(add(conv_a(q), conv_b(q)))).reshape(-1, 16))

    first, got, launches = support.counted_forward(head)
    summed = ar.add_u8(conv_a(q).numpy(), 120, f32(0.05), conv_b(q).numpy(), 130, f32(0.06), f32(0.07), 100, True)
    pooled = i8ie.global_avg_pool2d(i8ie.relu(add(conv_a(q), conv_b(q))))
    assert pooled.shape == (2, 16, 1, 1) and pooled.scale == pytest.approx(0.07) and pooled.zero_point == 100
    assert np.array_equal(pooled.numpy(), apr.global_avg_pool2d_u8(summed))
    want = fc(pooled.reshape(-1, 16)).numpy()  # the same Linear on the observed (NCHW) bytes
    assert got.shape == (2, 10) and np.array_equal(got, want) and np.array_equal(first, want)
    assert sum(v for k, v in launches.items() if k.startswith("avgpool_u8_nhwc")) == 1, launches
    assert sum(v for k, v in launches.items() if k.startswith("add_u8")) == 1, launches
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), launches


def test_surface_user_tensor_qparams_and_errors(i8ie):
    rng = np.random.default_rng(12)
    x = rng.uniform(-3, 3, (2, 5, 9, 11)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)  # a user-made tensor: NCHW bytes
    qv = q.numpy()
    for k, s in [(2, None), (3, 2), (3, 1), (9, 1)]:
        r = i8ie.avg_pool2d(q, k, s) if s is not None else i8ie.avg_pool2d(q, k)
        st = k if s is None else s
        assert r.scale == pytest.approx(0.025) and r.zero_point == 127
        assert np.array_equal(r.numpy(), apr.avg_pool2d_u8(qv, k, k, st)), (k, s)
        r = i8ie.relu(i8ie.avg_pool2d(q, k, st))
        assert np.array_equal(r.numpy(), apr.avg_pool2d_u8(qv, k, k, st, True, 127)), (k, s)
    g = i8ie.global_avg_pool2d(q)
    assert g.shape == (2, 5, 1, 1) and g.scale == pytest.approx(0.025) and g.zero_point == 127
    assert np.array_equal(g.numpy(), apr.global_avg_pool2d_u8(qv))
    assert np.array_equal(g.reshape(-1, 5).numpy(), apr.global_avg_pool2d_u8(qv).reshape(2, 5))
    # FP32, before convert()
    t = i8ie.tensor(x)
    mean, mag = apr.avg_pool2d_f64(x, 3, 3, 2)
    assert np.all(np.abs(i8ie.avg_pool2d(t, 3, 2).numpy() - mean) <= f64_ref.gamma(10) * mag)
    mean, mag = apr.avg_pool2d_f64(x, 9, 11, 1)
    gf = i8ie.global_avg_pool2d(t).numpy()
    assert gf.shape == (2, 5, 1, 1) and np.all(np.abs(gf - mean) <= f64_ref.gamma(100) * mag)
    for bad in (lambda: i8ie.avg_pool2d(q.reshape(2, -1), 2), lambda: i8ie.global_avg_pool2d(t.reshape(10, 9, 11)),
                lambda: i8ie.avg_pool2d(q, 0), lambda: i8ie.avg_pool2d(q, 2, 0), lambda: i8ie.avg_pool2d(t, -1, 1),
                lambda: i8ie.avg_pool2d(q, 10), lambda: i8ie.avg_pool2d(t, 10, 1)):
        with pytest.raises(RuntimeError):
            bad()


# ---- 5. the networks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("name,batch", [("resnet_tiny_gap", 2), ("resnet_tiny_gap", 66), ("resnet18_cifar", 2), ("resnet18_cifar", 9)])
def test_networks_bit_exact(i8ie, name, batch, per_channel, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, aqp = nc.calibrated(name, per_channel, calib_images=16)
    assert sorted(aqp) == sorted(wl.add_names(name)) and all(s > 0 and s != 1.0 for s, _ in aqp.values()), aqp  # the Adds were calibrated
    x = wl.synthetic_input(name, batch, seed=5)
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, aqp, per_channel)
    assert want.shape == (batch, 10)
    both = (name, batch) == ("resnet_tiny_gap", 2)
    nc.check_bit_exact(i8ie, net, name, x, want, fallback=True, graph=both, reload_dir=tmp_path if both else None, expect_jqp=aqp)


# ---- 6. FP32 resnet_tiny_gap before convert() --------------------------------------------------------------------------
def test_fp32_resnet_tiny_gap_layer_by_layer(i8ie):
    """Walk the spec by hand with the FP32 ops, every op fed the product's own previous output: conv / fc inside
    f64_ref.dot_bound of the float64 result (the bounds of test_gpu_fp32.py; a grouped conv against grouped_ref's float64
    form), the pools inside gamma(n + 1) * mean|x|, relu / add / flatten bit-identical; then net(x) in one call equals the
    walked result bit for bit."""
    from int8inferenceengine_amd import workloads as wl

    name = "resnet_tiny_gap"
    layers, spec, _ = wl.NETWORKS[name]
    sd = wl.synthetic_state_dict(name)
    net = wl.build(name)
    net.load(sd)
    x = wl.synthetic_input(name, 3, seed=5)

    def walk(ops, t, saved):
        for op in ops:
            prev = t.numpy()
            if op[0] == "layer":
                L, w, b = layers[op[1]], sd[op[1] + ".weight"], sd[op[1] + ".bias"]
                t = getattr(net, op[1])(t)
                got = t.numpy()
                if L[0] == "conv":
                    g = gr.layer_groups(L)
                    want, mag = gr.conv2d_f64(prev, w, b, g, L[4], L[5]), gr.conv2d_f64_mag(prev, w, b, g, L[4], L[5])
                    K = (L[1] // g) * L[3] * L[3]
                else:
                    want, mag, K = f64_ref.linear(prev, w, b), f64_ref.linear_mag(prev, w, b), L[1]
                err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, K)
                assert got.dtype == f32 and got.shape == want.shape and np.all(err <= bound), (op, float(np.nanmax(err / bound)))
            elif op[0] == "relu":
                t = i8ie.relu(t)
                assert support.bits_equal(t.numpy(), f64_ref.relu(prev)), op
            elif op[0] in ("avgpool", "gap"):
                kh, kw, s = (op[1], op[1], op[2]) if op[0] == "avgpool" else (prev.shape[2], prev.shape[3], 1)
                t = i8ie.avg_pool2d(t, op[1], op[2]) if op[0] == "avgpool" else i8ie.global_avg_pool2d(t)
                mean, mag = apr.avg_pool2d_f64(prev, kh, kw, s)
                got = t.numpy()
                assert got.shape == mean.shape and np.all(np.abs(got - mean) <= f64_ref.gamma(kh * kw + 1) * mag), op
            elif op[0] == "save":
                saved[op[1]] = t
            elif op[0] == "branch":
                saved[op[1]] = walk(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                other = saved[op[2]].numpy()
                t = getattr(net, op[1])(t, saved[op[2]])
                assert support.bits_equal(t.numpy(), (prev + other).astype(f32)), op
            else:
                t = t.reshape(-1, op[1])
                assert support.bits_equal(t.numpy(), prev.reshape(-1, op[1])), op
        return t

    walked = walk(spec, i8ie.tensor(x), {}).numpy()
    assert walked.shape == (3, 10)
    assert support.bits_equal(net(i8ie.tensor(x)).numpy(), walked)
