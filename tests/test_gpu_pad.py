"""pad / crop on the GPU (csrc/i8ie_pad.hip).  The op is a copy, so every comparison is bit for bit,
over every byte of the physical output with the guard bytes around it, against the numpy restatement of tests/pad_ref.py --
never against the code under test.  The case lists live in pad_ref.py (tests/test_pad_host.py keeps every class of case in
them)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import add_ref
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import pad_ref as pr
import pointwise_util as pu
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = 0xC7  # the input's border: a byte that is in no input below
KERNELS = (pr.FAST, pr.DIRECT)

ctx = support.ctx_fixture(pr)


def _bytes(shape, seed=0):
    return pr.channel_bytes(shape, seed, avoid=POISON)


def _same(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, "%d of %d differ" % (len(bad), want.size),
                           [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])


def _nhwc(ctx, q, mode, amounts, fill=0, relu=False, zp=0, ib=0, ob=0, in_s8=0, out_s8=0, skew=0, fallback=False):
    """q NCHW logical -> (the NHWC entry's result, NCHW logical again; the kernel that ran).  The input's border holds POISON;
    the result's border holds zp (re-biased where asked) and, like the guard bytes around both buffers, must come back
    untouched (pointwise_util.interior asserts it); the interior starts as 0xEE."""
    n, c, h, w = q.shape
    _, _, oh, ow = pr.output_shape(mode, *amounts, n, c, h, w)
    fi, _ = pu.phys(np.ascontiguousarray(q.transpose(0, 2, 3, 1)), ib, POISON, in_s8, skew)
    fo, oshape = pu.phys(np.full((n, oh, ow, c), 0xEE, np.uint8), ob, zp, out_s8, skew)
    di, do = ctx.put(fi), ctx.put(fo)
    ctx.set_force_fallback(fallback)
    try:
        _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_pad2d_u8_nhwc(
            ctx.h, C.c_void_p(di.ptr.value + pu.GUARD + skew), ib, in_s8, C.c_void_p(do.ptr.value + pu.GUARD + skew), ob, out_s8,
            n, c, h, w, mode, *amounts, fill, 1 if relu else 0, zp)))
        gi, go = di.get(), do.get()
    finally:
        ctx.set_force_fallback(False)
        di.free()
        do.free()
    assert np.array_equal(gi, fi), "the input (and its guards) must be untouched"
    assert len(names) == 1 and names[0] in KERNELS, names
    return np.ascontiguousarray(pu.interior(go, oshape, ob, zp, out_s8, skew).transpose(0, 3, 1, 2)), names[0]


def _check(ctx, q, mode, amounts, **kw):
    """one case: the bytes, pad_u8_nhwc ran, no border byte of the input came through, and the same bytes from pad_u8_direct
    under force-fallback"""
    want = pr.apply(q, mode, *amounts, kw.get("fill", 0), kw.get("relu", False), kw.get("zp", 0))
    tag = (pr.MODE_NAME[mode], q.shape, amounts, kw)
    got, name = _nhwc(ctx, q, mode, amounts, **kw)
    _same(got, want, tag)
    assert name == pr.FAST, tag
    assert POISON not in got, tag   # (no input, fill byte or zero point below is the poison byte)
    got, name = _nhwc(ctx, q, mode, amounts, fallback=True, **kw)
    assert name == pr.DIRECT, tag
    _same(got, want, ("fallback",) + tag)
    return want


RELU_ZP = [(False, 0)] + [(True, zp) for zp in pr.ZPS]


# ---- 1. the geometry cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pr.CHANNELS)
def test_geometry_cases(ctx, c):
    for (h, w, amounts, modes), (relu, zp) in itertools.product(pr.GEOMETRY_CASES, RELU_ZP):
        q = _bytes((pr.BATCH, c, h, w), c + h)
        for mode in modes:
            for fill in (pr.FILLS if mode == pr.CONSTANT else (0,)):
                _check(ctx, q, mode, amounts, fill=fill, relu=relu, zp=zp, ib=1)


def test_random_bytes(ctx):
    """every byte value (the poison byte excepted) through every mode"""
    q = np.random.default_rng(5).integers(0, 256, (3, 20, 5, 7), dtype=np.uint8)
    q[q == POISON] = 0
    for mode in pr.MODES:
        _check(ctx, q, mode, (2, 1, 3, 0), fill=33, relu=True, zp=127, ib=1, ob=1, out_s8=1)


# ---- 2. the seam between the inner and the edge waves ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,p", pr.SEAM_CASES, ids=["%d_%d" % t for t in pr.SEAM_CASES])
def test_inner_and_edge_waves(ctx, c, p):
    h, w = pr.SEAM_MAP
    q = _bytes((pr.BATCH, c, h, w), c + p)
    for mode in pr.MODES:
        want = _check(ctx, q, mode, (p, p, p, p), fill=9, ib=2, ob=1, in_s8=1, out_s8=1)
        got, _ = _nhwc(ctx, q, mode, (p, p, p, p), fill=9, ib=2, ob=1, in_s8=1, out_s8=1)
        assert POISON not in got
        # both sides of every seam, against the input itself: the first / last interior line, and the line next to it
        assert np.array_equal(got[:, :, p, p:p + w], q[:, :, 0]) and np.array_equal(got[:, :, p + h - 1, p:p + w], q[:, :, h - 1])
        assert np.array_equal(got[:, :, p:p + h, p], q[:, :, :, 0]) and np.array_equal(got[:, :, p:p + h, p + w - 1], q[:, :, :, w - 1])
        outside = {pr.CONSTANT: None, pr.REFLECT: (1, h - 2, 1, w - 2), pr.REPLICATE: (0, h - 1, 0, w - 1), pr.CIRCULAR: (h - 1, 0, w - 1, 0)}[mode]
        if outside is None:
            assert (got[:, :, p - 1] == 9).all() and (got[:, :, p + h] == 9).all() and (got[:, :, :, p - 1] == 9).all() and (got[:, :, :, p + w] == 9).all()
        else:
            top, bottom, left, right = outside
            assert np.array_equal(got[:, :, p - 1, p:p + w], q[:, :, top]) and np.array_equal(got[:, :, p + h, p:p + w], q[:, :, bottom])
            assert np.array_equal(got[:, :, p:p + h, p - 1], q[:, :, :, left]) and np.array_equal(got[:, :, p:p + h, p + w], q[:, :, :, right])
        assert np.array_equal(got, want)


# ---- 3. the layout matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pr.MODES, ids=[pr.MODE_NAME[m] for m in pr.MODES])
def test_layout_matrix(ctx, mode):
    c, h, w, amounts = pr.LAYOUT_CASE
    q = _bytes((pr.BATCH, c, h, w), c)
    for ib, in_s8, ob, out_s8, skew in itertools.product(pr.IN_BORDERS, (0, 1), pr.OUT_BORDERS, (0, 1), pr.SKEWS):
        relu, zp = ((ib + ob + skew) % 2 == 1), 127
        _check(ctx, q, mode, amounts, fill=200 if relu else 5, relu=relu, zp=zp, ib=ib, ob=ob, in_s8=in_s8, out_s8=out_s8, skew=skew)


# ---- 4. grids that wrap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.WRAP_CASES, ids=["c%d" % t[1] for t in pr.WRAP_CASES])
def test_many_blocks(ctx, case):
    """more items than the 2048 x 256 lanes of the largest grid, so the grid-stride loop goes round and the digits carry; the
    bytes of a counter pattern"""
    n, c, h, w, amounts, mode = case
    assert pr.items(n, c, *pr.output_shape(mode, *amounts, n, c, h, w)[2:]) > pr.MAX_LANES
    count = np.arange(n * c * h * w, dtype=np.uint64)
    q = ((count * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8).reshape(n, c, h, w)
    q[q == POISON] = 1
    want = pr.apply(q, mode, *amounts, 0, True, 100)
    got, name = _nhwc(ctx, q, mode, amounts, 0, True, 100, ib=1, ob=1, out_s8=1)
    assert name == pr.FAST
    _same(got, want, case)


# ---- 5. the flat NCHW entry and the FP32 entry -----------------------------------------------------------------------------------
ENTRY_CASES = [(pr.CONSTANT, (2, 3, 5, 7), (2, 1, 3, 0)), (pr.REFLECT, (2, 3, 5, 7), (2, 1, 3, 0)), (pr.REPLICATE, (2, 20, 1, 5), (3, 3, 3, 3)),
               (pr.CIRCULAR, (2, 16, 3, 4), (4, 4, 3, 3)), (pr.CONSTANT, (2, 5, 5, 7), (-1, 2, 1, -2)), (pr.CONSTANT, (3, 4, 4, 5), (-4, 0, -3, 0))]


def test_nchw_and_fp32_entries(ctx):
    rng = np.random.default_rng(9)
    nan_payload = np.array([0x7FC12345, 0xFFC00001], np.uint32).view(f32)
    for mode, shape, amounts in ENTRY_CASES:
        oshape = pr.output_shape(mode, *amounts, *shape)
        q = _bytes(shape, amounts[0] + 7)
        di, do = ctx.put(q), abi.GuardedU8(ctx, oshape, fill=0xEE)
        x = (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(f32)
        x.flat[1], x.flat[2], x.flat[-1] = np.inf, -0.0, -0.0
        x.view(np.uint32).flat[0], x.view(np.uint32).flat[3] = nan_payload.view(np.uint32)
        dx = ctx.put(x)
        try:
            _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_pad2d_u8(ctx.h, di.ptr, do.ptr, *shape, mode, *amounts, 77)))
            assert names == [pr.DIRECT]
            _same(do.get(), pr.apply(q, mode, *amounts, 77), (mode, shape, "nchw"))
            assert do.guards_ok()
            for value in (-0.0, 1.5):
                dy = ctx.guarded(oshape)
                try:
                    _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_pad2d_f32(ctx.h, dx.ptr, dy.ptr, *shape, mode, *amounts, value)))
                    got, ok = dy.read()
                finally:
                    dy.free()
                assert names == [pr.FP32_KERNEL]
                assert ok and support.same_bits(got, pr.apply(x, mode, *amounts, f32(value))), (mode, shape, "f32", value)
                assert abi.GuardedOut.unwritten(got) == 0
        finally:
            for d in (di, do, dx):
                d.free()
    want = pr.apply(np.zeros((1, 1, 1, 1), f32), pr.CONSTANT, 1, 0, 0, 0, f32(-0.0))
    assert np.signbit(want[0, 0, 0, 0]) and not np.signbit(want[0, 0, 0, 1])   # the restatement keeps the fill's sign bit


def test_c_entry_argument_errors(ctx):
    """with a live context too, nothing launches and no byte moves"""
    lib = abi.lib()
    buf = ctx.put(np.zeros(8192, np.uint8))
    try:
        h, p = ctx.h, buf.ptr
        o = C.c_void_p(p.value + 4096)
        bad, names = ctx.kernels_run(lambda: [
            lib.i8ie_pad2d_u8_nhwc(h, None, 0, 0, o, 0, 0, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0), lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, None, 0, 0, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0),
            lib.i8ie_pad2d_u8_nhwc(h, p, -1, 0, o, 0, 0, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0), lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, -1, 0, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0),
            lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, 0, 0, 1, 4, 2, 2, 4, 1, 1, 1, 1, 0, 0, 0), lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, 0, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0, 0, 0, 0),
            lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, 0, 0, 1, 4, 2, 2, 3, 0, 0, 3, 0, 0, 0, 0), lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, 0, 0, 1, 4, 2, 2, 2, -1, 0, 0, 0, 0, 0, 0),
            lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, o, 0, 0, 1, 4, 2, 2, 0, -1, -1, 0, 0, 0, 0, 0), lib.i8ie_pad2d_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0),
            lib.i8ie_pad2d_u8(h, p, p, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0), lib.i8ie_pad2d_u8(h, p, o, 1, 4, 2, 2, 1, 2, 0, 0, 0, 0), lib.i8ie_pad2d_u8(h, p, None, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0),
            lib.i8ie_pad2d_f32(h, p, o, 0, 4, 2, 2, 1, 1, 1, 1, 1, 0.0), lib.i8ie_pad2d_f32(h, p, p, 1, 4, 2, 2, 1, 1, 1, 1, 1, 0.0),
            lib.i8ie_pad2d_f32(h, p, o, 1, 4, 2, 2, 3, 3, 0, 0, 0, 0.0)])
        assert bad == [-1] * len(bad), bad
        assert names == [] and (buf.get() == 0).all()
    finally:
        buf.free()


# ---- 6. the Python surface -----------------------------------------------------------------------------------------------------
FOREIGN = support.GLUE_KERNELS + (pr.DIRECT, pr.FP32_KERNEL)


def _only(launches, own=KERNELS):
    """{kernel: launches} of the new kernels; no glue kernel and no fall-back form ran"""
    for k in launches:
        assert not k.startswith(FOREIGN), launches
    support.assert_no_glue_launches(launches)
    return {k: v for k, v in launches.items() if k in own}


def test_conv_reflect_pad_conv_is_three_launches(i8ie):
    q = support.activation(i8ie)
    conv0, conv_c = support.conv(i8ie, 16, 32, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 32, 16, 3, 0, 2, (0.05, 120))
    first, got, launches = support.counted_forward(lambda: conv_c(i8ie.pad(conv0(q), (1, 1, 1, 1), "reflect")))
    mid = i8ie.pad(conv0(q), (1, 1, 1, 1), "reflect")
    assert mid.shape == (2, 32, 10, 10) and mid.scale == pytest.approx(0.04) and mid.zero_point == 110
    want_mid = pr.apply(conv0(q).numpy(), pr.REFLECT, 1, 1, 1, 1)
    assert np.array_equal(mid.numpy(), want_mid)
    assert got.shape == (2, 16, 8, 8) and np.array_equal(got, support.conv_ref(conv_c, want_mid, 0.04, 110)) and np.array_equal(first, got)
    assert _only(launches) == {pr.FAST: 1} and sum(launches.values()) == 3, launches


def test_pad_relu_conv_is_two_launches(i8ie):
    """the relu folds into the pad's launch (fill bytes included: value -1 is a byte below the zero point), and the conv reads
    the padded map with the border and the re-bias it asked the pad for"""
    q = support.activation(i8ie)
    conv_c = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    forward = lambda: conv_c(i8ie.relu(i8ie.pad(q, (0, 1, 0, 1), value=-1.0)))  # noqa: E731
    first, got, launches = support.counted_forward(forward)
    s, zp = q.scale, q.zero_point
    fill = pr.fill_byte(-1.0, s, zp)
    assert fill < zp
    want_mid = pr.apply(q.numpy(), pr.CONSTANT, 0, 1, 0, 1, fill, True, zp)
    assert np.array_equal(i8ie.relu(i8ie.pad(q, (0, 1, 0, 1), value=-1.0)).numpy(), want_mid)
    assert np.array_equal(got, support.conv_ref(conv_c, want_mid, s, zp, pad=1)) and np.array_equal(first, got)
    assert _only(launches) == {pr.FAST: 1} and sum(launches.values()) == 2, launches


def test_crop_of_a_conv_result_feeds_a_concat(i8ie):
    q = support.activation(i8ie)
    qp = (0.04, 110)
    conv0, conv_b = support.conv(i8ie, 16, 16, 3, 1, 1, qp), support.conv(i8ie, 16, 16, 3, 0, 3, qp)

    def forward():
        y = conv0(q)
        return i8ie.cat([i8ie.crop(y, 1, 1, 6, 6), conv_b(y)], *qp)   # the original U-Net's centre crop of the skip tensor

    first, got, launches = support.counted_forward(forward)
    y = conv0(q).numpy()
    want = np.concatenate([y[:, :, 1:7, 1:7], support.conv_ref(conv_b, y, *qp)], axis=1)
    assert got.shape == (2, 32, 6, 6) and np.array_equal(got, want) and np.array_equal(first, want)
    assert _only(launches) == {pr.FAST: 1} and sum(launches.values()) == 4, launches
    assert np.array_equal(i8ie.crop(conv0(q), 7, 0, 1, 1).numpy(), y[:, :, 7:8, 0:1])


def test_zero_amounts_and_unconsumed_results_launch_nothing(i8ie):
    q = support.activation(i8ie)
    conv0 = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110))

    def forward():
        y = conv0(q)
        assert i8ie.pad(y, (0, 0, 0, 0), "reflect") is y and i8ie.crop(y, 0, 0, 8, 8) is y
        i8ie.pad(y, (2, 2, 2, 2), "circular")   # nobody consumes it
        return i8ie.pad(y, (0, 0), "replicate")

    _, got, launches = support.counted_forward(forward)
    assert np.array_equal(got, conv0(q).numpy())
    assert _only(launches) == {} and sum(launches.values()) == 1, launches


def test_surface_user_tensors_fp32_and_fill_values(i8ie):
    """a user-made NCHW u8 operand takes the flat entry in place (plus relu_u8 where asked); FP32 tensors bit for bit; the fill
    byte is the one quantize gives the value, below, inside and above what a byte represents"""
    rng = np.random.default_rng(12)
    x = rng.uniform(-3, 3, (2, 5, 4, 6)).astype(f32)
    x.flat[0] = -0.0
    s, zp = 0.025, 127
    q = i8ie.quantize(i8ie.tensor(x), s, zp)  # NCHW bytes
    qv, t = q.numpy(), i8ie.tensor(x)
    for mode, amounts in [(pr.CONSTANT, (2, 1, 3, 0)), (pr.REFLECT, (2, 1, 3, 0)), (pr.REPLICATE, (0, 7, 5, 0)), (pr.CIRCULAR, (6, 6, 4, 4)),
                          (pr.CONSTANT, (-1, 2, 1, -2)), (pr.REFLECT, (1, 2))]:
        name, full = pr.MODE_NAME[mode], tuple(amounts) + (0,) * (4 - len(amounts))
        r = i8ie.pad(q, amounts, name)
        assert r.scale == pytest.approx(s) and r.zero_point == zp
        assert np.array_equal(r.numpy(), pr.apply(qv, mode, *full, zp))
        assert np.array_equal(i8ie.relu(i8ie.pad(q, amounts, name)).numpy(), pr.apply(qv, mode, *full, zp, True, zp))
        assert support.same_bits(i8ie.pad(t, amounts, name).numpy(), pr.apply(x, mode, *full, f32(0)))
    for value in (-5.0, -1.0, 0.5, 3.0, 3.3, 40.0, -0.0):
        want = int(i8ie.quantize(i8ie.tensor(np.full((1, 1, 1, 1), value, f32)), s, zp).numpy()[0, 0, 0, 0])
        assert pr.fill_byte(value, s, zp) == want, value
        assert np.array_equal(i8ie.pad(q, (1, 1, 1, 1), value=value).numpy(), pr.apply(qv, pr.CONSTANT, 1, 1, 1, 1, want)), value
        assert support.same_bits(i8ie.pad(t, (1, 0, 0, 1), value=value).numpy(), pr.apply(x, pr.CONSTANT, 1, 0, 0, 1, f32(value))), value
    assert np.array_equal(i8ie.crop(q, 1, 2, 2, 3).numpy(), qv[:, :, 1:3, 2:5]) and support.same_bits(i8ie.crop(t, 3, 5, 1, 1).numpy(), x[:, :, 3:, 5:])


# ---- 7. step-by-step chains ------------------------------------------------------------------------------------------------------
def _replays(i8ie, forward, x, want):
    """eager, under force-fallback and replayed through GraphedForward: the same bytes"""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    assert np.array_equal(forward(i8ie.tensor(x)).numpy(), want)
    cx.force_fallback(True)
    try:
        assert np.array_equal(forward(i8ie.tensor(x)).numpy(), want)
    finally:
        cx.force_fallback(False)
    g = GraphedForward(forward, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy(), want)


def test_conv_pad_relu_conv_replays_in_a_graph(i8ie):
    s_in, zp_in, qp = 0.025, 127, (0.04, 110)
    c1, c2 = support.conv(i8ie, 3, 16, 3, 1, 1, qp), support.conv(i8ie, 16, 16, 3, 0, 2, (0.05, 120))

    def forward(t):
        return c2(i8ie.relu(i8ie.pad(c1(i8ie.quantize(t, s_in, zp_in)), (1, 1, 1, 1), "reflect")))

    x = np.random.default_rng(3).uniform(-2, 2, (3, 3, 8, 12)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), s_in, zp_in).numpy()
    mid = pr.apply(support.conv_ref(c1, q, s_in, zp_in, pad=1), pr.REFLECT, 1, 1, 1, 1, 0, True, qp[1])
    want = support.conv_ref(c2, mid, *qp)
    assert want.shape == (3, 16, 8, 12) and len(np.unique(want)) > 30
    _replays(i8ie, forward, x, want)


@pytest.mark.parametrize("c", [20, 32])
def test_generator_residual_block_step_by_step(i8ie, c):
    """one residual block of a Johnson / CycleGAN generator (without its norms): pad(reflect 1) -> 3x3 conv, padding 0 -> relu
    -> pad(reflect 1) -> 3x3 conv -> Add with the block's input, against pad_ref + the oracle composition support.conv_ref +
    add_ref; a channel count off and one on the 16-byte item"""
    s_in, zp_in, qp, qa = 0.025, 127, (0.04, 110), (0.06, 115)
    stem = support.conv(i8ie, 3, c, 3, 1, 1, qp)
    b1, b2 = support.conv(i8ie, c, c, 3, 0, 2, qp), support.conv(i8ie, c, c, 3, 0, 3, qp)

    def forward(t):
        y = i8ie.relu(stem(i8ie.quantize(t, s_in, zp_in)))
        r = b2(i8ie.pad(i8ie.relu(b1(i8ie.pad(y, (1, 1, 1, 1), "reflect"))), (1, 1, 1, 1), "reflect"))
        return i8ie.add(y, r, *qa)

    x = np.random.default_rng(c).uniform(-2, 2, (3, 3, 8, 8)).astype(f32)
    relu = lambda v: np.maximum(v, qp[1])  # noqa: E731
    y = relu(support.conv_ref(stem, i8ie.quantize(i8ie.tensor(x), s_in, zp_in).numpy(), s_in, zp_in, pad=1))
    m = relu(support.conv_ref(b1, pr.apply(y, pr.REFLECT, 1, 1, 1, 1), *qp))
    r = support.conv_ref(b2, pr.apply(m, pr.REFLECT, 1, 1, 1, 1), *qp)
    want = add_ref.add_u8(y, qp[1], qp[0], r, qp[1], qp[0], *qa)
    assert want.shape == (3, c, 8, 8) and len(np.unique(want)) > 30
    _replays(i8ie, forward, x, want)
