"""narrow / split / chunk / channel_shuffle / pixel_shuffle / pixel_unshuffle on the GPU (csrc/i8ie_rearrange.hip, DESIGN.md
section 8q).  Every op is a copy, so every comparison is bit for bit, over every byte of the physical output with the guard
bytes around it, against the numpy restatement of tests/rearrange_ref.py -- never against the code under test.  The case lists
live in rearrange_ref.py (tests/test_rearrange_host.py keeps every class of case in them)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import pointwise_util as pu
import rearrange_ref as rr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = 0xC7  # the input's border: a byte that is in no input below
KERNELS = (rr.NARROW_KERNEL, rr.FAST, rr.DIRECT)

ctx = support.ctx_fixture(rr)


def _bytes(shape, seed=0):
    """rr.channel_bytes without the poison byte (a border byte that was read shows as POISON in the result)"""
    q = rr.channel_bytes(shape, seed)
    q[q == POISON] = POISON ^ 1
    return q


def _same(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, "%d of %d differ" % (len(bad), want.size),
                           [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])


def _nhwc(ctx, kind, q, p0, p1=0, relu=False, zp=0, ib=0, ob=0, in_s8=0, out_s8=0, skew=0, fallback=False):
    """q NCHW logical -> (the NHWC entry's result, NCHW logical again; the kernel that ran).  The input's border holds POISON;
    the result's border holds zp (re-biased where asked) and, like the guard bytes around both buffers, must come back
    untouched (pointwise_util.interior asserts it); the interior starts as 0xEE."""
    n, c, h, w = q.shape
    _, oc, oh, ow = rr.output_shape(kind, p0, p1, n, c, h, w)
    fi, _ = pu.phys(np.ascontiguousarray(q.transpose(0, 2, 3, 1)), ib, POISON, in_s8, skew)
    fo, oshape = pu.phys(np.full((n, oh, ow, oc), 0xEE, np.uint8), ob, zp, out_s8, skew)
    di, do = ctx.put(fi), ctx.put(fo)
    ctx.set_force_fallback(fallback)
    try:
        _, names = ctx.kernels_run(lambda: abi.ck(abi.lib().i8ie_rearrange_u8_nhwc(
            ctx.h, C.c_void_p(di.ptr.value + pu.GUARD + skew), ib, in_s8, C.c_void_p(do.ptr.value + pu.GUARD + skew), ob, out_s8,
            n, c, h, w, kind, p0, p1, 1 if relu else 0, zp)))
        gi, go = di.get(), do.get()
    finally:
        ctx.set_force_fallback(False)
        di.free()
        do.free()
    assert np.array_equal(gi, fi), "the input (and its guards) must be untouched"
    assert len(names) == 1 and names[0] in KERNELS, names
    return np.ascontiguousarray(pu.interior(go, oshape, ob, zp, out_s8, skew).transpose(0, 3, 1, 2)), names[0]


def _check(ctx, kind, q, p0, p1=0, kernel=None, **kw):
    """one case: the bytes, the kernel that ran, and -- where that is not the direct form -- the same bytes under force-fallback"""
    want = rr.apply(kind, q, p0, p1, kw.get("relu", False), kw.get("zp", 0))
    got, name = _nhwc(ctx, kind, q, p0, p1, **kw)
    _same(got, want, (rr.KIND_NAME[kind], q.shape, p0, p1, kw, name))
    assert POISON not in got
    if kernel is not None:
        assert name == kernel, (rr.KIND_NAME[kind], q.shape, p0, p1, kw, name)
    if name != rr.DIRECT:
        got, fb = _nhwc(ctx, kind, q, p0, p1, fallback=True, **kw)
        assert fb == rr.DIRECT
        _same(got, want, ("fallback", rr.KIND_NAME[kind], q.shape, p0, p1, kw))


RELU_ZP = [(False, 0)] + [(True, zp) for zp in rr.ZPS]


# ---- 1. the case lists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,start,length", rr.NARROW_CASES, ids=["%d_%d_%d" % t for t in rr.NARROW_CASES])
def test_narrow(ctx, c, start, length):
    for (n, h, w), (relu, zp) in itertools.product(rr.NARROW_MAPS, RELU_ZP):
        _check(ctx, rr.NARROW, _bytes((n, c, h, w), c), start, length, kernel=rr.NARROW_KERNEL, relu=relu, zp=zp)


def test_narrow_rows(ctx):
    """rank 2 [5, 35]: the NCHW entry with h = w = 1"""
    m, f = rr.NARROW_ROWS
    q = _bytes((m, f, 1, 1), 3)
    for start, length in [(3, 5), (0, 35), (34, 1), (16, 16)]:
        di, do = ctx.put(q), abi.GuardedU8(ctx, (m, length, 1, 1), fill=0xEE)
        try:
            abi.ck(abi.lib().i8ie_rearrange_u8(ctx.h, di.ptr, do.ptr, m, f, 1, 1, rr.NARROW, start, length))
            _same(do.get(), rr.narrow(q, start, length), (start, length))
            assert do.guards_ok()
        finally:
            di.free()
            do.free()


@pytest.mark.parametrize("c,g", rr.SHUFFLE_CASES, ids=["%d_%d" % t for t in rr.SHUFFLE_CASES])
def test_channel_shuffle(ctx, c, g):
    for (n, h, w), (relu, zp) in itertools.product(rr.SHUFFLE_MAPS, RELU_ZP):
        _check(ctx, rr.CHANNEL_SHUFFLE, _bytes((n, c, h, w), c + g), g, kernel=rr.expected_kernel(rr.CHANNEL_SHUFFLE, c, g), relu=relu, zp=zp)


@pytest.mark.parametrize("co,r", rr.PIXEL_CASES, ids=["%d_%d" % t for t in rr.PIXEL_CASES])
def test_pixel_shuffle_and_unshuffle(ctx, co, r):
    h, w = rr.PIXEL_MAP
    for n, (relu, zp) in itertools.product((1, 5), RELU_ZP):
        q = _bytes((n, co * r * r, h, w), co + r)
        _check(ctx, rr.PIXEL_SHUFFLE, q, r, kernel=rr.expected_kernel(rr.PIXEL_SHUFFLE, co * r * r, r), relu=relu, zp=zp)
        y = _bytes((n, co, h * r, w * r), 7 * co + r)  # the matching output
        _check(ctx, rr.PIXEL_UNSHUFFLE, y, r, kernel=rr.expected_kernel(rr.PIXEL_UNSHUFFLE, co, r), relu=relu, zp=zp)
        _same(_nhwc(ctx, rr.PIXEL_UNSHUFFLE, rr.pixel_shuffle(q, r), r)[0], q, "unshuffle o shuffle")


def test_random_bytes(ctx):
    """the same entries on random bytes (every byte value, the poison byte excepted)"""
    rng = np.random.default_rng(5)
    for kind, c, p0, p1, h, w in rr.LAYOUT_CASES:
        q = rng.integers(0, 256, (3, c, h, w), dtype=np.uint8)
        q[q == POISON] = 0
        _check(ctx, kind, q, p0, p1, relu=True, zp=127, ib=1, ob=1)


# ---- 2. the layout matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.LAYOUT_CASES, ids=["%s_%d_%d" % (rr.KIND_NAME[t[0]], t[1], t[2]) for t in rr.LAYOUT_CASES])
def test_layout_matrix(ctx, case):
    kind, c, p0, p1, h, w = case
    q = _bytes((2, c, h, w), c)
    want_kernel = rr.expected_kernel(kind, c, p0, p1)
    for relu, zp in [(False, 0), (True, 127)]:
        for ib, in_s8, ob, out_s8 in itertools.product(rr.IN_BORDERS, (0, 1), rr.OUT_BORDERS, (0, 1)):
            _check(ctx, kind, q, p0, p1, kernel=want_kernel, relu=relu, zp=zp, ib=ib, ob=ob, in_s8=in_s8, out_s8=out_s8)


# ---- 3. a base pointer 4 bytes off ----------------------------------------------------------------------------------------------
def test_misaligned_base(ctx):
    """both buffers 4 bytes into an allocation: narrow keeps its kernel with 4-byte items, the permuting ops leave the
    16-byte kernel; the bytes are the same"""
    for kind, c, p0, p1, h, w in rr.LAYOUT_CASES:
        q = _bytes((2, c, h, w), c)
        want = rr.NARROW_KERNEL if kind == rr.NARROW else rr.DIRECT
        _check(ctx, kind, q, p0, p1, kernel=want, relu=True, zp=127, ib=1, ob=1, skew=4)


# ---- 4. grids that wrap ----------------------------------------------------------------------------------------------------------
WRAP = [(rr.NARROW, (4, 20, 191, 187), 4, 16), (rr.CHANNEL_SHUFFLE, (3, 20, 191, 187), 5, 0), (rr.CHANNEL_SHUFFLE, (3, 32, 420, 421), 2, 0),
        (rr.PIXEL_UNSHUFFLE, (3, 20, 190, 188), 2, 0)]


@pytest.mark.parametrize("case", WRAP, ids=["%s_%d" % (rr.KIND_NAME[t[0]], t[1][1]) for t in WRAP])
def test_many_blocks(ctx, case):
    """more work than the 2048 x 256 lanes (the 2048 tiles of the 16-byte kernel: 256 two-chunk pixels each) of the largest
    grid, so the grid-stride loops go round; sizes that are no multiple of anything"""
    kind, shape, p0, p1 = case
    n, c, h, w = shape
    if kind == rr.CHANNEL_SHUFFLE and c == 32:
        assert n * h * w > 2048 * 256
    else:
        assert int(np.prod(rr.output_shape(kind, p0, p1, *shape))) // (4 if kind == rr.NARROW else 1) > 2048 * 256
    q = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
    q[q == POISON] = 1
    want = rr.apply(kind, q, p0, p1, True, 100)
    got, name = _nhwc(ctx, kind, q, p0, p1, True, 100, ib=1, ob=1, out_s8=1)
    assert name == rr.expected_kernel(kind, c, p0, p1)
    _same(got, want, case)


# ---- 5. NCHW and FP32 entries ------------------------------------------------------------------------------------------------
ENTRY_CASES = [(rr.NARROW, (2, 35, 3, 5), 3, 5), (rr.CHANNEL_SHUFFLE, (2, 20, 3, 5), 5, 0), (rr.CHANNEL_SHUFFLE, (2, 32, 3, 5), 2, 0),
               (rr.PIXEL_SHUFFLE, (2, 36, 2, 3), 3, 0), (rr.PIXEL_SHUFFLE, (2, 64, 2, 3), 8, 0), (rr.PIXEL_UNSHUFFLE, (2, 3, 4, 6), 2, 0),
               (rr.PIXEL_UNSHUFFLE, (2, 5, 9, 6), 3, 0)]


def test_nchw_and_fp32_entries(ctx):
    rng = np.random.default_rng(9)
    for kind, shape, p0, p1 in ENTRY_CASES:
        oshape = rr.output_shape(kind, p0, p1, *shape)
        q = _bytes(shape, p0)
        di, do = ctx.put(q), abi.GuardedU8(ctx, oshape, fill=0xEE)
        x = (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(f32)
        x.flat[0], x.flat[1], x.flat[2] = np.nan, np.inf, -0.0
        dx, dy = ctx.put(x), ctx.guarded(oshape)
        try:
            abi.ck(abi.lib().i8ie_rearrange_u8(ctx.h, di.ptr, do.ptr, *shape, kind, p0, p1))
            _same(do.get(), rr.apply(kind, q, p0, p1), (kind, shape, "nchw"))
            assert do.guards_ok()
            abi.ck(abi.lib().i8ie_rearrange_f32(ctx.h, dx.ptr, dy.ptr, *shape, kind, p0, p1))
            got, ok = dy.read()
            assert ok and support.same_bits(got, rr.apply(kind, x, p0, p1)), (kind, shape, "f32")
        finally:
            for d in (di, do, dx, dy):
                d.free()


def test_c_entry_argument_errors(ctx):
    lib = abi.lib()
    buf = ctx.put(np.zeros(4096, np.uint8))
    try:
        p, h = buf.ptr, ctx.h
        bad = [lib.i8ie_rearrange_u8_nhwc(h, None, 0, 0, p, 0, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0), lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, None, 0, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0),
               lib.i8ie_rearrange_u8_nhwc(h, p, -1, 0, p, 0, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0), lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, -1, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0),
               lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 1, 3, 0, 0, 0), lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 0, 3, 2, 0, 0),
               lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 2, 9, 0, 0, 0), lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 3, 2, 3, 2, 0, 0, 0),
               lib.i8ie_rearrange_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 7, 2, 0, 0, 0), lib.i8ie_rearrange_u8(h, p, p, 1, 4, 2, 2, 1, 3, 0),
               lib.i8ie_rearrange_u8(h, p, None, 1, 4, 2, 2, 1, 2, 0), lib.i8ie_rearrange_f32(h, p, p, 0, 4, 2, 2, 1, 2, 0),
               lib.i8ie_rearrange_f32(h, p, p, 1, 4, 2, 2, 2, 3, 0)]
        assert bad == [-1] * len(bad), bad
        assert (buf.get() == 0).all()
    finally:
        buf.free()


# ---- 6. the Python surface -----------------------------------------------------------------------------------------------------
FOREIGN = support.GLUE_KERNELS + ("rearrange_u8_nchw", rr.DIRECT)


def _only(launches, own):
    """{kernel: launches} of the new kernels; no glue kernel and no fall-back form ran"""
    for k in launches:
        assert not k.startswith(FOREIGN), launches
    support.assert_no_glue_launches(launches)
    return {k: v for k, v in launches.items() if k in own}


def test_conv_channel_shuffle_relu_conv_is_three_launches(i8ie):
    q = support.activation(i8ie)
    conv0, conv_c = support.conv(i8ie, 16, 32, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 32, 16, 3, 1, 2, (0.05, 120))
    first, got, launches = support.counted_forward(lambda: conv_c(i8ie.relu(i8ie.channel_shuffle(conv0(q), 2))))
    mid = i8ie.relu(i8ie.channel_shuffle(conv0(q), 2))
    assert mid.shape == (2, 32, 8, 8) and mid.scale == pytest.approx(0.04) and mid.zero_point == 110
    assert np.array_equal(mid.numpy(), rr.channel_shuffle(conv0(q).numpy(), 2, True, 110))
    assert np.array_equal(got, conv_c(mid).numpy()) and np.array_equal(first, got)
    assert _only(launches, KERNELS) == {rr.FAST: 1} and sum(launches.values()) == 3, launches


def test_conv_pixel_shuffle_relu_conv_is_three_launches(i8ie):
    q = support.activation(i8ie)
    conv0, conv_c = support.conv(i8ie, 16, 64, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    first, got, launches = support.counted_forward(lambda: conv_c(i8ie.relu(i8ie.pixel_shuffle(conv0(q), 2))))
    mid = i8ie.relu(i8ie.pixel_shuffle(conv0(q), 2))
    assert mid.shape == (2, 16, 16, 16) and mid.zero_point == 110
    assert np.array_equal(mid.numpy(), rr.pixel_shuffle(conv0(q).numpy(), 2, True, 110))
    assert got.shape == (2, 16, 16, 16) and np.array_equal(got, conv_c(mid).numpy()) and np.array_equal(first, got)
    assert _only(launches, KERNELS) == {rr.FAST: 1} and sum(launches.values()) == 3, launches


def test_shuffle_unit_launch_counts(i8ie):
    """x1, x2 = chunk(conv(x), 2); cat([x1, conv(x2)]) -> channel_shuffle: producer, two narrows, the branch conv, the cat, the
    shuffle are six launches, the final conv the seventh; nothing converts, re-biases or fills"""
    q = support.activation(i8ie)
    qp = (0.04, 110)
    conv0, conv_b, conv_c = support.conv(i8ie, 16, 32, 3, 1, 1, qp), support.conv(i8ie, 16, 16, 1, 0, 3, qp), support.conv(i8ie, 32, 16, 3, 1, 2, (0.05, 120))

    def unit():
        x1, x2 = i8ie.chunk(conv0(q), 2)
        return i8ie.channel_shuffle(i8ie.cat([x1, conv_b(x2)], *qp), 2)

    first, got, launches = support.counted_forward(unit)
    y = conv0(q).numpy()
    want = rr.channel_shuffle(np.concatenate([y[:, :16], support.conv_ref(conv_b, y[:, 16:], *qp)], axis=1), 2)
    assert np.array_equal(got, want) and np.array_equal(first, want)
    assert _only(launches, KERNELS) == {rr.NARROW_KERNEL: 2, rr.FAST: 1} and sum(launches.values()) == 6, launches
    _, got7, launches = support.counted_forward(lambda: conv_c(unit()))
    assert _only(launches, KERNELS) == {rr.NARROW_KERNEL: 2, rr.FAST: 1} and sum(launches.values()) == 7, launches
    assert np.array_equal(got7, support.conv_ref(conv_c, want, *qp, pad=1))


def test_unconsumed_split_part_launches_nothing(i8ie):
    q = support.activation(i8ie)
    conv0 = support.conv(i8ie, 16, 32, 3, 1, 1, (0.04, 110))

    def forward():
        parts = i8ie.split(conv0(q), [8, 8, 16])
        assert [p.shape[1] for p in parts] == [8, 8, 16]
        return parts[2]

    first, got, launches = support.counted_forward(forward)
    assert np.array_equal(got, conv0(q).numpy()[:, 16:]) and np.array_equal(first, got)
    assert _only(launches, KERNELS) == {rr.NARROW_KERNEL: 1} and sum(launches.values()) == 2, launches


def test_surface_user_tensors_fp32_and_s8(i8ie):
    """a user-made NCHW u8 operand (the flat entry, plus relu_u8 where asked), rank-2 rows, FP32 tensors bit for bit, and the
    refusal of an int8 tensor"""
    import _CXX_i8ie as cx

    rng = np.random.default_rng(12)
    x = rng.uniform(-3, 3, (2, 36, 4, 6)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)  # NCHW bytes
    qv = q.numpy()
    t = i8ie.tensor(x)
    calls = [(lambda a: i8ie.narrow(a, 3, 5), lambda v, **kw: rr.narrow(v, 3, 5, **kw)),
             (lambda a: i8ie.channel_shuffle(a, 3), lambda v, **kw: rr.channel_shuffle(v, 3, **kw)),
             (lambda a: i8ie.pixel_shuffle(a, 3), lambda v, **kw: rr.pixel_shuffle(v, 3, **kw)),
             (lambda a: i8ie.pixel_unshuffle(a, 2), lambda v, **kw: rr.pixel_unshuffle(v, 2, **kw))]
    for op, ref in calls:
        r = op(q)
        assert r.scale == pytest.approx(0.025) and r.zero_point == 127
        assert r.shape == ref(qv).shape and np.array_equal(r.numpy(), ref(qv))
        assert np.array_equal(i8ie.relu(op(q)).numpy(), ref(qv, relu=True, zp=127))
        assert support.same_bits(op(t).numpy(), ref(x))
    for sizes in (7, [30, 6]):
        for got, want, gf in zip(i8ie.split(q, sizes), rr.split(qv, sizes), i8ie.split(t, sizes)):
            assert np.array_equal(got.numpy(), want) and gf.shape == want.shape
    assert [p.shape for p in i8ie.chunk(q, 5)] == [(2, 8, 4, 6)] * 4 + [(2, 4, 4, 6)]
    rows = i8ie.quantize(i8ie.tensor(x.reshape(8, 216)), 0.025, 127)
    assert np.array_equal(i8ie.narrow(rows, 100, 17).numpy(), rows.numpy()[:, 100:117])
    s8 = i8ie.Tensor(cx.tensor_s8(np.zeros((1, 4, 2, 2), np.int8), 0.5, 0))
    for name, call in [("narrow", lambda: i8ie.narrow(s8, 0, 2)), ("channel_shuffle", lambda: i8ie.channel_shuffle(s8, 2)),
                       ("pixel_shuffle", lambda: i8ie.pixel_shuffle(s8, 2)), ("pixel_unshuffle", lambda: i8ie.pixel_unshuffle(s8, 2))]:
        with pytest.raises(RuntimeError, match=name + ".*int8"):
            call()


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


@pytest.mark.parametrize("c", [20, 32])
def test_shufflenet_units_step_by_step(i8ie, c):
    """one ShuffleNetV2 basic unit (chunk, a conv branch, cat, channel_shuffle(2)) and one down-sampling unit (two stride-2
    branches, cat, channel_shuffle(2)) at c channels, against the oracle composition support.conv_ref + rearrange_ref"""
    h = c // 2
    s_in, zp_in, qp = 0.025, 127, (0.04, 110)
    stem = support.conv(i8ie, 3, c, 3, 1, 1, qp)
    b1, b2 = support.conv(i8ie, h, h, 1, 0, 2, qp), support.conv(i8ie, h, h, 3, 1, 3, qp)
    d1, d2a, d2b = support.conv(i8ie, c, c, 3, 1, 4, qp, stride=2), support.conv(i8ie, c, c, 1, 0, 5, qp), support.conv(i8ie, c, c, 3, 1, 6, qp, stride=2)

    def forward(t):
        y = i8ie.relu(stem(i8ie.quantize(t, s_in, zp_in)))
        x1, x2 = i8ie.chunk(y, 2)
        u = i8ie.channel_shuffle(i8ie.cat([x1, i8ie.relu(b2(i8ie.relu(b1(x2))))], *qp), 2)
        return i8ie.channel_shuffle(i8ie.cat([i8ie.relu(d1(u)), i8ie.relu(d2b(i8ie.relu(d2a(u))))], *qp), 2)

    x = np.random.default_rng(c).uniform(-2, 2, (3, 3, 8, 8)).astype(f32)
    relu = lambda v: np.maximum(v, qp[1])  # noqa: E731
    y = relu(support.conv_ref(stem, i8ie.quantize(i8ie.tensor(x), s_in, zp_in).numpy(), s_in, zp_in, pad=1))
    x1, x2 = rr.chunk(y, 2)
    assert x1.shape[1] == x2.shape[1] == h
    u = rr.channel_shuffle(np.concatenate([x1, relu(support.conv_ref(b2, relu(support.conv_ref(b1, x2, *qp)), *qp, pad=1))], axis=1), 2)
    left = relu(support.conv_ref(d1, u, *qp, pad=1, stride=2))
    right = relu(support.conv_ref(d2b, relu(support.conv_ref(d2a, u, *qp)), *qp, pad=1, stride=2))
    want = rr.channel_shuffle(np.concatenate([left, right], axis=1), 2)
    assert want.shape == (3, 2 * c, 4, 4) and len(np.unique(want)) > 30
    _replays(i8ie, forward, x, want)


def test_subpixel_chain_step_by_step(i8ie):
    """pixel_unshuffle(2) -> conv -> conv(c * 4) -> pixel_shuffle(2)"""
    s_in, zp_in, qp = 0.025, 127, (0.04, 110)
    c1, c2 = support.conv(i8ie, 12, 16, 3, 1, 1, qp), support.conv(i8ie, 16, 12, 1, 0, 2, (0.05, 120))

    def forward(t):
        return i8ie.pixel_shuffle(c2(i8ie.relu(c1(i8ie.pixel_unshuffle(i8ie.quantize(t, s_in, zp_in), 2)))), 2)

    x = np.random.default_rng(3).uniform(-2, 2, (3, 3, 8, 12)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), s_in, zp_in).numpy()
    mid = np.maximum(support.conv_ref(c1, rr.pixel_unshuffle(q, 2), s_in, zp_in, pad=1), qp[1])
    want = rr.pixel_shuffle(support.conv_ref(c2, mid, *qp), 2)
    assert want.shape == (3, 3, 8, 12) and len(np.unique(want)) > 30
    _replays(i8ie, forward, x, want)
