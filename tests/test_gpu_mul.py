"""The quantized broadcast Mul on the GPU (csrc/i8ie_binary.hip).  Every comparison is byte-exact against
the numpy restatement of the definition (tests/mul_ref.py), never against the code under test: all 65 536 byte pairs through
the flat entry and through the gate kernel at each item width for a range of quantisation parameters, the bordered /
re-biased NHWC entry in both forms with guard bytes, ragged lengths and aliasing, the edges of the gate kernel's tiling, the
FP32 entry as bit patterns, the Python surface, launch counts of a squeeze-and-excitation block, calibration, graph replay
and the two networks end to end."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import mul_ref as mr
import net_cases as nc
import pointwise_util as pu
import spec_ref as sr
import support
from support import i8ie, pairs  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
QP = dict(mr.QP)


ctx = support.ctx_fixture(mr)


def _mul_flat(ctx, pa, pb, po, n, qp, relu):
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    abi.ck(abi.lib().i8ie_mul_u8(ctx.h, pa, pb, po, n, float(s_a), int(zp_a), float(s_b), int(zp_b), float(s_out), int(zp_out),
                                 1 if relu else 0))


def _want(a, b, qp, relu):
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    return mr.mul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name,qp", mr.QP, ids=[q[0] for q in mr.QP])
def test_exhaustive_byte_pairs(ctx, pairs, name, qp, relu):
    a, b, da, db, do = pairs
    _mul_flat(ctx, da.ptr, db.ptr, do.ptr, a.size, qp, relu)
    got = do.get()
    want = _want(a, b, qp, relu)
    bad = np.flatnonzero(got != want)  # every one of the 65 536 elements is compared
    assert got.shape == want.shape == (65536,) and bad.size == 0, (name, bad[:8], a[bad[:8]], b[bad[:8]], got[bad[:8]], want[bad[:8]])


def _run_nhwc(ctx, a, b, gate, borders, flags, qp, relu, keep=None):
    """a: [n, h, w, c]; b: the same shape, or with gate [n, c].  Runs i8ie_mul_u8_nhwc on guarded, bordered buffers, checks
    that the operands, every guard and the result's border are untouched, and returns the result's interior [n, h, w, c].
    keep: a dict that holds the device copies of a and b between calls with the same operands."""
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    n, h, w, c = a.shape
    ba, bb, bo = borders
    a_s8, b_s8, o_s8 = flags
    key = (ba, bb, a_s8, b_s8)
    if keep is not None and key in keep:
        fa, fb, da, db = keep[key]
    else:
        fa, _ = pu.phys(a, ba, zp_a, a_s8)
        fb, _ = pu.phys(b.reshape(n, 1, 1, c) if gate else b, bb, zp_b, b_s8)
        da, db = ctx.put(fa), ctx.put(fb)
        if keep is not None:
            keep[key] = (fa, fb, da, db)
    fo, oshape = pu.phys(np.zeros_like(a) + np.uint8(0xEE), bo, zp_out, o_s8)  # the border as i8ie_fill_border_u8 leaves it
    do = ctx.put(fo)
    pa, pb, po = (C.c_void_p(d.ptr.value + pu.GUARD) for d in (da, db, do))
    abi.ck(abi.lib().i8ie_mul_u8_nhwc(ctx.h, pa, ba, a_s8, pb, bb, b_s8, 1 if gate else 0, po, bo, o_s8, n, c, h, w, float(s_a), int(zp_a),
                                      float(s_b), int(zp_b), float(s_out), int(zp_out), 1 if relu else 0))
    go = do.get()
    do.free()
    if keep is None:
        ga, gb = da.get(), db.get()
        da.free()
        db.free()
        assert np.array_equal(ga, fa) and np.array_equal(gb, fb), "operands (and their guards) must be untouched"
    return pu.interior(go, oshape, bo, int(zp_out), o_s8)  # (checks the guard bytes and the border ring)


def _free(keep):
    for fa, fb, da, db in keep.values():
        assert np.array_equal(da.get(), fa) and np.array_equal(db.get(), fb), "operands (and their guards) must be untouched"
        da.free()
        db.free()


def _nchw(x_nhwc):
    return np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2))


GATE_EXHAUSTIVE_SETS = mr.GATE_SETS + ["k128_zp_3_250_17", "pow2_k64", "pow2_k256", "thirds", "calibrated_0", "calibrated_3",
                                       "denormal_products", "zero_s_b", "overflowing_products", "equal_saturating"]


@pytest.mark.parametrize("gate_form", ["rows", "nhwc"])
@pytest.mark.parametrize("c", [16, 20, 3])
def test_exhaustive_byte_pairs_through_the_gate_kernel(ctx, c, gate_form):
    """every (a, g) pair occurs: the gate bytes of ceil(256 / c) images run through all 256 values, and the 256 pixels of every
    (image, channel) carry all 256 values of a.  c = 16, 20, 3: 16-, 4- and 1-byte items."""
    n = -(-256 // c)
    img, pix, ch = np.meshgrid(np.arange(n), np.arange(256), np.arange(c), indexing="ij")
    a = ((pix + 7 * ch + 3 * img) % 256).astype(np.uint8).reshape(n, 16, 16, c)
    g = ((np.arange(n)[:, None] * c + np.arange(c)[None, :]) % 256).astype(np.uint8)
    seen = np.zeros((256, 256), bool)
    seen[a.reshape(n, 256, c), np.broadcast_to(g[:, None, :], (n, 256, c))] = True
    assert seen.all(), "every (a, g) pair occurs"
    borders, flags = ((0, 0, 0), (0, 0, 0)) if gate_form == "rows" else ((0, 1, 0), (0, 1, 0))
    assert len(GATE_EXHAUSTIVE_SETS) >= len(mr.GATE_SETS) + 5 >= 10
    keep = {}
    try:
        for name, relu in itertools.product(GATE_EXHAUSTIVE_SETS, (False, True)):
            qp = QP[name]
            got = _run_nhwc(ctx, a, g, True, borders, flags, qp, relu, keep)
            want = support.nhwc(_want(_nchw(a), g, qp, relu))
            bad = np.argwhere(got != want)
            assert bad.size == 0, (name, relu, bad[:4], [(a[tuple(i)], g[i[0], i[3]], got[tuple(i)], want[tuple(i)]) for i in bad[:4]])
    finally:
        _free(keep)


@pytest.mark.parametrize("form", ["equal", "gate"])
@pytest.mark.parametrize("borders", [(0, 0, 0), (1, 0, 1), (0, 2, 1), (2, 1, 0)], ids=lambda b: "b%d%d%d" % b)
@pytest.mark.parametrize("c", [16, 20, 3])
def test_bordered_nhwc(ctx, c, borders, form):
    n, h, w = 2, 3, 5
    rng = np.random.default_rng(c * 10 + sum(borders))
    a = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    gate = form == "gate"
    b = rng.integers(0, 256, (n, c) if gate else (n, h, w, c), dtype=np.uint8)
    qp = QP["gate_zp100"] if gate else QP["k128_zp_3_250_17"]
    for i, flags in enumerate(itertools.product((0, 1), repeat=3)):
        relu = (i + c) % 2
        got = _run_nhwc(ctx, a, b, gate, borders, flags, qp, bool(relu))
        want = support.nhwc(_want(_nchw(a), b if gate else _nchw(b), qp, bool(relu)))
        assert np.array_equal(got, want), (flags, relu)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_ragged_lengths_and_aliasing(ctx, n):
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    qp = QP["calibrated_1"]
    pad = np.full(64, 0xA5, np.uint8)  # guard bytes behind the n elements
    for relu in (False, True):
        want = _want(a, b, qp, relu)
        da, db, do = ctx.put(np.concatenate([a, pad])), ctx.put(np.concatenate([b, pad])), ctx.put(np.concatenate([a ^ 0xFF, pad]))
        _mul_flat(ctx, da.ptr, db.ptr, do.ptr, n, qp, relu)  # a separate output
        got = do.get()
        assert np.array_equal(got[:n], want) and np.array_equal(got[n:], pad)
        assert np.array_equal(da.get()[:n], a) and np.array_equal(db.get()[:n], b)
        _mul_flat(ctx, db.ptr, db.ptr, do.ptr, n, qp, relu)  # a is b
        got = do.get()
        assert np.array_equal(got[:n], _want(b, b, qp, relu)) and np.array_equal(got[n:], pad)
        _mul_flat(ctx, da.ptr, db.ptr, da.ptr, n, qp, relu)  # out aliases a
        got = da.get()
        assert np.array_equal(got[:n], want) and np.array_equal(got[n:], pad)
        da.free()
        da = ctx.put(np.concatenate([a, pad]))
        _mul_flat(ctx, da.ptr, db.ptr, db.ptr, n, qp, relu)  # out aliases b
        got = db.get()
        assert np.array_equal(got[:n], want) and np.array_equal(got[n:], pad)
        for d in (da, db, do):
            d.free()


def _tile(c):
    """pixels of one image a block of the gate kernel covers: its whole pixels times the pixels a lane walks"""
    vec = 16 if c % 16 == 0 else (4 if c % 4 == 0 else 1)
    lanes_c = min(c // vec, mr.THREADS)
    return (mr.THREADS // lanes_c) * mr.WALK


# (n, c, h, w): h * w of 1, one less and one more than the pixels a lane walks; one less and one more than a block's tile at
# each item width (and with 36 items per pixel, which do not divide the block); a single image; more channel items than a
# block has lanes; and one unit more than the grid cap, where the block-stride loop takes its second pass
TILING_CASES = [(3, 16, 1, 1), (3, 16, 1, mr.WALK - 1), (3, 16, 3, 3), (1, 16, 23, 89), (1, 16, 3, 683), (2, 576, 5, 11), (2, 576, 3, 19),
                (1, 20, 11, 37), (2, 20, 1, 409), (1, 3, 7, 97), (2, 3, 3, 227), (1, 35, 4, 4), (2, 4112, 1, 3), (mr.MAX_BLOCKS + 1, 16, 1, 1)]


@pytest.mark.parametrize("shape", TILING_CASES, ids=lambda s: "n%d_c%d_%dx%d" % s)
def test_gate_kernel_tiling_edges(ctx, shape):
    n, c, h, w = shape
    assert _tile(16) == 2048 == 23 * 89 + 1 == 3 * 683 - 1 and _tile(576) == 56 and _tile(20) == 408 and _tile(3) == 680 and mr.WALK == 8
    rng = np.random.default_rng(n + c + h * w)
    a = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    g = rng.integers(0, 256, (n, c), dtype=np.uint8)
    qp = QP["gate_zp160"]
    borders, flags = ((1, 0, 1), (1, 0, 1)) if (h * w) % 2 else ((0, 1, 2), (0, 1, 0))
    got = _run_nhwc(ctx, a, g, True, borders, flags, qp, False)
    assert np.array_equal(got, support.nhwc(_want(_nchw(a), g, qp, False)))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1025])
def test_fp32_bit_patterns(ctx, n):
    """a * b as numpy float32 computes it, as bit patterns, in both forms (the gate form with n elements per gate value).
    (0 * inf is left out: IEEE 754 leaves the sign of a generated NaN open.  A NaN operand is propagated by both.)"""
    rng = np.random.default_rng(n)
    rows = 6
    a = (rng.standard_normal(rows * n).astype(f32) * f32(100)).astype(f32)
    b = rng.standard_normal(rows * n).astype(f32)
    inf, nan = f32(np.inf), f32(np.nan)
    special = [(-0.0, 5.0), (inf, -1.0), (nan, 1.0), (-inf, -inf), (-0.0, -0.0), (3e38, 3e38), (1e-30, 1e-30), (1e-40, 0.5),
               (16777217.0, 3.0), (1.0, nan)]
    for i, (x, y) in enumerate(special[:a.size]):
        a[i], b[i] = f32(x), f32(y)
    g = np.array([0.5, -0.0, 3.0, 1e-20, -7.25, 1.0], f32)
    lib = abi.lib()
    with np.errstate(all="ignore"):
        cases = [(a[:n], b[:n], 0, (a[:n] * b[:n]).astype(f32)), (a, g, n, (a.reshape(rows, n) * g[:, None]).astype(f32).ravel())]
    for x, y, run, want in cases:
        dx, dy, do = ctx.put(x), ctx.put(y), ctx.guarded((x.size,))
        try:
            abi.ck(lib.i8ie_mul_f32(ctx.h, dx.ptr, dy.ptr, do.ptr, x.size, run))
            got, guards_ok = do.read()
        finally:
            for d in (dx, dy, do):
                d.free()
        assert guards_ok
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (run, got, want)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def _linear(i8ie, fin, fout, seed, qp):
    rng = np.random.default_rng(seed)
    L = i8ie.Linear(fin, fout)
    L.load_weight((rng.uniform(-1, 1, (fout, fin)) * np.sqrt(6.0 / fin)).astype(f32))
    L.load_bias(rng.uniform(-0.1, 0.1, fout).astype(f32))
    L.set_output_qparams(*qp)
    L.convert()
    return L


def test_surface_shapes_mixed_layouts_and_errors(i8ie):
    rng = np.random.default_rng(11)
    x = rng.uniform(-2, 2, (2, 16, 8, 8)).astype(f32)
    conv = support.conv(i8ie, 16, 16, 3, 1, 5, (0.05, 120))
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)          # NCHW bytes
    qv = q.numpy()
    yv = conv(q).numpy()                                   # (observed on a tensor of its own: the operands below stay as they lie)
    gq = i8ie.quantize(i8ie.tensor(rng.uniform(0, 1, (2, 16)).astype(f32)), 1 / 255, 0)
    gv = gq.numpy()
    assert len(np.unique(gv)) >= 16
    s_g = f32(1 / 255)
    for relu in (False, True):
        # [n, c, h, w] . [n, c, h, w], an NCHW tensor against a pending conv result in the engine's layout, both ways round
        for swap in (False, True):
            y = conv(q)
            r = i8ie.mul(q, y, 0.01, 99) if swap else i8ie.mul(y, q, scale=0.01, zero_point=99)
            if relu:
                r = i8ie.relu(r)
            assert r.shape == (2, 16, 8, 8) and r.scale == pytest.approx(0.01) and r.zero_point == 99
            ops = (qv, 127, f32(0.025), yv, 120, f32(0.05)) if swap else (yv, 120, f32(0.05), qv, 127, f32(0.025))
            assert np.array_equal(r.numpy(), mr.mul_u8(*ops, f32(0.01), 99, relu)), (relu, swap)
        # . [n, c] and . [n, c, 1, 1], on the conv result (NHWC) and on the NCHW tensor (one layout conversion)
        for a_of, av, s_a, zp_a in ((lambda: conv(q), yv, f32(0.05), 120), (lambda: q, qv, f32(0.025), 127)):
            for gate in (gq, gq.reshape(2, 16, 1, 1)):
                r = i8ie.mul(a_of(), gate, 0.04, 110)
                if relu:
                    r = i8ie.relu(r)
                assert r.shape == (2, 16, 8, 8)
                assert np.array_equal(r.numpy(), mr.mul_u8(av, zp_a, s_a, gv, 0, s_g, f32(0.04), 110, relu))
    # the gate as a global pool leaves it, [n, c, 1, 1], straight into the mul
    pooled = i8ie.global_avg_pool2d(conv(q))
    pv = pooled.numpy()
    r = i8ie.mul(conv(q), i8ie.global_avg_pool2d(conv(q)), 0.02, 128)
    assert np.array_equal(r.numpy(), mr.mul_u8(yv, 120, f32(0.05), pv, 120, f32(0.05), f32(0.02), 128))
    # [m, f] . [m, f]: the flat form
    a2, b2 = q.reshape(2, -1), i8ie.quantize(i8ie.tensor(x[::-1].copy()), 0.03, 100).reshape(2, -1)
    r = i8ie.mul(a2, b2, 0.004, 128)
    assert np.array_equal(r.numpy(), mr.mul_u8(a2.numpy(), 127, f32(0.025), b2.numpy(), 100, f32(0.03), f32(0.004), 128))
    # a is b
    r = i8ie.mul(q, q, 0.02, 3)
    assert np.array_equal(r.numpy(), mr.mul_u8(qv, 127, f32(0.025), qv, 127, f32(0.025), f32(0.02), 3))
    # FP32, both forms
    t, tg = i8ie.tensor(x), i8ie.tensor(x[:, :, 0, 0].copy())
    assert np.array_equal(i8ie.mul(t, t).numpy().view(np.uint32), (x * x).view(np.uint32))
    for gate in (tg, tg.reshape(2, 16, 1, 1)):
        assert np.array_equal(i8ie.mul(t, gate).numpy().view(np.uint32), (x * x[:, :, :1, :1]).view(np.uint32))
    for bad in (q.reshape(2, -1), i8ie.quantize(i8ie.tensor(x[:1, :, :1, :1].copy()), 0.03, 100),       # [1, c, 1, 1]
                i8ie.quantize(i8ie.tensor(x[:, :1].copy()), 0.03, 100)):                                 # [n, 1, h, w]
        with pytest.raises(RuntimeError):
            i8ie.mul(q, bad, 0.05, 127)
    with pytest.raises(RuntimeError):
        i8ie.mul(gq.reshape(2, 16, 1, 1), q, 0.05, 127)    # only the second operand broadcasts
    with pytest.raises(RuntimeError):
        i8ie.mul(gq, gq.reshape(2, 16, 1, 1), 0.05, 127)   # a rank-2 a takes no gate
    with pytest.raises(RuntimeError):
        i8ie.mul(t, i8ie.tensor(x[:1]))
    with pytest.raises(TypeError):
        i8ie.mul(q, q)                                     # u8 needs the result's qparams
    with pytest.raises(TypeError):
        i8ie.mul(q, q, 0.05)
    with pytest.raises(TypeError):
        i8ie.mul(t, t, 0.05, 127)                          # ... and FP32 takes none
    with pytest.raises(RuntimeError):
        i8ie.mul(q, q, 0.05, 256)
    with pytest.raises(RuntimeError):
        i8ie.mul(q, q, 0.0, 1)
    with pytest.raises(RuntimeError):
        i8ie.Mul()(q, q)                                   # not converted
    m = i8ie.Mul()
    m.set_output_qparams(0.04, 110)
    m.convert()
    assert np.array_equal(m(conv(q), gq).numpy(), mr.mul_u8(yv, 120, f32(0.05), gv, 0, s_g, f32(0.04), 110))


def test_squeeze_excite_block_launch_counts(i8ie):
    """conv_c(relu(mul(x, g))) with x = conv0(..) and g = hardsigmoid(fc2(relu(fc1(gap(x))))) is exactly the launches of its
    producers -- x and g observed on their own, conv_c on an activation of the same shape -- plus ONE mul launch: conv0 feeds
    the pool and the mul from one launch, the relu folds into the mul, and the padded conv_c gets its border (and re-biased
    bytes, where it reads them) from the mul kernel; nothing converts, re-biases or fills."""
    conv0 = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110))
    conv_c = support.conv(i8ie, 16, 16, 3, 1, 6, (0.08, 90))
    fc1, fc2 = _linear(i8ie, 16, 8, 2, (0.02, 100)), _linear(i8ie, 8, 16, 3, (0.03, 128))
    hs = i8ie.Activation("hardsigmoid")
    hs.set_output_qparams(1 / 255, 0)
    hs.convert()
    mul = i8ie.Mul()
    mul.set_output_qparams(0.03, 100)
    mul.convert()
    xin = np.random.default_rng(4).uniform(-2, 2, (2, 3, 8, 8)).astype(f32)
    # an activation in the engine's layout that stays recorded (as in tests/test_gpu_add.py): the warm-up forward launches it
    # once, with the border its consumer asks for, and the counted forward finds that result
    q = i8ie.relu(support.conv(i8ie, 16, 16, 3, 1, 8, (0.05, 125))(i8ie.relu(support.conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))(
        i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))))

    def gate(x):
        return hs(fc2(i8ie.relu(fc1(i8ie.global_avg_pool2d(x).reshape(-1, 16)))))

    def producers():
        x = conv0(q)
        return [gate(x), x]

    def forward():
        x = conv0(q)
        return [conv_c(i8ie.relu(mul(x, gate(x))))]

    made = support.counted(producers)      # conv0 once, the pool, the two Linears (with whatever their routes launch), the hardsigmoid
    behind = support.counted(lambda: [conv_c(q)])
    whole = support.counted(forward)
    print(made, behind, whole)
    assert sum(behind.values()) == 1 and sum(v for k, v in made.items() if k.startswith(("avgpool", "lut_u8"))) == 2
    want_launches = dict(made)
    for k, v in behind.items():
        want_launches[k] = want_launches.get(k, 0) + v
    want_launches["mul_u8_gate"] = 1
    assert whole == want_launches, (whole, want_launches)
    for k in whole:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), whole
    # the expected bytes, from the observed producers of the same layers and the restatement of the mul
    got = forward()[0].numpy()
    xv, gv = conv0(q).numpy(), gate(conv0(q)).numpy()
    assert gv.shape == (2, 16) and len(np.unique(gv)) >= 8
    mid = mr.mul_u8(xv, 110, f32(0.04), gv, 0, f32(1 / 255), f32(0.03), 100, True)
    assert len(np.unique(mid)) > 30
    want, _ = gr.conv2d_grouped(mid, conv_c.layer.q_weight(), conv_c.layer.q_bias(), 1, 1, 1, f32(0.03), 100,
                                conv_c.weight_scale(), f32(0.08), 90)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_mul_is_calibrated_like_a_layer(i8ie, mode):
    import _CXX_i8ie as cx

    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, (5, 8, 10, 10)).astype(f32)
    g = rng.uniform(0, 1, (5, 8)).astype(f32)
    total = (a * g[:, :, None, None]).astype(f32)
    cx.set_calibration_mode(mode)
    cx.set_calibration_seed(7)
    try:
        mul = i8ie.Mul()
        mul.prepare()
        got = mul(i8ie.tensor(a), i8ie.tensor(g)).numpy()
        mul.convert()
        if mode == "host":
            want = tuple(cx.calibrator_range([total.ravel()], 1.0))
        else:
            want = tuple(cx.calibrator_device_samples([total.ravel()], 7)[2:])
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert np.array_equal(got.view(np.uint32), total.view(np.uint32))
    assert mul.layer.is_quantized() and mul.output_qparams() == want and want[0] != 1.0


# ---- the networks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [2, 66])
def test_se_tiny_bit_exact(i8ie, batch, per_channel, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    name = "se_tiny"
    net, qlayers, qp, jqp = nc.calibrated(name, per_channel)
    assert sorted(jqp) == sorted(wl.activation_names(name) + wl.mul_names(name))
    assert all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp  # the Muls and Activations were calibrated
    x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, per_channel, mr.tracer(wl.NETWORKS[name][1], trace))
    stats = mr.nontrivial(trace)  # the expected bytes discriminate
    print({a: (d, round(s, 3)) for a, (d, s) in stats.items()})
    assert list(trace) == wl.mul_names(name) and want.shape == (batch, 10)
    nc.check_bit_exact(i8ie, net, name, x, want, fallback=True, graph=batch == 2, reload_dir=tmp_path if batch == 2 else None,
                       expect_jqp=jqp)


def test_mobilenetv3_small_cifar_bit_exact(i8ie, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    name = "mobilenetv3_small_cifar"
    net, qlayers, qp, jqp = nc.calibrated(name, False)
    assert len(wl.mul_names(name)) == 9 and all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp
    x = wl.synthetic_input(name, 2, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, False, mr.tracer(wl.NETWORKS[name][1], trace))
    print({a: (len(np.unique(g)), round(float(((q == 0) | (q == 255)).mean()), 3)) for a, (g, q, _) in trace.items()})
    assert want.shape == (2, 10)
    nc.check_bit_exact(i8ie, net, name, x, want, reload_dir=tmp_path)
