"""The quantized LayerNorm on the GPU (csrc/i8ie_layernorm.hip).  Every byte is compared against the numpy
restatement of the definition (tests/layernorm_ref.py), never against the code under test: the flat entry over every width at
which the kernel changes its lane-group size or its form, through all three kernels, aligned, offset by a byte and in place;
the statistics extremes; the bordered / re-biased NHWC entry with guard bytes; the FP32 entry against float64; the Python
surface (shapes, launch counts, calibration, save / load, graph replay) and convnext_tiny."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import attention_ref as ar
import f64_ref
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import layernorm_ref as lr
import orc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
# the widths of the issue, and -1 / 0 / +1 around every width where layernorm_u8_group doubles its lanes per row
# (lr.GROUP_WIDTHS) and where rows pass to layernorm_u8_block (lr.GROUP_MAX_C)
WIDTHS = sorted(set([1, 2, 15, 16, 17, 48, 63, 64, 65, 96, 255, 256, 257, 1024, 1025, 4099, 16384]
                    + [w + d for w in lr.GROUP_WIDTHS + [lr.GROUP_MAX_C] for d in (-1, 0, 1)]))
QP = support.NORM_QP   # s_in, s_out, zp_out, eps


ctx = support.ctx_fixture(lr)


def _kernel(Cn, fallback, offset):
    if fallback or offset % 16:
        return "layernorm_u8_direct"
    return "layernorm_u8_group" if Cn <= lr.GROUP_MAX_C else "layernorm_u8_block"


def _flat(ctx, a, dg, db, qp=QP, relu=False, fallback=False, offset=0, in_place=False):
    rows, Cn = a.shape
    s_in, _, zp_out, eps = qp
    di = abi.GuardedU8(ctx, (rows * Cn + offset,))
    host = np.concatenate([np.zeros(offset, np.uint8), a.ravel()])
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, di.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
    do = di if in_place else abi.GuardedU8(ctx, (rows * Cn + offset,))
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_layernorm_u8(ctx.h, di.ptr.value + offset, do.ptr.value + offset, rows, Cn, dg.ptr, db.ptr, s_in, eps,
                                              1 if relu else 0, zp_out))
    finally:
        ctx.set_force_fallback(False)
    raw = do.get()
    assert do.guards_ok() and di.guards_ok()
    assert (raw[:offset] == (0 if in_place else 0xC3)).all()   # the bytes in front of an offset result are untouched
    assert names == {_kernel(Cn, fallback, offset): 1}, (names, Cn, fallback, offset)
    di.free()
    if not in_place:
        do.free()
    return raw[offset:].reshape(rows, Cn)


@pytest.mark.parametrize("Cn", WIDTHS)
def test_flat_rows_every_width_all_kernels(ctx, Cn):
    rng = np.random.default_rng(500 + Cn)
    gamma, beta, dg, db = support.norm_params(ctx, Cn, Cn)
    spread = set()
    for rows in (1, 3, 67):
        a = rng.integers(0, 256, (rows, Cn), dtype=np.uint8)
        if rows > 1:
            a[1] = (rng.integers(0, 9, Cn) + 60).astype(np.uint8)   # a narrow row
        for relu in (False, True):
            want = lr.layer_norm_u8(a, QP[0], QP[3], gamma, beta, QP[1], QP[2], relu)
            spread |= set(np.unique(want).tolist())
            for fallback, offset, in_place in ((False, 0, False), (False, 0, True), (True, 0, False), (True, 0, True), (False, 1, False),
                                               (False, 1, True)):
                got = _flat(ctx, a, dg, db, relu=relu, fallback=fallback, offset=offset, in_place=in_place)
                assert np.array_equal(got, want), (Cn, rows, relu, fallback, offset, in_place, np.argwhere(got != want)[:4])
    assert Cn <= 2 or len(spread) > 40
    dg.free(); db.free()


@pytest.mark.parametrize("name,a", lr.extreme_rows(), ids=[n for n, _ in lr.extreme_rows()])
def test_statistics_extremes_on_the_device(ctx, name, a):
    Cn = a.shape[1]
    for qp in (QP, (f32(0.1), f32(0.05), 100, f32(1e-6))):
        gamma, beta, dg, db = support.norm_params(ctx, Cn, 7 + Cn, qp)
        want = lr.layer_norm_u8(a, qp[0], qp[3], gamma, beta, qp[1], qp[2])
        for fallback in (False, True):
            got = _flat(ctx, a, dg, db, qp=qp, fallback=fallback)
            assert np.array_equal(got, want), (name, fallback, np.argwhere(got != want)[:4])
        dg.free(); db.free()


def test_direct_kernel_grid_strides(ctx):
    """the direct kernel's grid holds at most DIRECT_ROWS_PER_PASS lanes: one row more makes lane 0 walk a second row.  (The
    group and block kernels launch one group / block per row and do not stride.)"""
    rows, Cn = lr.DIRECT_ROWS_PER_PASS + 1, 2
    a = np.random.default_rng(1).integers(0, 256, (rows, Cn), dtype=np.uint8)
    gamma, beta, dg, db = support.norm_params(ctx, Cn, 3)
    gamma[:] = (1.5, -0.75)
    g, b = lr.affine(gamma, beta, QP[1], QP[2])
    dg.free(); db.free()
    dg, db = ctx.put(g), ctx.put(b)
    want = lr.layer_norm_u8(a, QP[0], QP[3], gamma, beta, QP[1], QP[2])
    got = _flat(ctx, a, dg, db, fallback=True)
    assert np.array_equal(got, want) and len(np.unique(want)) >= 3
    dg.free(); db.free()


@pytest.mark.parametrize("Cn", [16, 20, 35])
def test_nhwc_borders_rebias_relu_and_guards(ctx, Cn):
    rng = np.random.default_rng(40 + Cn)
    n, h, w = 2, 3, 5
    s_in, s_out, zp_out, eps = QP
    gamma, beta, dg, db = support.norm_params(ctx, Cn, Cn)
    q = rng.integers(0, 256, (n, Cn, h, w), dtype=np.uint8)
    for i, (bi, bo, in_s8, out_s8, relu) in enumerate(itertools.product((0, 1, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1))):
        fallback = bool(i % 3 == 2)
        want = lr.layer_norm_u8_nchw(q, s_in, eps, gamma, beta, s_out, zp_out, bool(relu))
        phys_in = rng.integers(0, 256, (n, h + 2 * bi, w + 2 * bi, Cn), dtype=np.uint8)   # a garbage border: it is never read
        phys_in[:, bi:bi + h, bi:bi + w, :] = q.transpose(0, 2, 3, 1) ^ np.uint8(0x80 if in_s8 else 0)
        ring = np.uint8(zp_out ^ (0x80 if out_s8 else 0))
        phys_out = np.full((n, h + 2 * bo, w + 2 * bo, Cn), ring, np.uint8)   # as i8ie_fill_border_u8 leaves it
        expect = phys_out.copy()
        expect[:, bo:bo + h, bo:bo + w, :] = want.transpose(0, 2, 3, 1) ^ np.uint8(0x80 if out_s8 else 0)
        di, do = abi.GuardedU8(ctx, phys_in.shape), abi.GuardedU8(ctx, phys_out.shape)
        for d, host in ((di, phys_in), (do, phys_out)):
            abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, d.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
        ctx.set_force_fallback(fallback)
        try:
            with ctx.launch_map() as names:
                abi.ck(abi.lib().i8ie_layernorm_u8_nhwc(ctx.h, di.ptr, bi, in_s8, do.ptr, bo, out_s8, n, Cn, h, w, dg.ptr, db.ptr, s_in, eps,
                                                       relu, zp_out))
        finally:
            ctx.set_force_fallback(False)
        got = do.get()
        assert do.guards_ok() and di.guards_ok() and np.array_equal(di.get(), phys_in)
        assert names == {"layernorm_u8_direct" if fallback else "layernorm_u8_group": 1}, names
        assert np.array_equal(got, expect), (Cn, bi, bo, in_s8, out_s8, relu, fallback, np.argwhere(got != expect)[:4])
        di.free(); do.free()
    dg.free(); db.free()


def test_argument_errors_launch_nothing(ctx):
    buf = ctx.put(np.zeros(4096, np.uint8))
    p = buf.ptr.value
    with ctx.launch_map() as names:
        for Cn, s_in, eps in ((0, 0.1, 1e-5), (16385, 0.1, 1e-5), (16, 0.0, 1e-5), (16, float("nan"), 1e-5), (16, 0.1, 0.0), (16, 0.1, float("inf"))):
            assert abi.lib().i8ie_layernorm_u8(ctx.h, p, p, 4, Cn, p + 1024, p + 2048, s_in, eps, 0, 0) == -1
            assert abi.lib().i8ie_layernorm_u8_nhwc(ctx.h, p, 0, 0, p, 0, 0, 1, Cn, 2, 2, p + 1024, p + 2048, s_in, eps, 0, 0) == -1
        assert abi.lib().i8ie_layernorm_u8(ctx.h, None, p, 4, 16, p + 1024, p + 2048, 0.1, 1e-5, 0, 0) == -1
        assert abi.lib().i8ie_layernorm_u8_nhwc(ctx.h, p, -1, 0, p, 0, 0, 1, 16, 2, 2, p + 1024, p + 2048, 0.1, 1e-5, 0, 0) == -1
    assert names == {}
    buf.free()


@pytest.mark.parametrize("Cn", [1, 17, 96, 1025])
def test_f32_against_float64(ctx, Cn):
    """bound: layernorm_ref.layer_norm_f32_bound, derived from C and the roundings of the fp32 sequence"""
    rng = np.random.default_rng(70 + Cn)
    x = rng.normal(0.3, 2.0, (5, Cn)).astype(f32)
    x[1] = 2.5   # a constant row: var = 0, out = beta
    gamma, beta = rng.normal(1, 0.5, Cn).astype(f32), rng.normal(0, 0.5, Cn).astype(f32)
    dg, db = ctx.put(gamma), ctx.put(beta)
    for inner in (1, 5):   # flat rows; the same values laid out [1, C, 5] (an NCHW tensor normalised over c)
        src = x if inner == 1 else np.ascontiguousarray(x.T)
        di, do = ctx.put(src), ctx.guarded(src.shape)
        abi.ck(abi.lib().i8ie_layernorm_f32(ctx.h, di.ptr, do.ptr, 5, Cn, dg.ptr, db.ptr, 1e-5, inner))
        got, ok = do.read()
        assert ok and abi.GuardedOut.unwritten(got) == 0
        got = got if inner == 1 else got.T
        err = np.abs(got.astype(np.float64) - lr.layer_norm_f64(x, gamma, beta, 1e-5))
        bound = lr.layer_norm_f32_bound(x, gamma, beta, 1e-5)
        print("layernorm_f32 C=%d inner=%d: max err %.3g, max err / bound %.3g" % (Cn, inner, err.max(), (err / bound).max()))
        assert (err <= bound).all()
        di.free(); do.free()
    dg.free(); db.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def _ln(i8ie, c, seed, qp, eps=1e-5):
    rng = np.random.default_rng(seed)
    L = i8ie.LayerNorm(c, eps)
    w, b = rng.uniform(0.5, 1.5, c).astype(f32), rng.uniform(-0.3, 0.3, c).astype(f32)
    L.load_weight(w)
    L.load_bias(b)
    L.set_output_qparams(*qp)
    L.convert()
    return L, w, b


def test_surface_shapes_and_errors(i8ie):
    rng = np.random.default_rng(80)
    w, b = rng.uniform(0.5, 1.5, 12).astype(f32), rng.uniform(-0.3, 0.3, 12).astype(f32)
    for shape in ((2, 12, 3, 4), (5, 12), (2, 5, 12)):
        xf = rng.uniform(-3, 3, shape).astype(f32)
        q = i8ie.quantize(i8ie.tensor(xf), 0.025, 127)
        qv = q.numpy()
        r = i8ie.relu(i8ie.layer_norm(q, w, b, 1e-5, 0.02, 120))
        assert r.shape == shape and r.scale == pytest.approx(0.02) and r.zero_point == 120
        assert np.array_equal(r.numpy(), lr.layer_norm_any(qv, f32(0.025), f32(1e-5), w, b, f32(0.02), 120, True)), shape
        r = i8ie.layer_norm(q, scale=0.02, zero_point=120)   # weight, bias default to ones, zeros
        assert np.array_equal(r.numpy(), lr.layer_norm_any(qv, f32(0.025), f32(1e-5), np.ones(12, f32), np.zeros(12, f32), f32(0.02), 120))
        got = i8ie.layer_norm(i8ie.tensor(xf), w, b).numpy()
        rows = xf.transpose(0, 2, 3, 1) if len(shape) == 4 else xf
        want, bound = lr.layer_norm_f64(rows, w, b, 1e-5), lr.layer_norm_f32_bound(rows, w, b, 1e-5)
        got_rows = got.transpose(0, 2, 3, 1) if len(shape) == 4 else got
        assert got.shape == shape and (np.abs(got_rows - want) <= bound).all()
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 12, 3, 4)).astype(f32)), 0.025, 127)
    ln = i8ie.LayerNorm(12)
    ln11, _, _ = _ln(i8ie, 11, 1, (0.02, 1))
    bad = [lambda: ln(q),                                                     # not converted
           lambda: ln11(q),                                                   # c != channels
           lambda: ln11(q.reshape(6, 48)),                                    # f != channels
           lambda: i8ie.layer_norm(q.reshape(-1), None, None, 1e-5, 0.02, 1),           # rank 1
           lambda: i8ie.layer_norm(q.reshape(1, 2, 12, 3, 4), None, None, 1e-5, 0.02, 1),   # rank 5
           lambda: i8ie.layer_norm(q, w[:11], b, 1e-5, 0.02, 1),
           lambda: i8ie.layer_norm(q, w, b, 0.0, 0.02, 1),
           lambda: i8ie.layer_norm(q, w, b, 1e-5, 0.0, 1),
           lambda: i8ie.layer_norm(q, w, b, 1e-5, 0.02, 256),
           lambda: i8ie.LayerNorm(11)(i8ie.tensor(np.zeros((2, 12), f32)))]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    for kw in ({}, {"scale": 0.2}, {"zero_point": 3}):
        with pytest.raises(TypeError):
            i8ie.layer_norm(q, w, b, **kw)


def test_launch_counts_borders_and_bytes(i8ie):
    """conv -> LN -> padded conv is three launches (the LN reads the conv's NHWC result as it lies and writes the border and
    re-bias the next conv asks for); one LN feeding three 1x1 convs is four; nothing converts a layout, re-biases or fills a
    border in between"""
    rng = np.random.default_rng(90)
    n, c, h, w = 3, 16, 6, 5   # (16 channels: the convs keep the engine's NHWC layout, as in tests/test_gpu_attention.py)
    stem0 = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128))
    stem1 = support.conv(i8ie, c, c, 3, 1, 11, (0.05, 128))
    stem = support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    ln, gam, bet = _ln(i8ie, c, 2, (0.02, 125))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    proj = [support.conv(i8ie, c, 16, 1, 0, sd, (0.06, 120 + sd)) for sd in (3, 4, 6)]
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, 3, h, w)).astype(f32)), 0.025, 127)
    # (two convs in front: the second one's result is an activation in the engine's layout, as in tests/test_gpu_mul.py)
    x = i8ie.relu(stem1(i8ie.relu(stem0(q))))

    launches = support.counted(lambda: [tail(i8ie.relu(ln(stem(x))))])
    print(launches)
    assert launches.get("layernorm_u8_group") == 1 and sum(launches.values()) == 3, launches
    y = stem(x)
    launches3 = support.counted(lambda: (lambda t: [p(t) for p in proj])(ln(y)))
    print(launches3)
    assert launches3.get("layernorm_u8_group") == 1 and sum(launches3.values()) == 4, launches3
    for k in list(launches) + list(launches3):
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), (launches, launches3)
    xv = x.numpy()
    yv = support.conv_ref(stem, xv, 0.05, 128, pad=1)
    lv = lr.layer_norm_u8_nchw(yv, f32(0.05), f32(1e-5), gam, bet, f32(0.02), 125)
    assert len(np.unique(lv)) > 40
    assert np.array_equal(ln(stem(x)).numpy(), lv)
    assert np.array_equal(tail(i8ie.relu(ln(stem(x)))).numpy(), support.conv_ref(tail, np.maximum(lv, 125), 0.02, 125, pad=1))
    t = ln(y)
    for p in proj:
        assert np.array_equal(p(t).numpy(), support.conv_ref(p, lv, 0.02, 125))
    # an NCHW input (user-made) goes through one layout conversion
    qn = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, c, h, w)).astype(f32)), 0.025, 127)
    qv = qn.numpy()
    assert np.array_equal(ln(qn).numpy(), lr.layer_norm_u8_nchw(qv, f32(0.025), f32(1e-5), gam, bet, f32(0.02), 125))


def test_calibrated_like_a_layer_round_trips_and_replays(i8ie, tmp_path):
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, (5, 20, 4, 3)).astype(f32)
    w, b = rng.uniform(0.5, 1.5, 20).astype(f32), rng.uniform(-0.3, 0.3, 20).astype(f32)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.norm1 = i8ie.LayerNorm(20)

        def forward(self, x):
            return self.norm1(x)

    cx.set_calibration_mode("host")
    cx.set_calibration_seed(7)
    try:
        net = Net()
        net.load({"norm1.weight": w, "norm1.bias": b})
        net.prepare()
        got = net(i8ie.tensor(a)).numpy()
        net.convert(per_channel=True)   # (accepted and ignored)
        want = tuple(cx.calibrator_range([got.ravel()], 1.0))
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    rows = a.transpose(0, 2, 3, 1)
    assert (np.abs(got.transpose(0, 2, 3, 1) - lr.layer_norm_f64(rows, w, b, 1e-5)) <= lr.layer_norm_f32_bound(rows, w, b, 1e-5)).all()
    assert net.norm1.layer.is_quantized() and net.norm1.output_qparams() == want and want[0] != 1.0 and not net.norm1.is_per_channel()
    sd = net.quantized_state_dict()
    assert list(sd) == ["norm1.weight", "norm1.bias", "norm1.qparams"]
    assert sd["norm1.weight"].dtype == np.float32 and np.array_equal(sd["norm1.weight"], w) and np.array_equal(sd["norm1.bias"], b)
    assert sd["norm1.qparams"].tolist() == [0.0, want[0], float(want[1])]
    path = str(tmp_path / "ln.npz")
    net.save_quantized(path)
    other = Net()
    other.load_quantized_file(path)
    assert other.norm1.output_qparams() == want and other.is_quant
    x = rng.normal(0.2, 1.5, (5, 20, 4, 3)).astype(f32)
    r1, r2 = net(i8ie.tensor(x)).numpy(), other(i8ie.tensor(x)).numpy()
    qx = orc.quantize(x, sr.pipeline.INPUT_SCALE, sr.pipeline.INPUT_ZP)
    ref = orc.dequantize(lr.layer_norm_u8_nchw(qx, sr.pipeline.INPUT_SCALE, f32(1e-5), w, b, f32(want[0]), want[1]), f32(want[0]), want[1])
    assert np.array_equal(r1.view(np.uint32), ref.view(np.uint32)) and np.array_equal(r2.view(np.uint32), ref.view(np.uint32))
    # set_output_qparams on a converted layer re-derives g and b
    other.norm1.set_output_qparams(0.05, 99)
    ref2 = orc.dequantize(lr.layer_norm_u8_nchw(qx, sr.pipeline.INPUT_SCALE, f32(1e-5), w, b, f32(0.05), 99), f32(0.05), 99)
    assert np.array_equal(other(i8ie.tensor(x)).numpy().view(np.uint32), ref2.view(np.uint32))
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy().view(np.uint32), ref.view(np.uint32))


# ---- convnext_tiny ----------------------------------------------------------------------------------------------------------
NAME = "convnext_tiny"


def _tracer(layers, into):
    """every LayerNorm's bytes, the attention block's scores, softmax and result, and every block's Add"""
    return sr.traces(lr.tracer(layers, into), ar.tracer(into), sr.outputs_of("add", into))


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_convnext_tiny_bit_exact(i8ie, batch, per_channel, tmp_path):
    import net_cases as nc
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = nc.calibrated(NAME, per_channel, calib_images=8)
    both = dict(qp, **jqp)
    assert all(s > 0 and s != 1.0 for s, _ in both.values()), both   # every layer, LayerNorm and join was calibrated
    entry = wl.network(NAME)
    x = wl.synthetic_input(NAME, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(entry, x, qlayers, qp, jqp, per_channel, _tracer(entry[0], trace))
    assert want.shape == (batch, 10) and len(np.unique(want)) > 1
    for k in ("stem_ln", "a_ln", "down_ln", "b_ln", "t_ln"):
        assert len(np.unique(trace[k])) >= 32 and ((trace[k] == 0) | (trace[k] == 255)).mean() < 0.05, k
    nc.check_bit_exact(i8ie, net, NAME, x, want, fallback=True, graph=True, reload_dir=tmp_path, expect_jqp=both)
    mine = {}
    nc.traced(i8ie, net, NAME, x, _tracer(entry[0], mine))
    assert sorted(mine) == sorted(trace) == sorted(["stem_ln", "a_ln", "down_ln", "b_ln", "t_ln", "head_ln", "a_add", "b_add", "t_add",
                                                    "t_scores", "t_softmax", "t_block"])
    for k in trace:
        assert mine[k].shape == trace[k].shape and np.array_equal(mine[k], trace[k]), k


def test_convnext_tiny_launches(i8ie):
    """six LayerNorms, one launch each: five on NHWC activations, one on [n, 20] rows"""
    import _CXX_i8ie as cx
    import net_cases as nc
    from int8inferenceengine_amd import workloads as wl

    net = nc.calibrated(NAME, False, calib_images=8)[0]
    x = wl.synthetic_input(NAME, 5, seed=sr.INPUT_SEED)
    net(i8ie.tensor(x)).numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        net(i8ie.tensor(x)).numpy()
    finally:
        prof = cx.profile_stop()
    launches = {}
    for k, v in prof.items():
        launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0]
    print(launches)
    assert launches.get("layernorm_u8_group") == 6 and "layernorm_u8_direct" not in launches, launches
