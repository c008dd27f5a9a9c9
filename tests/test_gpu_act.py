"""Table-driven quantized activations on the GPU (csrc/i8ie_lut.hip).  Every comparison is against the
numpy restatement of the definition (tests/act_ref.py), never against the code under test: all 256 bytes at every channel
position through both u8 entries, the bordered / re-biased NHWC entry over every byte of the physical result with guard bands,
the flat form at ragged lengths and alignments, the FP32 entry, the Python surface, launch counts, graph replay, calibration,
and the three networks end to end."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import act_ref as ar
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = sorted(ar.KINDS, key=ar.KINDS.get)


ctx = support.ctx_fixture(ar)


SENTINEL = 0x3C  # what the result's border holds before the call (no table below is the constant 0x3C everywhere)


def _run_nhwc(ctx, q, tab, in_border, in_s8, out_border, out_s8):
    """Returns (every byte of the physical result, the bytes expected there, guards untouched?).  The result's buffer starts
    with SENTINEL in the border and 0xC3 in the interior, as they lie (so a re-biased result holds them un-flipped)."""
    n, c, h, w = q.shape
    src = support.phys_nhwc(q, in_border, 0x11, in_s8)
    dev = ctx.put(src)
    start = support.phys_nhwc(np.full((n, c, h, w), 0xC3, np.uint8), out_border, SENTINEL, False)
    out = abi.GuardedU8(ctx, start.shape, fill=start.ravel())
    ptr, keep = ar.host_table(tab)
    try:
        abi.ck(abi.lib().i8ie_lut_u8_nhwc(ctx.h, dev.ptr, in_border, in_s8, out.ptr, out_border, out_s8, n, c, h, w, ptr))
        got = out.get()
        ok = out.guards_ok()
        assert np.array_equal(dev.get(), src), "the input was written"
    finally:
        out.free()
        dev.free()
    want = start.copy()
    inner = np.asarray(tab, np.uint8)[q].transpose(0, 2, 3, 1)
    want[:, out_border:out_border + h, out_border:out_border + w, :] = inner ^ np.uint8(0x80) if out_s8 else inner
    del keep
    return got, want, ok


def _run_flat(ctx, q, tab, in_off=0, out_off=0, in_place=False):
    """i8ie_lut_u8 over q's bytes, the buffers `in_off` / `out_off` bytes past an aligned address; (result, guards untouched?)"""
    q = np.ascontiguousarray(q, np.uint8).ravel()
    ptr, keep = ar.host_table(tab)
    if in_place:
        out = abi.GuardedU8(ctx, (q.size + in_off,), fill=np.concatenate([np.full(in_off, 0xC3, np.uint8), q]))
        src_ptr = dst_ptr = C.c_void_p(out.ptr.value + in_off)
        dev, off = None, in_off
    else:
        dev = ctx.put(np.concatenate([np.zeros(in_off, np.uint8), q]))
        out = abi.GuardedU8(ctx, (q.size + out_off,))
        src_ptr, dst_ptr, off = C.c_void_p(dev.ptr.value + in_off), C.c_void_p(out.ptr.value + out_off), out_off
    try:
        abi.ck(abi.lib().i8ie_lut_u8(ctx.h, src_ptr, dst_ptr, q.size, ptr))
        got = out.get()
        ok = out.guards_ok() and bool((got[:off] == 0xC3).all())
    finally:
        out.free()
        if dev is not None:
            dev.free()
    del keep
    return got[off:], ok


# ---- exhaustive arithmetic ---------------------------------------------------------------------------------------------
def _tables():
    a = np.arange(256, dtype=np.uint8)
    tabs = [("identity", a), ("reverse", (255 - a).astype(np.uint8)), ("permutation", np.random.default_rng(20261018).permutation(256).astype(np.uint8)),
            ("constant", np.full(256, 77, np.uint8))]
    sets = [(f32(0.05), 128, f32(0.0234375), 3), (f32(0.11), 40, f32(1.0 / 255), 0), (f32(0.02), 255, f32(0.004), 200)]
    for kind in KINDS:
        for i, (s_in, zp_in, s_out, zp_out) in enumerate(sets):
            tabs.append(("%s_%d" % (kind, i), ar.table(kind, 0.1 if kind == "leaky_relu" else 0.0, s_in, zp_in, s_out, zp_out)))
    return tabs


TABLES = _tables()


@pytest.mark.parametrize("entry", ["flat", "nhwc"])
@pytest.mark.parametrize("case", list(enumerate(TABLES)), ids=[t[0] for t in TABLES])
def test_exhaustive_bytes(ctx, case, entry):
    i, (name, tab) = case
    c = (16, 4, 3)[i % 3]
    q = support.byte_image(c)
    want = tab[q]
    if entry == "flat":
        got, ok = _run_flat(ctx, q, tab)
        got = got.reshape(want.shape)
    else:  # bordered and re-biased buffers: the NHWC kernel proper
        ib, ob, ix, ox = (i + 1) % 3, 1 + i % 2, i % 2, (i // 2) % 2
        got, wantp, ok = _run_nhwc(ctx, q, tab, ib, ix, ob, ox)
        assert np.array_equal(got, wantp)
        got = (got ^ np.uint8(0x80) if ox else got)[:, ob:ob + 16, ob:ob + 16, :].transpose(0, 3, 1, 2)
    bad = np.argwhere(got != want)  # all 256 bytes at every channel position
    assert ok and got.shape == want.shape == (1, c, 16, 16) and bad.size == 0, (name, bad[:8])


@pytest.mark.parametrize("c", [1, 3, 4, 16, 20, 35])
def test_layout_matrix(ctx, c):
    """every (in border, out border, in re-biased, out re-biased): only the interior of the result changes; the sentinel border
    and the guard bands stay as they were"""
    rng = np.random.default_rng(100 + c)
    q = rng.integers(0, 256, (2, c, 5, 7), dtype=np.uint8)
    tab = ar.table("hardswish", 0.0, f32(0.04), 120, f32(0.031), 13)
    assert len(np.unique(tab)) > 40
    for ib, ob, ix, ox in itertools.product((0, 1, 2), (0, 1, 2), (0, 1), (0, 1)):
        got, want, ok = _run_nhwc(ctx, q, tab, ib, ix, ob, ox)
        assert ok and np.array_equal(got, want), (c, ib, ob, ix, ox, np.argwhere(got != want)[:6])


SECOND_TRIP = ar.MAX_BLOCKS * ar.THREADS * ar.VEC + 3 * ar.VEC + 5  # 16-byte items: three lanes go round again, then a tail


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4101, SECOND_TRIP])
def test_flat_form(ctx, n):
    rng = np.random.default_rng(n % 9973)
    q = rng.integers(0, 256, n, dtype=np.uint8)
    tab = rng.permutation(256).astype(np.uint8)
    want = tab[q]
    offsets = [(0, 0), (1, 1), (3, 3), (1, 3), (0, 1), (4, 4), (4, 0), (3, 0)] if n != SECOND_TRIP else [(0, 0), (4, 4), (1, 3)]
    for in_off, out_off in offsets:
        got, ok = _run_flat(ctx, q, tab, in_off, out_off)
        assert ok and np.array_equal(got, want), (n, in_off, out_off, np.flatnonzero(got != want)[:6])
    for off in (0, 1, 3, 4):
        got, ok = _run_flat(ctx, q, tab, off, in_place=True)
        assert ok and np.array_equal(got, want), (n, off, "in place")


# ---- the FP32 entry ------------------------------------------------------------------------------------------------------
def _f32_inputs():
    rng = np.random.default_rng(5)
    special = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754944e-38, -3, 0, 3, 6, -6, np.nextafter(f32(-3), f32(0)),
               np.nextafter(f32(3), f32(4)), np.nextafter(f32(6), f32(0)), 3.4e38, -3.4e38, 88.7, -88.7, 103.9, -103.9, 20.0, -20.0]
    x = np.concatenate([np.array(special, f32), rng.normal(0, 3, 4000).astype(f32), rng.uniform(-9, 9, 97).astype(f32),
                        (rng.normal(0, 1, 500) * 1e-3).astype(f32)])
    return x


def _run_f32(ctx, kind, param, x):
    dev = ctx.put(x)
    out = abi.GuardedOut(ctx, x.shape)
    try:
        abi.ck(abi.lib().i8ie_activation_f32(ctx.h, ar.KINDS[kind], float(param), dev.ptr, out.ptr, x.size))
        got, ok = out.read()
    finally:
        out.free()
        dev.free()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    return got


@pytest.mark.parametrize("kind,param", [("relu6", 0.0), ("leaky_relu", 0.1), ("leaky_relu", -0.5), ("leaky_relu", 0.0), ("hardsigmoid", 0.0),
                                        ("hardswish", 0.0)])
def test_fp32_entry_is_the_restatement_bit_for_bit(ctx, kind, param):
    x = _f32_inputs()
    got, want = _run_f32(ctx, kind, param, x), ar.act_f32(kind, x, param)
    nan = np.isnan(want)  # (hardswish(-inf) = -inf * 0: a NaN on both sides, whose sign and payload are the machine's)
    assert np.array_equal(np.isnan(got), nan) and int(nan.sum()) <= 1
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (kind, x[bad[:6]], got[bad[:6]], want[bad[:6]])


# Documented maximum error of the double-precision device functions the kernel calls (ROCm HIP math API reference,
# double-precision table): exp 1 ULP, tanh 1 ULP.
EXP_ULP, TANH_ULP = 1, 1


@pytest.mark.parametrize("kind", ["sigmoid", "tanh"])
def test_fp32_entry_sigmoid_and_tanh_within_the_documented_bound(ctx, kind):
    """y = (float)g(double x).  In double: exp / tanh within its documented ULPs of the true value; sigmoid's sum and quotient
    round once each (half an ULP each, taken as one each here).  Then one rounding to float: at most one float32 ULP (DESIGN.md
    section 8f).  The float64 yardstick's own error (numpy's libm, under 1 ULP of a double) is covered by one more double ULP."""
    x = _f32_inputs()
    got = _run_f32(ctx, kind, 0.0, x).astype(np.float64)
    want = ar.act_f64(kind, x.astype(np.float64))
    ulps64 = (EXP_ULP + 2 if kind == "sigmoid" else TANH_ULP) + 1
    bound = np.spacing(np.abs(want).astype(f32)).astype(np.float64) + ulps64 * np.spacing(np.abs(want))
    err = np.abs(got - want)
    print(kind, "largest error in float32 ULPs: %.3f" % float((err / np.spacing(np.abs(want).astype(f32))).max()))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (kind, x[bad[:6]], got[bad[:6]], want[bad[:6]])


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_surface(i8ie, tmp_path):
    rng = np.random.default_rng(11)
    x = rng.uniform(-2, 2, (2, 16, 8, 8)).astype(f32)
    conv = support.conv(i8ie, 16, 20, 3, 1, 5, (0.05, 120))
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)          # NCHW bytes
    qv = q.numpy()
    yv = conv(q).numpy()
    assert len(np.unique(yv)) > 60
    srcs = {"nchw": (lambda: q, qv, f32(0.025), 127), "conv": (lambda: conv(q), yv, f32(0.05), 120)}  # (the conv result still pending)
    for kind, (src, (make, v, s, zp)), relu in itertools.product(KINDS, srcs.items(), (False, True)):
        param = 0.2 if kind == "leaky_relu" else None
        s_out, zp_out = (0.03, 100) if kind in ("leaky_relu", "hardswish") else (0.02, 30)
        r = i8ie.activation(make(), kind, s_out, zp_out, param=param)
        if relu:
            r = i8ie.relu(r)
        assert r.shape == v.shape and r.scale == pytest.approx(s_out) and r.zero_point == zp_out
        want = ar.act_u8(v, kind, param or 0.0, s, zp, f32(s_out), zp_out, relu)
        assert np.array_equal(r.numpy(), want), (kind, src, relu)
    # 2-D rows, one the flatten of an NHWC activation; a user table
    tab = rng.permutation(256).astype(np.uint8)
    for t, v in ((q.reshape(2, -1), qv), (conv(q).reshape(2, -1), yv)):
        r = i8ie.lut(t, tab, 0.5, 9)
        assert r.shape == (2, v.size // 2) and (r.scale, r.zero_point) == (0.5, 9) and np.array_equal(r.numpy(), tab[v.reshape(2, -1)])
        r = i8ie.relu(i8ie.lut(t, tab, 0.5, 9))
        assert np.array_equal(r.numpy(), np.maximum(tab[v.reshape(2, -1)], 9))
    assert np.array_equal(i8ie.lut(conv(q), tab, 0.5, 9).numpy(), tab[yv])
    # FP32: f itself
    t = i8ie.tensor(x)
    assert np.array_equal(i8ie.activation(t, "hardswish").numpy().view(np.uint32), ar.act_f32("hardswish", x).view(np.uint32))
    assert np.array_equal(i8ie.activation(t, "leaky_relu", param=0.3).numpy().view(np.uint32), ar.act_f32("leaky_relu", x, 0.3).view(np.uint32))
    with pytest.raises(TypeError):
        i8ie.activation(q, "tanh")
    with pytest.raises(TypeError):
        i8ie.activation(t, "tanh", 0.5, 3)
    with pytest.raises(RuntimeError):
        i8ie.activation(q, "tanh", 0.5, 256)
    with pytest.raises(RuntimeError):
        i8ie.activation(q, "tanh", 0.0, 3)
    with pytest.raises(RuntimeError):
        i8ie.Activation("tanh")(q)                         # not converted

    # the layer: FP32 before convert(), the table after it, `<attr>.qparams` only in the state dict
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.act1 = i8ie.Activation("hardsigmoid")

        def forward(self, x):
            return self.act1(x)

    net = Net()
    assert np.array_equal(net(t).numpy().view(np.uint32), ar.act_f32("hardsigmoid", x).view(np.uint32))
    net.prepare()
    net.act1.set_output_qparams(1 / 255, 0)
    net(t)
    net.convert()
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["act1.qparams"] and sd["act1.qparams"].tolist() == [0.0, float(f32(1 / 255)), 0.0]
    path = str(tmp_path / "act.npz")
    net.save_quantized(path)
    fresh = Net()
    fresh.load_quantized_file(path)
    assert fresh.is_quant and fresh.act1.output_qparams() == net.act1.output_qparams()
    want_q = ar.act_u8(qv, "hardsigmoid", 0.0, f32(0.025), 127, f32(1 / 255), 0)
    want = (want_q.astype(np.int32).astype(f32) * f32(1 / 255)).astype(f32)
    for m in (net, fresh):
        assert np.array_equal(m(t).numpy().view(np.uint32), want.view(np.uint32))


def _counted_luts(forward):
    """(the output, (lookup launches, all other launches, {name: launches})) of the second of two equal forwards"""
    first, again, launches = support.counted_forward(forward)
    assert np.array_equal(again, first)
    return first, support.split_launches(launches, "lut_u8")


def test_launch_counts(i8ie):
    """conv_c(act(conv_a(x))): two conv launches and ONE lookup launch -- the padded conv_c gets its border (and re-biased
    bytes, where it reads them) from the lookup kernel; relu(act(x)) is one launch: the relu is folded into the table."""
    conv_a = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    conv_c = support.conv(i8ie, 16, 16, 3, 1, 6, (0.08, 90))
    act = i8ie.Activation("hardswish")
    act.set_output_qparams(0.04, 25)
    act.convert()
    xin = np.random.default_rng(4).uniform(-2, 2, (2, 3, 8, 8)).astype(f32)
    # an activation in the engine's layout that stays recorded (as in tests/test_gpu_add.py): the warm-up forward launches it
    # once, with the border its consumer asks for, and the counted forward finds that result
    q = i8ie.relu(support.conv(i8ie, 16, 16, 3, 1, 8, (0.05, 125))(i8ie.relu(support.conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))(
        i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))))

    got, (luts, others, launches) = _counted_luts(lambda: conv_c(act(conv_a(q))))
    print(launches)
    assert luts == 1 and others == 2, launches
    av = conv_a(q).numpy()
    mid = ar.act_u8(av, "hardswish", 0.0, f32(0.05), 120, f32(0.04), 25)
    assert np.array_equal(act(conv_a(q)).numpy(), mid) and len(np.unique(mid)) > 30
    want, _ = gr.conv2d_grouped(mid, conv_c.layer.q_weight(), conv_c.layer.q_bias(), 1, 1, 1, f32(0.04), 25,
                                conv_c.weight_scale(), f32(0.08), 90)
    assert np.array_equal(got, want)

    a = conv_a(q)
    a.data.layout()
    got, (luts, others, launches) = _counted_luts(lambda: i8ie.relu(act(a)))
    print(launches)
    assert luts == 1 and others == 0, launches
    assert np.array_equal(got, np.maximum(mid, 25))


@pytest.mark.parametrize("mode", ["host", "device"])
def test_activation_is_calibrated_like_a_layer(i8ie, mode):
    import _CXX_i8ie as cx

    a = np.random.default_rng(8).normal(0.2, 2.5, (5, 8, 10, 10)).astype(f32)
    total = ar.act_f32("hardswish", a)
    cx.set_calibration_mode(mode)
    cx.set_calibration_seed(7)
    try:
        act = i8ie.Activation("hardswish")
        act.prepare()
        got = act(i8ie.tensor(a)).numpy()
        act.convert()
        if mode == "host":
            want = tuple(cx.calibrator_range([total.ravel()], 1.0))
        else:
            want = tuple(cx.calibrator_device_samples([total.ravel()], 7)[2:])
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert np.array_equal(got.view(np.uint32), total.view(np.uint32))
    assert act.layer.is_quantized() and act.output_qparams() == want and want[0] != 1.0
    # injected parameters win over the calibrator's
    act = i8ie.Activation("tanh")
    act.prepare()
    act.set_output_qparams(0.03, 41)
    act(i8ie.tensor(a))
    act.convert()
    assert act.output_qparams() == (float(f32(0.03)), 41)


# ---- the networks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("name", ["mobilenetv2_tiny", "act_tiny"])
def test_tiny_networks_bit_exact(i8ie, name, batch, per_channel, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = nc.calibrated(name, per_channel)
    assert sorted(jqp) == sorted(wl.activation_names(name) + wl.add_names(name))
    assert all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp
    x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, per_channel, sr.outputs_of("act", trace))
    stats = ar.nontrivial(trace)  # the expected bytes discriminate
    print({a: (d, round(s, 3)) for a, (d, s) in stats.items()})
    assert list(trace) == wl.activation_names(name) and want.shape == (batch, 10)
    more = batch == 5 and not per_channel
    # (mobilenetv2_tiny replayed as one HIP graph: the table travels in the kernel arguments)
    nc.check_bit_exact(i8ie, net, name, x, want, fallback=True, graph=more and name == "mobilenetv2_tiny",
                       reload_dir=tmp_path if more else None, expect_jqp=jqp)


def test_mobilenetv2_cifar_bit_exact(i8ie):
    from int8inferenceengine_amd import workloads as wl

    name = "mobilenetv2_cifar"
    net, qlayers, qp, jqp = nc.calibrated(name, False)
    assert len(jqp) == 35 + 10 and all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp
    x = wl.synthetic_input(name, 2, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, False, sr.outputs_of("act", trace))
    stats = ar.nontrivial(trace)
    print({a: (d, round(s, 3)) for a, (d, s) in stats.items()})
    assert want.shape == (2, 10)
    nc.check_bit_exact(i8ie, net, name, x, want)
