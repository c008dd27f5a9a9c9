"""Quantized channel concatenation on the GPU (csrc/i8ie_concat.hip).  Every comparison is byte-exact
against the numpy restatement of the definition (tests/concat_ref.py), never against the code under test: all 256 bytes at
every channel position for a range of quantisation parameters through both u8 entries, the bordered / re-biased NHWC entry
over every byte of the physical result with guard bands, the run form at ragged lengths, the FP32 entry as bit patterns,
launch counts, the Python surface, calibration, and the two fire networks end to end."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import concat_ref as cr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32


ctx = support.ctx_fixture(cr)


def _run_nhwc(ctx, inputs, borders, s8s, s_out, zp_out, relu, out_border, out_s8, same=None):
    """inputs: [(q nchw, s, zp)].  Returns (every byte of the physical result, the bytes expected there, guards untouched?).
    The result's buffer starts as i8ie_fill_border_u8 leaves it, with 0xC3 in the interior (0x43 when re-biased)."""
    n, _, h, w = inputs[0][0].shape
    ctot = sum(q.shape[1] for q, _, _ in inputs)
    devs = []
    for i, ((q, _, zp), b, x) in enumerate(zip(inputs, borders, s8s)):
        devs.append(devs[same[i]] if same and same[i] is not None else ctx.put(support.phys_nhwc(q, b, zp, x)))
    start = support.phys_nhwc(np.full((n, ctot, h, w), 0xC3, np.uint8), out_border, zp_out, False)
    start = start ^ np.uint8(0x80) if out_s8 else start
    out = abi.GuardedU8(ctx, start.shape, fill=start.ravel())
    try:
        abi.ck(cr.concat_u8_nhwc(abi.lib(), ctx.h, [d.ptr for d in devs], [q.shape[1] for q, _, _ in inputs], borders, s8s,
                                 [s for _, s, _ in inputs], [zp for _, _, zp in inputs], out.ptr, out_border, out_s8, n, h, w,
                                 s_out, zp_out, relu))
        got = out.get()
        ok = out.guards_ok()
        for (q, _, zp), b, x, d in zip(inputs, borders, s8s, devs):
            assert np.array_equal(d.get(), support.phys_nhwc(q, b, zp, x)), "an input was written"
    finally:
        out.free()
        for d in {id(d): d for d in devs}.values():
            d.free()
    want = support.phys_nhwc(cr.cat_u8(inputs, s_out, zp_out, relu), out_border, zp_out, out_s8)
    return got, want, ok


def _run_rows(ctx, inputs, s_out, zp_out, relu):
    """the run form on [outer, len_i] arrays (an NCHW tensor is [n, c_i * h * w]); the result with its guard check"""
    outer = inputs[0][0].shape[0]
    rows = [np.ascontiguousarray(q).reshape(outer, -1) for q, _, _ in inputs]
    devs = [ctx.put(r) for r in rows]
    out = abi.GuardedU8(ctx, (outer, sum(r.shape[1] for r in rows)))
    try:
        abi.ck(cr.concat_u8(abi.lib(), ctx.h, [d.ptr for d in devs], [r.shape[1] for r in rows], [s for _, s, _ in inputs],
                            [zp for _, _, zp in inputs], out.ptr, outer, s_out, zp_out, relu))
        got = out.get()
        ok = out.guards_ok()
    finally:
        out.free()
        for d in devs:
            d.free()
    return got, ok


# ---- exhaustive arithmetic ---------------------------------------------------------------------------------------------
def _arith_cases():
    so = f32(0.05)
    rng = np.random.default_rng(20261018)
    cal = [(f32(s), int(z)) for s, z in zip(rng.uniform(0.004, 0.2, 3), rng.integers(0, 256, 3))]
    kinds = [(so, 128), (so, 3), (so / f32(3), 120), (so * f32(3), 131), (so * f32(64), 128), (so / f32(64), 7), (f32(1e-40), 128), cal[0]]
    cases = [
        # (name, s_out, zp_out, [(s_i, zp_i)], [c_i])        16- and 4-byte items (offsets 0 16 32 36 40 56 64 68 of 80)
        ("kinds_wide", so, 128, kinds, [16, 16, 4, 4, 16, 8, 4, 12]),
        # the same kinds moved round by three positions, byte items (an odd total)
        ("kinds_bytes", so, 128, kinds[3:] + kinds[:3], [3, 5, 16, 1, 4, 2, 7, 1]),
        # ... and by five, all 16-byte items
        ("kinds_16", so, 128, kinds[5:] + kinds[:5], [16] * 8),
        ("calibrated", cal[1][0], cal[1][1], [cal[2], cal[0], cal[1], (cal[1][0], cal[1][1] ^ 0x55)], [16, 4, 16, 12]),
        # s_out small enough to saturate at both ends (t = d * 100 + zp), a copy in the middle
        ("saturating", f32(0.0005), 128, [(so, 128), (f32(0.0005), 128), (so, 0), (so, 255)], [16, 16, 4, 12]),
        ("denormal_everywhere", f32(0.03), 100, [(f32(1e-40), 0), (f32(1e-45), 255), (f32(0.0), 17), (f32(-0.03), 100)], [16, 4, 4, 8]),
    ]
    for zp_out in (0, 128, 255):
        qs = [(f32(0.031), 0), (f32(0.031), 128), (f32(0.031), 255), (f32(0.052), 0), (f32(0.052), 128), (f32(0.052), 255),
              (f32(0.09), zp_out)]
        cases.append(("zp_out_%d" % zp_out, f32(0.052), zp_out, qs, [16, 4, 12, 16, 16, 4, 12]))
    return cases


ARITH = _arith_cases()


@pytest.mark.parametrize("entry", ["run", "nhwc"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", ARITH, ids=[c[0] for c in ARITH])
def test_exhaustive_bytes(ctx, case, relu, entry):
    name, s_out, zp_out, qps, cs = case
    inputs = [(support.byte_image(c), s, zp) for (s, zp), c in zip(qps, cs)]
    assert any(cr.same_qparams(s, zp, s_out, zp_out) for s, zp in qps) or name == "denormal_everywhere"
    want = cr.cat_u8(inputs, s_out, zp_out, relu)
    if entry == "run":
        got, ok = _run_rows(ctx, inputs, s_out, zp_out, relu)
        got = got.reshape(want.shape)
    else:  # bordered and re-biased buffers: the NHWC kernel proper
        k = len(inputs)
        got, wantp, ok = _run_nhwc(ctx, inputs, [(i + 1) % 3 for i in range(k)], [i % 2 for i in range(k)], s_out, zp_out, relu, 1,
                                   1 if relu else 0)
        assert np.array_equal(got, wantp)
        got = (got ^ np.uint8(0x80) if relu else got)[:, 1:17, 1:17, :].transpose(0, 3, 1, 2)
    bad = np.argwhere(got != want)  # all 256 bytes at every channel position of every input
    assert ok and got.shape == want.shape == (1, sum(cs), 16, 16) and bad.size == 0, (name, bad[:8])


# ---- the layout matrix -------------------------------------------------------------------------------------------------
CHANNELS = [(16, 32), (4, 12), (3, 5), (16, 4), (1, 16), (16,), (4,) * 8, "twice"]


@pytest.mark.parametrize("cs", CHANNELS, ids=lambda c: c if isinstance(c, str) else "c" + "_".join(map(str, c)))
def test_layout_matrix(ctx, cs):
    """n = 2, 5 x 3 pixels; every buffer with border 0 / 1 / 2 and plain or re-biased, independently (all 6^(k+1) combinations
    for k <= 2 buffers, 40 drawn ones for eight inputs); EVERY byte of the physical result is compared, border included."""
    twice = cs == "twice"
    if twice:
        cs = (16, 16)
    k = len(cs)
    n, h, w = 2, 5, 3
    rng = np.random.default_rng(sum(cs) * 8 + k)
    data = [rng.integers(0, 256, (n, c, h, w), dtype=np.uint8) for c in cs]
    s_out, zp_out = f32(0.061), 97
    # input 0 is in the result's quantisation (the copy rule), the others alternate between two foreign ones
    qps = [(s_out, zp_out) if i % 3 == 0 else ((f32(0.043), 119) if i % 3 == 1 else (f32(0.0875), 131)) for i in range(k)]
    same = None
    if twice:
        data[1], qps[1], same = data[0], qps[0], [None, 0]
    inputs = [(d, s, zp) for d, (s, zp) in zip(data, qps)]
    kinds = list(itertools.product((0, 1, 2), (0, 1)))  # (border, re-biased)
    if twice:
        combos = [(a, a, o) for a in kinds for o in kinds]
    elif k <= 2:
        combos = list(itertools.product(kinds, repeat=k + 1))
    else:
        combos = [tuple(kinds[j] for j in rng.integers(0, 6, k + 1)) for _ in range(40)]
    for i, combo in enumerate(combos):
        relu = i % 2
        got, want, ok = _run_nhwc(ctx, inputs, [b for b, _ in combo[:k]], [x for _, x in combo[:k]], s_out, zp_out, relu,
                                  combo[k][0], combo[k][1], same)
        assert ok, ("guard band", combo)
        assert np.array_equal(got, want), (combo, relu, np.argwhere(got != want)[:6])


# ---- the run form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1, 15, 16, 17, 64), (16, 64, 16), (15, 17), (4, 12, 64), (64,), (17,), (1, 1, 1, 1, 1, 1, 1, 1)],
                         ids=lambda v: "len" + "_".join(map(str, v)))
def test_run_form_rows(ctx, lens):
    """[m, f_i] rows, m = 3: lengths around the item sizes; the first case's total (113) is no multiple of 4"""
    rng = np.random.default_rng(sum(lens))
    s_out, zp_out = f32(0.05), 77
    qps = [(s_out, zp_out), (f32(0.02), 130), (f32(0.11), 5)]
    inputs = [(rng.integers(0, 256, (3, f), dtype=np.uint8),) + qps[i % 3] for i, f in enumerate(lens)]
    for relu in (False, True):
        got, ok = _run_rows(ctx, inputs, s_out, zp_out, relu)
        assert ok and np.array_equal(got, cr.cat_u8(inputs, s_out, zp_out, relu)), (lens, relu)


@pytest.mark.parametrize("cs,hw", [((1, 3), (5, 3)), ((16, 1, 4), (4, 4)), ((2, 2), (1, 1)), ((5,), (3, 7))])
def test_run_form_nchw(ctx, cs, hw):
    rng = np.random.default_rng(sum(cs) + hw[0])
    s_out, zp_out = f32(0.05), 200
    qps = [(f32(0.07), 200), (s_out, zp_out), (f32(0.013), 0)]
    inputs = [(rng.integers(0, 256, (2, c) + hw, dtype=np.uint8),) + qps[i % 3] for i, c in enumerate(cs)]
    want = cr.cat_u8(inputs, s_out, zp_out, True)
    got, ok = _run_rows(ctx, inputs, s_out, zp_out, True)
    assert ok and np.array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("lens", [(1, 3, 4, 5), (4, 8), (7,), (1,) * 8])
def test_fp32_is_a_copy_bit_for_bit(ctx, lens):
    rng = np.random.default_rng(len(lens))
    parts = [rng.standard_normal((3, f)).astype(f32) for f in lens]
    bits = parts[0].view(np.uint32)
    bits[0, 0] = 0x7FC12345   # a quiet NaN with a payload
    bits[1, 0] = 0x80000000   # -0.0
    bits[2, 0] = 0xFFA00001   # a signalling NaN pattern
    parts[-1].view(np.uint32)[2, -1] = 0x00000001  # a denormal
    devs = [ctx.put(p) for p in parts]
    out = abi.GuardedU8(ctx, (3, sum(lens)), np.float32)
    try:
        abi.ck(cr.concat_f32(abi.lib(), ctx.h, [d.ptr for d in devs], list(lens), out.ptr, 3))
        got = out.get()
        ok = out.guards_ok()
    finally:
        out.free()
        for d in devs:
            d.free()
    want = np.concatenate([p.view(np.uint32) for p in parts], axis=1)
    assert ok and np.array_equal(got.view(np.uint32), want)


def test_error_paths_reach_no_kernel(ctx):
    """with a live context: every refused call returns I8IE_ERR_ARG (-1) and leaves the result buffer as it was"""
    lib = abi.lib()
    a = ctx.put(np.zeros((1, 2, 2, 16), np.uint8))
    out = abi.GuardedU8(ctx, (1, 2, 2, 32))
    before = out.get()
    nan = float("nan")

    def nhwc(ins=None, k=2, b_in=(0, 0), ob=0, s_in=(1.0, 0.5), s_out=1.0, outp=None):
        ins = [a.ptr] * k if ins is None else ins
        return cr.concat_u8_nhwc(lib, ctx.h, ins, [16] * k, list(b_in) * (k // 2 or 1), [0] * k, (list(s_in) * 5)[:k], [0] * k,
                                 out.ptr if outp is None else outp, ob, 0, 1, 2, 2, s_out, 0, 0)

    def rows(ins=None, k=2, s_in=(1.0, 0.5), s_out=1.0, outp=None):
        ins = [a.ptr] * k if ins is None else ins
        return cr.concat_u8(lib, ctx.h, ins, [16] * k, (list(s_in) * 5)[:k], [0] * k, out.ptr if outp is None else outp, 4, s_out, 0, 0)

    try:
        for f in (nhwc, rows):
            assert f(ins=[a.ptr, None]) == -1 and f(outp=C.c_void_p()) == -1
            assert f(k=0) == -1 and f(k=9) == -1
            assert f(s_out=0.0) == -1 and f(s_in=(nan, 1.0)) == -1
        assert nhwc(b_in=(0, -1)) == -1 and nhwc(ob=-1) == -1
        assert cr.concat_f32(lib, ctx.h, [a.ptr] * 9, [4] * 9, out.ptr, 1) == -1
        ctx.sync()
        assert np.array_equal(out.get(), before) and out.guards_ok()
    finally:
        out.free()
        a.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_surface_mixed_layouts(i8ie):
    rng = np.random.default_rng(11)
    x = rng.uniform(-2, 2, (2, 16, 8, 8)).astype(f32)
    conv = support.conv(i8ie, 16, 16, 3, 1, 5, (0.05, 120))
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)          # NCHW bytes
    qv = q.numpy()
    yv = conv(q).numpy()                                   # (observed on a tensor of its own: the input below stays as it lies)
    ins = {"q": (qv, f32(0.025), 127), "y": (yv, f32(0.05), 120)}
    for relu in (False, True):
        for order in ("qy", "yq", "yqy", "q", "qq"):
            y = conv(q)                                    # a conv result in the engine's layout, still pending
            r = i8ie.cat([q if o == "q" else y for o in order], 0.05, 120)
            if relu:
                r = i8ie.relu(r)
            assert r.shape == (2, 16 * len(order), 8, 8) and r.scale == pytest.approx(0.05) and r.zero_point == 120
            assert np.array_equal(r.numpy(), cr.cat_u8([ins[o] for o in order], f32(0.05), 120, relu)), (relu, order)
    # 2-D rows, one of them the flatten of an NHWC activation
    a2, b2 = q.reshape(2, -1), conv(q).reshape(2, -1)
    r = i8ie.cat([a2, b2, a2], scale=0.04, zero_point=128)
    want = cr.cat_u8([(qv.reshape(2, -1), f32(0.025), 127), (yv.reshape(2, -1), f32(0.05), 120), (qv.reshape(2, -1), f32(0.025), 127)],
                     f32(0.04), 128)
    assert r.shape == (2, 3072) and np.array_equal(r.numpy(), want)
    # FP32: a copy
    t, u = i8ie.tensor(x), i8ie.tensor(x[:, :3])
    s = i8ie.cat([t, u, t])
    assert np.array_equal(s.numpy().view(np.uint32), np.concatenate([x, x[:, :3], x], axis=1).view(np.uint32))
    with pytest.raises(RuntimeError):
        i8ie.cat([q, q.reshape(2, -1)], 0.05, 127)
    with pytest.raises(RuntimeError):
        i8ie.cat([q, t], 0.05, 127)                        # mixed dtypes
    with pytest.raises(RuntimeError):
        i8ie.cat([q, q], 0.05, 256)
    with pytest.raises(RuntimeError):
        i8ie.cat([q, q], 0.0, 1)
    with pytest.raises(RuntimeError):
        i8ie.Concat()([q, q])                              # not converted


def test_fire_launch_counts(i8ie):
    """conv_c(relu(cat(conv_a(x), conv_b(x)))): three conv launches and ONE concat launch -- the relu folds into the concat,
    and the padded conv_c gets its border (and re-biased bytes, where it reads them) from the concat kernel."""
    import _CXX_i8ie as cx

    conv_a = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    conv_b = support.conv(i8ie, 16, 16, 3, 1, 3, (0.06, 130))
    conv_c = support.conv(i8ie, 32, 16, 3, 1, 6, (0.08, 90))
    cat = i8ie.Concat()
    cat.set_output_qparams(0.06, 130)  # conv_b's: a copy; conv_a's result is requantised
    cat.convert()
    q = support.activation(i8ie)

    def forward():
        return conv_c(i8ie.relu(cat([conv_a(q), conv_b(q)])))

    first = forward().numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        y = forward()
        y.data.layout()  # launches what is pending; the bytes are observed outside the counted region
    finally:
        prof = cx.profile_stop()
    got = y.numpy()
    av, bv = conv_a(q).numpy(), conv_b(q).numpy()
    want_cat = cr.cat_u8([(av, f32(0.05), 120), (bv, f32(0.06), 130)], f32(0.06), 130, True)
    assert np.array_equal(i8ie.relu(cat([conv_a(q), conv_b(q)])).numpy(), want_cat)
    assert np.array_equal(got, first)
    cats, others, launches = support.split_launches(support.launch_counts(prof), "concat_u8")
    print(launches)
    assert cats == 1 and others == 3, launches


@pytest.mark.parametrize("skip_first", [False, True], ids=["cat_fx_x", "cat_x_fx"])
def test_input_launched_for_another_consumer_is_read_as_it_lies(i8ie, skip_first):
    """cat(relu(conv_a(x)), x) with x = relu(conv0(..)): x is made bordered for conv_a and read by the concat as it lies, in
    either order: two conv launches and one concat launch"""
    import _CXX_i8ie as cx

    conv0 = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110))
    conv_a = support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    cat = i8ie.Concat()
    cat.set_output_qparams(0.04, 110)
    cat.convert()
    q = support.activation(i8ie)

    def forward():
        x = i8ie.relu(conv0(q))
        fx = i8ie.relu(conv_a(x))
        return cat([x, fx] if skip_first else [fx, x])

    first = forward().numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        y = forward()
        y.data.layout()
    finally:
        prof = cx.profile_stop()
    got = y.numpy()
    xv = i8ie.relu(conv0(q)).numpy()
    fv = i8ie.relu(conv_a(i8ie.relu(conv0(q)))).numpy()
    ops = [(xv, f32(0.04), 110), (fv, f32(0.05), 120)]
    want = cr.cat_u8(ops if skip_first else ops[::-1], f32(0.04), 110)
    assert np.array_equal(got, want) and np.array_equal(first, want)
    cats, others, launches = support.split_launches(support.launch_counts(prof), "concat_u8")
    print(launches)
    assert cats == 1 and others == 2, launches


@pytest.mark.parametrize("mode", ["host", "device"])
def test_concat_is_calibrated_like_a_layer(i8ie, mode, tmp_path):
    import _CXX_i8ie as cx

    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, (5, 8, 10, 10)).astype(f32)
    b = rng.normal(-0.1, 0.7, (5, 3, 10, 10)).astype(f32)
    total = np.concatenate([a, b], axis=1)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.cat1 = i8ie.Concat()

        def forward(self, x):
            return self.cat1([x, x])

    cx.set_calibration_mode(mode)
    cx.set_calibration_seed(7)
    try:
        cat = i8ie.Concat()
        cat.prepare()
        got = cat([i8ie.tensor(a), i8ie.tensor(b)]).numpy()
        cat.convert()
        if mode == "host":
            want = tuple(cx.calibrator_range([total.ravel()], 1.0))
        else:
            want = tuple(cx.calibrator_device_samples([total.ravel()], 7)[2:])
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert np.array_equal(got.view(np.uint32), total.view(np.uint32))
    assert cat.layer.is_quantized() and cat.output_qparams() == want and want[0] != 1.0
    # injected parameters win over the calibrator's, and survive the state dict and the file
    net = Net()
    net.prepare()
    net.cat1.set_output_qparams(0.03, 41)
    net(i8ie.tensor(a))
    net.convert()
    assert net.cat1.output_qparams() == (float(f32(0.03)), 41)
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["cat1.qparams"] and sd["cat1.qparams"].tolist() == [0.0, float(f32(0.03)), 41.0]
    path = str(tmp_path / "cat.npz")
    net.save_quantized(path)
    fresh = Net()
    fresh.load_quantized_file(path)
    assert fresh.is_quant and fresh.cat1.output_qparams() == net.cat1.output_qparams()
    x = rng.uniform(-1, 1, (2, 4, 3, 3)).astype(f32)
    y = fresh(i8ie.tensor(x)).numpy()
    q0 = np.asarray(i8ie.quantize(i8ie.tensor(x), 0.025, 127).numpy())
    want_q = cr.cat_u8([(q0, f32(0.025), 127)] * 2, f32(0.03), 41)
    assert np.array_equal(y, ((want_q.astype(np.int32) - 41).astype(f32) * f32(0.03)).astype(f32))


# ---- the fire networks -------------------------------------------------------------------------------------------------
def _saturated(trace, jqp):
    """(clamped, literal): two shares of the Concats' expected bytes.
    clamped  bytes that sit on a clamp: 255, or 0 where 0 is not the zero point itself.  Behind a ReLU the calibrated zero
             point is 0 and a byte 0 is the value zero, not a clipped one.  This is the share held under 20 %.
    literal  every byte 0 or 255.  A ReLU zeroes the negative half of a roughly zero-mean pre-activation, so about half of
             the bytes of a concat of ReLU outputs are 0 whatever the scales are (on the CPU, with min / max scales, the
             restatement gives 0.30-0.31 for fire_tiny and 0.53 for squeezenet_cifar); the other half must stay
             discriminating, and allowing a tenth on top of the half for clipping gives the 60 % this share is held under."""
    total = float(sum(q.size for q in trace.values()))
    literal = sum(int((q == 255).sum()) + int((q == 0).sum()) for q in trace.values())
    clamped = sum(int((q == 255).sum()) + (int((q == 0).sum()) if jqp[a][1] != 0 else 0) for a, q in trace.items())
    return clamped / total, literal / total


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [2, 66])
def test_fire_tiny_bit_exact(i8ie, batch, per_channel, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    name = "fire_tiny"
    net, qlayers, qp, jqp = nc.calibrated(name, per_channel)
    assert sorted(jqp) == ["facat", "fbcat", "rcat"] and all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp
    x = wl.synthetic_input(name, batch, seed=5)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, per_channel, sr.outputs_of("concat", trace))
    sat, literal = _saturated(trace, jqp)
    print("concat bytes on a clamp: %.4f, bytes 0 / 255: %.4f" % (sat, literal), jqp)
    assert sorted(trace) == sorted(jqp) and sat < 0.2 and literal < 0.6, (sat, literal)  # the expected bytes discriminate
    assert want.shape == (batch, 10)
    nc.check_bit_exact(i8ie, net, name, x, want, fallback=True, graph=batch == 2, reload_dir=tmp_path if batch == 2 else None,
                       expect_jqp=jqp)


def test_squeezenet_cifar_bit_exact(i8ie):
    from int8inferenceengine_amd import workloads as wl

    name = "squeezenet_cifar"
    net, qlayers, qp, jqp = nc.calibrated(name, False)
    assert sorted(jqp) == sorted(wl.concat_names(name)) and len(jqp) == 8 and all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp
    x = wl.synthetic_input(name, 2, seed=5)
    trace = {}
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, False, sr.outputs_of("concat", trace))
    sat, literal = _saturated(trace, jqp)
    print("concat bytes on a clamp: %.4f, bytes 0 / 255: %.4f" % (sat, literal))
    assert sat < 0.2 and literal < 0.6, (sat, literal)
    assert want.shape == (2, 10)
    nc.check_bit_exact(i8ie, net, name, x, want)
