"""The grouped / depthwise Conv2d kernels (csrc/i8ie_gconv.hip) at their edges: every case of tests/grouped_cases.py
(EDGE_CASES and the seeded sweep) through a layer handle, the kernel that ran against grouped_cases.dispatch(), the
accumulators and every byte of the physical output (interior, border, a guard band either side of the allocation)
against the per-group composition of the oracle; both kernels on the same case in NHWC with ReLU; the stateless, the
pool, the re-biased and the FP32 entry points; and a G = 1 layer inside a converted Module."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi
import f64_ref
import grouped_cases as gc
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import spec_ref as sr
import support

pytestmark = pytest.mark.gpu

EDGE = gc.EDGE_CASES
FUZZ = gc.fuzz_cases()
BY_NAME = {c.name: c for c in EDGE}
GCONV = {"gconv_mfma", "gconv_direct"}


ctx = support.ctx_fixture(gr)


def run(ctx, case, relu, names=None, guard=None, **over):
    """the case through i8ie_layer_forward_fused / _pool on a grouped handle; `over` replaces layout arguments"""
    d = gc.reference(case)
    kw = dict(in_nhwc=case.in_nhwc, out_nhwc=case.out_nhwc, in_border=case.ib, out_border=case.ob)
    kw.update(over)
    ctx.set_force_fallback(case.force)
    try:
        with gr.grouped_handles(abi.lib(), case.groups, d["s_wv"] if case.pc else None):
            return ctx.layer_forward_pool(d["q"], d["qw"], d["qb"], gc.S_IN, case.zp_in, float(d["s_w"]), d["s_out"], gc.ZP_OUT,
                                          case.stride, case.pad, relu=relu, names=names, guard=guard, **kw)
    finally:
        ctx.set_force_fallback(False)


def check(ctx, case):
    d = gc.reference(case)
    disp = gc.dispatch(case)
    print("%s: %s G=%s dot4=%s pc=%d vec_out=%d Ng=%d Kg=%d M=%d" % ((case.name,) + tuple(disp[:3]) + (disp.pc, disp.vec_out)
                                                                    + gc.geom(case)[1:3] + gc.geom(case)[5:]))
    for relu in (False, True):
        want = np.maximum(d["want"], np.uint8(gc.ZP_OUT)) if relu else d["want"]
        names, guard = [], {}
        got, acc = run(ctx, case, relu, names, guard)
        tag = "%s relu=%d" % (case.name, relu)
        assert GCONV & set(names) == {disp.kernel}, (tag, names)
        assert np.array_equal(acc, d["acc"]), tag + ": accumulators"
        assert np.array_equal(got, want), tag
        assert guard["ok"], tag + ": a byte outside the output or the accumulators was written"
        if case.out_nhwc:  # the whole physical tensor: nothing but the interior differs from the border value
            assert np.array_equal(guard["phys"], abi.Ctx.to_phys(want, case.ob, gc.ZP_OUT)), tag + ": physical output"


@pytest.mark.parametrize("case", EDGE, ids=[c.name for c in EDGE])
def test_edge_case(ctx, case):
    check(ctx, case)


@pytest.mark.parametrize("case", FUZZ, ids=[c.name for c in FUZZ])
def test_fuzz_case(ctx, case):
    check(ctx, case)


MFMA_EDGE = [c for c in EDGE if gc.dispatch(c).kernel == "gconv_mfma"]


@pytest.mark.parametrize("case", MFMA_EDGE, ids=[c.name for c in MFMA_EDGE])
def test_both_kernels_agree_nhwc_relu(ctx, case):
    """every MFMA edge case once more through gconv_direct (force-fallback), NHWC in and out, ReLU fused"""
    d = gc.reference(case)
    forced = case._replace(force=True, in_nhwc=True, out_nhwc=True, ib=case.pad, ob=1 if case.kc % 16 == 0 else 0)
    assert gc.dispatch(forced).kernel == "gconv_direct"
    want = np.maximum(d["want"], np.uint8(gc.ZP_OUT))
    for c in (forced._replace(force=False), forced):
        names, guard = [], {}
        got, acc = run(ctx, c, True, names, guard)
        print("%s: %s" % (c.name, sorted(GCONV & set(names))))
        assert GCONV & set(names) == {gc.dispatch(c).kernel}, names
        assert np.array_equal(acc, d["acc"]) and np.array_equal(got, want), (c.name, c.force)
        assert guard["ok"] and np.array_equal(guard["phys"], abi.Ctx.to_phys(want, c.ob, gc.ZP_OUT))


@contextlib.contextmanager
def kernels(ctx, names):
    """`names` receives the kernels launched inside"""
    lib = abi.lib()
    abi.ck(lib.i8ie_profile_start(ctx.h, 0))
    try:
        yield
    finally:
        ents, cnt = (abi.ProfEntry * 64)(), C.c_int(0)
        abi.ck(lib.i8ie_profile_stop(ctx.h, ents, 64, C.byref(cnt)))
        names.extend(ents[i].name.decode().split("|")[0] for i in range(cnt.value))


@pytest.mark.parametrize("name", ["g1_cg7_ng4_kg63_m15-pt", "g4_cg8_kg128_ng63_m129-pt", "g1_cg6_ng3_m1-pt"])
def test_stateless(ctx, name):
    """i8ie_conv2d_u8s8_grouped on G = 1 and on Ng % 4 != 0 through the MFMA kernel"""
    case = BY_NAME[name]
    d = gc.reference(case)
    _, _, Kg, oh, ow, _ = gc.geom(case)
    assert gc.dispatch(case).kernel == "gconv_mfma"
    lib = abi.lib()
    di, dw, db = ctx.put(d["q"]), ctx.put(d["qw"]), ctx.put(d["qb"])
    oc = ctx.empty((case.kc,), np.int32)
    out, acc = abi.GuardedU8(ctx, (case.m, case.kc, oh, ow)), abi.GuardedU8(ctx, (case.m, oh * ow, case.kc), np.int32)
    names = []
    try:
        abi.ck(lib.i8ie_conv_offsets(ctx.h, dw.ptr, db.ptr, case.kc, Kg, C.c_float(gc.S_IN), C.c_uint8(case.zp_in), oc.ptr))
        with kernels(ctx, names):
            abi.ck(lib.i8ie_conv2d_u8s8_grouped(ctx.h, di.ptr, case.m, case.c, case.h, case.w, dw.ptr, case.kc, case.kh, case.kw,
                                                case.stride, case.pad, case.groups, case.zp_in, oc.ptr, gc.S_IN, d["s_w"],
                                                d["s_out"], gc.ZP_OUT, out.ptr, acc.ptr))
        got, gacc = out.get(), acc.get()
        ok = out.guards_ok() and acc.guards_ok()
    finally:
        for b in (di, dw, db, oc, out, acc):
            b.free()
    print("%s: %s" % (name, sorted(GCONV & set(names))))
    assert GCONV & set(names) == {"gconv_mfma"}, names
    assert ok and np.array_equal(gacc, d["acc"]) and np.array_equal(got, d["want"])


def test_pool_behind_a_grouped_layer(ctx):
    # kc % 16 != 0 with NHWC requested: the pool runs in NCHW and the result is laid out afterwards
    case = BY_NAME["mfma_g1_ib2_pad1-pt"]
    assert case.kc % 16 != 0
    d = gc.reference(case)
    want = orc.max_pool2d(np.maximum(d["want"], np.uint8(gc.ZP_OUT)), 2, 2)
    for ob in (0, 1):
        names, guard = [], {}
        got, acc = run(ctx, case, True, names, guard, out_nhwc=True, out_border=ob, pool=(2, 2))
        print("%s pool ob=%d: %s" % (case.name, ob, sorted(set(names))))
        assert "gconv_mfma" in names and any(n.startswith("maxpool") for n in names), names
        assert np.array_equal(acc, d["acc"]) and np.array_equal(got, want)
        assert guard["ok"] and np.array_equal(guard["phys"], abi.Ctx.to_phys(want, ob, gc.ZP_OUT))
    # re-biased NHWC in and out on a G = 4 layer, alone and with the pool
    for name in ("mfma_ib0_pad1-pt", "mfma_ib0_pad1-pc"):
        case = BY_NAME[name]
        d = gc.reference(case)
        assert gc.dispatch(case).G == 4 and case.kc % 16 == 0
        relu = np.maximum(d["want"], np.uint8(gc.ZP_OUT))
        for pool, want in ((None, relu), ((2, 2), orc.max_pool2d(relu, 2, 2))):
            names, guard = [], {}
            got, acc = run(ctx, case, True, names, guard, in_s8=True, out_s8=True, pool=pool)
            print("%s s8 pool=%s: %s" % (name, pool, sorted(set(names))))
            assert "gconv_mfma" in names and "gconv_direct" not in names, names
            assert np.array_equal(acc, d["acc"]) and np.array_equal(got, want), (name, pool)
            assert guard["ok"] and np.array_equal(guard["phys"], abi.Ctx.to_phys(want, case.ob, gc.ZP_OUT))


def test_rejections_come_before_the_convolution(ctx):
    """what the header refuses for a grouped layer: the message, and no grouped kernel, conversion or pool launched"""
    case = BY_NAME["mfma_nhwc_out_kc6_ob0-pt"]
    ran = lambda names: [n for n in names if n in GCONV or "nhwc" in n or "nchw" in n or "pool" in n or "rebias" in n]
    names = []
    with pytest.raises(abi.AbiError, match="re-biased NHWC output needs out features % 16 == 0"):
        run(ctx, case, False, names, None, out_nhwc=True, out_s8=True)
    assert ran(names) == [], names
    for over in (dict(in_nhwc=False, in_border=1), dict(out_nhwc=False, out_border=1)):
        names = []
        with pytest.raises(abi.AbiError, match="only NHWC tensors carry a border"):
            run(ctx, case, False, names, None, **over)
        assert names == [], names


# ---- FP32 grouped (i8ie_conv2d_f32_grouped): tile tails inside a group --------------------------------------------------
# (name, m, c, kc, groups, (kh, kw), stride, pad, h, w): 2 groups, Ng around the 128-feature tile, Kg around the 16-deep K
# block, M around the 128-pixel tile
F32 = [
    ("ng127_kg15_m127", 127, 10, 254, 2, (1, 3), 1, 0, 1, 3),
    ("ng128_kg16_m128", 2, 8, 256, 2, (2, 2), 1, 0, 9, 9),
    ("ng129_kg17_m129", 43, 34, 258, 2, (1, 1), 1, 0, 1, 3),
    ("ng130_kg31_pad_ge_k", 3, 62, 260, 2, (1, 1), 1, 1, 3, 2),
    ("ng129_5x1_pad2_m128", 2, 6, 258, 2, (5, 1), 1, 2, 8, 4),
    ("g3_3x1_pad3_s2", 2, 9, 15, 3, (3, 1), 2, 3, 5, 6),
]


@pytest.mark.parametrize("case", F32, ids=[c[0] for c in F32])
def test_fp32_grouped_tails(ctx, case):
    name, m, c, kc, g, (kh, kw), stride, pad, h, w = case
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    x = rng.standard_normal((m, c, h, w)).astype(np.float32)
    wt = (rng.standard_normal((kc, c // g, kh, kw)) * 0.1).astype(np.float32)
    b = rng.standard_normal(kc).astype(np.float32)
    ref = gr.conv2d_f64(x, wt, b, g, stride, pad)
    bound = f64_ref.dot_bound(gr.conv2d_f64_mag(x, wt, b, g, stride, pad), (c // g) * kh * kw)
    di, dw, db, o = ctx.put(x), ctx.put(wt), ctx.put(b), ctx.guarded(ref.shape)
    names = []
    try:
        with kernels(ctx, names):
            abi.ck(abi.lib().i8ie_conv2d_f32_grouped(ctx.h, di.ptr, m, c, h, w, dw.ptr, db.ptr, kc, kh, kw, stride, pad, g, o.ptr))
        got, guards_ok = o.read()
    finally:
        for dd in (di, dw, db, o):
            dd.free()
    assert "conv2d_f32_mfma" in names, names
    assert guards_ok and abi.GuardedOut.unwritten(got) == 0
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: conv2d_f32_mfma Ng=%d Kg=%d M=%d max err / bound = %.3g" % (name, kc // g, (c // g) * kh * kw, ref.size // kc,
                                                                            float((err / bound).max())))
    assert np.all(err <= bound)


# ---- the Python surface: a G = 1 grouped layer between two dense ones ------------------------------------------------
TINY = (
    {"conv1": ("conv", 3, 12, 3, 1, 1), "conv2": ("conv", 12, 10, 3, 1, 1, 2), "conv3": ("conv", 10, 16, 3, 1, 1),
     "fc": ("fc", 16 * 4 * 4, 10)},
    [("layer", "conv1"), ("relu",), ("layer", "conv2"), ("relu",), ("pool", 2, 2), ("layer", "conv3"), ("relu",),
     ("flatten", 16 * 4 * 4), ("layer", "fc")],
    (3, 8, 8),
)


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
def test_module_with_a_g1_layer(per_channel, monkeypatch):
    """conv2 has Cg = 6 (Kg = 54) and Ng = 5: gconv_mfma's byte gather, reached through prepare() / convert()"""
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    name = "grouped_edges_tiny"
    monkeypatch.setitem(wl.NETWORKS, name, TINY)
    sd = wl.synthetic_state_dict(name)
    net = wl.calibrated(name, sd, per_channel=per_channel)
    assert net.conv2.groups() == 2
    x = wl.synthetic_input(name, 3, seed=5)
    net(i8ie.tensor(x)).numpy()
    cx.synchronize()
    cx.profile_start()
    got = net(i8ie.tensor(x)).numpy()
    launched = set(k.split("|")[0] for k in cx.profile_stop())
    print("module per_channel=%d: %s" % (per_channel, sorted(GCONV & launched)))
    assert GCONV & launched == {"gconv_mfma"}, launched
    qp = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
    want = sr.forward(TINY, x, sr.quantize_layers(TINY, sd, per_channel), qp, per_channel=per_channel)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
