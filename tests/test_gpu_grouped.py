"""Grouped / depthwise Conv2d on the GPU (csrc/i8ie_gconv.hip): layer handles made by i8ie_conv2d_create_grouped(_per_channel)
bit for bit against the per-group composition of the oracle (tests/grouped_ref.py), through both kernels, every layout, the
pool call, the stateless and the FP32 entry points, and the paper's AlexNet (groups = 2 on conv2 / conv4 / conv5) end to end."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import orc
import spec_ref as sr
import support

pytestmark = pytest.mark.gpu


ctx = support.ctx_fixture(gr)


# (name, m, c, kc, groups, k, stride, pad, h, w)
MFMA = [
    ("paper_conv2", 2, 96, 256, 2, 5, 1, 2, 27, 27),   # Cg = 48, K tail 1200 % 64
    ("paper_conv4", 2, 384, 384, 2, 3, 1, 1, 13, 13),
    ("paper_conv5", 2, 384, 256, 2, 3, 1, 1, 13, 13),
    ("g4_1x1", 3, 64, 32, 4, 1, 1, 0, 5, 5),           # Cg = 16, Kg = 16, Ng = 8: below the rule's 32, so gconv_direct takes it
    ("ng12_s2", 3, 40, 24, 2, 3, 2, 1, 9, 11),         # Ng = 12, Cg = 20, h != w, stride 2
    ("resnext", 2, 128, 128, 32, 3, 1, 1, 14, 14),     # Cg = 4, Kg = 36
]
DIRECT = [
    ("dw_s1", 2, 32, 32, 32, 3, 1, 1, 15, 15),
    ("dw_s2", 2, 32, 32, 32, 3, 2, 1, 15, 15),
    ("dw_5x5", 3, 24, 24, 24, 5, 1, 2, 7, 7),
    ("multiplier", 3, 8, 16, 8, 3, 1, 0, 6, 6),
    ("c6_kc9_g3", 3, 6, 9, 3, 3, 1, 1, 7, 9),
]
S_IN, ZP_IN, ZP_OUT = np.float32(0.03), 121, 37
_cache = {}


def expected_kernel(case):
    _, _, c, _, g, k = case[:6]
    return "gconv_mfma" if (c // g) * k * k >= 32 else "gconv_direct"


def make(case):
    """inputs and both references of a case, computed once and left unchanged"""
    name, m, c, kc, g, k, stride, pad, h, w = case
    if name not in _cache:
        rng = np.random.default_rng(sum(map(ord, name)))
        q = rng.integers(0, 256, (m, c, h, w), dtype=np.uint8)
        qw = rng.integers(-127, 128, (kc, c // g, k, k), dtype=np.int8)
        qb = rng.integers(-127, 128, kc, dtype=np.int8)
        Kg = (c // g) * k * k
        s_wv = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, kc)) * 2e-3).astype(np.float32)
        s_w = np.float32(np.median(s_wv))
        s_out = np.float32(S_IN * float(s_w) * np.sqrt(Kg) * 40.0 / 64.0)  # spreads the results over the u8 range
        pt = gr.conv2d_grouped(q, qw, qb, g, stride, pad, S_IN, ZP_IN, s_w, s_out, ZP_OUT)
        pc = gr.conv2d_grouped_pc(q, qw, qb, g, stride, pad, S_IN, ZP_IN, s_wv, s_out, ZP_OUT)
        for a in (q, qw, qb, s_wv) + pt + pc:
            a.setflags(write=False)
        _cache[name] = dict(q=q, qw=qw, qb=qb, s_w=s_w, s_wv=s_wv, s_out=s_out, pt=pt, pc=pc)
    return _cache[name]


def run(ctx, case, d, scales=None, names=None, **kw):
    _, _, _, _, g, _, stride, pad = case[:8]
    with gr.grouped_handles(abi.lib(), g, scales):
        return ctx.layer_forward_pool(d["q"], d["qw"], d["qb"], S_IN, ZP_IN, float(d["s_w"]), d["s_out"], ZP_OUT, stride, pad,
                                      names=names, **kw)


@pytest.mark.parametrize("case", MFMA + DIRECT, ids=[c[0] for c in MFMA + DIRECT])
def test_layer_parity(ctx, case):
    d = make(case)
    kc, pad = case[3], case[7]
    layouts = [(False, False)] + ([(True, True)] if kc % 16 == 0 else [])
    for scales, (want, want_acc) in ((None, d["pt"]), (d["s_wv"], d["pc"])):
        for relu in (False, True):
            wr = np.maximum(want, np.uint8(ZP_OUT)) if relu else want
            for in_nhwc, out_nhwc in layouts:
                names = []
                got, acc = run(ctx, case, d, scales, names, in_nhwc=in_nhwc, out_nhwc=out_nhwc, relu=relu,
                               in_border=pad if in_nhwc else 0, out_border=1 if out_nhwc else 0)
                tag = "%s pc=%d relu=%d nhwc=%d" % (case[0], scales is not None, relu, in_nhwc)
                exp = expected_kernel(case)
                assert exp in names and ("gconv_direct" if exp == "gconv_mfma" else "gconv_mfma") not in names, (tag, names)
                assert np.array_equal(acc, want_acc), tag + ": accumulators"
                assert np.array_equal(got, wr), tag


def test_extremes(ctx):
    """paper conv2, every input byte 255, weight rows alternating 127 / -128, a zp_in = 255 border: exact accumulators"""
    case = MFMA[0]
    _, m, c, kc, g, k, stride, pad, h, w = case
    q = np.full((m, c, h, w), 255, np.uint8)
    qw = np.empty((kc, c // g, k, k), np.int8)
    qw[0::2], qw[1::2] = 127, -128
    qb = np.where(np.arange(kc) % 3 == 0, 127, -128).astype(np.int8)
    s_w, s_out = np.float32(2e-3), np.float32(9.0)
    want, want_acc = gr.conv2d_grouped(q, qw, qb, g, stride, pad, S_IN, 255, s_w, s_out, ZP_OUT)
    with gr.grouped_handles(abi.lib(), g):
        for nhwc in (False, True):
            names = []
            got, acc = ctx.layer_forward_pool(q, qw, qb, S_IN, 255, float(s_w), s_out, ZP_OUT, stride, pad, in_nhwc=nhwc,
                                              out_nhwc=nhwc, in_border=pad if nhwc else 0, out_border=1 if nhwc else 0, names=names)
            assert "gconv_mfma" in names
            assert np.array_equal(acc, want_acc) and np.array_equal(got, want)


@pytest.mark.parametrize("case", MFMA, ids=[c[0] for c in MFMA])
def test_both_kernels_agree(ctx, case):
    d = make(case)
    ctx.set_force_fallback(True)
    try:
        for scales, (want, want_acc) in ((None, d["pt"]), (d["s_wv"], d["pc"])):
            names = []
            got, acc = run(ctx, case, d, scales, names, relu=False)
            assert "gconv_direct" in names and "gconv_mfma" not in names, names
            assert np.array_equal(acc, want_acc) and np.array_equal(got, want)
    finally:
        ctx.set_force_fallback(False)


def test_groups1_is_the_dense_layer(ctx):
    """AlexNet conv3 at batch 2 through the grouped create calls with groups = 1: the dense layer's kernels and bytes"""
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (2, 256, 13, 13), dtype=np.uint8)
    qw = rng.integers(-127, 128, (384, 256, 3, 3), dtype=np.int8)
    qb = rng.integers(-127, 128, 384, dtype=np.int8)
    s_w, s_out = np.float32(2e-3), np.float32(0.09)
    res = []
    for grouped in (False, True):
        names = []
        cm = gr.grouped_handles(abi.lib(), 1) if grouped else contextlib.nullcontext()
        with cm:
            got, acc = ctx.layer_forward_pool(q, qw, qb, S_IN, ZP_IN, float(s_w), s_out, ZP_OUT, 1, 1, in_nhwc=True, out_nhwc=True,
                                              in_border=1, out_border=1, relu=True, names=names)
        res.append((got, acc, sorted(names)))
    assert res[0][2] == res[1][2] and not {"gconv_mfma", "gconv_direct"} & set(res[1][2])
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    lib, L, n = abi.lib(), C.c_void_p(), C.c_int(-1)
    qw1 = np.ones((4, 16), np.int8)
    abi.ck(lib.i8ie_linear_create(ctx.h, qw1.ctypes.data_as(C.c_void_p), qw1.ctypes.data_as(C.c_void_p), 4, 16, C.c_float(0.5), C.byref(L)))
    abi.ck(lib.i8ie_layer_groups(L, C.byref(n)))
    lib.i8ie_layer_destroy(L)
    assert n.value == 1


def test_pool_and_layouts(ctx):
    case = MFMA[0]
    d = make(case)
    pad = case[7]
    want = orc.max_pool2d(np.maximum(d["pt"][0], np.uint8(ZP_OUT)), 3, 2)
    for in_nhwc, out_nhwc, s8 in ((False, False, False), (True, True, False), (True, True, True)):
        names = []
        got, acc = run(ctx, case, d, None, names, in_nhwc=in_nhwc, out_nhwc=out_nhwc, relu=True, in_border=pad if in_nhwc else 0,
                       out_border=1 if out_nhwc else 0, pool=(3, 2), in_s8=s8, out_s8=s8)
        assert "gconv_mfma" in names and any(n.startswith("maxpool") for n in names), names
        assert np.array_equal(acc, d["pt"][1])
        assert np.array_equal(got, want), (in_nhwc, s8)
    # NHWC_S8 in / out without a pool: the same values re-biased (the helper undoes the re-bias)
    got, _ = run(ctx, case, d, None, None, in_nhwc=True, out_nhwc=True, in_border=pad, out_border=1, in_s8=True, out_s8=True)
    assert np.array_equal(got, d["pt"][0])
    # what the handle answers
    lib, L = abi.lib(), C.c_void_p()
    qw, qb = d["qw"], d["qb"]
    abi.ck(lib.i8ie_conv2d_create_grouped(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), 256, 96, 5, 5, 1, 2,
                                          2, C.c_float(0.5), C.byref(L)))
    a, b, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    abi.ck(lib.i8ie_layer_fuses_pool(L, 2, 27, 27, 3, 2, C.byref(a)))
    assert a.value == 0
    abi.ck(lib.i8ie_layer_rebiased_io(L, 2, 27, 27, 3, 2, C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (0, 0)
    abi.ck(lib.i8ie_layer_accepts_f32_input(L, 27, 27, C.byref(a)))
    assert a.value == 0
    abi.ck(lib.i8ie_layer_groups(L, C.byref(n)))
    assert n.value == 2
    lib.i8ie_layer_destroy(L)


def test_stateless(ctx):
    case = DIRECT[4]
    d = make(case)
    _, m, c, kc, g, k, stride, pad, h, w = case
    oh, ow = (h - k + 2 * pad) // stride + 1, (w - k + 2 * pad) // stride + 1
    lib = abi.lib()
    di, dw, db = ctx.put(d["q"]), ctx.put(d["qw"]), ctx.put(d["qb"])
    oc, out, acc = ctx.empty((kc,), np.int32), ctx.empty((m, kc, oh, ow), np.uint8), ctx.empty((m, oh * ow, kc), np.int32)
    abi.ck(lib.i8ie_conv_offsets(ctx.h, dw.ptr, db.ptr, kc, (c // g) * k * k, C.c_float(S_IN), C.c_uint8(ZP_IN), oc.ptr))
    abi.ck(lib.i8ie_conv2d_u8s8_grouped(ctx.h, di.ptr, m, c, h, w, dw.ptr, kc, k, k, stride, pad, g, ZP_IN, oc.ptr, S_IN,
                                        d["s_w"], d["s_out"], ZP_OUT, out.ptr, acc.ptr))
    got, gacc, goc = out.get(), acc.get(), oc.get()
    for b in (di, dw, db, oc, out, acc):
        b.free()
    assert np.array_equal(goc, orc.conv_offsets(d["qw"].reshape(kc, -1), d["qb"], S_IN, ZP_IN))
    assert np.array_equal(gacc, d["pt"][1]) and np.array_equal(got, d["pt"][0])


# ---- FP32: the path taken before convert() and while calibrating -------------------------------------------------
F32 = [("paper_conv2", 2, 96, 256, 2, 5, 1, 2, 27, 27), ("dw_s2", 2, 32, 32, 32, 3, 2, 1, 15, 15), ("c6_kc9_g3", 3, 6, 9, 3, 3, 1, 1, 7, 9)]


@pytest.mark.parametrize("case", F32, ids=[c[0] for c in F32])
def test_fp32_grouped(ctx, case):
    import i8ie

    name, m, c, kc, g, k, stride, pad, h, w = case
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    x = rng.standard_normal((m, c, h, w)).astype(np.float32)
    wt = (rng.standard_normal((kc, c // g, k, k)) * 0.1).astype(np.float32)
    b = rng.standard_normal(kc).astype(np.float32)
    ref = gr.conv2d_f64(x, wt, b, g, stride, pad)
    bound = f64_ref.dot_bound(gr.conv2d_f64_mag(x, wt, b, g, stride, pad), (c // g) * k * k)
    di, dw, db, o = ctx.put(x), ctx.put(wt), ctx.put(b), ctx.guarded(ref.shape)
    try:
        abi.ck(abi.lib().i8ie_conv2d_f32_grouped(ctx.h, di.ptr, m, c, h, w, dw.ptr, db.ptr, kc, k, k, stride, pad, g, o.ptr))
        got, guards_ok = o.read()
    finally:
        for dd in (di, dw, db, o):
            dd.free()
    assert guards_ok and abi.GuardedOut.unwritten(got) == 0
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: max err / bound = %.3g" % (name, float((err / bound).max())))
    assert np.all(err <= bound)
    # the Python layer before convert()
    L = i8ie.Conv2d(c, kc, k, stride=stride, padding=pad, groups=g)
    L.load_weight(wt)
    L.load_bias(b)
    got2 = L(i8ie.tensor(x)).numpy()
    assert got2.shape == ref.shape and np.all(np.abs(got2.astype(np.float64) - ref) <= bound)


# ---- the paper's AlexNet ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [2, 66])
def test_alexnet_paper_bit_exact(batch, per_channel, tmp_path):
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    name = "alexnet_paper"
    net, qlayers, qp, _ = nc.calibrated(name, per_channel)
    x = wl.synthetic_input(name, batch, seed=5)
    want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, per_channel=per_channel)
    nc.check_bit_exact(i8ie, net, name, x, want, graph=batch == 2, reload_dir=tmp_path if batch == 2 else None)
    if batch != 2:
        return
    path = str(tmp_path / (name + ".npz"))  # (what check_bit_exact saved)
    fresh = wl.build(name)
    fresh.load_quantized_file(path)
    assert [getattr(fresh, a).groups() for a in ("conv2", "conv3")] == [2, 1]
    with pytest.raises(RuntimeError):  # the grouped weight shapes do not fit the dense architecture
        wl.build("alexnet").load_quantized_file(path)
