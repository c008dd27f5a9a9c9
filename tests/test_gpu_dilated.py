"""Dilated Conv2d on the GPU: every case of tests/dilated_ref.py through a layer handle -- the kernel
that ran against dilated_ref.dispatch(), the INT32 accumulators and every byte of the physical output with guard bands,
against the oracle on the inflated weights, with and without ReLU; the layout matrix; the identity cases; the stateless and
the FP32 entry; the Python surface; and the two networks end to end."""
import ctypes as C
import zlib

import numpy as np
import pytest

import abi
import dilated_ref as dl
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import orc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401
import upsample_ref as ur

pytestmark = pytest.mark.gpu
f32 = np.float32
GCONV = dl.KERNELS  # the three kernels a dilated layer can reach
CONV_KERNELS = GCONV | {"igemm", "pconv", "tconv", "gemm_v1", "im2col"}


ctx = support.ctx_fixture(dl)


def run(ctx, case, relu, names=None, guard=None, **kw):
    """the case through i8ie_layer_forward_fused / _pool on a dilated handle (NCHW in and out unless `kw` says otherwise)"""
    d = dl.reference(case)
    ctx.set_force_fallback(case.force)
    try:
        with dl.dilated_handles(abi.lib(), d["qw"], case.g, case.d, d["s_wv"] if case.pc else None):
            return ctx.layer_forward_pool(d["q"], d["qwi"], d["qb"], dl.S_IN, case.zp_in, float(d["s_w"]), d["s_out"], dl.ZP_OUT,
                                          case.s, case.p, relu=relu, names=names, guard=guard, **kw)
    finally:
        ctx.set_force_fallback(False)


@pytest.mark.parametrize("case", dl.CASES, ids=[c.name for c in dl.CASES])
def test_case(ctx, case):
    d = dl.reference(case)
    disp = dl.dispatch(case)
    for relu in (False, True):
        want = np.maximum(d["want"], np.uint8(dl.ZP_OUT)) if relu else d["want"]
        names, guard = [], {}
        got, acc = run(ctx, case, relu, names, guard)
        tag = "%s relu=%d" % (case.name, relu)
        print(tag, sorted(names))
        assert GCONV & set(names) == {disp.kernel}, (tag, names)
        assert np.array_equal(acc, d["acc"]), tag + ": accumulators"
        assert np.array_equal(got, want), tag
        assert guard["ok"], tag + ": a byte outside the output or the accumulators was written"


@pytest.mark.parametrize("name", dl.LAYOUT_CASES)
def test_layout_matrix(ctx, name):
    case = dl.BY_NAME[name]
    d = dl.reference(case)
    relu_want = np.maximum(d["want"], np.uint8(dl.ZP_OUT))
    lays = [dict(in_nhwc=False, out_nhwc=False)]
    for ib in (0, 1, case.p):
        for ob in (0, 1):
            lays.append(dict(in_nhwc=True, out_nhwc=True, in_border=ib, out_border=ob))
    lays += [dict(in_nhwc=True, out_nhwc=False, in_border=1), dict(in_nhwc=False, out_nhwc=True, out_border=1),
             dict(in_nhwc=True, out_nhwc=True, in_border=1, out_border=1, in_s8=True),
             dict(in_nhwc=True, out_nhwc=True, in_border=0, out_border=1, out_s8=True),
             dict(in_nhwc=True, out_nhwc=True, in_border=case.p, out_border=0, in_s8=True, out_s8=True)]
    for kw in lays:
        names, guard = [], {}
        got, acc = run(ctx, case, True, names, guard, **kw)
        assert GCONV & set(names) == {dl.dispatch(case).kernel}, (kw, names)
        assert np.array_equal(acc, d["acc"]) and np.array_equal(got, relu_want), kw
        assert guard["ok"], kw
        if kw["out_nhwc"]:
            assert np.array_equal(guard["phys"], abi.Ctx.to_phys(relu_want, kw.get("out_border", 0), dl.ZP_OUT)), kw
    # a following max-pool through the peel passes, plain and re-biased
    pooled = orc.max_pool2d(relu_want, 2, 2)
    for kw in (dict(in_nhwc=True, out_nhwc=True, in_border=1, out_border=1), dict(in_nhwc=False, out_nhwc=False),
               dict(in_nhwc=True, out_nhwc=True, in_border=0, out_border=1, out_s8=True)):
        names, guard = [], {}
        got, acc = run(ctx, case, True, names, guard, pool=(2, 2), **kw)
        assert GCONV & set(names) == {dl.dispatch(case).kernel}, (kw, names)
        assert np.array_equal(acc, d["acc"]) and np.array_equal(got, pooled) and guard["ok"], kw


def test_layout_queries(ctx):
    lib = abi.lib()
    case = dl.BY_NAME["phases_unequal-pt"]
    d = dl.reference(case)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    qw, qb = np.ascontiguousarray(d["qw"]), np.ascontiguousarray(d["qb"])
    for dil, k, want_pad in ((2, 3, 0), (1, 3, case.p)):
        L = C.c_void_p()
        abi.ck(lib.i8ie_conv2d_create_dilated(ctx.h, P(qw), P(qb), case.kc, case.c, k, k, 1, case.p, 1, dil, C.c_float(0.01), C.byref(L)))
        pad, got = C.c_int(-1), C.c_int(-1)
        abi.ck(lib.i8ie_layer_padding(L, C.byref(pad)))
        abi.ck(lib.i8ie_layer_dilation(L, C.byref(got)))
        q = ctx.layer_queries(L, 2, case.h, case.w, 2, 2)
        lib.i8ie_layer_destroy(L)
        assert pad.value == want_pad and got.value == dil
        if dil > 1:
            assert q == dict(fuses_pool=0, reads_s8=0, stores_s8=0, accepts_f32=0, preferred_layout=1), q
    # out features that are no multiple of 16: NCHW, as every NHWC-writing handle answers (the engine's NHWC consumers take
    # 16-channel items)
    L = C.c_void_p()
    abi.ck(lib.i8ie_conv2d_create_dilated(ctx.h, P(qw), P(qb), 20, case.c, 3, 3, 1, case.p, 1, 2, C.c_float(0.01), C.byref(L)))
    q = ctx.layer_queries(L, 2, case.h, case.w, 0, 0)
    lib.i8ie_layer_destroy(L)
    assert q["preferred_layout"] == 0 and q["fuses_pool"] == 0


def _handle_bytes(ctx, create, q, s_in, zp_in, s_out, zp_out, h, w, oshape):
    lib = abi.lib()
    L = C.c_void_p()
    create(L)
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(s_out), C.c_uint8(zp_out)))
    di, out = ctx.put(q), ctx.empty(oshape, np.uint8)
    ents, cnt = (abi.ProfEntry * 64)(), C.c_int(0)
    abi.ck(lib.i8ie_profile_start(ctx.h, 0))
    try:
        abi.ck(lib.i8ie_layer_forward(L, di.ptr, q.shape[0], h, w, C.c_float(s_in), C.c_uint8(zp_in), out.ptr, None))
    finally:
        abi.ck(lib.i8ie_profile_stop(ctx.h, ents, 64, C.byref(cnt)))
    got = out.get()
    dil = C.c_int(-1)
    abi.ck(lib.i8ie_layer_dilation(L, C.byref(dil)))
    lib.i8ie_layer_destroy(L)
    di.free()
    out.free()
    return got, sorted(ents[i].name.decode().split("|")[0] for i in range(cnt.value)), dil.value


@pytest.mark.parametrize("k,d,g,c", [(1, 3, 1, 32), (3, 1, 1, 32), (3, 1, 2, 32), (1, 2, 1, 6), (3, 1, 1, 6)])
def test_identity_cases_are_the_old_layer(ctx, k, d, g, c):
    """k == 1 or dilation == 1 through the new entry: the kernels and the bytes of the old entry"""
    lib = abi.lib()
    rng = np.random.default_rng(k * 10 + d)
    kc, h, w, p = 16, 7, 9, k // 2
    q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (kc, c // g, k, k), dtype=np.int8)
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    s_out = f32(0.03 * 0.002 * np.sqrt(c // g * k * k) * 74 * 73 / 20)
    new = lambda L: abi.ck(lib.i8ie_conv2d_create_dilated(ctx.h, P(qw), P(qb), kc, c, k, k, 1, p, g, d, C.c_float(0.002), C.byref(L)))  # noqa: E731
    old = lambda L: abi.ck(lib.i8ie_conv2d_create_grouped(ctx.h, P(qw), P(qb), kc, c, k, k, 1, p, g, C.c_float(0.002), C.byref(L)))  # noqa: E731
    a, na, da = _handle_bytes(ctx, new, q, 0.03, 121, s_out, 37, h, w, (2, kc, h, w))
    b, nb, db = _handle_bytes(ctx, old, q, 0.03, 121, s_out, 37, h, w, (2, kc, h, w))
    want, _ = gr.conv2d_grouped(q, qw, qb, g, 1, p, f32(0.03), 121, f32(0.002), s_out, 37)
    print(na)
    assert na == nb and np.array_equal(a, b) and np.array_equal(a, want)
    assert (da, db) == (d, 1)


@pytest.mark.parametrize("name", ["phases_unequal-pt", "byte_gather-pt", "depthwise_s2-pt"])
def test_stateless(ctx, name):
    case = dl.BY_NAME[name]
    d = dl.reference(case)
    _, _, Kg, oh, ow = dl.geom(case)
    lib = abi.lib()
    di, dw, db = ctx.put(d["q"]), ctx.put(d["qw"]), ctx.put(d["qb"])
    oc = ctx.empty((case.kc,), np.int32)
    out, acc = abi.GuardedU8(ctx, (case.m, case.kc, oh, ow)), abi.GuardedU8(ctx, (case.m, oh * ow, case.kc), np.int32)
    try:
        abi.ck(lib.i8ie_conv_offsets(ctx.h, dw.ptr, db.ptr, case.kc, Kg, C.c_float(dl.S_IN), C.c_uint8(case.zp_in), oc.ptr))
        abi.ck(lib.i8ie_conv2d_u8s8_dilated(ctx.h, di.ptr, case.m, case.c, case.h, case.w, dw.ptr, case.kc, case.k, case.k, case.s,
                                            case.p, case.g, case.d, case.zp_in, oc.ptr, dl.S_IN, d["s_w"], d["s_out"], dl.ZP_OUT,
                                            out.ptr, acc.ptr))
        got, gacc = out.get(), acc.get()
        ok = out.guards_ok() and acc.guards_ok()
    finally:
        for b in (di, dw, db, oc, out, acc):
            b.free()
    assert ok and np.array_equal(gacc, d["acc"]) and np.array_equal(got, d["want"])


# ---- FP32 -----------------------------------------------------------------------------------------------------------------
def _f32(ctx, x, w, b, s, p, g, d, grouped_entry=False):
    lib = abi.lib()
    n, c, h, wd = x.shape
    kc, _, k, _ = w.shape
    oh, ow = dl.out_hw(h, wd, k, s, p, d)
    di, dw, db, o = ctx.put(x), ctx.put(w), ctx.put(b), ctx.guarded((n, kc, oh, ow))
    try:
        if grouped_entry:
            abi.ck(lib.i8ie_conv2d_f32_grouped(ctx.h, di.ptr, n, c, h, wd, dw.ptr, db.ptr, kc, k, k, s, p, g, o.ptr))
        else:
            abi.ck(lib.i8ie_conv2d_f32_dilated(ctx.h, di.ptr, n, c, h, wd, dw.ptr, db.ptr, kc, k, k, s, p, g, d, o.ptr))
        return o.read()
    finally:
        for t in (di, dw, db, o):
            t.free()


F32_CASES = [t for _, t in dl.DENSE_S1[:3] + dl.DENSE_S1[6:9] + dl.GENERAL]


@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("t", F32_CASES, ids=["-".join(map(str, t)) for t in F32_CASES])
def test_conv2d_f32_dilated(ctx, t, cls):
    m, c, kc, g, k, s, p, d, h, w = t
    rng = np.random.default_rng(zlib.crc32((repr(t) + cls).encode()))
    xs, ws = (m, c, h, w), (kc, c // g, k, k)
    if cls == "exact":
        x, wt, b = (rng.integers(-8, 9, xs).astype(f32), rng.integers(-8, 9, ws).astype(f32), rng.integers(-64, 65, kc).astype(f32))
    else:
        x, wt, b = (rng.uniform(-1, 1, xs).astype(f32), rng.uniform(-1, 1, ws).astype(f32), rng.uniform(-1, 1, kc).astype(f32))
    got, ok = _f32(ctx, x, wt, b, s, p, g, d)
    want = gr.conv2d_f64(x, dl.inflate(wt, d), b, g, s, p)
    assert ok and got.shape == want.shape and abi.GuardedOut.unwritten(got) == 0
    if cls == "exact":
        assert np.abs(want).max() < 2.0 ** 24 and np.array_equal(got.view(np.uint32), (want + 0.0).astype(f32).view(np.uint32))
    else:
        mag = gr.conv2d_f64_mag(x, dl.inflate(wt, d), b, g, s, p)
        err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, (c // g) * k * k)  # (the true K)
        assert np.all(err <= bound), float(np.nanmax(err / bound))


@pytest.mark.parametrize("g", [1, 2])
def test_conv2d_f32_dilation_1_is_the_grouped_entry(ctx, g):
    rng = np.random.default_rng(g)
    x, wt, b = rng.uniform(-1, 1, (2, 12, 9, 7)).astype(f32), rng.uniform(-1, 1, (10, 12 // g, 3, 3)).astype(f32), rng.uniform(-1, 1, 10).astype(f32)
    a, oka = _f32(ctx, x, wt, b, 2, 1, g, 1)
    c, okc = _f32(ctx, x, wt, b, 2, 1, g, 1, grouped_entry=True)
    assert oka and okc and np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def _conv(i8ie, cin, cout, k, pad, seed, qp, **kw):  # (not support.conv: groups / dilation in kw, and w and b are returned too)
    rng = np.random.default_rng(seed)
    L = i8ie.Conv2d(cin, cout, k, padding=pad, **kw)
    wshape = (cout, cin // kw.get("groups", 1), k, k)
    w = (rng.uniform(-1, 1, wshape) * np.sqrt(6.0 / (wshape[1] * k * k))).astype(f32)
    b = rng.uniform(-0.1, 0.1, cout).astype(f32)
    L.load_weight(w)
    L.load_bias(b)
    L.set_output_qparams(*qp)
    L.convert()
    return L, w, b


def test_nhwc_dilated_conv_relu_is_one_launch(i8ie):
    """an activation in the engine's layout -> Conv2d(dilation=2) -> relu: one launch of the grouped kernel, no border, fill,
    layout or relu pass, and the oracle's bytes on the inflated weights"""
    import _CXX_i8ie as cx

    xin = np.random.default_rng(4).uniform(-2, 2, (2, 3, 8, 8)).astype(f32)
    # (an activation as it is inside a network, test_gpu_upsample.py's construction: the second conv writes NHWC)
    q = i8ie.relu(_conv(i8ie, 16, 16, 3, 1, 8, (0.05, 125))[0](i8ie.relu(_conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))[0](
        i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))))
    assert q.data.layout() == 1  # NHWC
    L, w, b = _conv(i8ie, 16, 32, 3, 2, 5, (0.04, 110), dilation=2)
    assert L.dilation() == 2
    forward = lambda: i8ie.relu(L(q))  # noqa: E731
    first = forward().numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        y = forward()
        y.data.layout()
    finally:
        prof = cx.profile_stop()
    launches = {}
    for k, v in prof.items():
        launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0]
    print(launches)
    assert launches == {"dconv_mfma": 1}, launches
    qw, qb, s_w = orc.quantize_weight(w, b)
    want, _ = gr.conv2d_grouped(q.numpy(), dl.inflate(qw, 2), qb, 1, 1, 2, f32(q.scale), q.zero_point, s_w, f32(0.04), 110)
    want = orc.relu(want, 110)
    assert np.array_equal(y.numpy(), want) and np.array_equal(first, want) and y.shape == (2, 32, 8, 8)
    with pytest.raises(RuntimeError):  # 3x3 at rate 4 spans 9; 8 + 0 rows do not hold it
        _conv(i8ie, 16, 16, 3, 0, 6, (0.04, 110), dilation=4)[0](q).numpy()


def test_prepare_convert_save_load(i8ie, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    net = nc.calibrated("aspp_tiny", False, calib_images=8)[0]  # (prepare() -> an FP32 batch through the dilated FP32 conv -> convert())
    x = wl.synthetic_input("aspp_tiny", 3, seed=sr.INPUT_SEED)
    want = net(i8ie.tensor(x)).numpy()
    path = str(tmp_path / "aspp.npz")
    net.save_quantized(path)
    fresh = wl.build("aspp_tiny")
    fresh.load_quantized_file(path)
    assert [getattr(fresh, a).dilation() for a in ("atr", "a3", "a4d", "a1")] == [2, 3, 2, 1]
    assert np.array_equal(fresh(i8ie.tensor(x)).numpy().view(np.uint32), want.view(np.uint32))


# ---- the networks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_channel", [("aspp_tiny", False), ("aspp_tiny", True), ("deeplabv3_cifar", False)],
                         ids=["aspp_tiny-per_tensor", "aspp_tiny-per_channel", "deeplabv3_cifar-per_tensor"])
def test_networks_bit_exact(i8ie, name, per_channel):
    from int8inferenceengine_amd import workloads as wl

    batch = 2 if name == "deeplabv3_cifar" else 5
    net, qlayers, qp, jqp = nc.calibrated(name, per_channel, calib_images=8)
    x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
    trace = []
    want = sr.forward(wl.network(name), x, qlayers, qp, jqp, per_channel, ur.tracer(trace))
    assert len(trace) == 2 and all(len(np.unique(q)) > 30 for _, q in trace[1:])  # (the head's maps are not saturated)
    assert want.shape == (batch, 10, 32, 32)
    nc.check_bit_exact(i8ie, net, name, x, want, graph=name == "aspp_tiny")


def test_fp32_deeplabv3_convs_layer_by_layer(i8ie):
    """Before convert(): every conv of deeplabv3_cifar fed the product's own previous output, inside f64_ref.dot_bound (true
    K) of the float64 reference on inflated weights; then net(x) in one call equals the walked result bit for bit."""
    from int8inferenceengine_amd import workloads as wl

    name = "deeplabv3_cifar"
    layers, spec, _ = wl.network(name)
    sd = wl.synthetic_state_dict(name)
    net = wl.build(name)
    net.load(sd)
    x = wl.synthetic_input(name, 2, seed=5)
    dilated = []

    def walk(ops, t, saved):
        for op in ops:
            if op[0] == "layer":
                L, w, b = layers[op[1]], sd[op[1] + ".weight"], sd[op[1] + ".bias"]
                prev = t.numpy()
                t = getattr(net, op[1])(t)
                got = t.numpy()
                d = wl.conv_dilation(L)
                want, mag = gr.conv2d_f64(prev, dl.inflate(w, d), b, 1, L[4], L[5]), gr.conv2d_f64_mag(prev, dl.inflate(w, d), b, 1, L[4], L[5])
                err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, L[1] * L[3] * L[3])
                assert got.dtype == f32 and got.shape == want.shape and np.all(err <= bound), (op, float(np.nanmax(err / bound)))
                if d > 1:
                    dilated.append(op[1])
            elif op[0] == "relu":
                t = i8ie.relu(t)
            elif op[0] == "gap":
                t = i8ie.global_avg_pool2d(t)
            elif op[0] == "upsample":
                t = i8ie.upsample(t, op[1], op[2])
            elif op[0] == "save":
                saved[op[1]] = t
            elif op[0] == "branch":
                saved[op[1]] = walk(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                t = getattr(net, op[1])(t, saved[op[2]])
            elif op[0] == "concat":
                t = getattr(net, op[1])([t] + [saved[tag] for tag in op[2]])
            else:
                raise AssertionError(op)
        return t

    walked = walk(spec, i8ie.tensor(x), {}).numpy()
    assert walked.shape == (2, 10, 32, 32) and len(dilated) == 7
    assert np.array_equal(net(i8ie.tensor(x)).numpy().view(np.uint32), walked.view(np.uint32))
