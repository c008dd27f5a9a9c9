"""ConvTranspose2d on the GPU (csrc/i8ie_deconv.hip, route T of csrc/i8ie_layer.hip): every case of tests/deconv_ref.py
through a layer handle -- the kernel that ran against deconv_ref.dispatch(), the accumulators and every byte of the physical
output (interior, border, a 4 KiB guard band either side) against the equivalent problem on the oracle, with and without
ReLU; every MFMA case again through deconv_direct; the re-biased layouts, the pool, the stateless and the FP32 entries; the
Python surface; and the two U-Nets bit for bit against the oracle composition."""
import ctypes as C
import zlib

import numpy as np
import pytest

import abi
import deconv_ref as dr
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import orc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
DECONV = {"deconv_mfma", "deconv_direct"}
BY_NAME = {c.name: c for c in dr.CASES}


ctx = support.ctx_fixture(dr)


def _launched(r):
    """the kernels of a forward, without the offset vector's (made on a handle's first call per (s_in, zp_in))"""
    return [n for n in r["names"] if "offsets" not in n]


def _check(r, d, case, relu, tag):
    want = np.maximum(d["want"], np.uint8(dr.ZP_OUT)) if relu else d["want"]
    assert np.array_equal(r["acc"], d["acc"]), tag + ": accumulators"
    assert np.array_equal(r["out"], want), tag
    assert r["ok"], tag + ": a byte outside the output or the accumulators was written"
    if case.out_nhwc:  # the whole physical tensor: nothing but the interior differs from the border value
        assert np.array_equal(r["phys"], abi.Ctx.to_phys(want, case.ob, dr.ZP_OUT)), tag + ": physical output"


@pytest.mark.parametrize("case", dr.CASES, ids=[c.name for c in dr.CASES])
def test_case(ctx, case):
    d, disp = dr.reference(case), dr.dispatch(case)
    print("%s: %s geom=%s" % (case.name, tuple(disp), dr.geom(case)))
    for relu in (False, True):
        r = dr.run_handle(ctx, case, relu)
        tag = "%s relu=%d" % (case.name, relu)
        assert DECONV & set(r["names"]) == {disp.kernel}, (tag, r["names"])
        if case.in_nhwc and case.out_nhwc:
            assert _launched(r) == [disp.kernel], (tag, r["names"])  # an NHWC forward is one launch
        _check(r, d, case, relu, tag)


MFMA = [c for c in dr.CASES if dr.dispatch(c).kernel == "deconv_mfma"]


@pytest.mark.parametrize("case", MFMA, ids=[c.name for c in MFMA])
def test_mfma_case_again_through_the_direct_kernel(ctx, case):
    """force-fallback, NHWC in and out, ReLU fused"""
    d = dr.reference(case)
    forced = case._replace(force=True, in_nhwc=True, out_nhwc=True, ib=1, ob=1)
    assert dr.dispatch(forced).kernel == "deconv_direct"
    r = dr.run_handle(ctx, forced, True)
    assert _launched(r) == ["deconv_direct"], r["names"]
    _check(r, d, forced, True, case.name + " forced")


@pytest.mark.parametrize("name", ["lay_hh-pt", "lay_hh-pc", "geo_k2s2-pt"])
def test_rebiased_layouts_and_pool(ctx, name):
    """NHWC_S8 on either side is converted around the kernel; a max-pool runs behind it (nothing is folded)"""
    case = BY_NAME[name]._replace(in_nhwc=True, out_nhwc=True, ib=1, ob=1)
    assert case.kc % 16 == 0
    d = dr.reference(case)
    relu = np.maximum(d["want"], np.uint8(dr.ZP_OUT))
    for in_s8, out_s8, pool in ((True, False, None), (False, True, None), (True, True, (2, 2)), (False, False, (2, 2))):
        r = dr.run_handle(ctx, case, True, pool=pool, in_s8=in_s8, out_s8=out_s8)
        want = relu if pool is None else orc.max_pool2d(relu, *pool)
        print(name, in_s8, out_s8, pool, r["names"])
        assert DECONV & set(r["names"]) == {"deconv_mfma"}
        assert np.array_equal(r["acc"], d["acc"]) and np.array_equal(r["out"], want) and r["ok"], (in_s8, out_s8, pool)
        assert np.array_equal(r["phys"], abi.Ctx.to_phys(want, case.ob, dr.ZP_OUT))


def test_handle_answers_like_a_grouped_one(ctx):
    lib = abi.lib()
    case = BY_NAME["geo_k2s2-pt"]
    L = dr.create(lib, ctx, dr.reference(case), case)
    try:
        a, b = C.c_int(-1), C.c_int(-1)
        abi.ck(lib.i8ie_layer_fuses_pool(L, 2, 3, 4, 2, 2, C.byref(a)))
        assert a.value == 0
        abi.ck(lib.i8ie_layer_accepts_f32_input(L, 3, 4, C.byref(a)))
        assert a.value == 0
        abi.ck(lib.i8ie_layer_rebiased_io(L, 2, 3, 4, 0, 0, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (0, 0)
        abi.ck(lib.i8ie_layer_padding(L, C.byref(a)))
        assert a.value == 0
        rc = lib.i8ie_layer_forward_dequant(L, C.c_void_p(256), 0, 2, 3, 4, C.c_float(1), C.c_uint8(0), 0, C.c_void_p(256), C.c_void_p(256))
        assert rc == -1 and b"Linear layers only" in lib.i8ie_last_error()
    finally:
        lib.i8ie_layer_destroy(L)


@pytest.mark.parametrize("name", ["geo_k3s2p1op1-pt", "geo_k1s2op1-pt", "in1_direct-pt", "phk65_in65-pt"])
def test_stateless(ctx, name):
    case = BY_NAME[name]
    d = dr.reference(case)
    oh, ow, K = dr.geom(case)[:3]
    lib = abi.lib()
    di, dw, db = ctx.put(d["q"]), ctx.put(np.ascontiguousarray(d["qw"])), ctx.put(d["qb"])
    oc = ctx.empty((case.kc,), np.int32)
    out, acc = abi.GuardedU8(ctx, (case.m, case.kc, oh, ow)), abi.GuardedU8(ctx, (case.m, oh * ow, case.kc), np.int32)
    try:
        abi.ck(lib.i8ie_conv_offsets(ctx.h, dw.ptr, db.ptr, case.kc, K, C.c_float(dr.S_IN), C.c_uint8(case.zp_in), oc.ptr))
        abi.ck(lib.i8ie_conv_transpose2d_u8s8(ctx.h, di.ptr, case.m, case.c, case.h, case.w, dw.ptr, case.kc, case.k, case.s, case.p,
                                              case.op, case.zp_in, oc.ptr, dr.S_IN, d["s_w"], d["s_out"], dr.ZP_OUT, out.ptr, acc.ptr))
        got, gacc = out.get(), acc.get()
        ok = out.guards_ok() and acc.guards_ok()
    finally:
        for b in (di, dw, db, oc, out, acc):
            b.free()
    assert ok and np.array_equal(gacc, d["acc"]) and np.array_equal(got, d["want"])


# ---- FP32 (i8ie_conv_transpose2d_f32), the two data classes of tests/test_gpu_fp32.py -------------------------------------
@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("geo", dr.GEOMETRIES, ids=lambda g: "k%ds%dp%dop%d" % g)
def test_fp32(ctx, geo, cls):
    """EXACT: integer data, bit equality with float64.  REAL: |err| <= gamma(K + 1) * mag with K = in * k * k, the bound of a
    chain of at most K fp32 products and sums plus the bias (the kernel sums a subset of the K taps, in one chain)."""
    k, s, p, op = geo
    n, c, kc, h, w = 2, 5, 7, 3, 4
    rng = np.random.default_rng(zlib.crc32(("deconv%s%s" % (geo, cls)).encode()))
    if cls == "exact":
        x, wt, b = (rng.integers(-8, 9, (n, c, h, w)).astype(f32), rng.integers(-8, 9, (c, kc, k, k)).astype(f32),
                    rng.integers(-64, 65, kc).astype(f32))
    else:
        x, wt, b = (rng.uniform(-1, 1, (n, c, h, w)).astype(f32), rng.uniform(-1, 1, (c, kc, k, k)).astype(f32),
                    rng.uniform(-1, 1, kc).astype(f32))
    want = dr.scatter(x, wt, b, s, p, op)
    di, dw, db, o = ctx.put(x), ctx.put(wt), ctx.put(b), ctx.guarded(want.shape)
    try:
        abi.ck(abi.lib().i8ie_conv_transpose2d_f32(ctx.h, di.ptr, n, c, h, w, dw.ptr, db.ptr, kc, k, s, p, op, o.ptr))
        got, guards_ok = o.read()
    finally:
        for dd in (di, dw, db, o):
            dd.free()
    assert guards_ok and got.shape == want.shape and abi.GuardedOut.unwritten(got) == 0
    if cls == "exact":
        assert np.abs(want).max() < 2.0 ** 24 and np.array_equal(want, np.rint(want))
        assert np.array_equal(got.view(np.uint32), (want + 0.0).astype(f32).view(np.uint32))
    else:
        err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(dr.scatter_mag(x, wt, b, s, p, op), c * k * k)
        print("%s: worst err / bound = %.3g" % (geo, float((err / bound).max())))
        assert np.all(err <= bound)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def _conv(i8ie, cin, cout, k, pad, seed, qp):  # (not support.conv: the bias is uniform(-1, 1) * 0.1, which rounds differently)
    rng = np.random.default_rng(seed)
    L = i8ie.Conv2d(cin, cout, k, stride=1, padding=pad)
    L.load_weight((rng.uniform(-1, 1, (cout, cin, k, k)) * np.sqrt(6.0 / (cin * k * k))).astype(f32))
    L.load_bias((rng.uniform(-1, 1, cout) * 0.1).astype(f32))
    L.set_output_qparams(*qp)
    L.convert()
    return L


def _deconv(i8ie, cin, cout, geo, seed, qp, per_channel=False):
    k, s, p, op = geo
    rng = np.random.default_rng(seed)
    L = i8ie.ConvTranspose2d(cin, cout, k, stride=s, padding=p, output_padding=op)
    L.load_weight((rng.uniform(-1, 1, (cin, cout, k, k)) * np.sqrt(6.0 * s * s / (cin * k * k))).astype(f32))
    L.load_bias((rng.uniform(-1, 1, cout) * 0.1).astype(f32))
    L.set_output_qparams(*qp)
    L.convert(per_channel)
    return L


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
def test_conv_deconv_relu_conv_launches_and_bytes(i8ie, per_channel):
    """conv -> ConvTranspose2d -> relu -> conv(pad 1): the launches of the producers on their own plus ONE deconv launch; the
    relu folds in, the input is read as its producer left it and the padded conv gets its border from the deconv kernel"""
    conv0 = _conv(i8ie, 16, 32, 3, 1, 1, (0.05, 120))
    up = _deconv(i8ie, 32, 16, (2, 2, 0, 0), 2, (0.04, 110), per_channel)
    conv_c = _conv(i8ie, 16, 16, 3, 1, 3, (0.08, 90))
    xin = np.random.default_rng(4).uniform(-2, 2, (2, 3, 6, 5)).astype(f32)
    # activations in the engine's layout that stay recorded (as in tests/test_gpu_mul.py): the warm-up forward launches them
    # once, with the border their consumer asks for, and the counted forward finds that result
    q = i8ie.relu(_conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))(i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))
    mid_in = i8ie.relu(up(i8ie.relu(conv0(q))))

    made = support.counted(lambda: [i8ie.relu(conv0(q))])
    behind = support.counted(lambda: [conv_c(mid_in)])
    whole = support.counted(lambda: [conv_c(i8ie.relu(up(i8ie.relu(conv0(q)))))])
    print(made, behind, whole)
    want_launches = dict(made)
    for k, v in behind.items():
        want_launches[k] = want_launches.get(k, 0) + v
    want_launches["deconv_mfma"] = want_launches.get("deconv_mfma", 0) + 1
    assert whole == want_launches, (whole, want_launches)
    for k in set(whole) - set(made):  # (what the producers launch for themselves is theirs)
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), whole
    # bytes: the observed producer, the restated layer, the observed consumer
    xv = i8ie.relu(conv0(q)).numpy()
    qw_eq = dr.equivalent_weight(up.layer.q_weight())
    assert up.layer.q_weight().shape == (32, 16, 2, 2) and up.is_per_channel() == per_channel
    if per_channel:
        mid, acc = dr.deconv_u8_pc(xv, qw_eq, up.layer.q_bias(), 2, 0, 0, f32(0.05), 120, up.weight_scales(), f32(0.04), 110)
    else:
        mid, acc = dr.deconv_u8(xv, qw_eq, up.layer.q_bias(), 2, 0, 0, f32(0.05), 120, up.weight_scale(), f32(0.04), 110)
    out_dbg, acc_dbg = up.forward_debug(i8ie.relu(conv0(q)))
    assert np.array_equal(acc_dbg, acc) and np.array_equal(out_dbg.numpy(), mid)
    mid = orc.relu(mid, 110)
    assert len(np.unique(mid)) > 30
    want, _ = gr.conv2d_grouped(mid, conv_c.layer.q_weight(), conv_c.layer.q_bias(), 1, 1, 1, f32(0.04), 110, conv_c.weight_scale(),
                                f32(0.08), 90)
    assert np.array_equal(conv_c(i8ie.relu(up(i8ie.relu(conv0(q))))).numpy(), want)


def test_calibration_and_quantisation_rules(i8ie):
    """prepare() samples the FP32 output, convert() quantises the equivalent kernel by the layers' rules"""
    import _CXX_i8ie as cx

    rng = np.random.default_rng(8)
    x = rng.normal(0.2, 1.0, (3, 6, 4, 5)).astype(f32)
    w = (rng.uniform(-1, 1, (6, 9, 3, 3)) * 0.3).astype(f32)
    b = rng.uniform(-0.2, 0.2, 9).astype(f32)
    total = dr.scatter(x, w, b, 2, 1, 1)
    for per_channel in (False, True):
        cx.set_calibration_mode("host")
        cx.set_calibration_seed(7)
        try:
            L = i8ie.ConvTranspose2d(6, 9, 3, stride=2, padding=1, output_padding=1)
            L.load_weight(w)
            L.load_bias(b)
            L.prepare()
            got = L(i8ie.tensor(x)).numpy()
            L.convert(per_channel)
            want_qp = tuple(cx.calibrator_range([got.ravel()], 1.0))
        finally:
            cx.set_calibration_mode("auto")
            cx.set_calibration_seed(-1)
        err = np.abs(got.astype(np.float64) - total)
        assert got.shape == total.shape and np.all(err <= f64_ref.dot_bound(dr.scatter_mag(x, w, b, 2, 1, 1), 6 * 9))
        assert L.output_qparams() == want_qp and want_qp[0] != 1.0
        eq = dr.equivalent_weight(w)
        if per_channel:
            qw, qb, s_w = dr.pcp.quantize_weight_pc(eq, b)
            assert np.array_equal(L.weight_scales(), s_w)
        else:
            qw, qb, s_w = orc.quantize_weight(eq, b)
            assert L.weight_scale() == s_w
        assert np.array_equal(dr.equivalent_weight(L.layer.q_weight()), qw) and np.array_equal(L.layer.q_bias(), qb)


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
def test_save_load_round_trip_of_one_layer(i8ie, per_channel, tmp_path):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.up = i8ie.ConvTranspose2d(6, 9, 3, stride=2, padding=1, output_padding=1)

        def forward(self, x):
            return self.up(x)

    rng = np.random.default_rng(11)
    net = Net()
    net.load({"up.weight": (rng.uniform(-1, 1, (6, 9, 3, 3)) * 0.3).astype(f32), "up.bias": rng.uniform(-0.2, 0.2, 9).astype(f32)})
    net.up.set_output_qparams(0.05, 120)
    net.convert(per_channel)
    sd = net.quantized_state_dict()
    assert sd["up.q_weight"].shape == (6, 9, 3, 3) and sd["up.q_bias"].shape == (9,) and ("up.w_scales" in sd) == per_channel
    path = str(tmp_path / "up.npz")
    net.save_quantized(path)
    fresh = Net()
    fresh.load_quantized_file(path)
    assert fresh.up.output_qparams() == (np.float32(0.05), 120) and fresh.up.is_per_channel() == per_channel
    assert np.array_equal(fresh.up.layer.q_weight(), sd["up.q_weight"]) and np.array_equal(fresh.up.weight_scales(), net.up.weight_scales())
    x = i8ie.tensor(rng.uniform(-2, 2, (2, 6, 4, 5)).astype(f32))
    got, again = net(x).numpy(), fresh(x).numpy()
    assert len(np.unique(got)) > 30 and np.array_equal(got.view(np.uint32), again.view(np.uint32))


# ---- the networks ------------------------------------------------------------------------------------------------------
_WANT = {}


def _want(name, batch, per_channel):
    from int8inferenceengine_amd import workloads as wl

    if (name, batch, per_channel) not in _WANT:
        net, qlayers, qp, jqp = nc.calibrated(name, per_channel, calib_images=8)
        x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
        trace = {}
        want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, per_channel, dr.tracer(wl.NETWORKS[name][0], trace))
        _WANT[(name, batch, per_channel)] = (x, want, trace)
    return _WANT[(name, batch, per_channel)]


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [2, 66])
@pytest.mark.parametrize("name", ["unet_tiny", "unet_cifar"])
def test_unet_bit_exact(i8ie, name, batch, per_channel, tmp_path):
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = nc.calibrated(name, per_channel, calib_images=8)
    x, want, trace = _want(name, batch, per_channel)
    ups = [a for a, L in wl.NETWORKS[name][0].items() if L[0] == "deconv"]
    assert sorted(trace) == sorted(ups) and len(ups) == 3 and sorted(jqp) == sorted(wl.concat_names(name))
    print({a: round(float(((q == 0) | (q == 255)).mean()), 3) for a, q in trace.items()})
    assert want.shape == (batch, 10, 32, 32)
    # unet_tiny also replayed as one HIP graph (the packed phase panels keep their addresses), at both batch sizes
    tiny = name == "unet_tiny"
    nc.check_bit_exact(i8ie, net, name, x, want, fallback=tiny, graph=tiny, reload_dir=tmp_path if tiny and batch == 2 else None,
                       expect_jqp=jqp)
