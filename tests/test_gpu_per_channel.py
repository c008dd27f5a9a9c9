"""Per-output-channel weight scales on the GPU: layer handles made by i8ie_*_create_per_channel, bit for bit against
the oracle's accumulators requantised per column (tests/pc_pipeline.py), through every kernel a Conv2d or Linear layer
can reach; whole networks converted with Module.convert(per_channel=True); graph replay, save / load, the kernels
launched, and the accuracy the mode exists for."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import pc_pipeline as pcp
from requant_ref import row_scales, s_out_for  # (shared with the requantiser's dense sweeps)
import support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ctx = support.ctx_fixture()


CONVS = [  # (name, m, c, h, kc, k, stride, pad)
    ("alexnet_conv1", 2, 3, 224, 96, 11, 4, 2), ("alexnet_conv2", 2, 96, 27, 256, 5, 1, 2),
    ("alexnet_conv3", 2, 256, 13, 384, 3, 1, 1), ("alexnet_conv4", 2, 384, 13, 384, 3, 1, 1),
    ("alexnet_conv5", 2, 384, 13, 256, 3, 1, 1), ("simple_conv1", 3, 3, 32, 20, 5, 1, 0),
    ("simple_conv2", 3, 20, 28, 50, 5, 1, 0), ("simple_conv3", 3, 50, 12, 120, 5, 1, 0),
    ("two_conv1", 4, 1, 28, 20, 5, 1, 0), ("two_conv2", 4, 20, 12, 50, 5, 1, 0),
]


@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_conv_layer_parity(ctx, case):
    name, m, c, h, kc, k, stride, pad = case
    rng = np.random.default_rng(sum(map(ord, name)))
    q = rng.integers(0, 256, (m, c, h, h), dtype=np.uint8)
    qw = rng.integers(-127, 128, (kc, c, k, k), dtype=np.int8)
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    s_w = row_scales(kc, rng)
    s_in, zp_in, zp_out = np.float32(0.03), 121, 37
    s_out = s_out_for(s_in, s_w, c * k * k)
    want, want_acc = pcp.conv2d_pc(q, qw, qb, stride, pad, s_in, zp_in, s_w, s_out, zp_out)
    nhwc_ok = kc % 16 == 0
    layouts = [(False, False), (True, True)] if nhwc_ok else [(False, False)]
    pk = (3, 2) if name.startswith("alexnet") else (2, 2)
    with pcp.per_channel_handles(abi.lib(), s_w):
        for relu in (False, True):
            wr = np.maximum(want, np.uint8(zp_out)) if relu else want
            for in_nhwc, out_nhwc in layouts:
                got, acc = ctx.layer_forward_pool(q, qw, qb, s_in, zp_in, 0.0, s_out, zp_out, stride, pad, in_nhwc=in_nhwc,
                                                  out_nhwc=out_nhwc, relu=relu, in_border=pad if in_nhwc else 0,
                                                  out_border=1 if out_nhwc else 0)
                assert np.array_equal(acc, want_acc), "%s: accumulators" % name
                assert np.array_equal(got, wr), "%s relu=%d nhwc=%d/%d" % (name, relu, in_nhwc, out_nhwc)
            # a folded max-pool (3x3/2 for AlexNet's convs, 2x2/2 for the small nets), re-biased layouts on AlexNet conv2-5
            wp = orc.max_pool2d(wr, *pk)
            forms = [(nhwc_ok, nhwc_ok, False, False)]
            if nhwc_ok and name.startswith("alexnet") and name != "alexnet_conv1":
                forms.append((True, True, True, True))
            for in_nhwc, out_nhwc, in_s8, out_s8 in forms:
                got, acc = ctx.layer_forward_pool(q, qw, qb, s_in, zp_in, 0.0, s_out, zp_out, stride, pad, in_nhwc=in_nhwc,
                                                  out_nhwc=out_nhwc, relu=relu, in_border=pad if in_nhwc else 0, pool=pk,
                                                  in_s8=in_s8, out_s8=out_s8)
                assert np.array_equal(got, wp), "%s pool relu=%d s8=%d" % (name, relu, out_s8)


LINEARS = [("fc6", 5, 9216, 4096), ("fc7", 300, 4096, 4096), ("fc8", 7, 4096, 10), ("two_conv_fc1", 9, 800, 500),
           ("n10", 33, 256, 10), ("n20", 130, 512, 20), ("n50", 64, 1024, 50), ("n100", 3, 784, 100)]


@pytest.mark.parametrize("case", LINEARS, ids=[c[0] for c in LINEARS])
def test_linear_layer_parity(ctx, case):
    name, m, k, n = case
    rng = np.random.default_rng(sum(map(ord, name)))
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    qw = rng.integers(-127, 128, (n, k), dtype=np.int8)
    qb = rng.integers(-127, 128, n, dtype=np.int8)
    s_w = row_scales(n, rng)
    s_in, zp_in, zp_out = np.float32(0.02), 130, 61
    s_out = s_out_for(s_in, s_w, k)
    want, a0, _ = pcp.linear_pc(q, qw, qb, s_in, zp_in, s_w, s_out, zp_out)
    with pcp.per_channel_handles(abi.lib(), s_w):
        for relu in (False, True):
            got, acc, _ = ctx.layer_forward_fused("linear", q, qw, qb, s_in, zp_in, 0.0, s_out, zp_out, relu=relu)
            assert np.array_equal(acc, a0), name
            assert np.array_equal(got, np.maximum(want, np.uint8(zp_out)) if relu else want), "%s relu=%d" % (name, relu)
        ctx.set_force_fallback(True)  # the exact any-geometry kernel
        try:
            got, _, _ = ctx.layer_forward_fused("linear", q, qw, qb, s_in, zp_in, 0.0, s_out, zp_out)
        finally:
            ctx.set_force_fallback(False)
        assert np.array_equal(got, want), "%s fallback" % name


def test_weight_scales_and_bad_scales(ctx):
    lib = abi.lib()
    qw = np.ones((4, 16), np.int8)
    qb = np.zeros(4, np.int8)
    L = C.c_void_p()
    for bad in ([1e-3, -1e-3, 1e-3, 1e-3], [1e-3, np.inf, 1e-3, 1e-3], [np.nan, 1e-3, 1e-3, 1e-3]):
        s = np.float32(bad)
        rc = lib.i8ie_linear_create_per_channel(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), 4, 16,
                                                s.ctypes.data_as(C.c_void_p), C.byref(L))
        assert rc != 0
    s = np.float32([1e-3, 0.0, 2e-3, 5e-4])
    abi.ck(lib.i8ie_linear_create_per_channel(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), 4, 16,
                                              s.ctypes.data_as(C.c_void_p), C.byref(L)))
    out, pc = np.empty(4, np.float32), C.c_int(-1)
    abi.ck(lib.i8ie_layer_weight_scales(L, out.ctypes.data_as(C.c_void_p), 4, C.byref(pc)))
    assert pc.value == 1 and np.array_equal(out, s)
    lib.i8ie_layer_destroy(L)
    abi.ck(lib.i8ie_linear_create(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), 4, 16, C.c_float(0.5),
                                  C.byref(L)))
    abi.ck(lib.i8ie_layer_weight_scales(L, out.ctypes.data_as(C.c_void_p), 4, C.byref(pc)))
    assert pc.value == 0 and np.all(out == 0.5)
    lib.i8ie_layer_destroy(L)


def test_standalone_down_scale_per_channel(ctx):
    rng = np.random.default_rng(8)
    acc = rng.integers(-2**22, 2**22, (37, 19)).astype(np.int32)
    s_w = row_scales(19, rng)
    s_w[4] = 0.0
    want = pcp.down_scale_pc(acc, np.float32(0.03), s_w, np.float32(0.2), 9)
    da, ds, do = ctx.put(acc), ctx.put(s_w), ctx.empty(acc.shape, np.uint8)
    abi.ck(abi.lib().i8ie_down_scale_per_channel(ctx.h, da.ptr, do.ptr, C.c_int64(37), 19, C.c_float(0.03), ds.ptr,
                                                 C.c_float(0.2), C.c_uint8(9)))
    got = do.get()
    for b in (da, ds, do):
        b.free()
    assert np.array_equal(got, want)


def u8_tensor(q):
    """an i8ie u8 tensor holding q with scale 1, zero point 0 (x / 1 + 0 truncates to x exactly)"""
    import _CXX_i8ie as cx
    import i8ie

    return i8ie.Tensor(cx.quantize(cx.tensor(np.asarray(q, np.float32)), 1.0, 0))


def test_exact_replay_columns_and_zero_scale():
    """Scales that put C * ms[j] exactly on half-integers in some columns (the guard replays them), and a column with
    s_w[j] = 0, restored through load_quantized."""
    import i8ie

    rng = np.random.default_rng(21)
    m, k, n = 64, 256, 32
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    qw = rng.integers(-20, 21, (n, k), dtype=np.int8)
    qb = rng.integers(-50, 51, n, dtype=np.int8)
    s_w = row_scales(n, rng) * np.float32(10)
    s_w[1::4] = np.float32(0.5)  # ms = 0.5: every odd C lands on a rounding boundary
    s_w[2::4] = np.float32(0.25)
    s_w[3] = 0.0
    lin = i8ie.Linear(k, n)
    lin.layer.load_quantized(qw, qb, s_w, 1.0, 100)
    assert lin.is_per_channel() and np.array_equal(lin.weight_scales(), s_w)
    with pytest.raises(RuntimeError):
        lin.weight_scale()
    got = lin(u8_tensor(q)).numpy()
    want, _, _ = pcp.linear_pc(q, qw, qb, np.float32(1), 0, s_w, np.float32(1), 100)
    assert np.array_equal(got, want)
    assert np.all(got[:, 3] == 100)


# ---- whole networks -------------------------------------------------------------------------------------------
def pc_net(name, seed=42):
    from int8inferenceengine_amd import workloads as wl

    sd = wl.synthetic_state_dict(name, seed)
    return wl.calibrated(name, sd, per_channel=True), sd


@pytest.mark.parametrize("name,batch", [("alexnet", 100), ("alexnet", 1000), ("simple_conv", 50), ("two_conv", 64),
                                        ("mnist_fc", 100)])
def test_network_bit_exact(name, batch):
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    net, sd = pc_net(name)
    x = wl.synthetic_input(name, batch, seed=5)
    got = net(i8ie.tensor(x)).numpy()
    rows = np.r_[0:6, batch - 6:batch] if batch > 200 else np.arange(batch)  # (images are independent)
    qp = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
    want = pcp.forward_pc(wl.NETWORKS[name], x[rows], pcp.quantize_layers_pc(wl.NETWORKS[name], sd), qp)
    assert np.array_equal(got[rows].view(np.uint32), want.view(np.uint32))
    for a in wl.layer_names(name):  # the net holds the per-channel weights
        L = getattr(net, a)
        qw, _, s = pcp.quantize_weight_pc(sd[a + ".weight"], sd[a + ".bias"])
        assert L.is_per_channel() and np.array_equal(L.weight_scales(), s) and np.array_equal(L.layer.q_weight(), qw)


def test_graph_replay_equals_eager():
    import i8ie
    from int8inferenceengine_amd import workloads as wl
    from int8inferenceengine_amd.graph import GraphedForward

    net, _ = pc_net("alexnet", seed=5)
    x = wl.synthetic_input("alexnet", 125, seed=3)
    want = net(i8ie.tensor(x)).numpy()
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy().view(np.uint32), want.view(np.uint32))


def test_save_load_round_trip(tmp_path):
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    names = wl.layer_names("two_conv")
    net, _ = pc_net("two_conv", seed=9)
    x = wl.synthetic_input("two_conv", 32, seed=4)
    want = net(i8ie.tensor(x)).numpy()
    assert set(net.quantized_state_dict()) == {a + s for a in names for s in (".q_weight", ".q_bias", ".qparams", ".w_scales")}
    path = str(tmp_path / "pc.npz")
    net.save_quantized(path)
    fresh = wl.build("two_conv")
    fresh.load_quantized_file(path)
    assert np.array_equal(fresh(i8ie.tensor(x)).numpy().view(np.uint32), want.view(np.uint32))
    pt = wl.calibrated("two_conv", wl.synthetic_state_dict("two_conv", 9))  # a per-tensor net keeps exactly its keys
    assert set(pt.quantized_state_dict()) == {a + s for a in names for s in (".q_weight", ".q_bias", ".qparams")}


@pytest.mark.parametrize("batch", [125, 1000])
def test_same_kernels_as_per_tensor(batch):
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    x = wl.synthetic_input("alexnet", batch, seed=3)
    launched = []
    for pc in (False, True):
        net = wl.calibrated("alexnet", wl.synthetic_state_dict("alexnet"), per_channel=pc)
        net(i8ie.tensor(x)).numpy()  # (caches built)
        cx.synchronize()
        cx.profile_start()
        net(i8ie.tensor(x)).numpy()
        launched.append({k: v[0] for k, v in cx.profile_stop().items()})
    assert launched[0] == launched[1]


def test_accuracy_gain_on_row_scaled_layer():
    """One Linear layer whose weight rows are scaled log-uniformly over [1/30, 1]: the dequantized per-channel output's
    error against FP32 is below half the per-tensor one's."""
    import _CXX_i8ie as cx
    import i8ie

    rng = np.random.default_rng(5)
    k, n, m = 512, 256, 64
    w = (rng.standard_normal((n, k)) * 0.05 * np.exp(rng.uniform(np.log(1 / 30), 0, n))[:, None]).astype(np.float32)
    b = (rng.standard_normal(n) * 0.001).astype(np.float32)
    xf = rng.uniform(0, 3, (m, k)).astype(np.float32)
    ref = xf @ w.T + b
    errs = []
    for pc in (False, True):
        lin = i8ie.Linear(k, n)
        lin.load_weight(w)
        lin.load_bias(b)
        lin.convert(per_channel=pc)
        lin.set_output_qparams(float(np.abs(ref).max() * 2 / 255), 128)
        y = cx.dequantize(lin.layer(cx.quantize(cx.tensor(xf), 3.0 / 255, 0))).numpy()
        errs.append(float(np.abs(y - ref).mean()))
    assert errs[1] < 0.5 * errs[0], errs


# ---- kernel variants ------------------------------------------------------------------------------------------
NAMED = [0, 3, 5, 11, 12, 13, 50, 54, 70, 80, 81, 83, 84, 85]  # tests/test_gpu_variants.py
CASES = [("alexnet", 125), ("alexnet", 260), ("two_conv", 16)]
CHILD = r'''
import json, sys
import numpy as np
root, out, cases, fallback = sys.argv[1], sys.argv[2], json.loads(sys.argv[3]), sys.argv[4] == "1"
sys.path.insert(0, root)
import int8inferenceengine_amd  # noqa: F401
import _CXX_i8ie as cx
import i8ie
from int8inferenceengine_amd import workloads as wl
if fallback:
    cx.force_fallback(True)
logits, qparams = {}, {}
for name, batch in cases:
    key = "%s_%d" % (name, batch)
    net = wl.calibrated(name, wl.synthetic_state_dict(name), per_channel=True)
    logits[key] = net(i8ie.tensor(wl.synthetic_input(name, batch, seed=5))).numpy()
    qparams[key] = {a: [float(s), int(z)] for a, (s, z) in ((a, getattr(net, a).output_qparams()) for a in wl.layer_names(name))}
np.savez(out + ".npz", **logits)
with open(out + ".json", "w") as f:
    json.dump(qparams, f)
'''


def test_every_variant_and_fallback(tmp_path):
    from int8inferenceengine_amd import workloads as wl

    oracle = {}

    def want(name, batch, qp):
        key = (name, batch, json.dumps(qp, sort_keys=True))
        if key not in oracle:
            sd = wl.synthetic_state_dict(name)
            x = wl.synthetic_input(name, batch, seed=5)
            oracle[key] = pcp.forward_pc(wl.NETWORKS[name], x, pcp.quantize_layers_pc(wl.NETWORKS[name], sd),
                                         {a: (s, z) for a, (s, z) in qp.items()})
        return oracle[key]

    failed = []
    for v, fb in [(v, False) for v in NAMED] + [(0, True)]:
        tag = "fallback" if fb else "variant %d" % v
        out = str(tmp_path / ("v%d_%d" % (v, fb)))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out, json.dumps(CASES), "1" if fb else "0"], cwd=ROOT,
                           env=dict(os.environ, I8IE_KERNEL_VARIANT=str(v)), capture_output=True, text=True, timeout=600)
        if r.returncode < 0:
            pytest.fail("%s: child died by signal %d (no further children started)\n%s" % (tag, -r.returncode, r.stderr[-3000:]))
        if r.returncode != 0:
            failed.append("%s: exit %d: %s" % (tag, r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
            continue
        got = np.load(out + ".npz")
        with open(out + ".json") as f:
            qps = json.load(f)
        for name, batch in CASES:
            key = "%s_%d" % (name, batch)
            w = want(name, batch, qps[key])
            if got[key].shape != w.shape or not np.array_equal(got[key].view(np.uint32), w.view(np.uint32)):
                failed.append("%s: %s logits differ from the per-channel oracle" % (tag, key))
    assert not failed, "\n".join(failed)
