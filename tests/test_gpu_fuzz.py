"""Seeded random differential sweep of the layer entry points against the oracle: random conv / linear
geometries (all three conv paths, ragged channels, strides, paddings, kernel = image ...), random layouts,
borders, fused ReLU and kernel variants.  Every case compares INT32 accumulators and u8 outputs bit-exactly.
I8IE_FUZZ_CASES raises the case count for a long hunt (default: a quick sweep that fits the suite)."""
import os

import numpy as np
import pytest

import abi
import support
import synth

pytestmark = pytest.mark.gpu
N_CASES = int(os.environ.get("I8IE_FUZZ_CASES", "48"))


gpu = support.ctx_fixture()


@pytest.fixture(scope="module")
def orc():
    import orc as o

    return o


def _conv_geom(rng):
    kind = rng.integers(0, 4)
    if kind == 0:    # path A candidates: channels % 16 == 0
        c = int(rng.choice([16, 32, 48, 64, 96, 128]))
    elif kind == 1:  # small-C path candidates (stride % 4 == 0 chosen below)
        c = int(rng.integers(1, 5))
    else:            # anything
        c = int(rng.integers(1, 40))
    k = int(rng.choice([1, 2, 3, 5, 7, 11]))
    stride = int(rng.choice([4, 8])) if kind == 1 else int(rng.integers(1, 4))
    pad = int(rng.integers(0, k // 2 + 2))
    h = int(rng.integers(max(k - 2 * pad, 1), 30))
    w = int(rng.integers(max(k - 2 * pad, 1), 30))
    h, w = max(h, k - 2 * pad), max(w, k - 2 * pad)
    kc = int(rng.choice([1, 7, 16, 20, 32, 33, 64, 96, 130, 200]))
    n = int(rng.integers(1, 6))
    return n, c, h, w, kc, k, stride, pad


@pytest.mark.parametrize("case", range(N_CASES))
def test_random_conv_against_oracle(gpu, orc, case):
    rng = np.random.default_rng(10_000 + case)
    n, c, h, w, kc, k, stride, pad = _conv_geom(rng)
    zp_in = int(rng.integers(0, 256))
    cs = synth.conv_case(orc, 20_000 + case, n, c, h, w, kc, k, stride, pad, s_in=float(rng.uniform(0.005, 0.05)),
                         zp_in=zp_in)
    in_nhwc = bool(rng.integers(0, 2))
    out_nhwc = bool(rng.integers(0, 2))
    ib = int(rng.choice([0, pad, pad + 1])) if in_nhwc else 0
    ob = int(rng.integers(0, 3)) if (out_nhwc and kc % 16 == 0) else 0
    relu = bool(rng.integers(0, 2))
    variant = int(rng.choice([0, 0, 3, 5]))
    fallback = bool(rng.integers(0, 6) == 0)
    lib = abi.lib()
    abi.ck(lib.i8ie_ctx_set_option(gpu.h, 2, variant))
    gpu.set_force_fallback(fallback)
    try:
        out, acc, _ = gpu.layer_forward_fused("conv", cs["q_in"], cs["qw"], cs["qb"], cs["s_in"], cs["zp_in"], cs["s_w"],
                                              cs["s_out"], cs["zp_out"], stride=stride, pad=pad, in_nhwc=in_nhwc,
                                              out_nhwc=out_nhwc, relu=relu, in_border=ib, out_border=ob)
    finally:
        gpu.set_force_fallback(False)
        abi.ck(lib.i8ie_ctx_set_option(gpu.h, 2, 0))
    want = orc.relu(cs["out"], cs["zp_out"]) if relu else cs["out"]
    ctx = "geom %s nhwc %s/%s borders %d/%d relu %s variant %d fallback %s" % (
        (n, c, h, w, kc, k, stride, pad), in_nhwc, out_nhwc, ib, ob, relu, variant, fallback)
    assert np.array_equal(acc, cs["acc"]), ctx
    assert np.array_equal(out, want), ctx


@pytest.mark.parametrize("case", range(max(N_CASES // 2, 8)))
def test_random_linear_against_oracle(gpu, orc, case):
    rng = np.random.default_rng(30_000 + case)
    m = int(rng.choice([1, 3, 31, 64, 125, 130, 257]))
    k = int(rng.choice([1, 7, 16, 64, 100, 784, 800, 1024, 4096]))
    n = int(rng.choice([1, 3, 10, 16, 17, 40, 100, 256, 500]))
    cs = synth.linear_case(orc, 40_000 + case, m, k, n, s_in=float(rng.uniform(0.005, 0.05)),
                           zp_in=int(rng.integers(0, 256)))
    relu = bool(rng.integers(0, 2))
    fallback = bool(rng.integers(0, 6) == 0)
    flat = None
    if k % 4 == 0 and rng.integers(0, 2):
        hw = int(rng.choice([d for d in (4, 2) if k % d == 0]))
        flat = (k // hw, hw // 2 if hw == 4 else 1, 2)  # (c, h, w) with h * w == hw
    gpu.set_force_fallback(fallback)
    try:
        out, acc, _ = gpu.layer_forward_fused("linear", cs["q_in"], cs["qw"], cs["qb"], cs["s_in"], cs["zp_in"],
                                              cs["s_w"], cs["s_out"], cs["zp_out"], relu=relu,
                                              in_nhwc=flat is not None, flat_chw=flat)
    finally:
        gpu.set_force_fallback(False)
    want = orc.relu(cs["out"], cs["zp_out"]) if relu else cs["out"]
    ctx = "m %d k %d n %d relu %s fallback %s flat %s" % (m, k, n, relu, fallback, flat)
    assert np.array_equal(acc, cs["acc"]), ctx
    assert np.array_equal(out, want), ctx


# ---- random small networks through the i8ie surface (deferred launches, layouts, borders, flatten, fused head)
def _random_network(rng):
    c = int(rng.choice([1, 3, 4, 16]))
    h = int(rng.integers(14, 34))
    w = int(rng.integers(14, 34))
    layers, spec = {}, []
    ch, hh, ww = c, h, w
    for i in range(int(rng.integers(1, 4))):
        k = int(rng.choice([1, 3, 5]))
        stride = int(rng.choice([1, 1, 2, 4]))
        pad = int(rng.integers(0, k // 2 + 1))
        oh, ow = (hh - k + 2 * pad) // stride + 1, (ww - k + 2 * pad) // stride + 1
        if oh < 3 or ow < 3:
            break
        oc = int(rng.choice([8, 16, 20, 32, 48, 64]))
        layers["conv%d" % i] = ("conv", ch, oc, k, stride, pad)
        spec.append(("layer", "conv%d" % i))
        ch, hh, ww = oc, oh, ow
        if rng.integers(0, 4):
            spec.append(("relu",))
        if rng.integers(0, 2):
            pk, ps = (2, 2) if rng.integers(0, 2) else (3, 2)
            if hh >= pk + 1 and ww >= pk + 1:
                spec.append(("pool", pk, ps))
                hh, ww = (hh - pk) // ps + 1, (ww - pk) // ps + 1
                if rng.integers(0, 3) == 0:
                    spec.append(("relu",))
    feat = ch * hh * ww
    spec.append(("flatten", feat))
    dims = [feat] + [int(rng.choice([16, 50, 64, 100])) for _ in range(int(rng.integers(0, 3)))]
    dims.append(int(rng.choice([1, 10, 16, 17])))
    for j in range(len(dims) - 1):
        layers["fc%d" % j] = ("fc", dims[j], dims[j + 1])
        spec.append(("layer", "fc%d" % j))
        if j < len(dims) - 2 and rng.integers(0, 3):
            spec.append(("relu",))
    return layers, spec, (c, h, w)


@pytest.mark.parametrize("case", range(max(N_CASES // 4, 12)))
def test_random_network_logits_against_oracle(orc, case):
    import int8inferenceengine_amd  # noqa: F401
    import i8ie
    import pipeline
    from int8inferenceengine_amd import workloads as wl

    rng = np.random.default_rng(50_000 + case)
    entry = _random_network(rng)
    name = "_fuzz_%d" % case
    wl.NETWORKS[name] = entry
    try:
        sd = wl.synthetic_state_dict(name, seed=60_000 + case)
        net = wl.calibrated(name, sd, calib_batch=wl.synthetic_input(name, 24, seed=case))
        batch = int(rng.choice([1, 5, 32]))
        x = wl.synthetic_input(name, batch, seed=70_000 + case)
        got = net(i8ie.tensor(x)).numpy()
        qlayers = pipeline.quantize_layers(entry, sd)
        qparams = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
        want = pipeline.forward(entry, x, qlayers, qparams)
        assert got.shape == want.shape, (entry, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), entry
        # a second forward reuses cached buffers / borders: same answer
        assert np.array_equal(net(i8ie.tensor(x)).numpy().view(np.uint32), want.view(np.uint32)), entry
    finally:
        del wl.NETWORKS[name]


# ---- random MID-SIZE networks at batches of a few hundred images: the shapes the fused kernels are built for (first-stage
#      kernel with its pool, patch-stationary convs with and without a fused pool, re-biased storage between them, bordered
#      hand-overs, the few-row / tiled Linear kernels) reached through the i8ie surface with random geometry
def _random_midsize_network(rng):
    c = 3
    h = int(rng.integers(52, 100))
    w = int(rng.integers(52, 100))
    layers, spec = {}, []
    k0 = int(rng.choice([5, 7, 11]))
    s0 = int(rng.choice([4, 4, 4, 2]))
    p0 = int(rng.integers(0, k0 // 2 + 1))
    oc0 = int(rng.choice([32, 64, 96]))
    layers["conv0"] = ("conv", c, oc0, k0, s0, p0)
    spec.append(("layer", "conv0"))
    ch, hh, ww = oc0, (h - k0 + 2 * p0) // s0 + 1, (w - k0 + 2 * p0) // s0 + 1
    if rng.integers(0, 4):
        spec.append(("relu",))
    if s0 == 2 or rng.integers(0, 3) == 0:  # (stride 2 leaves large maps: always pool them)
        pk, ps = (2, 2) if rng.integers(0, 2) else (3, 2)
        spec.append(("pool", pk, ps))
        hh, ww = (hh - pk) // ps + 1, (ww - pk) // ps + 1
    for i in range(1, int(rng.integers(2, 4))):
        k = int(rng.choice([3, 3, 5, 1]))
        pad = int(rng.choice([k // 2, k // 2, 0]))
        oh, ow = hh - k + 2 * pad + 1, ww - k + 2 * pad + 1
        if oh < 4 or ow < 4:
            break
        oc = int(rng.choice([192, 256, 320, 384]))
        layers["conv%d" % i] = ("conv", ch, oc, k, 1, pad)
        spec.append(("layer", "conv%d" % i))
        ch, hh, ww = oc, oh, ow
        if rng.integers(0, 5):
            spec.append(("relu",))
        if rng.integers(0, 2) and hh >= 4 and ww >= 4:
            pk, ps = (2, 2) if rng.integers(0, 3) == 0 else (3, 2)
            spec.append(("pool", pk, ps))
            hh, ww = (hh - pk) // ps + 1, (ww - pk) // ps + 1
    feat = ch * hh * ww
    spec.append(("flatten", feat))
    dims = [feat, int(rng.choice([64, 256])), 10]
    for j in range(2):
        layers["fc%d" % j] = ("fc", dims[j], dims[j + 1])
        spec.append(("layer", "fc%d" % j))
        if j == 0:
            spec.append(("relu",))
    return layers, spec, (c, h, w)


@pytest.mark.parametrize("case", range(max(N_CASES // 8, 6)))
def test_random_midsize_network_logits_against_oracle(orc, case):
    import int8inferenceengine_amd  # noqa: F401
    import i8ie
    import pipeline
    from int8inferenceengine_amd import workloads as wl

    rng = np.random.default_rng(90_000 + case)
    entry = _random_midsize_network(rng)
    name = "_fuzzmid_%d" % case
    wl.NETWORKS[name] = entry
    try:
        sd = wl.synthetic_state_dict(name, seed=91_000 + case)
        net = wl.calibrated(name, sd, calib_batch=wl.synthetic_input(name, 16, seed=case))
        batch = int(rng.choice([200, 260, 330]))
        x = wl.synthetic_input(name, batch, seed=92_000 + case)
        got = net(i8ie.tensor(x)).numpy()
        qlayers = pipeline.quantize_layers(entry, sd)
        qparams = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
        want = pipeline.forward(entry, x, qlayers, qparams)
        assert got.shape == want.shape, (entry, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (entry, batch)
        # a second forward (cached weight packings, borders, layouts): same answer; and one at a small batch, where other
        # kernels take the same layers
        assert np.array_equal(net(i8ie.tensor(x)).numpy().view(np.uint32), want.view(np.uint32)), (entry, batch)
        small = net(i8ie.tensor(x[:7])).numpy()
        assert np.array_equal(small.view(np.uint32), want[:7].view(np.uint32)), (entry, batch)
    finally:
        del wl.NETWORKS[name]
