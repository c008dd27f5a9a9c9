"""ConvTranspose2d without a GPU: the flip and padding convention (the scatter definition against the equivalent convolution,
in float64 and in exact integers, and against torch), the argument rules of the C entries, the Python surface and state
machine, the workloads, the case list of the GPU tests, and that the expected bytes of those tests discriminate."""
import ctypes as C

import numpy as np
import pytest

import abi
import deconv_ref as dr
import pinned_networks as pn
import spec_ref as sr
from support import i8ie  # noqa: F401

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _feature():
    """every test of this file is about the transposed layer: the library must export its entries"""
    dr.bind(abi.lib())


# every geometry of the GPU cases, and the ones the issue names
KSPO = sorted(set(dr.GEOMETRIES) | {(c.k, c.s, c.p, c.op) for c in dr.CASES})


@pytest.mark.parametrize("geo", KSPO, ids=lambda g: "k%ds%dp%dop%d" % g)
def test_scatter_form_equals_equivalent_convolution(geo, orc):
    k, s, p, op = geo
    rng = np.random.default_rng(k * 1000 + s * 100 + p * 10 + op)
    h, w = (3, 4) if (2 * s - 2 * p + k + op) > 0 else (4, 5)
    x = rng.integers(-9, 10, (2, 3, h, w))
    wt = rng.integers(-9, 10, (3, 5, k, k))
    b = rng.integers(-9, 10, 5)
    a = dr.scatter(x, wt, b, s, p, op)
    assert a.shape == (2, 5) + dr.out_hw(h, w, k, s, p, op)
    assert np.array_equal(a, dr.equivalent_f64(x, wt, b, s, p, op))                       # float64 (integers: exact)
    ai = dr.scatter(x, wt, b, s, p, op, dtype=np.int64)
    assert ai.dtype == np.int64 and np.array_equal(ai, a.astype(np.int64))
    # exact integers through the oracle's own u8 x s8 -> s32 convolution of the equivalent problem
    zp = 121
    q = rng.integers(0, 256, (2, 3, h, w), dtype=np.uint8)
    qw_t = rng.integers(-127, 128, (3, 5, k, k), dtype=np.int8)
    qb = np.zeros(5, np.int8)
    _, acc = dr.deconv_u8(q, dr.equivalent_weight(qw_t), qb, s, p, op, f32(0.03), zp, f32(0.002), f32(1.0), 0)
    oc = orc.conv_offsets(dr.equivalent_weight(qw_t), qb, f32(0.03), zp)
    oh, ow = dr.out_hw(h, w, k, s, p, op)
    real = dr.scatter(q.astype(np.int64) - zp, qw_t, qb, s, p, op, dtype=np.int64)  # sum of (x - zp) w over the real taps
    full = acc.reshape(2, oh, ow, 5).transpose(0, 3, 1, 2).astype(np.int64)
    wsum = qw_t.astype(np.int64).sum(axis=(0, 2, 3))
    # the oracle's accumulator is the full-K sum over x~ (zp_in at every inserted position) plus its offset vector
    assert np.array_equal(full, real + (zp * wsum + oc.astype(np.int64)).reshape(1, -1, 1, 1))
    # ... and one changed input byte moves exactly the outputs its k x k patch reaches
    q2 = q.copy()
    q2[0, 0, 0, 0] ^= 0x55
    _, acc2 = dr.deconv_u8(q2, dr.equivalent_weight(qw_t), qb, s, p, op, f32(0.03), zp, f32(0.002), f32(1.0), 0)
    real2 = dr.scatter(q2.astype(np.int64) - zp, qw_t, qb, s, p, op, dtype=np.int64)
    assert np.array_equal((acc2.astype(np.int64) - acc).reshape(2, oh, ow, 5).transpose(0, 3, 1, 2), real2 - real)


@pytest.mark.parametrize("geo", KSPO, ids=lambda g: "k%ds%dp%dop%d" % g)
def test_definition_equals_torch(geo):
    import torch

    k, s, p, op = geo
    rng = np.random.default_rng(7)
    x = rng.integers(-9, 10, (2, 3, 4, 5)).astype(np.float64)
    wt = rng.integers(-9, 10, (3, 5, k, k)).astype(np.float64)
    b = rng.integers(-9, 10, 5).astype(np.float64)
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=s, padding=p,
                                                output_padding=op).numpy()
    assert want.shape[2:] == dr.out_hw(4, 5, k, s, p, op)
    assert np.array_equal(dr.scatter(x, wt, b, s, p, op), want)


def test_argument_rules_before_any_device_call():
    lib = dr.bind(abi.lib())
    qw, qb, sw = np.zeros(4 * 3 * 9, np.int8), np.zeros(4, np.int8), np.ones(4, f32)
    L = C.c_void_p()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    #        kc c  k  s  p  op
    bad = [(4, 3, 3, 0, 0, 0, b"stride"), (4, 3, 3, -1, 0, 0, b"stride"), (4, 3, 3, 2, 3, 0, b"padding"), (4, 3, 3, 2, -1, 0, b"padding"),
           (4, 3, 3, 2, 0, 2, b"output_padding"), (4, 3, 3, 1, 0, 1, b"output_padding"), (4, 3, 3, 2, 0, -1, b"output_padding"),
           (0, 3, 3, 1, 0, 0, b"non-positive"), (4, 0, 3, 1, 0, 0, b"non-positive"), (4, 3, 0, 1, 0, 0, b"non-positive")]
    for kc, c, k, s, p, op, msg in bad:
        # (a null ctx: an argument error must come first, the device is never reached)
        rc = lib.i8ie_conv_transpose2d_create(None, P(qw), P(qb), kc, c, k, s, p, op, C.c_float(1.0), C.byref(L))
        assert rc == -1 and msg in lib.i8ie_last_error(), (kc, c, k, s, p, op, lib.i8ie_last_error())
        rc = lib.i8ie_conv_transpose2d_create_per_channel(None, P(qw), P(qb), kc, c, k, s, p, op, P(sw), C.byref(L))
        assert rc == -1 and msg in lib.i8ie_last_error()
        rc = lib.i8ie_conv_transpose2d_u8s8(None, None, 1, c, 2, 2, None, kc, k, s, p, op, 0, None, 1.0, 1.0, 1.0, 0, None, None)
        assert rc == -1 and msg in lib.i8ie_last_error()
        rc = lib.i8ie_conv_transpose2d_f32(None, None, 1, c, 2, 2, None, None, kc, k, s, p, op, None)
        assert rc == -1 and msg in lib.i8ie_last_error(), (kc, c, k, s, p, op)
    bad_scale = np.array([1, -1, 1, 1], f32)
    rc = lib.i8ie_conv_transpose2d_create_per_channel(None, P(qw), P(qb), 4, 3, 3, 1, 0, 0, P(bad_scale), C.byref(L))
    assert rc == -1 and b"scale" in lib.i8ie_last_error()
    rc = lib.i8ie_conv_transpose2d_create(None, P(qw), P(qb), 4, 3, 3, 1, 0, 0, C.c_float(1.0), C.byref(L))
    assert rc == -1 and b"null" in lib.i8ie_last_error()  # valid geometry: the null ctx is what is refused
    rc = lib.i8ie_conv_transpose2d_f32(None, None, 1, 3, 2, 2, None, None, 4, 3, 1, 0, 0, None)
    assert rc == -1 and b"null" in lib.i8ie_last_error()
    for kc, c, k in ((4, 3, 65536), (4, 1 << 20, 1 << 10)):  # the size guards, on every entry alike
        assert lib.i8ie_conv_transpose2d_f32(None, None, 1, c, 2, 2, None, None, kc, k, 1, 0, 0, None) == -1
        assert b"null" not in lib.i8ie_last_error()
        assert lib.i8ie_conv_transpose2d_create(None, P(qw), P(qb), kc, c, k, 1, 0, 0, C.c_float(1.0), C.byref(L)) == -1
        assert b"null" not in lib.i8ie_last_error()


def test_surface_and_state_machine(i8ie):
    """Up to prepare().  convert() and load_quantized() of a layer WITH weights create the device handle (as for Conv2d and
    Linear), so the save / load round trip of a transposed layer cannot run here: it is in tests/test_gpu_deconv.py
    (test_unet_bit_exact, batch 2, and test_save_load_round_trip_of_one_layer).  What runs here without a device: the shape
    and value checks of load_quantized, which come before the handle is made."""
    import _CXX_i8ie as cx

    assert "ConvTranspose2d" in i8ie.__all__ and hasattr(cx, "ConvTranspose2d")
    L = i8ie.ConvTranspose2d(3, 5, 4, stride=2, padding=1)
    assert isinstance(L, i8ie.Layer) and L.groups() == 1 and L.output_qparams() == (1.0, 0)
    for kw in (dict(stride=0), dict(stride=-1), dict(padding=4), dict(padding=-1), dict(stride=2, output_padding=2),
               dict(output_padding=1), dict(output_padding=-1)):
        with pytest.raises(RuntimeError, match="ConvTranspose2d"):
            i8ie.ConvTranspose2d(3, 5, 4, **kw)
    for a in ((0, 5, 3), (3, 0, 3), (3, 5, 0)):
        with pytest.raises(RuntimeError):
            i8ie.ConvTranspose2d(*a)
    L.load_weight(np.ones((3, 5, 4, 4), f32))   # torch's layout
    L.load_bias(np.zeros(5, f32))
    for shape in ((5, 3, 4, 4), (3, 5, 3, 3), (3, 5, 4)):
        with pytest.raises(RuntimeError, match=r"\[in, out, k, k\]"):
            L.load_weight(np.ones(shape, f32))
    L.set_output_qparams(0.5, 17)
    assert L.output_qparams() == (0.5, 17)
    with pytest.raises(RuntimeError):
        L.layer.q_weight()  # not converted yet
    L.prepare()  # (no device call)
    with pytest.raises(RuntimeError, match=r"\[in, out, k, k\]"):
        L.layer.load_quantized(np.zeros((5, 3, 4, 4), np.int8), np.zeros(5, np.int8), 0.1, 0.5, 3)
    with pytest.raises(RuntimeError):
        L.layer.load_quantized(np.zeros((3, 5, 4, 4), np.int8), np.zeros(5, np.int8), 0.1, 0.5, 256)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.conv = i8ie.Conv2d(2, 3, 3, padding=1)
            self.up = i8ie.ConvTranspose2d(3, 4, 2, stride=2)
            self.cat = i8ie.Concat()

        def forward(self, x):
            return self.cat([self.up(self.conv(x))])

    net = Net()
    net.load({"conv.weight": np.ones((3, 2, 3, 3), f32), "conv.bias": np.zeros(3, f32), "up.weight": np.ones((3, 4, 2, 2), f32),
              "up.bias": np.zeros(4, f32)})
    assert [k for k, _ in net._layers()] == ["conv", "up", "cat"]
    net.prepare()
    with pytest.raises(RuntimeError, match="up|conv"):
        net.quantized_state_dict()


def test_swap_flip_is_the_equivalent_weight():
    w = np.arange(2 * 3 * 2 * 2).reshape(2, 3, 2, 2)
    e = dr.equivalent_weight(w)
    assert e.shape == (3, 2, 2, 2) and e[1, 0, 0, 1] == w[0, 1, 1, 0] and np.array_equal(dr.equivalent_weight(e), w)


def _check_spec(name):
    from int8inferenceengine_amd import workloads as wl

    layers, spec, shape = wl.NETWORKS[name]
    saved, used, macs, cats = {}, set(), {}, {}

    def run(ops, cur):
        for op in ops:
            if op[0] == "layer":
                L = layers[op[1]]
                assert op[1] not in used and cur[0] == L[1], (name, op, cur)
                used.add(op[1])
                if L[0] == "conv":
                    cur = (L[2], (cur[1] - L[3] + 2 * L[5]) // L[4] + 1, (cur[2] - L[3] + 2 * L[5]) // L[4] + 1)
                    macs[op[1]] = cur[1] * cur[2] * L[2] * L[1] * L[3] * L[3]
                else:
                    assert L[0] == "deconv" and len(L) == 7
                    macs[op[1]] = cur[1] * cur[2] * L[1] * L[2] * L[3] * L[3]
                    cur = (L[2],) + dr.out_hw(cur[1], cur[2], L[3], L[4], L[5], L[6])
            elif op[0] == "save":
                assert op[1] not in saved
                saved[op[1]] = cur
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]])
            elif op[0] == "concat":
                parts = [cur] + [saved.pop(t) for t in op[2]]
                assert all(p[1:] == cur[1:] for p in parts), (name, op, parts)
                cats[op[1]] = [p[0] for p in parts]
                cur = (sum(p[0] for p in parts),) + cur[1:]
            elif op[0] == "pool":
                cur = (cur[0], (cur[1] - op[1]) // op[2] + 1, (cur[2] - op[1]) // op[2] + 1)
            else:
                assert op[0] == "relu", op
        return cur

    out = run(spec, shape)
    assert not saved and used == set(layers)
    return out, cats, macs


def test_unet_tiny_workload(i8ie):
    from int8inferenceengine_amd import workloads as wl

    out, cats, macs = _check_spec("unet_tiny")
    layers, spec, shape = wl.NETWORKS["unet_tiny"]
    assert shape == (3, 32, 32) and out == (10, 32, 32) and [op for op in spec if op[0] == "pool"] == [("pool", 2, 2)] * 2
    ups = {a: L[3:] for a, L in layers.items() if L[0] == "deconv"}
    assert sorted(ups.values()) == [(2, 2, 0, 0), (3, 2, 1, 1), (4, 2, 1, 0)]
    assert cats == {"cat2": [20, 7, 20], "cat1": [12, 12]}
    counts = [c for cs in cats.values() for c in cs] + [sum(cs) for cs in cats.values()]
    assert any(c % 16 for c in counts) and any(c % 4 for c in counts)
    for cat, conv in (("cat2", "dec2"), ("cat1", "dec1")):  # a 3x3 pad-1 conv behind each join
        i = [op[:2] for op in spec].index(("concat", cat))
        assert spec[i + 1] == ("layer", conv) and layers[conv][3:6] == (3, 1, 1)
    assert layers["head"] == ("conv", 12, 10, 1, 1, 0) and spec[-1] == ("layer", "head")
    sd = wl.synthetic_state_dict("unet_tiny")
    assert sd["up2b.weight"].shape == (32, 7, 4, 4) and sd["up2b.bias"].shape == (7,) and sd["up1.weight"].shape == (20, 12, 3, 3)
    # the main path (the conv / deconv of a branch is not counted, as in resnet_tiny)
    assert wl.macs_per_image("unet_tiny") == sum(v for a, v in macs.items() if a != "up2b")
    net = wl.build("unet_tiny")
    assert isinstance(net.up1, i8ie.ConvTranspose2d) and isinstance(net.cat1, i8ie.Concat)
    net.load(sd)


def test_unet_cifar_workload():
    from int8inferenceengine_amd import workloads as wl

    out, cats, macs = _check_spec("unet_cifar")
    layers, spec, shape = wl.NETWORKS["unet_cifar"]
    assert shape == (3, 32, 32) and out == (10, 32, 32)
    assert {a: L for a, L in layers.items() if L[0] == "deconv"} == {"up3": ("deconv", 512, 256, 2, 2, 0, 0),
                                                                     "up2": ("deconv", 256, 128, 2, 2, 0, 0),
                                                                     "up1": ("deconv", 128, 64, 2, 2, 0, 0)}
    assert cats == {"cat3": [256, 256], "cat2": [128, 128], "cat1": [64, 64]}
    assert all(L[3:6] == (3, 1, 1) for a, L in layers.items() if L[0] == "conv" and a != "head") and layers["head"] == ("conv", 64, 10, 1, 1, 0)
    assert macs["up3"] == 4 * 4 * 512 * 256 * 4 and macs["up1"] == 16 * 16 * 128 * 64 * 4
    assert wl.macs_per_image("unet_cifar") == sum(macs.values())


def test_existing_networks_keep_their_macs():
    from int8inferenceengine_amd import workloads as wl

    before = pn.NAMES[:pn.NAMES.index("unet_tiny")]
    assert len(before) == 15 and {n: wl.macs_per_image(n) for n in before} == {n: pn.MACS[n] for n in before}
    sd = wl.synthetic_state_dict("two_conv")  # (the draw order of the existing networks is unchanged)
    assert sd["conv1.weight"].shape == (20, 1, 5, 5)


def test_case_list_contains_every_class():
    have = set(c for case in dr.CASES for c in case.classes)
    assert not [c for c in dr.CLASSES if c not in have]
    by = lambda cls: [c for c in dr.CASES if cls in c.classes]
    assert {(c.k, c.s, c.p, c.op) for c in by("geo")} == set(dr.GEOMETRIES)
    for n in (1, 3, 4, 16, 20, 64, 65):
        assert all(c.c == n for c in by("in%d" % n))
    for n in (31, 32, 63, 64, 65, 128):
        assert all(dr.geom(c)[3] == n for c in by("phk%d" % n))
    for n in (1, 3, 16, 17, 63, 64, 65):
        assert all(c.kc == n for c in by("out%d" % n))
    for n in (1, 15, 16, 17, 127, 128, 129):
        # (the kernel tiles the (image, qy, qx) cell grid: the count that matters is geom()'s, over more than one image)
        assert by("cells%d" % n) and all(dr.geom(c)[4] == n and (c.m > 1 or n == 1) for c in by("cells%d" % n))
    assert all(dr.geom(c)[4] % 16 not in (0, 1) and dr.dispatch(c).nph == 1 for c in by("ragged_phase_loop"))
    assert all((c.h, c.w) == (1, 1) for c in by("in1x1")) and all(c.h == 1 and c.w > 1 for c in by("in1xw"))
    assert all(c.w == 1 and c.h > 1 for c in by("inhx1"))
    assert all(c.k < c.s for c in by("empty_phase") + by("direct_empty_phase")) and all(c.s == 1 for c in by("single_phase"))
    assert all(c.p == c.k - 1 for c in by("p_eq_k1")) and all(c.op == c.s - 1 and c.k == c.s for c in by("op_eq_s1"))
    for lay in ("cc", "ch", "hc", "hh"):
        assert all((c.in_nhwc, c.out_nhwc) == (lay[0] == "h", lay[1] == "h") for c in by("lay_" + lay))
    for b in (0, 1, 2):
        assert all(c.in_nhwc and c.ib == b for c in by("ib%d" % b)) and all(c.out_nhwc and c.ob == b for c in by("ob%d" % b))
    assert all(c.zp_in == 0 for c in by("zp0")) and all(c.zp_in == 255 for c in by("zp255"))
    assert all(c.extreme for c in by("extreme")) and all(c.zero_col and c.pc for c in by("zero_col"))
    # both kernels, every gather width, both scale modes, the shared-fragment form and the phase loop
    disp = [dr.dispatch(c) for c in dr.CASES]
    assert {d.kernel for d in disp} == {"deconv_mfma", "deconv_direct"}
    assert {(d.G, d.pc, d.nph) for d in disp if d.kernel == "deconv_mfma"} >= {(g, pc, n) for g in (16, 4, 1) for pc in (False, True) for n in (1,)}
    assert {(d.G, d.nph) for d in disp if d.kernel == "deconv_mfma"} >= {(16, 4), (1, 4)}
    assert {(d.dot4, d.pc, d.vec_out) for d in disp if d.kernel == "deconv_direct"} >= {(True, False, 0), (False, True, 0), (False, False, 1)}


@pytest.mark.parametrize("case", dr.CASES, ids=[c.name for c in dr.CASES])
def test_expected_bytes_are_not_clamped(case):
    """the oracle alone: at most 10 % of the expected bytes of a GPU case on 0 or 255 without ReLU"""
    want = dr.reference(case)["want"]
    share = float(((want == 0) | (want == 255)).mean())
    assert share <= 0.10, (case.name, share)
    assert len(np.unique(want)) >= 4


@pytest.mark.parametrize("name", ["unet_tiny", "unet_cifar"])
def test_network_deconv_outputs_are_not_clamped(name):
    """the oracle alone, with the float64 stand-in for calibration: at most 20 % of every up-conv's expected bytes on a clamp"""
    from int8inferenceengine_amd import workloads as wl

    sd = wl.synthetic_state_dict(name, sr.WEIGHT_SEED)
    qp, jqp = sr.fp32_qparams(wl.NETWORKS[name], sd, wl.synthetic_input(name, sr.CALIB_IMAGES, seed=sr.CALIB_SEED))
    assert sorted(qp) == sorted(wl.layer_names(name)) and sorted(jqp) == sorted(wl.concat_names(name))
    trace = {}
    x = wl.synthetic_input(name, 1, seed=sr.INPUT_SEED)
    y = sr.forward(wl.NETWORKS[name], x, sr.quantize_layers(wl.NETWORKS[name], sd), qp, jqp, False, dr.tracer(wl.NETWORKS[name][0], trace))
    assert y.shape == (1, 10, 32, 32) and len(trace) == 3
    for a, q in trace.items():
        share = float(((q == 0) | (q == 255)).mean())
        print(a, round(share, 3), len(np.unique(q)))
        assert share <= 0.20 and len(np.unique(q)) > 16, (a, share)
