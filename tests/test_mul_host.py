"""The quantized broadcast Mul without a GPU: the numpy restatement against an independent integer formulation where that
one is exact, the parameter sets of the GPU tests (that they cannot pass on clamps alone), the Python / extension / C
surface and its argument checks, the Mul's state machine and place in Module, the two new workloads, and the non-triviality
of the network tests on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import abi
import mul_ref as mr
import pinned_networks as pn
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

f32 = np.float32


# powers of two: fa, fb, their product and the quotient by s_out are exact in fp32 (|da * db| < 2^16), and so is the sum with
# zp_out (a multiple of 2^-m below 2^17), so the restatement must equal the integer formula
@pytest.mark.parametrize("scales", [(2.0 ** -4, 2.0 ** -3, 2.0 ** -1), (0.5, 0.25, 16.0), (2.0 ** -6, 2.0 ** -7, 2.0 ** -5), (1.0, 1.0, 1.0),
                                    (4.0, 0.125, 32.0)], ids=lambda s: "k%g" % (s[0] * s[1] / s[2]))
@pytest.mark.parametrize("zps", [(0, 0, 0), (128, 128, 128), (255, 0, 128), (3, 250, 255), (17, 99, 0), (128, 0, 128)])
@pytest.mark.parametrize("relu", [False, True])
def test_restatement_equals_integer_arithmetic_for_power_of_two_scales(scales, zps, relu):
    """q = clamp(trunc((a - zp_a)(b - zp_b) k + zp_out)), k = s_a s_b / s_out = 2^-m, in integers: a negative value clamps to
    0 and a non-negative one truncates by the floor of the shift."""
    a, b = support.byte_pairs()
    s_a, s_b, s_out = scales
    zp_a, zp_b, zp_out = zps
    k = s_a * s_b / s_out
    m = int(round(-np.log2(k)))
    assert m >= 0 and 2.0 ** -m == k
    num = (a.astype(np.int64) - zp_a) * (b.astype(np.int64) - zp_b) + (zp_out << m)
    want = np.where(num < 0, 0, np.minimum(num >> m, 255))
    if relu:
        want = np.maximum(want, zp_out)
    got = mr.mul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu)
    assert got.dtype == np.uint8 and got.shape == (65536,) and np.array_equal(got, want)


@pytest.mark.parametrize("name,qp", mr.QP, ids=[q[0] for q in mr.QP])
def test_restatement_commutes_with_swapped_parameters(name, qp):
    a, b = support.byte_pairs()
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    for relu in (False, True):
        assert np.array_equal(mr.mul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu), mr.mul_u8(b, zp_b, s_b, a, zp_a, s_a, s_out, zp_out, relu))


def test_saturation_relu_floor_and_gate_broadcast():
    a = np.array([255, 255, 0, 0, 130, 128], np.uint8)
    b = np.array([255, 0, 0, 255, 131, 7], np.uint8)
    # (a - 128)(b - 128) / 4 + 128 with s_out = 4
    got = mr.mul_u8(a, 128, 1.0, b, 128, 1.0, 4.0, 128)
    assert got.tolist() == [255, 0, 255, 0, 129, 128]
    # the relu floor is the RESULT's zero point
    got = mr.mul_u8(a, 128, 1.0, b, 128, 1.0, 4.0, 100, relu=True)
    assert got.tolist() == [255, 100, 255, 100, 101, 100]
    # truncation toward zero of a positive t: 1 * 1 / 3 = 0.33 -> 0, 5 * 1 / 3 = 1.67 -> 1
    assert mr.mul_u8(np.array([1, 5], np.uint8), 0, 1.0, np.ones(2, np.uint8), 0, 1.0, 3.0, 0).tolist() == [0, 1]
    # a negative t inside (-1, 0) is 0 by the clamp, not by the cast
    assert mr.mul_u8(np.array([0], np.uint8), 1, 1.0, np.array([1], np.uint8), 0, 1.0, 3.0, 0).tolist() == [0]
    # a gate [n, c] (or [n, c, 1, 1]) multiplies every pixel of its image and channel
    x = np.arange(2 * 3 * 2 * 2, dtype=np.uint8).reshape(2, 3, 2, 2)
    g = np.array([[0, 1, 2], [3, 4, 5]], np.uint8)
    want = (x.astype(np.int32) * g.reshape(2, 3, 1, 1)).astype(np.uint8)
    for gate in (g, g.reshape(2, 3, 1, 1)):
        assert np.array_equal(mr.mul_u8(x, 0, 1.0, gate, 0, 1.0, 1.0, 0), want)
    with pytest.raises(AssertionError):
        mr.mul_u8(x, 0, 1.0, g[:1], 0, 1.0, 1.0, 0)


def test_parameter_sets_cannot_pass_on_clamps_alone():
    a, b = support.byte_pairs()
    assert len(mr.QP) >= 30 and len({n for n, _ in mr.QP}) == len(mr.QP) and len(mr.GATE_SETS) >= 5
    names = {n for n, _ in mr.QP}
    assert {"zero_s_a", "denormal_s_a", "denormal_products", "overflowing_products", "equal_saturating"} <= names
    mostly_inside = 0
    for name, (s_a, zp_a, s_b, zp_b, s_out, zp_out) in mr.QP:
        q = mr.mul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out)
        clamped = float(((q == 0) | (q == 255)).mean())
        mostly_inside += int(clamped < 0.5)
        if name in mr.GATE_SETS:
            # a hardsigmoid gate against a's own parameters: |t - zp| <= |a - zp| (to rounding), so only a few pairs touch an end
            assert (f32(s_b), zp_b) == (f32(1.0 / 255), 0) and (s_out, zp_out) == (s_a, zp_a)
            assert clamped < 0.01 and np.unique(q).size >= 200, (name, clamped, np.unique(q).size)
    assert mostly_inside * 2 >= len(mr.QP), mostly_inside


lib = support.lib_fixture(mr)


def test_new_symbols_are_declared_and_exported(lib):
    names = abi.declared_symbols()
    for n in ["i8ie_mul_u8", "i8ie_mul_u8_nhwc", "i8ie_mul_f32"]:
        assert n in names and hasattr(lib, n), n
    assert lib.i8ie_version() == 1


def test_entry_points_check_arguments_before_any_device_call(lib):
    one, ctx = C.c_void_p(16), C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)

    def flat(ctx=ctx, a=one, b=one, o=one, n=16, s=(1.0, 1.0, 1.0)):
        return lib.i8ie_mul_u8(ctx, a, b, o, n, s[0], 0, s[1], 0, s[2], 0, 0), lib.i8ie_last_error()

    def nhwc(ctx=ctx, a=one, b=one, o=one, ab=0, bb=0, ob=0, gate=1, n=1, c=16, h=1, w=1, s=(1.0, 1.0, 1.0)):
        return lib.i8ie_mul_u8_nhwc(ctx, a, ab, 0, b, bb, 0, gate, o, ob, 0, n, c, h, w, s[0], 0, s[1], 0, s[2], 0, 0), lib.i8ie_last_error()

    def fp(ctx=ctx, a=one, b=one, o=one, n=4, run=0):
        return lib.i8ie_mul_f32(ctx, a, b, o, n, run), lib.i8ie_last_error()

    for f in (flat, nhwc, fp):
        for kw in ({"ctx": None}, {"a": None}, {"b": None}, {"o": None}):
            rc, msg = f(**kw)
            assert rc == -1 and b"null" in msg, (f.__name__, kw)
    bad_scales = [(1.0, 1.0, 0.0), (1.0, 1.0, -0.5), (1.0, 1.0, float("inf")), (1.0, 1.0, float("nan")), (float("nan"), 1.0, 1.0),
                  (1.0, float("inf"), 1.0)]
    for s in bad_scales:
        for f, kws in ((flat, [{}]), (nhwc, [{"gate": 0}, {"gate": 1}])):
            for kw in kws:
                rc, msg = f(s=s, **kw)
                assert rc == -1 and b"scale" in msg, (f.__name__, s)
    rc, msg = flat(n=-1)
    assert rc == -1 and b"negative" in msg
    for kw in ({"n": -4}, {"run": -1}):
        rc, msg = fp(**kw)
        assert rc == -1 and b"negative" in msg
    rc, msg = fp(n=6, run=4)
    assert rc == -1 and b"divide" in msg
    for gate in (0, 1):
        for kw in ({"ab": -1}, {"bb": -1}, {"ob": -1}, {"n": 0}, {"n": -1}, {"c": 0}, {"h": 0}, {"w": -2}, {"h": 1 << 16, "w": 1 << 16}):
            rc, msg = nhwc(gate=gate, **kw)
            assert rc == -1 and b"dimension" in msg, kw
    odd = C.c_void_p(18)
    for kw in ({"a": odd}, {"b": odd}, {"o": odd}):
        rc, msg = flat(**kw)
        assert rc == -1 and b"aligned" in msg, kw
        rc, msg = fp(**kw)
        assert rc == -1 and b"aligned" in msg, kw
    rc, msg = fp(b=odd, n=8, run=4)           # a gate is read element by element, but as floats
    assert rc == -1 and b"aligned" in msg
    assert flat(n=0)[0] == 0 and fp(n=0)[0] == 0 and fp(n=0, run=4)[0] == 0  # nothing to do: no device call either


def test_surface_names_and_argument_rules(i8ie):
    import _CXX_i8ie as cx

    for n in ("Mul", "mul"):
        assert n in i8ie.__all__ and hasattr(i8ie, n) and hasattr(cx, n)
    assert isinstance(i8ie.Mul(), i8ie.layer.Weightless)
    x = i8ie.tensor(np.zeros((1, 2), np.float32))
    u8 = i8ie.Tensor(getattr(cx, "6TensorIhE")())  # an empty uint8 tensor: made without a device
    for kw in ({"scale": 0.5}, {"zero_point": 3}, {"scale": 0.5, "zero_point": 3}):
        with pytest.raises(TypeError, match="FP32"):
            i8ie.mul(x, x, **kw)
    for kw in ({}, {"scale": 0.5}, {"zero_point": 3}):
        with pytest.raises(TypeError, match="uint8"):
            i8ie.mul(u8, u8, **kw)
    # shapes are checked before anything touches the device
    def t(*shape):
        return i8ie.tensor(np.zeros(shape, np.float32))

    for a, b in ((t(2, 4, 3, 3), t(1, 4, 1, 1)), (t(2, 4, 3, 3), t(2, 1, 3, 3)), (t(2, 4, 1, 1), t(2, 4, 3, 3)), (t(2, 4), t(2, 4, 1, 1)),
                 (t(2, 4, 3, 3), t(2, 4, 1)), (t(2, 4, 3, 3), t(4,)), (t(2, 4, 3), t(2, 4, 3)), (t(2, 4, 3, 3), t(2, 4, 3, 1))):
        with pytest.raises(RuntimeError, match="mul"):
            i8ie.mul(a, b)
        with pytest.raises(RuntimeError, match="mul"):
            i8ie.Mul()(a, b)
    with pytest.raises(RuntimeError):
        i8ie.mul(u8, u8, 0.5, 3)   # (an empty tensor has no shape to multiply)


def _net(i8ie, with_conv):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            if with_conv:
                self.conv = i8ie.Conv2d(2, 2, 3, padding=1)
            self.mul1 = i8ie.Mul()
            self.add1 = i8ie.Add()
            self.mul2 = i8ie.Mul()

        def forward(self, x):
            y = self.mul1(self.conv(x), x) if with_conv else self.mul1(x, x)
            return self.mul2(self.add1(y, x), i8ie.global_avg_pool2d(x))

    return Net()


def test_mul_state_machine_and_module_without_a_gpu(i8ie, tmp_path):
    mul = i8ie.Mul()
    assert mul.output_qparams() == (1.0, 0) and mul.layer.is_quantized() is False
    assert mul.groups() == 1 and mul.is_per_channel() is False
    mul.set_output_qparams(0.5, 17)
    assert mul.output_qparams() == (0.5, 17)
    for bad in (-1, 256):
        with pytest.raises(RuntimeError):
            mul.set_output_qparams(0.5, bad)
    for f in (mul.load_weight, mul.load_bias, mul.forward_debug):
        with pytest.raises(RuntimeError, match="no weights"):
            f(np.zeros((1, 1), np.float32))
    for f in (mul.weight_scale, mul.weight_scales):
        with pytest.raises(RuntimeError, match="no weights"):
            f()
    mul.prepare()
    mul.convert(per_channel=True)  # (the flag is ignored; no sample was seen: the injected qparams stay)
    assert mul.layer.is_quantized() and mul.output_qparams() == (0.5, 17)
    with pytest.raises(RuntimeError):
        i8ie.Mul().layer.load_quantized(0.25, 256)

    net = _net(i8ie, True)
    assert [k for k, _ in net._layers()] == ["conv", "mul1", "add1", "mul2"]
    net.load({"conv.weight": np.ones((2, 2, 3, 3), np.float32), "conv.bias": np.zeros(2, np.float32)})  # ignores the Muls
    net.prepare()  # (no device call: reaches the conv, the Add and both Muls)
    # converting a Conv2d needs the device; a module of weightless layers alone goes through the whole state machine here
    net = _net(i8ie, False)
    net.load({})
    net.prepare()
    net.mul1.set_output_qparams(0.125, 9)
    net.add1.set_output_qparams(0.25, 10)
    net.mul2.set_output_qparams(0.5, 255)
    net.convert(per_channel=True)
    assert net.is_quant and net.mul1.layer.is_quantized() and net.mul2.layer.is_quantized()
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["add1.qparams", "mul1.qparams", "mul2.qparams"]  # no q_weight / q_bias keys
    assert sd["mul1.qparams"].dtype == np.float64 and sd["mul1.qparams"].tolist() == [0.0, 0.125, 9.0]
    path = str(tmp_path / "muls.npz")
    net.save_quantized(path)
    other = _net(i8ie, False)
    other.load_quantized_file(path)
    assert other.is_quant and other.mul1.output_qparams() == (0.125, 9) and other.mul2.output_qparams() == (0.5, 255)
    assert other.mul2.layer.is_quantized()
    half = _net(i8ie, False)
    half.mul1.convert()
    half.add1.convert()
    with pytest.raises(RuntimeError, match="mul2"):
        half.quantized_state_dict()


# ---- workloads ---------------------------------------------------------------------------------------------------------
def _check_spec(name):
    """channel / size bookkeeping through a spec with branches: every conv and Linear gets the input its tuple names, every
    Add joins equal shapes, every Mul gets x's shape or its gate, every saved tag and layer is used.  Returns the output
    shape, the shape at every Mul with its second operand's, and the MACs of every layer (branches included)."""
    from int8inferenceengine_amd import workloads as wl

    layers, spec, shape = wl.NETWORKS[name]
    saved, used, muls, macs = {}, set(), {}, {}

    def run(ops, cur):
        for op in ops:
            if op[0] == "layer":
                L = layers[op[1]]
                assert op[1] not in used
                used.add(op[1])
                if L[0] == "conv":
                    assert len(cur) == 3 and cur[0] == L[1], (name, op, cur)
                    assert L[1] % wl.conv_groups(L) == 0 and L[2] % wl.conv_groups(L) == 0
                    cur = (L[2], (cur[1] - L[3] + 2 * L[5]) // L[4] + 1, (cur[2] - L[3] + 2 * L[5]) // L[4] + 1)
                    macs[op[1]] = cur[1] * cur[2] * L[2] * (L[1] // wl.conv_groups(L)) * L[3] * L[3]
                else:
                    assert cur == (L[1],), (name, op, cur)
                    cur = (L[2],)
                    macs[op[1]] = L[1] * L[2]
            elif op[0] == "save":
                assert op[1] not in saved
                saved[op[1]] = cur
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]])
            elif op[0] == "add":
                assert saved.pop(op[2]) == cur
            elif op[0] == "mul":
                assert op[2] in saved, "every mul tag is saved"
                other = saved.pop(op[2])
                assert other == cur or (len(cur) == 3 and other == (cur[0],)), (name, op, cur, other)
                assert op[1] not in layers and op[1] not in muls
                muls[op[1]] = (cur, other)
            elif op[0] == "gap":
                cur = (cur[0], 1, 1)
            elif op[0] == "flatten":
                assert int(np.prod(cur)) == op[1], (name, op, cur)
                cur = (op[1],)
            else:
                assert op[0] in ("relu", "act"), op
        return cur

    out = run(spec, shape)
    assert not saved and used == set(layers)
    assert list(muls) == wl.mul_names(name)
    return out, muls, macs


def test_se_tiny_workload(i8ie):
    from int8inferenceengine_amd import workloads as wl

    out, muls, _ = _check_spec("se_tiny")
    layers, spec, shape = wl.NETWORKS["se_tiny"]
    assert out == (10,) and shape == (3, 32, 32)
    assert muls == {"s1mul": ((16, 32, 32), (16,)), "s2mul": ((20, 16, 16), (20,)), "s3mul": ((35, 16, 16), (35,)),
                    "mab": ((16, 16, 16), (16, 16, 16))}
    i = spec.index(("mul", "s1mul", "s1"))
    assert spec[i + 1] == ("layer", "c2") and layers["c2"][3:6] == (3, 2, 1)  # a gate mul -> 3x3 pad 1
    assert spec[i - 1] == ("branch", "s1", [("gap",), ("flatten", 16), ("layer", "s1fc1"), ("relu",), ("layer", "s1fc2"),
                                            ("act", "s1hs", "hardsigmoid")]) and spec[i - 2] == ("save", "s1")
    assert mr.relu_follows(spec) == {"mab"}
    j = spec.index(("mul", "mab", "m"))
    assert spec[j - 2:j] == [("layer", "c4a"), ("branch", "m", [("layer", "c4b")])]  # the product of two conv outputs ...
    assert spec[j + 1:j + 3] == [("relu",), ("layer", "c5")] and layers["c5"][3:6] == (3, 1, 1)  # ... -> relu -> 3x3 pad 1
    sd = wl.synthetic_state_dict("se_tiny")
    assert sorted(sd) == sorted(a + s for a in layers for s in (".weight", ".bias"))
    assert sd["s3fc1.weight"].shape == (12, 35) and sd["s3fc2.weight"].shape == (35, 12) and sd["c4b.weight"].shape == (16, 35, 3, 3)
    net = wl.build("se_tiny")
    names = wl.layer_names("se_tiny") + wl.mul_names("se_tiny") + wl.activation_names("se_tiny")
    assert sorted(k for k, _ in net._layers()) == sorted(names) and isinstance(net.s2mul, i8ie.Mul) and isinstance(net.s2fc1, i8ie.Linear)
    net.load(sd)
    # the main path and the Linears of the SE branches (the conv of a branch is not counted, as in resnet_tiny)
    want = (1024 * 16 * 27 + 256 * (20 * 144 + 35 * 20 + 16 * 35 + 16 * 144) + 160
            + 2 * (16 * 8 + 20 * 8 + 35 * 12))
    assert wl.macs_per_image("se_tiny") == want


def test_mobilenetv3_small_cifar_workload():
    from int8inferenceengine_amd import workloads as wl

    name = "mobilenetv3_small_cifar"
    out, muls, macs = _check_spec(name)
    layers, spec, shape = wl.NETWORKS[name]
    assert out == (10,) and shape == (3, 32, 32)
    # Howard et al. 2019, table 2: kernel, expansion, output channels, SE, hardswish (else relu), stride; the first block at
    # stride 1 for 32 x 32 input
    table = [(3, 16, 16, 1, 0, 1), (3, 72, 24, 0, 0, 2), (3, 88, 24, 0, 0, 1), (5, 96, 40, 1, 1, 2), (5, 240, 40, 1, 1, 1),
             (5, 240, 40, 1, 1, 1), (5, 120, 48, 1, 1, 1), (5, 144, 48, 1, 1, 1), (5, 288, 96, 1, 1, 2), (5, 576, 96, 1, 1, 1),
             (5, 576, 96, 1, 1, 1)]
    assert layers["stem"] == ("conv", 3, 16, 3, 1, 1)
    want_macs = 32 * 32 * 16 * 27
    c, hw, squeezes, n_mul = 16, 32, [], 0
    for i, (k, exp, oc, se, hs, s) in enumerate(table, start=1):
        p = "b%d" % i
        if exp != c:
            assert layers[p + "e"] == ("conv", c, exp, 1, 1, 0)
            want_macs += hw * hw * exp * c
        else:
            assert p + "e" not in layers
        assert layers[p + "d"] == ("conv", exp, exp, k, s, k // 2, exp)
        hw //= s
        want_macs += hw * hw * exp * k * k
        j = spec.index(("layer", p + "d"))
        assert spec[j + 1] == (("act", p + "da", "hardswish") if hs else ("relu",))
        if se:
            sq = layers[p + "sefc1"][2]
            squeezes.append(sq)
            assert layers[p + "sefc1"] == ("fc", exp, sq) and layers[p + "sefc2"] == ("fc", sq, exp)
            assert spec[j + 2] == ("save", p + "se") and spec[j + 4] == ("mul", p + "semul", p + "se")  # behind the depthwise activation
            assert spec[j + 5] == ("layer", p + "p")                                                      # ... and before the projection
            assert muls[p + "semul"] == ((exp, hw, hw), (exp,))
            want_macs += 2 * exp * sq
            n_mul += 1
        else:
            assert p + "sefc1" not in layers and spec[j + 2] == ("layer", p + "p")
        assert layers[p + "p"] == ("conv", exp, oc, 1, 1, 0)
        want_macs += hw * hw * oc * exp
        assert ((p + "add") in wl.add_names(name)) == (s == 1 and c == oc)
        c = oc
    assert hw == 4 and squeezes == [8, 24, 64, 64, 32, 40, 72, 144, 144] and sorted(set(squeezes)) == [8, 24, 32, 40, 64, 72, 144]
    assert [wl.make_divisible(e / 4, 8) for e in (16, 96, 240, 120, 144, 288, 576)] == [8, 24, 64, 32, 40, 72, 144]
    assert n_mul == 9 and len(wl.mul_names(name)) == 9 and wl.add_names(name) == ["b1add", "b3add", "b5add", "b6add", "b8add", "b10add", "b11add"]
    assert layers["head"] == ("conv", 96, 576, 1, 1, 0) and layers["fc1"] == ("fc", 576, 1024) and layers["fc2"] == ("fc", 1024, 10)
    assert spec[-7:] == [("layer", "head"), ("act", "heada", "hardswish"), ("gap",), ("flatten", 576), ("layer", "fc1"),
                         ("act", "fc1a", "hardswish"), ("layer", "fc2")]
    want_macs += 16 * 576 * 96 + 576 * 1024 + 1024 * 10
    assert wl.macs_per_image(name) == want_macs == sum(macs.values())
    sd = wl.synthetic_state_dict(name)
    assert sorted(sd) == sorted(a + s for a in layers for s in (".weight", ".bias"))
    assert sd["b4d.weight"].shape == (96, 1, 5, 5) and sd["b11sefc1.weight"].shape == (144, 576) and sd["fc1.weight"].shape == (1024, 576)


def test_existing_networks_have_no_muls_and_keep_their_macs():
    from int8inferenceengine_amd import workloads as wl

    before = pn.NAMES[:pn.NAMES.index("se_tiny")]
    assert len(before) == 13 and {n: wl.macs_per_image(n) for n in before} == {n: pn.MACS[n] for n in before}
    assert all(wl.mul_names(n) == [] for n in before)


# ---- the network tests are not trivial: checked on the oracle alone -------------------------------------------------------
def test_se_tiny_oracle_forward_has_live_gates_and_unclamped_products():
    from int8inferenceengine_amd import workloads as wl

    name = "se_tiny"
    sd = wl.synthetic_state_dict(name, sr.WEIGHT_SEED)
    qp, jqp = sr.fp32_qparams(wl.NETWORKS[name], sd, wl.synthetic_input(name, sr.CALIB_IMAGES, seed=sr.CALIB_SEED))
    assert sorted(jqp) == sorted(wl.activation_names(name) + wl.mul_names(name)) and sorted(qp) == sorted(wl.layer_names(name))
    trace = {}
    x = wl.synthetic_input(name, 2, seed=sr.INPUT_SEED)
    y = sr.forward(wl.NETWORKS[name], x, sr.quantize_layers(wl.NETWORKS[name], sd), qp, jqp, False, mr.tracer(wl.NETWORKS[name][1], trace))
    assert y.shape == (2, 10) and list(trace) == wl.mul_names(name)
    stats = mr.nontrivial(trace)
    print({a: (d, round(s, 3)) for a, (d, s) in stats.items()})
    assert [a for a, (d, _) in stats.items() if d is not None] == ["s1mul", "s2mul", "s3mul"]
