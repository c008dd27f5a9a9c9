"""Quantized channel concatenation without a GPU: the numpy restatement against integer arithmetic where that is exact, the
copy rule, the Python / extension / C surface, the Concat's state machine, its place in Module and the two fire workloads."""
import ctypes as C

import numpy as np
import pytest

import abi
import concat_ref as cr
import pinned_networks as pn
from support import i8ie  # noqa: F401

f32 = np.float32
BYTES = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)


@pytest.mark.parametrize("s_out", [0.5, 0.0234375, 3.0])  # few mantissa bits: every product and quotient below is exact
@pytest.mark.parametrize("shift", [-6, -1, 0, 1, 6])      # s_i / s_out = 2 ** shift
@pytest.mark.parametrize("zp_i", [0, 128, 255])
@pytest.mark.parametrize("zp_out", [0, 128, 255])
@pytest.mark.parametrize("relu", [False, True])
def test_restatement_equals_integer_arithmetic_for_power_of_two_ratios(s_out, shift, zp_i, zp_out, relu):
    """f = d * s_i and f / s_out = d * 2^shift are exact, and so is t = d * 2^shift + zp_out (a dyadic fraction below 2^15):
    q = clamp(floor(t), 0, 255), t < 0 going to 0 (floor and truncation agree from 0 upwards)."""
    s_i = f32(s_out) * f32(2.0 ** shift)
    d = BYTES.astype(np.int64) - zp_i
    num, den = (2 ** shift, 1) if shift >= 0 else (1, 2 ** -shift)
    want = np.clip((d * num + zp_out * den) // den, 0, 255)
    if relu:
        want = np.maximum(want, zp_out)
    got = cr.cat_u8([(BYTES, s_i, zp_i)], f32(s_out), zp_out, relu)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


COPY_SCALES = [f32(v) for v in np.random.default_rng(20261018).uniform(0.002, 0.3, 24)] + [f32(0.025), f32(0.05)]


def test_copy_rule_keeps_bytes_the_literal_sequence_would_change():
    moved = 0
    for i, s in enumerate(COPY_SCALES):
        zp = (37 * i + 5) % 256
        literal = cr.requant_u8(BYTES, s, zp, s, zp)
        moved += int(not np.array_equal(literal, BYTES))
        for relu in (False, True):
            got = cr.cat_u8([(BYTES, s, zp), (BYTES, s, zp)], s, zp, relu)
            want = np.concatenate([BYTES, BYTES], axis=1)
            assert np.array_equal(got, np.maximum(want, zp) if relu else want)
        # one ulp away in the scale, or another zero point, is NOT a copy
        other = np.nextafter(s, f32(1))
        assert np.array_equal(cr.cat_u8([(BYTES, other, zp)], s, zp), cr.requant_u8(BYTES, other, zp, s, zp))
        assert np.array_equal(cr.cat_u8([(BYTES, s, zp ^ 1)], s, zp), cr.requant_u8(BYTES, s, zp ^ 1, s, zp))
    assert moved >= 1, "no scale in the list shows why the copy rule is part of the definition"
    print("literal sequence differs from the identity at %d of %d scales" % (moved, len(COPY_SCALES)))


def test_guarded_estimate_agrees_with_the_restatement_where_the_guard_accepts_it():
    """The kernel's guarded evaluation (csrc/i8ie_concat.hip) emulated in float64: e = fma(f, fl(1 / s_out), zp_out - 0.5)
    (the product of two float32 is exact in float64), rounded to nearest even and saturated as v_cvt_pk_u8_f32 does.  Wherever
    e is at least 2^-13 away from a rounding boundary the result must be the restatement's byte; the rest replays."""
    rng = np.random.default_rng(3)
    a = np.arange(256, dtype=np.uint8)
    sets = [(f32(s), int(z), f32(so), int(zo)) for s, z, so, zo in zip(rng.uniform(0.002, 0.3, 600), rng.integers(0, 256, 600),
                                                                        rng.uniform(0.002, 0.3, 600), rng.integers(0, 256, 600))]
    sets += [(f32(0.05), 3, f32(0.05), 128), (f32(0.05) / f32(3), 120, f32(0.05), 128), (f32(3.2), 128, f32(0.05), 128),
             (f32(0.05), 0, f32(0.0005), 128), (f32(0.05) / f32(64), 7, f32(0.05), 128)]
    accepted = replayed = 0
    for s, z, so, zo in sets:
        f = ((a.astype(f32) - f32(z)) * s).astype(f32)
        e = (f.astype(np.float64) * np.float64(f32(1) / so) + np.float64(f32(zo) - f32(0.5))).astype(f32)
        ok = np.abs((e - np.floor(e)) - f32(0.5)) >= f32(2.0 ** -13)
        for relu in (False, True):
            want = cr.cat_u8([(a.reshape(1, -1), s, z)], so, zo, relu)[0] if not cr.same_qparams(s, z, so, zo) else a
            q = np.clip(np.rint(np.maximum(e, f32(zo) if relu else f32(-1)).astype(np.float64)), 0, 255).astype(np.uint8)
            assert np.array_equal(q[ok], want[ok]), (s, z, so, zo, relu)
        accepted += int(ok.sum())
        replayed += int((~ok).sum())
    assert replayed >= 256 and accepted > 100 * replayed  # (equal scales replay everything; ordinary parameters hardly ever)


def test_restatement_joins_along_axis_one_and_saturates():
    a = np.array([[0, 255, 10]], np.uint8)
    b = np.array([[200, 100]], np.uint8)
    got = cr.cat_u8([(a, 1.0, 0), (b, 1.0, 128)], 0.25, 128)
    assert got.tolist() == [[128, 255, 168, 255, 16]]
    assert cr.cat_u8([(a, 1.0, 0), (b, 1.0, 128)], 0.25, 128, relu=True).tolist() == [[128, 255, 168, 255, 128]]
    # a negative t inside (-1, 0) is 0 by the clamp; truncation toward zero of a positive t
    assert cr.cat_u8([(np.array([[0, 6]], np.uint8), 1.0, 1)], 3.0, 0).tolist() == [[0, 1]]
    x = np.arange(2 * 3 * 2 * 2, dtype=np.uint8).reshape(2, 3, 2, 2)
    got = cr.cat_u8([(x, 0.5, 3), (x[:, :1], 0.5, 3), (x, 0.5, 3)], 0.5, 3)
    assert got.shape == (2, 7, 2, 2) and np.array_equal(got, np.concatenate([x, x[:, :1], x], axis=1))


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    assert callable(i8ie.cat) and isinstance(i8ie.Concat(), i8ie.layer.Layer)
    assert isinstance(i8ie.Concat(), i8ie.layer.Weightless) and isinstance(i8ie.Add(), i8ie.layer.Weightless)
    assert hasattr(cx, "cat") and hasattr(cx, "Concat")
    assert "Concat" in i8ie.__all__ and "cat" in i8ie.__all__


def test_new_symbols_are_declared_and_exported():
    names = abi.declared_symbols()
    lib = cr.bind(abi.lib())
    for n in ["i8ie_concat_u8", "i8ie_concat_u8_nhwc", "i8ie_concat_f32"]:
        assert n in names and hasattr(lib, n), n
    assert "I8IE_CONCAT_MAX_INPUTS 8" in open(abi.HEADER).read()
    assert lib.i8ie_version() == 1


def test_entry_points_check_arguments_before_any_device_call():
    lib = cr.bind(abi.lib())
    one = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)
    ctx = C.c_void_p(16)

    def run(k=2, ctx=ctx, out=one, ins=None, lens=None, s_in=None, s_out=1.0, outer=1):
        ins = [one] * k if ins is None else ins
        return cr.concat_u8(lib, ctx, ins, lens or [16] * k, s_in or [1.0] * k, [0] * k, out, outer, s_out, 0, 0)

    def nhwc(k=2, ctx=ctx, out=one, ins=None, c_in=None, b_in=None, s_in=None, s_out=1.0, ob=0, n=1):
        ins = [one] * k if ins is None else ins
        return cr.concat_u8_nhwc(lib, ctx, ins, c_in or [16] * k, b_in or [0] * k, [0] * k, s_in or [1.0] * k, [0] * k, out, ob, 0,
                                 n, 2, 2, s_out, 0, 0)

    for f in (run, nhwc):
        assert f(ctx=None) == -1 and b"null" in lib.i8ie_last_error()
        assert f(out=None) == -1 and b"null" in lib.i8ie_last_error()
        assert f(ins=[one, None]) == -1 and b"null" in lib.i8ie_last_error()
        assert f(k=0) == -1 and b"inputs" in lib.i8ie_last_error()
        assert f(k=9) == -1 and b"inputs" in lib.i8ie_last_error()
        for s_in, s_out in [([1.0, 1.0], 0.0), ([1.0, 1.0], -0.5), ([1.0, 1.0], float("inf")), ([float("nan"), 1.0], 1.0),
                            ([1.0, float("inf")], 1.0), ([1.0, 1.0], float("nan"))]:
            assert f(s_in=s_in, s_out=s_out) == -1 and b"scale" in lib.i8ie_last_error()
    assert run(lens=[16, 0]) == -1 and run(outer=-1) == -1
    assert nhwc(b_in=[0, -1]) == -1 and nhwc(ob=-1) == -1 and nhwc(c_in=[0, 16]) == -1 and nhwc(n=0) == -1
    assert cr.concat_f32(lib, None, [one], [4], one, 1) == -1 and b"null" in lib.i8ie_last_error()
    assert cr.concat_f32(lib, ctx, [], [], one, 1) == -1 and cr.concat_f32(lib, ctx, [one] * 9, [4] * 9, one, 1) == -1
    assert cr.concat_f32(lib, ctx, [one, None], [4, 4], one, 1) == -1
    assert cr.concat_f32(lib, ctx, [C.c_void_p(18)], [4], one, 1) == -1 and b"aligned" in lib.i8ie_last_error()


def test_concat_state_machine_without_a_gpu(i8ie):
    cat = i8ie.Concat()
    assert cat.output_qparams() == (1.0, 0)
    assert cat.layer.is_quantized() is False
    cat.set_output_qparams(0.5, 17)
    assert cat.output_qparams() == (0.5, 17)
    for bad in (-1, 256):
        with pytest.raises(RuntimeError):
            cat.set_output_qparams(0.5, bad)
    assert cat.groups() == 1 and cat.is_per_channel() is False
    for f in (cat.weight_scale, cat.weight_scales):
        with pytest.raises(RuntimeError, match="no weights"):
            f()
    with pytest.raises(RuntimeError, match="no weights"):
        cat.load_weight(np.zeros((1, 1), np.float32))
    cat.prepare()
    cat.convert(per_channel=True)  # (the flag is ignored; no sample was seen: the injected qparams stay)
    assert cat.layer.is_quantized() and cat.output_qparams() == (0.5, 17)
    fresh = i8ie.Concat()
    fresh.layer.load_quantized(0.25, 200)
    assert fresh.layer.is_quantized() and fresh.output_qparams() == (0.25, 200)
    with pytest.raises(RuntimeError):
        i8ie.Concat().layer.load_quantized(0.25, 256)


def test_shape_and_dtype_errors_need_no_device(i8ie):
    """every message below comes from the shape check in front of the first device call (`cat:`), not from a missing GPU"""
    import _CXX_i8ie as cx

    def t(*shape):
        return i8ie.tensor(np.zeros(shape, np.float32))

    u8 = i8ie.Tensor(getattr(cx, "6TensorIhE")())  # an empty uint8 tensor: made without a device
    cases = {
        "no input": [],
        "nine inputs": [t(1, 2, 2, 2)] * 9,
        "rank 3": [t(2, 2, 2), t(2, 2, 2)],
        "rank 1": [t(4)],
        "ranks differ": [t(2, 4), t(2, 1, 2, 2)],
        "axis 0 differs": [t(2, 3, 2, 2), t(1, 3, 2, 2)],
        "axis 2 differs": [t(2, 3, 2, 2), t(2, 3, 1, 2)],
        "rows differ": [t(2, 3), t(3, 3)],
        "mixed dtypes": [t(2, 3), u8],
    }
    for name, tensors in cases.items():
        for f in (i8ie.cat, i8ie.Concat()):
            with pytest.raises(RuntimeError, match="cat:"):
                f(tensors)
    with pytest.raises(RuntimeError, match="cat:"):
        cx.cat([u8.data, t(2, 3).data], 0.5, 3)  # ... and in the uint8 form


def test_cat_parameter_rules(i8ie):
    import _CXX_i8ie as cx

    x = i8ie.tensor(np.zeros((1, 2), np.float32))
    u8 = i8ie.Tensor(getattr(cx, "6TensorIhE")())
    for kw in ({"scale": 0.5}, {"zero_point": 3}, {"scale": 0.5, "zero_point": 3}):
        with pytest.raises(TypeError, match="FP32"):
            i8ie.cat([x, x], **kw)
    for kw in ({}, {"scale": 0.5}, {"zero_point": 3}):
        with pytest.raises(TypeError, match="uint8"):
            i8ie.cat([u8, u8], **kw)
    with pytest.raises(RuntimeError, match="cat:"):
        i8ie.cat([u8, u8], 0.5, 3)  # (an empty tensor has no rank: refused by the shape check)


def _net(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.cat1 = i8ie.Concat()
            self.add1 = i8ie.Add()
            self.cat2 = i8ie.Concat()

        def forward(self, x):
            return self.cat2([self.add1(self.cat1([x, x]), self.cat1([x, x])), x])

    return Net()


def test_module_treats_the_concat_as_it_treats_the_add(i8ie, tmp_path):
    net = _net(i8ie)
    assert [k for k, _ in net._layers()] == ["cat1", "add1", "cat2"]
    net.load({})  # ignores the layers without weights
    net.prepare()
    net.cat1.set_output_qparams(0.125, 9)
    net.add1.set_output_qparams(0.25, 10)
    net.cat2.set_output_qparams(0.5, 255)
    net.convert(per_channel=True)
    assert net.is_quant and net.cat1.layer.is_quantized() and net.cat2.layer.is_quantized()
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["add1.qparams", "cat1.qparams", "cat2.qparams"]  # no q_weight / q_bias keys
    assert sd["cat1.qparams"].dtype == np.float64 and sd["cat1.qparams"].tolist() == [0.0, 0.125, 9.0]
    path = str(tmp_path / "joins.npz")
    net.save_quantized(path)
    other = _net(i8ie)
    other.load_quantized_file(path)
    assert other.is_quant and other.cat1.output_qparams() == (0.125, 9) and other.cat2.output_qparams() == (0.5, 255)
    assert other.cat1.layer.is_quantized() and other.add1.output_qparams() == (0.25, 10)
    half = _net(i8ie)
    half.cat1.convert()
    half.add1.convert()
    with pytest.raises(RuntimeError, match="cat2"):
        half.quantized_state_dict()


def _check_spec(name):
    """channel / size bookkeeping through the spec: every conv gets the channels its layer tuple names, every concat joins
    tensors of one size, every saved tag is used.  Returns the output shape and the channels each Concat joins."""
    from int8inferenceengine_amd import workloads as wl

    layers, spec, (c, h, w) = wl.NETWORKS[name]
    joined, used = {}, set()

    def run(ops, cur, saved):
        for op in ops:
            if op[0] == "layer":
                L = layers[op[1]]
                used.add(op[1])
                if L[0] == "conv":
                    assert len(cur) == 3 and cur[0] == L[1], (name, op, cur)
                    assert L[1] % wl.conv_groups(L) == 0 and L[2] % wl.conv_groups(L) == 0
                    cur = (L[2], (cur[1] - L[3] + 2 * L[5]) // L[4] + 1, (cur[2] - L[3] + 2 * L[5]) // L[4] + 1)
                else:
                    assert cur == (L[1],), (name, op, cur)
                    cur = (L[2],)
            elif op[0] in ("pool", "avgpool"):
                cur = (cur[0], (cur[1] - op[1]) // op[2] + 1, (cur[2] - op[1]) // op[2] + 1)
            elif op[0] == "gap":
                cur = (cur[0], 1, 1)
            elif op[0] == "save":
                saved[op[1]] = cur
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                assert saved.pop(op[2]) == cur
            elif op[0] == "concat":
                parts = [cur] + [saved.pop(t) for t in op[2]]
                assert 1 <= len(parts) <= 8 and len({p[1:] for p in parts}) == 1 and min(parts[0][1:]) >= 1, (name, op, parts)
                joined[op[1]] = [p[0] for p in parts]
                cur = (sum(joined[op[1]]),) + cur[1:]
            elif op[0] == "flatten":
                assert int(np.prod(cur)) == op[1], (name, op, cur)
                cur = (op[1],)
            else:
                assert op[0] == "relu", op
        return cur

    saved = {}
    out = run(spec, (c, h, w), saved)
    assert not saved and used == set(layers), (name, saved, set(layers) - used)
    assert sorted(joined) == sorted(wl.concat_names(name)) and not (set(joined) & set(layers))
    return out, joined


def test_fire_tiny_workload(i8ie):
    from int8inferenceengine_amd import workloads as wl

    out, joined = _check_spec("fire_tiny")
    assert out == (10,) and wl.NETWORKS["fire_tiny"][2] == (3, 32, 32)
    assert joined == {"facat": [16, 16], "fbcat": [20, 12], "rcat": [32, 16, 16]}
    layers, spec, _ = wl.NETWORKS["fire_tiny"]
    assert wl.conv_groups(layers["rg"]) == 4 and layers["stem"] == ("conv", 3, 16, 3, 1, 1) and layers["fc"] == ("fc", 64, 10)
    i = spec.index(("concat", "fbcat", ["fb"]))
    assert spec[i + 1] == ("relu",) and spec[i - 2] == ("layer", "fbe1")  # fire B: one ReLU, behind the concat
    net = wl.build("fire_tiny")
    assert sorted(k for k, _ in net._layers()) == sorted(wl.layer_names("fire_tiny") + wl.concat_names("fire_tiny"))
    assert isinstance(net.rcat, i8ie.Concat) and net.rg.groups() == 4 and wl.add_names("fire_tiny") == []
    net.load(wl.synthetic_state_dict("fire_tiny"))


def test_squeezenet_cifar_workload():
    from int8inferenceengine_amd import workloads as wl

    out, joined = _check_spec("squeezenet_cifar")
    assert out == (10,)
    widths = [64, 64, 128, 128, 192, 192, 256, 256]
    assert joined == {"fire%dcat" % i: [e, e] for i, e in zip(range(2, 10), widths)}
    layers, spec, _ = wl.NETWORKS["squeezenet_cifar"]
    assert [layers["fire%ds" % i][2] for i in range(2, 10)] == [16, 16, 32, 32, 48, 48, 64, 64]
    assert layers["classifier"] == ("conv", 512, 10, 1, 1, 0) and spec[-2:] == [("gap",), ("flatten", 10)]
    assert [op for op in spec if op[0] == "pool"] == [("pool", 3, 2)] * 3
    assert len(wl.layer_names("squeezenet_cifar")) == 1 + 8 * 3 + 1


def test_macs_of_the_existing_networks_are_unchanged():
    from int8inferenceengine_amd import workloads as wl

    before = pn.NAMES[:pn.NAMES.index("fire_tiny")]
    assert len(before) == 8 and {n: wl.macs_per_image(n) for n in before} == {n: pn.MACS[n] for n in before}
    assert all(wl.concat_names(n) == [] for n in before)
    # the main-path rule: the squeeze and the 1x1 expand of a fire module, not its 3x3 branch
    assert wl.macs_per_image("fire_tiny") == (32 * 32 * (16 * 27 + 8 * 16 + 16 * 8 + 12 * 32 + 20 * 12) + 64 * 10)
