"""The quantized residual Add without a GPU: the numpy restatement against an independent integer formulation where that
one is exact, the Python / extension / C surface, the Add's state machine, its place in Module and the residual workload."""
import ctypes as C

import numpy as np
import pytest

import abi
import add_ref as ar
import support
from support import i8ie  # noqa: F401


@pytest.mark.parametrize("scale", [0.5, 0.0234375, 3.0])  # powers of two and 3: every product and quotient below is exact
@pytest.mark.parametrize("zps", [(0, 0, 0), (128, 128, 128), (255, 0, 128), (3, 250, 255), (17, 99, 0)])
@pytest.mark.parametrize("relu", [False, True])
def test_restatement_equals_integer_add_for_equal_scales(scale, zps, relu):
    """s_a = s_b = s_out = s: fa, fb and their sum are (small integer) * s, exact in fp32 for these s, and the quotient by
    s is that integer again; so q = clamp(a - zp_a + b - zp_b + zp_out, 0, 255) in integers."""
    a, b = support.byte_pairs()
    zp_a, zp_b, zp_out = zps
    want = np.clip(a.astype(np.int64) - zp_a + b.astype(np.int64) - zp_b + zp_out, 0, 255)
    if relu:
        want = np.maximum(want, zp_out)
    got = ar.add_u8(a, zp_a, scale, b, zp_b, scale, scale, zp_out, relu)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_saturation_and_relu_floor():
    a = np.array([255, 255, 0, 0, 10, 200], np.uint8)
    b = np.array([255, 0, 0, 255, 10, 200], np.uint8)
    # both ends: (a - 128 + b - 128) * 4 + 128 with s_out = s / 4
    got = ar.add_u8(a, 128, 1.0, b, 128, 1.0, 0.25, 128)
    assert got.tolist() == [255, 124, 0, 124, 0, 255]
    # the relu floor is the RESULT's zero point
    got = ar.add_u8(a, 128, 1.0, b, 128, 1.0, 0.25, 128, relu=True)
    assert got.tolist() == [255, 128, 128, 128, 128, 255]
    # truncation toward zero of a positive t: (1 + 0) * 1 / 3 + 0 = 0.33 -> 0, (5 + 0) / 3 = 1.67 -> 1
    assert ar.add_u8(np.array([1, 5], np.uint8), 0, 1.0, np.zeros(2, np.uint8), 0, 1.0, 3.0, 0).tolist() == [0, 1]
    # a negative t inside (-1, 0) is 0 by the clamp, not by the cast
    assert ar.add_u8(np.array([0], np.uint8), 1, 1.0, np.array([0], np.uint8), 0, 1.0, 3.0, 0).tolist() == [0]


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    assert callable(i8ie.add) and isinstance(i8ie.Add(), i8ie.layer.Layer)
    assert hasattr(cx, "add") and hasattr(cx, "Add")
    assert "Add" in i8ie.__all__ and "add" in i8ie.__all__


def test_new_symbols_are_declared_and_exported():
    names = abi.declared_symbols()
    lib = ar.bind(abi.lib())
    for n in ["i8ie_add_u8", "i8ie_add_u8_nhwc", "i8ie_add_f32"]:
        assert n in names and hasattr(lib, n), n
    assert lib.i8ie_version() == 1


def test_entry_points_check_arguments_before_any_device_call():
    lib = ar.bind(abi.lib())
    one = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)
    assert lib.i8ie_add_u8(None, one, one, one, 16, 1.0, 0, 1.0, 0, 1.0, 0, 0) == -1 and b"null" in lib.i8ie_last_error()
    assert lib.i8ie_add_f32(None, one, one, one, 4) == -1 and b"null" in lib.i8ie_last_error()
    assert lib.i8ie_add_u8_nhwc(None, one, 0, 0, one, 0, 0, one, 0, 0, 1, 16, 1, 1, 1.0, 0, 1.0, 0, 1.0, 0, 0) == -1
    ctx = C.c_void_p(16)
    for s_a, s_b, s_out in [(1.0, 1.0, 0.0), (1.0, 1.0, -0.5), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0),
                            (1.0, float("inf"), 1.0)]:
        assert lib.i8ie_add_u8(ctx, one, one, one, 16, s_a, 0, s_b, 0, s_out, 0, 0) == -1
        assert b"scale" in lib.i8ie_last_error()
        assert lib.i8ie_add_u8_nhwc(ctx, one, 0, 0, one, 0, 0, one, 0, 0, 1, 16, 1, 1, s_a, 0, s_b, 0, s_out, 0, 0) == -1
        assert b"scale" in lib.i8ie_last_error()
    assert lib.i8ie_add_u8(ctx, one, one, one, -1, 1.0, 0, 1.0, 0, 1.0, 0, 0) == -1
    assert lib.i8ie_add_u8_nhwc(ctx, one, -1, 0, one, 0, 0, one, 0, 0, 1, 16, 1, 1, 1.0, 0, 1.0, 0, 1.0, 0, 0) == -1


def test_add_state_machine_without_a_gpu(i8ie):
    add = i8ie.Add()
    assert add.output_qparams() == (1.0, 0)
    assert add.layer.is_quantized() is False
    add.set_output_qparams(0.5, 17)
    assert add.output_qparams() == (0.5, 17)
    for bad in (-1, 256):
        with pytest.raises(RuntimeError):
            add.set_output_qparams(0.5, bad)
    assert add.groups() == 1 and add.is_per_channel() is False
    for f in (add.weight_scale, add.weight_scales):
        with pytest.raises(RuntimeError):
            f()
    with pytest.raises(RuntimeError):
        add.load_weight(np.zeros((1, 1), np.float32))
    add.prepare()
    add.convert(per_channel=True)  # (the flag is ignored; no sample was seen: the injected qparams stay)
    assert add.layer.is_quantized() and add.output_qparams() == (0.5, 17)
    fresh = i8ie.Add()
    fresh.layer.load_quantized(0.25, 200)
    assert fresh.layer.is_quantized() and fresh.output_qparams() == (0.25, 200)
    with pytest.raises(RuntimeError):
        i8ie.Add().layer.load_quantized(0.25, 256)


def _net(i8ie, with_conv):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            if with_conv:
                self.conv = i8ie.Conv2d(2, 2, 3, padding=1)
            self.add1 = i8ie.Add()
            self.add2 = i8ie.Add()

        def forward(self, x):
            y = self.add1(self.conv(x), x) if with_conv else self.add1(x, x)
            return self.add2(y, x)

    return Net()


def test_module_lists_the_add_and_load_ignores_it(i8ie):
    net = _net(i8ie, True)
    assert [k for k, _ in net._layers()] == ["conv", "add1", "add2"]
    net.load({"conv.weight": np.ones((2, 2, 3, 3), np.float32), "conv.bias": np.zeros(2, np.float32)})
    net.prepare()  # (no device call: reaches the conv and both Adds)
    # converting a Conv2d needs the device; a module of Adds alone goes through the whole state machine on the host
    net = _net(i8ie, False)
    net.prepare()
    net.add1.set_output_qparams(0.125, 9)
    net.add2.set_output_qparams(0.5, 255)
    net.convert(per_channel=True)
    assert net.is_quant and net.add1.layer.is_quantized() and net.add2.layer.is_quantized()
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["add1.qparams", "add2.qparams"]  # no q_weight / q_bias keys
    assert sd["add1.qparams"].dtype == np.float64 and sd["add1.qparams"].tolist() == [0.0, 0.125, 9.0]
    other = _net(i8ie, False)
    other.load_quantized(sd)
    assert other.is_quant and other.add1.output_qparams() == (0.125, 9) and other.add2.output_qparams() == (0.5, 255)
    assert other.add1.layer.is_quantized()


def test_quantized_state_dict_round_trips_through_a_file(i8ie, tmp_path):
    net = _net(i8ie, False)
    net.add1.set_output_qparams(0.3, 1)
    net.add2.set_output_qparams(0.7, 2)
    net.convert()
    path = str(tmp_path / "adds.npz")
    net.save_quantized(path)
    other = _net(i8ie, False)
    other.load_quantized_file(path)
    assert other.add1.output_qparams() == net.add1.output_qparams() == (float(np.float32(0.3)), 1)
    assert other.add2.output_qparams() == net.add2.output_qparams()


def test_quantized_state_dict_needs_a_converted_add(i8ie):
    net = _net(i8ie, False)
    net.add1.set_output_qparams(1.0, 0)
    net.add1.convert()
    with pytest.raises(RuntimeError, match="add2"):
        net.quantized_state_dict()


def test_resnet_tiny_workload():
    from int8inferenceengine_amd import workloads as wl

    layers, spec, shape = wl.NETWORKS["resnet_tiny"]
    assert shape == (3, 32, 32)
    assert wl.layer_names("resnet_tiny") == ["stem", "b1c1", "b1c2", "b2c1", "b2c2", "b2proj", "b3c1", "b3c2", "fc"]
    assert wl.add_names("resnet_tiny") == ["add1", "add2", "add3"]
    sd = wl.synthetic_state_dict("resnet_tiny")
    assert sorted(sd) == sorted(a + s for a in layers for s in (".weight", ".bias"))
    assert sd["stem.weight"].shape == (16, 3, 3, 3) and sd["b2c1.weight"].shape == (32, 16, 3, 3)
    assert sd["b2proj.weight"].shape == (32, 16, 1, 1) and sd["b3c1.weight"].shape == (32, 8, 3, 3)
    assert sd["b3c2.weight"].shape == (32, 32, 1, 1) and sd["fc.weight"].shape == (10, 2048) and sd["fc.bias"].shape == (10,)
    net = wl.build("resnet_tiny")
    names = [k for k, _ in net._layers()]
    assert sorted(names) == sorted(wl.layer_names("resnet_tiny") + wl.add_names("resnet_tiny"))
    assert net.b3c1.groups() == 4 and net.add2.groups() == 1
    net.load(sd)
    # the main path only (the Adds and the projection branch are not counted)
    main = (32 * 32 * 16 * 3 * 9 + 2 * 32 * 32 * 16 * 16 * 9 + 16 * 16 * 32 * 16 * 9 + 16 * 16 * 32 * 32 * 9
            + 16 * 16 * 32 * 8 * 9 + 16 * 16 * 32 * 32 + 2048 * 10)
    assert wl.macs_per_image("resnet_tiny") == main
    # the existing networks' names are what they were
    assert wl.layer_names("alexnet") == ["conv1", "conv2", "conv3", "conv4", "conv5", "fc1", "fc2", "fc3"]
    assert wl.add_names("alexnet") == []
