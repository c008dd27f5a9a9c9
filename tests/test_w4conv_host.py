"""4-bit weights for k x k Conv2d, the host side: which layers convert(weight_bits=4, spatial=True) and Module.convert(spatial=True)
accept and which they refuse, the argument errors of i8ie_conv2d_create_w4_geom and the kernel-key rules of load_quantized, all up
to the first device call.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi
from support import i8ie  # noqa: F401


@pytest.mark.parametrize("kw", [dict(kernel_size=3), dict(kernel_size=3, stride=2, padding=1), dict(kernel_size=(5, 5), padding=(2, 2)),
                                dict(kernel_size=3, padding=2, dilation=2), dict(kernel_size=1, stride=2), dict(kernel_size=1)])
def test_a_square_dense_conv_is_accepted(i8ie, kw):
    from i8ie.layer import check_spatial, is_spatial

    conv = i8ie.Conv2d(8, 4, **kw)
    assert is_spatial(conv) and check_spatial(conv, True, 4) and not check_spatial(conv, False) and not conv.layer.is_quantized()


@pytest.mark.parametrize("make,kw", [(lambda m: m.Conv2d(8, 4, (1, 3)), dict(weight_bits=4)), (lambda m: m.Conv2d(8, 4, 3, stride=(1, 2)), dict(weight_bits=4)),
                                     (lambda m: m.Conv2d(8, 4, 3, groups=2), dict(weight_bits=4)), (lambda m: m.Linear(8, 4), dict(weight_bits=4)),
                                     (lambda m: m.ConvTranspose2d(8, 4, 3), dict(weight_bits=4)), (lambda m: m.Add(), dict(weight_bits=4)),
                                     (lambda m: m.Conv2d(8, 4, 3), dict()), (lambda m: m.Conv2d(8, 4, 3), dict(weight_bits=8)),
                                     (lambda m: m.Conv2d(8, 4, 3), dict(weight_bits=4, group_size=64)),
                                     (lambda m: m.Conv2d(8, 4, 3), dict(weight_bits=4, sparsity="2:4"))])
def test_everything_else_is_refused(i8ie, make, kw):
    layer = make(i8ie)
    with pytest.raises(ValueError):
        layer.convert(spatial=True, **kw)
    assert layer.weight_bits() == 8 and not layer.layer.is_quantized()


def test_module_keyword_and_kernel_key(i8ie):
    from int8inferenceengine_amd import workloads as wl

    net = i8ie.Module()
    net.conv = i8ie.Conv2d(64, 16, 3, padding=1)
    for kw in (dict(), dict(weight_bits=8), dict(weight_bits=4, group_size=64), dict(weight_bits=8, sparsity="2:4")):
        with pytest.raises(ValueError):
            net.convert(spatial=True, **kw)
    assert not net.is_quant and not net.conv.layer.is_quantized()
    for f in (i8ie.Module.convert, i8ie.Layer.convert, wl.calibrated):
        assert inspect.signature(f).parameters["spatial"].default is False
    state = {"conv.qparams": np.array([0.0, 1.0, 0.0]), "conv.q_weight4": np.zeros((16, 288), np.uint8)}
    with pytest.raises(RuntimeError, match="only a Linear"):   # no kernel key: today's refusal
        net.load_quantized(state)
    with pytest.raises(ValueError, match="disagrees"):
        net.load_quantized(dict(state, **{"conv.q_weight4_kernel": np.array([5, 5], np.int32)}))
    other = i8ie.Module()
    other.rect = i8ie.Conv2d(64, 16, (3, 1))   # the kernel agrees, but a rectangular layer takes no 4-bit weights
    with pytest.raises(ValueError, match="disagrees"):
        other.load_quantized({"rect.qparams": state["conv.qparams"], "rect.q_weight4": np.zeros((16, 96), np.uint8),
                              "rect.q_weight4_kernel": np.array([3, 1], np.int32)})


@pytest.mark.parametrize("args,text", [((16, 32, 0, 1, 1, 1), "non-positive dimension"), ((16, 32, 3, 0, 1, 1), "stride must be positive"),
                                       ((16, 32, 3, 1, -1, 1), "negative padding"), ((16, 32, 3, 1, 1, 0), "dilation must be >= 1"),
                                       ((0, 32, 3, 1, 1, 1), "non-positive dimension"), ((16, 8192, 3, 1, 1, 1), "at most 65536")])
def test_create_argument_errors_need_no_device(args, text):
    lib, L = abi.lib(), C.c_void_p()
    buf = (C.c_uint8 * 16)()
    assert lib.i8ie_conv2d_create_w4_geom(None, buf, buf, buf, *args, C.byref(L)) != 0 and L.value is None
    assert text in lib.i8ie_last_error().decode()
