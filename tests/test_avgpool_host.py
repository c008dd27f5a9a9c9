"""Quantized average pooling without a GPU: the numpy restatement against a brute-force Python-integer / fractions
computation, the Python / extension / C surface, the argument checks (raised before any device call), and the two new
workloads."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import abi
import avgpool_ref as apr
from support import i8ie  # noqa: F401

f32 = np.float32


@pytest.mark.parametrize("shape,kh,kw,s", [((2, 3, 7, 9), 2, 2, 2), ((1, 2, 9, 11), 3, 3, 2), ((2, 1, 6, 7), 3, 4, 1),
                                           ((1, 3, 5, 4), 5, 4, 1), ((1, 1, 4, 4), 1, 1, 3), ((1, 2, 13, 13), 7, 7, 3)])
def test_u8_restatement_equals_rational_rounding(shape, kh, kw, s):
    """(S + n // 2) // n in Python integers, and the same thing said with fractions: floor(mean + 1/2), i.e. round to
    nearest with ties up."""
    rng = np.random.default_rng(kh * 100 + kw * 10 + s)
    q = rng.integers(0, 256, shape, dtype=np.uint8)
    q[0, 0, :kh, :kw] = 255  # the largest sum
    got = apr.avg_pool2d_u8(q, kh, kw, s)
    oh, ow = apr.out_hw(shape[2], shape[3], kh, kw, s)
    assert got.shape == (shape[0], shape[1], oh, ow) and got.dtype == np.uint8 and got[0, 0, 0, 0] == 255
    n = kh * kw
    for i in range(shape[0]):
        for c in range(shape[1]):
            for y in range(oh):
                for x in range(ow):
                    S = sum(int(q[i, c, y * s + m, x * s + l]) for m in range(kh) for l in range(kw))
                    assert int(got[i, c, y, x]) == (S + n // 2) // n == math.floor(Fraction(S, n) + Fraction(1, 2)), (i, c, y, x)


def test_u8_ties_go_up_relu_floor_and_global():
    q = np.array([[[[0, 1], [0, 0]], [[1, 1], [0, 0]], [[1, 1], [1, 0]], [[255, 254], [255, 255]]]], np.uint8)  # sums 1, 2, 3, 1019
    assert apr.avg_pool2d_u8(q, 2, 2, 2).ravel().tolist() == [0, 1, 1, 255]  # 0.25 -> 0, the tie 0.5 -> 1, 0.75 -> 1, 254.75 -> 255
    assert apr.avg_pool2d_u8(q, 2, 2, 2, relu=True, zp=1).ravel().tolist() == [1, 1, 1, 255]
    assert np.array_equal(apr.global_avg_pool2d_u8(q), apr.avg_pool2d_u8(q, 2, 2, 1))
    assert apr.global_avg_pool2d_u8(q).shape == (1, 4, 1, 1)
    # truncation would sit half an LSB low on average; this rule does not
    rng = np.random.default_rng(3)
    r = rng.integers(0, 256, (1, 1, 64, 64), dtype=np.uint8)
    exact = r.reshape(32, 2, 32, 2).transpose(0, 2, 1, 3).reshape(32, 32, 4).mean(-1)
    assert abs(float((apr.avg_pool2d_u8(r, 2, 2, 2)[0, 0] - exact).mean()) - 0.125) < 0.05  # (ties up: +1/8 LSB for n = 4)


def test_f32_restatement_against_fractions():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1, 2, 5, 6)) * 3).astype(f32)
    got = apr.avg_pool2d_f32(x, 2, 3, 2)
    mean, mag = apr.avg_pool2d_f64(x, 2, 3, 2)
    assert got.dtype == f32 and got.shape == mean.shape == (1, 2, 2, 2)
    for idx in np.ndindex(got.shape):
        i, c, y, xx = idx
        exact = sum(Fraction(float(x[i, c, y * 2 + m, xx * 2 + l])) for m in range(2) for l in range(3)) / 6
        assert abs(Fraction(float(got[idx])) - exact) <= Fraction(7 * 2.0 ** -24) * Fraction(float(mag[idx])) * Fraction(101, 100)
        assert abs(Fraction(float(mean[idx])) - exact) <= Fraction(2.0 ** -48) * Fraction(float(mag[idx]))
    # window order, rows outer and columns inner: 2^24 + 1 + 1 + ... loses every 1 only in that order
    w = np.array([[[[16777216.0, 1.0], [1.0, 1.0]]]], f32)
    assert apr.avg_pool2d_f32(w, 2, 2, 1).ravel().tolist() == [4194304.0]
    assert apr.avg_pool2d_f32(w[:, :, ::-1, ::-1].copy(), 2, 2, 1).ravel().tolist() == [4194305.0]  # (3 + 2^24 is exact in the sum)


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    assert callable(i8ie.avg_pool2d) and callable(i8ie.global_avg_pool2d)
    assert hasattr(cx, "avg_pool2d") and hasattr(cx, "global_avg_pool2d")
    assert "avg_pool2d" in i8ie.__all__ and "global_avg_pool2d" in i8ie.__all__
    assert "stride" in i8ie.avg_pool2d.__doc__ and i8ie.global_avg_pool2d.__doc__


def test_new_symbols_are_declared_and_exported():
    names = abi.declared_symbols()
    lib = apr.bind(abi.lib())
    for n in ["i8ie_avgpool2d_u8", "i8ie_avgpool2d_u8_nhwc", "i8ie_avgpool2d_f32"]:
        assert n in names and hasattr(lib, n), n
    assert lib.i8ie_version() == 1


def test_entry_points_check_arguments_before_any_device_call():
    lib = apr.bind(abi.lib())
    one = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)
    ctx = C.c_void_p(16)

    def nchw(f, c=ctx, i=one, o=one, n=1, ch=4, h=8, w=8, kh=2, kw=2, s=2):
        return f(c, i, o, n, ch, h, w, kh, kw, s)

    def nhwc(c=ctx, i=one, ib=0, o=one, ob=0, n=1, ch=4, h=8, w=8, kh=2, kw=2, s=2):
        return lib.i8ie_avgpool2d_u8_nhwc(c, i, ib, 0, o, ob, 0, n, ch, h, w, kh, kw, s, 0, 0)

    calls = [lambda **k: nchw(lib.i8ie_avgpool2d_u8, **k), lambda **k: nchw(lib.i8ie_avgpool2d_f32, **k), nhwc]
    for call in calls:
        for bad in (dict(c=None), dict(i=None), dict(o=None)):
            assert call(**bad) == -1 and b"null" in lib.i8ie_last_error(), bad
        for bad in (dict(n=0), dict(ch=0), dict(h=-1), dict(w=0), dict(kh=0), dict(kw=-2), dict(s=0)):
            assert call(**bad) == -1 and b"dimension" in lib.i8ie_last_error(), bad
        for bad in (dict(kh=9), dict(kw=9), dict(h=1)):
            assert call(**bad) == -1 and b"larger" in lib.i8ie_last_error(), bad
        assert call(h=300, w=300, kh=256, kw=257) == -1 and b"65536" in lib.i8ie_last_error()  # n = 65792
    for bad in (dict(ib=-1), dict(ob=-1)):
        assert nhwc(**bad) == -1 and b"dimension" in lib.i8ie_last_error(), bad


def test_python_errors_are_raised_before_any_device_call():
    """_CXX_i8ie.Tensor() is default-constructible without a device; the shape checks come first for every overload."""
    import _CXX_i8ie as cx

    tried = 0
    for cls in ("6TensorIfE", "6TensorIhE"):  # the FP32 and the u8 tensor, as the reference's module names them
        e = getattr(cx, cls)()
        assert e.shape() == []
        for call in (lambda: cx.avg_pool2d(e, 2, 2), lambda: cx.global_avg_pool2d(e), lambda: cx.avg_pool2d(e, 0, 1)):
            with pytest.raises(RuntimeError, match="expects an NCHW tensor"):
                call()
            tried += 1
    assert tried == 6


def test_workloads():
    from int8inferenceengine_amd import workloads as wl

    # ResNet-18 for CIFAR-10, main path (the projection branches are not counted, as for resnet_tiny):
    #   stem 32*32*64*27; stage 1: four 3x3 convs 64 -> 64 at 32x32; stages 2-4: one strided 3x3 conv in -> out and three
    #   out -> out at half the size -- the same 37 748 736 MACs per out -> out conv in every stage; fc 512 * 10
    same = 32 * 32 * 64 * 64 * 9
    assert same == 16 * 16 * 128 * 128 * 9 == 8 * 8 * 256 * 256 * 9 == 4 * 4 * 512 * 512 * 9 == 37748736
    hand = 32 * 32 * 64 * 27 + 4 * same + 3 * (same // 2 + 3 * same) + 5120
    assert hand == 549131264
    assert wl.macs_per_image("resnet18_cifar") == hand
    layers, spec, shape = wl.NETWORKS["resnet18_cifar"]
    assert shape == (3, 32, 32) and len(wl.layer_names("resnet18_cifar")) == 21 and len(wl.add_names("resnet18_cifar")) == 8
    assert layers["stem"] == ("conv", 3, 64, 3, 1, 1) and layers["fc"] == ("fc", 512, 10)
    assert [k for k in layers if k.endswith("proj")] == ["s2b1proj", "s3b1proj", "s4b1proj"]
    assert layers["s3b1proj"] == ("conv", 128, 256, 1, 2, 0) and layers["s3b1c1"] == ("conv", 128, 256, 3, 2, 1)
    assert spec[-3:] == [("gap",), ("flatten", 512), ("layer", "fc")] and not any(op[0] == "pool" for op in spec)
    # resnet_tiny with the pooled head
    tl, ts, tshape = wl.NETWORKS["resnet_tiny_gap"]
    rl, rs, _ = wl.NETWORKS["resnet_tiny"]
    assert tshape == (3, 32, 32) and ts[:-4] == rs[:-3] and ts[-4:] == [("avgpool", 2, 2), ("gap",), ("flatten", 32), ("layer", "fc")]
    assert tl["fc"] == ("fc", 32, 10) and {k: v for k, v in tl.items() if k != "fc"} == {k: v for k, v in rl.items() if k != "fc"}
    assert wl.macs_per_image("resnet_tiny_gap") == wl.macs_per_image("resnet_tiny") - 2048 * 10 + 32 * 10
    # the existing entries are what they were
    assert rs[-3:] == [("pool", 2, 2), ("flatten", 2048), ("layer", "fc")] and rl["fc"] == ("fc", 2048, 10)
    assert wl.macs_per_image("alexnet") == wl.ALEXNET_MACS_PER_IMAGE
    net = wl.build("resnet18_cifar")
    assert sorted(k for k, _ in net._layers()) == sorted(wl.layer_names("resnet18_cifar") + wl.add_names("resnet18_cifar"))
    net.load(wl.synthetic_state_dict("resnet18_cifar"))
