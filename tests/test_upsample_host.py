"""Quantized upsampling without a GPU: the integer restatement of tests/upsample_ref.py against torch's
CPU interpolate in float64 for every factor pair, the 16-bit bound behind the factor limit of 8, the spec op in workloads.py
(no pre-existing network's MACs move, the walkers see the new op) and the Python surface (exported; argument errors raised
before any device call)."""
import itertools

import numpy as np
import pytest

import abi
from support import i8ie  # noqa: F401
import upsample_ref as ur

f32 = np.float32
SHAPES = [(1, 1), (1, 3), (2, 2), (3, 5), (7, 4)]
PAIRS = list(itertools.product(range(1, 9), repeat=2))


def _bytes(h, w, seed):
    """[2, 3, h, w] u8: random bytes with both extremes present"""
    q = np.random.default_rng(seed).integers(0, 256, (2, 3, h, w), dtype=np.uint8)
    q.flat[0], q.flat[-1] = 0, 255
    return q


@pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_restatement_against_torch_float64(h, w):
    """all 64 factor pairs: S / D is torch's bilinear value (align_corners=False) to 1e-9, the rounded byte within half a
    code of it, and nearest is torch's nearest exactly"""
    import torch
    import torch.nn.functional as F

    q = _bytes(h, w, 100 * h + w)
    t = torch.from_numpy(q.astype(np.float64))
    worst = 0.0
    for fh, fw in PAIRS:
        want = F.interpolate(t, scale_factor=(fh, fw), mode="bilinear", align_corners=False).numpy()
        S, D = ur.bilinear_sd(q, fh, fw)
        out = ur.upsample_u8(q, fh, fw, "bilinear")
        assert out.shape == want.shape == (2, 3, h * fh, w * fw) and out.dtype == np.uint8
        err = np.abs(S / float(D) - want).max()
        worst = max(worst, float(err))
        assert err <= 1e-9, (fh, fw, err)
        assert np.abs(out.astype(np.float64) - want).max() <= 0.5 + 1e-9, (fh, fw)
        val, mag = ur.bilinear_f64(q, fh, fw)
        assert np.array_equal(val, S / float(D)) and mag.max() <= 255
        near = F.interpolate(t, scale_factor=(fh, fw), mode="nearest").numpy()
        assert np.array_equal(ur.upsample_u8(q, fh, fw, "nearest"), near.astype(np.uint8)), (fh, fw)
    print("%dx%d: worst |S/D - torch| = %.3g" % (h, w, worst))


def test_rounding_is_to_nearest_ties_up_and_relu_is_a_floor():
    q = _bytes(3, 5, 1)
    for fh, fw in [(2, 2), (3, 2), (8, 8)]:
        S, D = ur.bilinear_sd(q, fh, fw)
        out = ur.upsample_u8(q, fh, fw, "bilinear").astype(np.int64)
        assert np.array_equal(out, np.floor(S / float(D) + 0.5).astype(np.int64))  # (S / D + 1/2 is exact in float64)
        tie = (S % D) * 2 == D
        assert np.array_equal(out[tie] * D, S[tie] + D // 2)
        for zp in (0, 128, 255):
            assert np.array_equal(ur.upsample_u8(q, fh, fw, "bilinear", True, zp), np.maximum(out, zp).astype(np.uint8))
            assert np.array_equal(ur.upsample_u8(q, fh, fw, "nearest", True, zp), np.maximum(ur.nearest(q, fh, fw), zp))


def test_weights_sum_and_sixteen_bit_bound():
    """w0 + w1 = 2 f on every output index, so S <= 255 D; S + D / 2 < 2^16 for every factor pair within 1..8 (65 408 at
    8 x 8) and not at 9 x 9: the reason for the bound of 8"""
    for f in range(1, 9):
        for L in (1, 2, 5):
            i0, i1, w0, w1 = ur.taps(L, f)
            assert np.array_equal(w0 + w1, np.full(L * f, 2 * f)) and w0.min() >= 0 and w1.min() >= 0
            assert i0.min() >= 0 and i1.max() <= L - 1 and np.all(i1 - i0 <= 1) and np.all(i1 >= i0)
    full = np.full((1, 1, 3, 3), 255, np.uint8)
    worst = 0
    for fh, fw in PAIRS:
        S, D = ur.bilinear_sd(full, fh, fw)
        assert S.max() == S.min() == 255 * D
        worst = max(worst, int(S.max()) + D // 2)
        assert int(S.max()) + D // 2 < 65536, (fh, fw)
    assert worst == 65408
    assert 255 * 4 * 9 * 9 + 2 * 9 * 9 >= 65536


def test_fp32_restatement_close_to_float64():
    """the FP32 sequence stays inside the bound the GPU test uses, 16 * 2^-24 * max|window|"""
    x = np.random.default_rng(3).standard_normal((2, 3, 5, 4)).astype(f32)
    for fh, fw in [(1, 1), (2, 2), (3, 2), (2, 3), (8, 8)]:
        val, mag = ur.bilinear_f64(x, fh, fw)
        got = ur.upsample_f32(x, fh, fw, "bilinear")
        assert got.dtype == f32 and np.all(np.abs(got.astype(np.float64) - val) <= 16 * 2.0 ** -24 * mag), (fh, fw)
        assert np.array_equal(ur.upsample_f32(x, fh, fw, "nearest").view(np.uint32), ur.nearest(x, fh, fw).view(np.uint32))


# ---- workloads.py ------------------------------------------------------------------------------------------------------------
def test_macs_of_existing_networks_unchanged():
    """(the figures of the networks before the ("upsample", ...) spec op: tests/test_workloads_host.py)"""
    from int8inferenceengine_amd import workloads as wl

    # a bilinear x2 and a 1x1 conv at four times the pixels cost what the 2x2 stride-2 up-conv costs
    assert wl.macs_per_image("unet_bilinear_cifar") == wl.macs_per_image("unet_cifar")
    # upsample_tiny by hand: (pixels, out_c, in_c * k * k) of every conv outside a branch
    convs = [(32 * 32, 16, 27), (16 * 16, 20, 144), (8 * 8, 35, 180), (4 * 4, 35, 315), (8 * 8, 20, 315), (16 * 16, 16, 180),
             (32 * 32, 16, 144), (16 * 16, 20, 144), (32 * 32, 16, 324), (32 * 48, 16, 144), (32 * 48, 10, 16)]
    assert wl.macs_per_image("upsample_tiny") == sum(p * o * k for p, o, k in convs)


def test_spec_op_is_walked():
    from int8inferenceengine_amd import workloads as wl

    ups = [op for op in wl._walk(wl.NETWORKS["upsample_tiny"][1]) if op[0] == "upsample"]
    assert ups == [("upsample", 2, "nearest")] * 3 + [("upsample", 2, "bilinear"), ("upsample", (2, 3), "bilinear")]
    assert wl.upsample_factors(2) == (2, 2) and wl.upsample_factors((2, 3)) == (2, 3)
    assert wl.layer_names("upsample_tiny") == ["c1", "c2", "c3", "c4", "l3", "p3", "l2", "p2", "l1", "p1", "d1", "dec", "e1", "head"]
    assert wl.add_names("upsample_tiny") == ["a3", "a2", "a1"] and wl.concat_names("upsample_tiny") == ["cat1"]
    layers, spec, _ = wl.NETWORKS["unet_bilinear_cifar"]
    base_layers, base_spec, _ = wl.NETWORKS["unet_cifar"]
    assert [op for op in wl._walk(spec) if op[0] == "upsample"] == [("upsample", 2, "bilinear")] * 3
    assert [op for op in spec if op[0] != "upsample"] == base_spec and list(layers) == list(base_layers)
    for attr, L in base_layers.items():
        assert layers[attr] == (("conv", L[1], L[2], 1, 1, 0) if L[0] == "deconv" else L), attr
    assert wl.layer_names("unet_bilinear_cifar") == wl.layer_names("unet_cifar")
    sd = wl.synthetic_state_dict("unet_bilinear_cifar")
    assert sd["up3.weight"].shape == (256, 512, 1, 1) and sd["up1.weight"].shape == (64, 128, 1, 1)


# ---- the surface --------------------------------------------------------------------------------------------------------------
def test_surface_exports_upsample(i8ie):
    import _CXX_i8ie as cx

    assert "upsample" in i8ie.__all__ and callable(i8ie.upsample) and hasattr(cx, "upsample")
    lib = ur.bind(abi.lib())
    for name in ("i8ie_upsample2d_u8", "i8ie_upsample2d_u8_nhwc", "i8ie_upsample2d_f32"):
        assert name in abi.declared_symbols() and hasattr(lib, name)
    header = open(abi.HEADER).read()
    assert "#define I8IE_UPSAMPLE_NEAREST 0" in header and "#define I8IE_UPSAMPLE_BILINEAR 1" in header
    # a null context is an argument error like everywhere else
    assert lib.i8ie_upsample2d_u8(None, None, None, 1, 1, 1, 1, 2, 2, 0) == -1 and b"null" in lib.i8ie_last_error()


def test_surface_errors_come_before_any_device_call(i8ie):
    """(there is no GPU here: anything that reached the device would fail with another message)"""
    t = i8ie.tensor(np.zeros((2, 3, 4, 5), f32))
    for bad in (lambda: i8ie.upsample(t, 0), lambda: i8ie.upsample(t, 9), lambda: i8ie.upsample(t, (2, 9)),
                lambda: i8ie.upsample(t, (-1, 2), "bilinear"), lambda: i8ie.upsample(t, 2, "bicubic"),
                lambda: i8ie.upsample(t.reshape(6, 20), 2), lambda: i8ie.upsample(t.reshape(2, 3, 20), 2, "bilinear")):
        with pytest.raises(RuntimeError, match="upsample"):
            bad()
    for bad in (lambda: i8ie.upsample(t, 2.0), lambda: i8ie.upsample(t, (2, 1.5)), lambda: i8ie.upsample(t, (2, 2, 2)),
                lambda: i8ie.upsample(t, "2"), lambda: i8ie.upsample(t, True)):
        with pytest.raises(TypeError):
            bad()
