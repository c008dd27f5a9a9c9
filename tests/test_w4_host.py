"""4-bit weights for Linear, the host side (include/i8ie_hip.h, "4-bit weights for Linear"): the quantiser entry against its
float32 restatement, pack / unpack, and the argument rules of convert(weight_bits=).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
from support import i8ie  # noqa: F401

f32 = np.float32


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def quantize_w4_ref(w, b):
    a = np.maximum(np.abs(w).max(axis=1), np.abs(b) * f32(7) / f32(127)).astype(f32)
    s = np.where(a == 0, f32(1), a / f32(7)).astype(f32)
    qw = np.clip(np.rint(w / s[:, None]), -7, 7).astype(np.int8)
    qb = np.clip(np.rint(b / s), -127, 127).astype(np.int8)
    return qw, qb, s


def test_quantizer_matches_the_restatement():
    rng = np.random.default_rng(11)
    w = rng.normal(0, 0.05, (9, 37)).astype(f32)
    b = rng.normal(0, 0.05, 9).astype(f32)
    b[1], b[2] = 40.0, -3.0          # a dominant bias: it sets the scale (row 1) / it does not (row 2)
    w[3], b[3] = 0.0, 0.0            # an all-zero row: scale 1
    w[4, :14] = (np.arange(-7, 7) + f32(0.5)) * f32(0.5)   # with a_4 = 3.5, s = 0.5: w / s = -6.5 ... 6.5, all ties
    w[4, 14:], b[4] = 3.5, 0.25                            # (and b / s = 0.5: a tie as well)
    qw, qb, s = np.empty(w.shape, np.int8), np.empty(9, np.int8), np.empty(9, f32)
    assert abi.lib().i8ie_quantize_weight_w4(ptr(w), 9, C.c_int64(37), ptr(b), ptr(qw), ptr(qb), ptr(s)) == 0
    rw, rb, rs = quantize_w4_ref(w, b)
    assert np.array_equal(s, rs) and np.array_equal(qw, rw) and np.array_equal(qb, rb)
    assert s[3] == 1 and s[4] == f32(0.5) and list(qw[4, :4]) == [-6, -6, -4, -4] and qb[1] == 127 and np.abs(qw).max() == 7


@pytest.mark.parametrize("k", [1, 8, 37])
def test_pack_and_unpack_are_inverse(k):
    qw = np.random.default_rng(k).integers(-8, 8, (5, k), dtype=np.int8)
    qw[0, 0], qw[4, k - 1] = -8, 7
    packed = np.full((5, (k + 1) // 2), 0xFF, np.uint8)
    assert abi.lib().i8ie_pack_w4(ptr(qw), 5, k, ptr(packed)) == 0
    want = (qw[:, 0::2] & 15).astype(np.uint8)
    want[:, :k // 2] |= (qw[:, 1::2] & 15).astype(np.uint8) << 4    # (an odd tail's high nibble stays 0)
    assert np.array_equal(packed, want)
    back = np.empty_like(qw)
    assert abi.lib().i8ie_unpack_w4(ptr(packed), 5, k, ptr(back)) == 0 and np.array_equal(back, qw)
    qw[2, 0] = 8
    assert abi.lib().i8ie_pack_w4(ptr(qw), 5, k, ptr(packed)) != 0


def test_weight_bits_argument_rules(i8ie):
    conv, lin = i8ie.Conv2d(2, 3, 3), i8ie.Linear(8, 4)
    with pytest.raises(ValueError):
        conv.convert(weight_bits=4)
    for layer in (conv, lin, i8ie.Add()):
        with pytest.raises(ValueError):
            layer.convert(weight_bits=5)
    with pytest.raises(ValueError):
        i8ie.Module().convert(weight_bits=16)
    assert lin.weight_bits() == 8 and conv.weight_bits() == 8 and not lin.layer.is_quantized()
    net = i8ie.Module()
    net.conv = conv
    with pytest.raises(RuntimeError, match="only a Linear"):   # 4-bit weights saved for a layer that cannot take them
        net.load_quantized({"conv.qparams": np.array([0.0, 1.0, 0.0]), "conv.q_weight4": np.zeros((3, 9), np.uint8)})
