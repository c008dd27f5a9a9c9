"""i8ie_quantize_weight_per_channel (host side of the per-channel mode) through the C-ABI, bit for bit against the
numpy restatement of DESIGN.md "Per-channel weight scales"; the per-tensor quantizer still matches the oracle on the
same data.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
import orc
import pc_pipeline


def quantize_pc_abi(w, b):
    w = np.ascontiguousarray(w, np.float32)
    rows = w.shape[0]
    qw = np.empty(w.shape, np.int8)
    qb = np.empty(rows, np.int8)
    s = np.empty(rows, np.float32)
    bp = None if b is None else np.ascontiguousarray(b, np.float32)
    abi.ck(abi.lib().i8ie_quantize_weight_per_channel(
        w.ctypes.data_as(C.c_void_p), rows, C.c_int64(w.size // rows), None if bp is None else bp.ctypes.data_as(C.c_void_p),
        qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
    return qw, qb, s


def cases():
    rng = np.random.default_rng(11)
    w = rng.standard_normal((24, 3, 5, 5)).astype(np.float32) * np.exp(rng.uniform(-3.4, 0, 24)).astype(np.float32)[:, None, None, None]
    b = rng.standard_normal(24).astype(np.float32) * 0.1
    w[3] = 0.0  # an all-zero row (and bias): s_w = 1
    b[3] = 0.0
    w[5] *= 0.01  # a row whose max-abs is its bias
    b[5] = -0.75
    w[7] = np.abs(w[7]) + 0.5  # an all-positive row
    b[7] = 0.25
    yield "conv", w, b
    # x / s_w exactly a half-integer in fp32: a = 127 * 2^-3, s_w = 2^-3, x = (k + 0.5) * 2^-3
    halves = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 125.5, -126.5], np.float32) * np.float32(0.125)
    wl = np.zeros((3, 9), np.float32)
    wl[:, :8] = halves
    wl[:, 8] = np.float32(127 * 0.125)
    yield "half", wl, np.zeros(3, np.float32)
    yield "linear", (rng.standard_normal((50, 64)) * 0.05).astype(np.float32), (rng.standard_normal(50) * 0.01).astype(np.float32)


@pytest.mark.parametrize("name,w,b", list(cases()), ids=[c[0] for c in cases()])
def test_per_channel_quantizer_matches_numpy_restatement(name, w, b):
    qw, qb, s = quantize_pc_abi(w, b)
    ew, eb, es = pc_pipeline.quantize_weight_pc(w, b)
    assert np.array_equal(s.view(np.uint32), es.view(np.uint32))
    assert np.array_equal(qw, ew) and np.array_equal(qb, eb)
    assert np.abs(qw.astype(np.int32)).max() <= 127 and np.abs(qb.astype(np.int32)).max() <= 127
    # the per-tensor rule on the same data is untouched
    pw, pb, ps = orc.quantize_weight(w, b)
    qw1, qb1, s1 = np.empty(w.shape, np.int8), np.empty(b.shape, np.int8), C.c_float()
    abi.ck(abi.lib().i8ie_quantize_weight(np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), C.c_int64(w.size),
                                          np.ascontiguousarray(b).ctypes.data_as(C.c_void_p), C.c_int64(b.size),
                                          qw1.ctypes.data_as(C.c_void_p), qb1.ctypes.data_as(C.c_void_p), C.byref(s1)))
    assert np.float32(s1.value) == ps and np.array_equal(qw1, pw) and np.array_equal(qb1, pb)


def test_special_rows():
    _, w, b = next(iter(cases()))
    qw, qb, s = quantize_pc_abi(w, b)
    assert s[3] == 1.0 and not qw[3].any() and qb[3] == 0  # all-zero row
    assert qb[5] == -127 and s[5] == np.float32(np.float32(0.75) / np.float32(127))  # max-abs is the bias
    assert qw[7].min() > 0 and qw[7].max() == 127  # all-positive row: symmetric, no overflow
    _, wl, bl = list(cases())[1]
    qw, _, s = quantize_pc_abi(wl, bl)
    assert np.all(s == np.float32(0.125))
    assert qw[0, :8].tolist() == [0, 2, 2, 0, -2, -2, 126, -126]  # round half to even


def test_null_bias_is_zero_bias():
    rng = np.random.default_rng(2)
    w = rng.standard_normal((8, 20)).astype(np.float32)
    qw, qb, s = quantize_pc_abi(w, None)
    ew, eb, es = pc_pipeline.quantize_weight_pc(w, np.zeros(8, np.float32))
    assert np.array_equal(qw, ew) and not qb.any() and np.array_equal(s, es)


def test_numpy_down_scale_matches_oracle_per_column():
    rng = np.random.default_rng(4)
    acc = rng.integers(-2**20, 2**20, (64, 6)).astype(np.int32)
    s_w = np.float32([1e-3, 2.5e-4, 0.0, 7.1e-3, 1.0, 3.3e-5])
    got = pc_pipeline.down_scale_pc(acc, np.float32(0.025), s_w, np.float32(0.31), 17)
    for j in range(6):
        assert np.array_equal(got[:, j], orc.down_scale(acc[:, j], np.float32(0.025), s_w[j], np.float32(0.31), 17))
