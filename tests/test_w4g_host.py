"""4-bit weights with group-wise scales along K, the host side (include/i8ie_hip.h, "4-bit weights for Linear with group-wise
scales"): the quantiser entry against its float32 restatement, the argument rules of convert(group_size=), what create and the
state-dict loader refuse.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
from support import i8ie  # noqa: F401
import w4g_ref

f32 = np.float32


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("gs", [64, 128, 256])
def test_quantizer_matches_the_restatement(gs):
    rng = np.random.default_rng(gs)
    n, k = 6, 2 * gs + 37                                  # (a partial last group of 37)
    w = rng.normal(0, 0.05, (n, k)).astype(f32)
    b = rng.normal(0, 0.05, n).astype(f32)
    w[0], b[0] = 0.0, 0.0                                  # a zero row: scale 1 / 32, every m = 1
    b[1] = 40.0                                            # a bias-dominated row: a_1 = 40 * 7 / 127, every group small
    w[2] = np.clip(w[2] * f32(0.5), -0.09, 0.09)           # one outlier group: m = 32 beside m = 1 (32 * 0.09 / 3 < 1) ...
    w[2, 5], w[2, gs + 3] = 0.08, 3.0                      # ... where 0.08 is level 6 (it is 0 at the row's scale 3 / 7)
    w[3, :gs], w[3, gs:], b[3] = 3.5, 0.0, 0.25            # a_3 = 3.5, S = 0.5 ...
    w[3, gs:gs + 14] = (np.arange(-7, 7) + f32(0.5)) * f32(0.5) * f32(0.5)   # ... group 1: top 1.625, m = 15, step 0.234375
    w[3, 2 * gs:2 * gs + 14] = (np.arange(-7, 7) + f32(0.5)) * f32(0.0625)   # group 2: top 0.40625, m = 4, step 0.0625: all ties
    q, m, qb, s = np.empty((n, k), np.int8), np.empty((n, 3), np.uint8), np.empty(n, np.int8), np.empty(n, f32)
    assert abi.lib().i8ie_quantize_weight_w4g(ptr(w), n, C.c_int64(k), ptr(b), gs, ptr(q), ptr(m), ptr(qb), ptr(s)) == 0
    rq, rm, rb, rs = w4g_ref.quantize_w4g(w, b, gs)
    assert np.array_equal(s, rs) and np.array_equal(m, rm) and np.array_equal(q, rq) and np.array_equal(qb, rb)
    assert s[0] == f32(1) / 32 and list(m[0]) == [1, 1, 1] and qb[1] == 127 and m[1].max() <= 4
    assert list(m[2]) == [1, 32, 1] and q[2, 5] == 6 and q[2, gs + 3] == 7
    assert list(m[3]) == [32, 15, 4] and list(q[3, 2 * gs:2 * gs + 4]) == [-6, -6, -4, -4] and qb[3] == 0
    assert abi.lib().i8ie_quantize_weight_w4g(ptr(w), n, C.c_int64(k), ptr(b), 100, ptr(q), ptr(m), ptr(qb), ptr(s)) != 0


def test_group_size_argument_rules(i8ie):
    conv, lin = i8ie.Conv2d(2, 3, 3), i8ie.Linear(8, 4)
    for layer, kw in ((conv, {"weight_bits": 4, "group_size": 128}), (conv, {"group_size": 128}), (i8ie.Add(), {"group_size": 64}),
                      (lin, {"weight_bits": 8, "group_size": 128}), (lin, {"group_size": 128}), (lin, {"weight_bits": 4, "group_size": 100}),
                      (lin, {"weight_bits": 4, "group_size": True}), (lin, {"sparsity": "2:4", "group_size": 128}),
                      (lin, {"weight_bits": 4, "sparsity": "2:4", "group_size": 128})):
        with pytest.raises(ValueError):
            layer.convert(**kw)
    for kw in ({"group_size": 128}, {"weight_bits": 4, "group_size": 32}, {"sparsity": "2:4", "group_size": 64}):
        with pytest.raises(ValueError):
            i8ie.Module().convert(**kw)
    assert lin.group_size() is None and conv.group_size() is None and not lin.layer.is_quantized()
    with pytest.raises(RuntimeError):
        lin.group_scales()


def test_create_refuses_bad_multipliers_and_sizes():
    """the values are checked before the context is used: each refusal names its own reason"""
    def create(m, k=128, gs=64):
        n = m.shape[0]
        rc = abi.lib().i8ie_linear_create_w4g(None, ptr(np.zeros((n, (k + 1) // 2), np.uint8)), ptr(m), ptr(np.zeros(n, np.int8)),
                                              ptr(np.ones(n, f32)), n, k, gs, C.byref(C.c_void_p()))
        return rc, abi.lib().i8ie_last_error().decode()

    good = np.array([[1, 32], [16, 7]], np.uint8)
    rc, why = create(good)
    assert rc != 0 and "context" in why                    # (no device here: only the missing context is left to refuse)
    for bad in (0, 33):
        m = good.copy()
        m[1, 0] = bad
        rc, why = create(m)
        assert rc != 0 and "outside [1, 32]" in why and "feature 1, group 0" in why, why
    rc, why = create(np.ones((2, 129), np.uint8), k=32769, gs=256)
    assert rc != 0 and "32768" in why
    rc, why = create(good, gs=100)
    assert rc != 0 and "group_size" in why


def test_state_dict_loader_checks_host_arrays(i8ie):
    """a saved grouped layer is .q_weight4 + .q_group_scales + .group_size; anything malformed is a ValueError before a device call"""
    net = i8ie.Module()
    net.fc = i8ie.Linear(128, 4)
    q, m, qb, s_w = w4g_ref.quantize_w4g(np.random.default_rng(1).normal(0, 1, (4, 128)), np.zeros(4), 64)
    packed = np.empty((4, 64), np.uint8)
    assert abi.lib().i8ie_pack_w4(ptr(q), 4, 128, ptr(packed)) == 0
    good = {"fc.qparams": np.array([0.0, 1.0, 0.0]), "fc.q_weight4": packed, "fc.q_bias": qb, "fc.w_scales": s_w,
            "fc.q_group_scales": m, "fc.group_size": np.array([64], np.int32)}
    for key, value in (("fc.group_size", np.array([100], np.int32)), ("fc.q_group_scales", np.where(m == m.max(), 33, m).astype(np.uint8)),
                       ("fc.q_group_scales", np.zeros_like(m)), ("fc.q_group_scales", m[:, :1]), ("fc.group_size", None)):
        state = {k: v for k, v in dict(good, **{key: value}).items() if v is not None}
        with pytest.raises(ValueError):
            net.load_quantized(state)
    assert not net.fc.layer.is_quantized() and net.fc.group_size() is None
