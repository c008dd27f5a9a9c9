"""2:4 structured-sparse weights for Linear, the host side (include/i8ie_hip.h, "2:4 structured-sparse weights for Linear"): the
pruning rule and the compressed form against a numpy restatement, and the argument rules of convert(sparsity=).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
from support import i8ie  # noqa: F401


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def groups_of(qw):
    """[rows, G, 4]: the rows cut into aligned groups of four, a partial last group padded with zeros"""
    rows, k = qw.shape
    g = -(-k // 4)
    return np.pad(qw, ((0, 0), (0, 4 * g - k))).reshape(rows, g, 4)


def prune_ref(qw):
    """keep the two entries of largest |q| in every group, ties to the lower k (a stable sort on -|q|)"""
    g = groups_of(qw)
    order = np.argsort(-np.abs(g.astype(np.int32)), axis=2, kind="stable")
    keep = np.zeros(g.shape, bool)
    np.put_along_axis(keep, order[:, :, :2], True, axis=2)
    return np.where(keep, g, 0).reshape(qw.shape[0], -1)[:, :qw.shape[1]].astype(np.int8)


def pack_ref(qw):
    """(values [rows, 2 G], index [rows, ceil(G / 2)]): the non-zero positions, filled up with the lowest other positions"""
    g = groups_of(qw)
    rows, G, _ = g.shape
    values, index = np.zeros((rows, 2 * G), np.int8), np.zeros((rows, (G + 1) // 2), np.uint8)
    for j in range(rows):
        for i in range(G):
            pos = [p for p in range(4) if g[j, i, p] != 0]
            pos = sorted(pos + [p for p in range(4) if g[j, i, p] == 0][:2 - len(pos)])
            values[j, 2 * i:2 * i + 2] = g[j, i, pos]
            index[j, i // 2] |= (pos[0] | pos[1] << 2) << (4 * (i % 2))
    return values, index


def prune(qw):
    out = np.empty_like(qw)
    assert abi.lib().i8ie_prune_2_4(ptr(qw), qw.shape[0], qw.shape[1], ptr(out)) == 0
    return out


def pack(qw):
    G = -(-qw.shape[1] // 4)
    values, index = np.full((qw.shape[0], 2 * G), 99, np.int8), np.full((qw.shape[0], (G + 1) // 2), 0xFF, np.uint8)
    rc = abi.lib().i8ie_pack_2_4(ptr(qw), qw.shape[0], qw.shape[1], ptr(values), ptr(index))
    return rc, values, index


CRAFTED = np.array([[5, -5, 5, -5,    3, 3, 3, 3,      0, 0, 0, 0,    0, 0, -7, 0],    # ties, all equal, all zero, one non-zero
                    [1, -128, 127, 2, 0, 9, 0, -9,     -1, 0, 0, 1,   4, -3, 2, 1],
                    [0, 0, 0, 6,      -128, 127, 127, -128,  2, 1, 0, 0,  0, 1, 2, 0]], np.int8)


def test_pruning_rule_on_crafted_groups():
    got = prune(CRAFTED)
    assert np.array_equal(got, prune_ref(CRAFTED))
    assert list(got[0]) == [5, -5, 0, 0, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, -7, 0] and list(got[1, :4]) == [0, -128, 127, 0]
    assert list(got[2, 4:8]) == [-128, 0, 0, -128] and np.array_equal(prune(got), got)   # (2:4 already: unchanged)
    six = np.array([[1, 2, 3, 4, 5, 6], [9, 0, 0, 9, 0, -1]], np.int8)                  # K = 6: the last group is (q4, q5, 0, 0)
    assert np.array_equal(prune(six), prune_ref(six)) and list(prune(six)[0]) == [0, 0, 3, 4, 5, 6]
    rnd = np.random.default_rng(1).integers(-128, 128, (7, 37), dtype=np.int8)
    assert np.array_equal(prune(rnd), prune_ref(rnd)) and np.array_equal(np.abs(prune(rnd)).max(1), np.abs(rnd).max(1))


@pytest.mark.parametrize("k", [4, 6, 8, 37])
def test_pack_unpack_pack_identity_and_canonical_form(k):
    qw = prune_ref(np.random.default_rng(k).integers(-3, 4, (5, k), dtype=np.int8))   # (small values: many zeros, fill-ups occur)
    qw[0] = 0
    rc, values, index = pack(qw)
    rv, ri = pack_ref(qw)
    assert rc == 0 and np.array_equal(values, rv) and np.array_equal(index, ri)
    back = np.full_like(qw, 77)
    assert abi.lib().i8ie_unpack_2_4(ptr(values), ptr(index), 5, k, ptr(back)) == 0 and np.array_equal(back, qw)
    rc, v2, i2 = pack(back)
    assert rc == 0 and np.array_equal(v2, values) and np.array_equal(i2, index)
    assert index[0, 0] & 15 == 0b0100                                                # all-zero group: positions 0 and 1
    dense = qw.copy()
    dense[1, :3] = (1, 2, 3)
    assert pack(dense)[0] != 0                                                         # three non-zeros in one group
    index[2, 0] = 0b0001                                                               # first position 1, second 0
    assert abi.lib().i8ie_unpack_2_4(ptr(values), ptr(index), 5, k, ptr(back)) != 0


def test_sparsity_argument_rules(i8ie):
    conv, lin = i8ie.Conv2d(2, 3, 3), i8ie.Linear(8, 4)
    for layer, kw in ((conv, {"sparsity": "2:4"}), (i8ie.Add(), {"sparsity": "2:4"}), (lin, {"sparsity": "1:2"}), (lin, {"sparsity": 2}),
                      (i8ie.Add(), {"sparsity": "4:8"}), (lin, {"sparsity": "2:4", "weight_bits": 4})):
        with pytest.raises(ValueError):
            layer.convert(**kw)
    for kw in ({"sparsity": "dense"}, {"sparsity": "2:4", "weight_bits": 4}):
        with pytest.raises(ValueError):
            i8ie.Module().convert(**kw)
    assert lin.sparsity() is None and conv.sparsity() is None and not lin.layer.is_quantized()
    with pytest.raises(ValueError):   # dense integers that are not 2:4: nothing is pruned at load
        lin.load_quantized(np.ones((4, 8), np.int8), np.zeros(4, np.int8), 0.5, 1.0, 0, sparsity="2:4")
    with pytest.raises(ValueError):
        conv.load_quantized(np.zeros((3, 2, 3, 3), np.int8), np.zeros(3, np.int8), 0.5, 1.0, 0, sparsity="2:4")
    assert lin.sparsity() is None and not lin.layer.is_quantized()
    net = i8ie.Module()
    net.conv = conv
    with pytest.raises(RuntimeError, match="only a Linear"):   # 2:4 weights saved for a layer that cannot take them
        net.load_quantized({"conv.qparams": np.array([0.5, 1.0, 0.0]), "conv.q_weight24": np.zeros((3, 10), np.int8),
                            "conv.q_index24": np.zeros((3, 3), np.uint8), "conv.q_bias": np.zeros(3, np.int8)})
