"""The numpy model of the requantiser's guard (tests/requant_ref.py) and the cases built on it (tests/requant_cases.py), on the
CPU: the model's fma against exact rational arithmetic, the class conditions of every GPU case of
tests/test_gpu_requant_replay.py from the numpy references alone, and the guard's claim -- a value further than 2^-13 from a
rounding boundary gets the exact byte from the estimate -- over dense accumulator ranges."""
from fractions import Fraction

import numpy as np
import pytest

import attention_ref as ar
import mha_ref as mr
import requant_cases as rc
import requant_ref as rq

f32 = np.float32


def _round_f32(x):
    """the Fraction x rounded to nearest-even float32"""
    c = f32(float(x))
    best = None
    for cand in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.asarray(cand, f32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 1500), rng.integers(-70000, 70000, 1500)]).astype(np.int32).astype(f32)
    b = np.exp(rng.uniform(np.log(1e-8), np.log(3e4), a.size)).astype(f32)
    b[::7] = f32(0.5)
    c = (rng.integers(0, 256, a.size) - 0.5).astype(f32)
    # sums that fall exactly between two floats at 24 bits once rounded at 53: a b = 2^24 + 1 + 2^-30 against c = 0.5 - 2^-30 ...
    a[:4], b[:4] = f32(2 ** 24), f32(1 + 2 ** -23)
    c[:4] = [f32(-0.5), f32(0.5), f32(1.5), f32(-1.5)]
    got = rq.fma32(a, b, c)
    for i in range(a.size):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (a[i], b[i], c[i], got[i], want)


def test_fract_and_replays():
    e = f32([0.0, 0.5, 1.25, -0.25, -1e-10, 126.5, -3.5])
    assert np.array_equal(rq.fract32(e), f32([0.0, 0.5, 0.25, 0.75, np.nextafter(f32(1), f32(0)), 0.5, 0.5]))
    worst = f32([[1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 2.0 ** -14]])
    assert np.array_equal(rq.replays(worst), [[True, False], [False, True]])
    assert np.array_equal(rq.replays(worst.T, quad_axis=0), np.array([[True, False], [False, True]]).T)
    assert np.array_equal(rq.value_replays(worst), [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1]])
    assert rq.fast(0.25, 2.0 ** -9, 2.0 ** -8) and not rq.fast(2.0 ** -103, 2.0 ** -9, 2.0 ** -109)
    assert rq.fast(0.25, f32([2.0 ** -9, 0.0]), 2.0 ** -8) and not rq.fast(0.25, f32([2.0 ** -9, 1e-31]), 2.0 ** -8)


@pytest.mark.parametrize("cid", list(rc.CASES))
def test_class_conditions_of_layer_cases(cid):
    cs = rc.CASES[cid]
    d = rc.operands(cs)
    acc = rc.accumulators(cs, d)
    rep = rc.report(cs, d, acc)
    print("%-40s quads %.3f inside %.3f distinct %3d below %.3f fast %d" % (cid, rep["quads"], rep["inside"], rep["distinct"],
                                                                           rep["below"], rep["fast"]))
    rq.check_class(rep, cs["relu"])
    s_in, s_w, s_out, zp = rc.scales(cs, d)
    if cs["cls"] in ("ALL", "EXACT"):   # both sequences are exact: the bytes are clamp(zp + sum x w'), and EXACT's are ALL's
        t = d["t"] if cs["pc"] else 3
        ints = np.where(np.asarray(s_w) == 0, 0, acc >> t)
        assert np.array_equal(ints << t, np.where(np.asarray(s_w) == 0, 0, acc))
        assert np.array_equal(rq.exact(acc, s_in, s_w, s_out, zp), np.clip(ints + zp, 0, 255).astype(np.uint8))
    if cs["zero"]:
        cols = np.flatnonzero(d["s_wv"] == 0)
        assert cols.size == -(-(cs["n"] - 5) // 16) and (cols % 4 != 0).all()
        assert (rq.exact(acc, s_in, s_w, s_out, zp)[..., cols] == zp).all()
        assert (rq.estimate(acc, s_in, s_w, s_out, zp)[1][..., cols] == 0).all()
    want = rc.expected(cs, d, acc)   # (the shape the GPU case compares against)
    assert want.dtype == np.uint8 and want.ndim in (2, 4)


def test_case_list_reaches_every_site_form():
    rc.check_case_list()


@pytest.mark.parametrize("cls", rq.CLASSES)
def test_class_conditions_of_matmul_and_attention(cls):
    for relu in (False, True):
        o = rq.matmul_class(cls, *rc.BMM, seed=31)
        acc = ar.matmul_acc(o["A"], o["zp_a"], o["B"], o["zp_b"])
        rep = rq.class_report(cls, acc, o["s_a"], o["s_b"], o["s_out"], o["zp_out"], relu)
        print("bmm", rep)
        rq.check_class(rep, relu)
    b, heads, d, tq = rc.ATT
    for tk in (16, 64):
        q, k, v, qp = rq.attention_class(cls, b, heads, d, tq, tk, seed=rc.ATT_SEED + tk)
        S, P, acc, O = mr.attention_u8(q, k, v, heads, relu=True, **qp)
        assert (S == qp["zp_s"]).all() and (P == 256 // tk).all()
        rep = rq.class_report(cls, acc, mr.P_SCALE, qp["s_v"], qp["s_o"], qp["zp_o"], True)
        print("attention O tk %d" % tk, rep)
        rq.check_class(rep, True)
        q, k, v, qp = rq.scores_class(cls, b, heads, d, tq, tk, seed=rc.ATT_SEED + tk)
        sacc = np.stack([ar.matmul_acc(q[:, :, h * d:(h + 1) * d], qp["zp_q"], k[:, :, h * d:(h + 1) * d], qp["zp_k"], transpose_b=True)
                         for h in range(heads)], axis=1)
        rep = rq.class_report(cls, sacc, qp["s_q"], qp["s_k"], qp["s_s"], qp["zp_s"], False)
        print("attention S tk %d" % tk, rep)
        rq.check_class(rep, False)


# ---- the guard's claim on dense data ---------------------------------------------------------------------------------------------
WINDOW, WINDOWS, WHOLE = 1 << 15, 256, 1 << 21


def dense_ranges(ms, zp):
    """(accumulators, whole): every accumulator from 2^12 below the one that reaches byte 0 to 2^12 above the one that reaches
    255 (clipped to INT32), whole = True.  Only where that is more than 2^21 values -- of the 36 scale sets below the one with
    ms = 1e-7, 2.55e9 accumulators -- 256 contiguous windows of 2^15, evenly spaced, the first and the last at the two ends,
    whole = False."""
    lo = max(-2.0 ** 31, np.floor(-zp / ms) - 4096)
    hi = min(2.0 ** 31 - 1, np.ceil((255 - zp) / ms) + 4096)
    lo, hi = int(lo), int(hi)
    if hi - lo + 1 <= WHOLE:
        return np.arange(lo, hi + 1, dtype=np.int64).astype(np.int32), True
    starts = np.linspace(lo, hi - WINDOW + 1, WINDOWS).astype(np.int64)
    return (starts[:, None] + np.arange(WINDOW)[None, :]).ravel().astype(np.int32), False


def test_guard_claim_on_dense_accumulators():
    sets = [(a, b, c, z, "per tensor") for a, b, c, z in rq.sweep_combos()]
    rows = rq.row_scales(12, np.random.default_rng(21))
    s_in = f32(0.03)
    s_out = rq.s_out_for(s_in, rows, 512.0)
    sets += [(s_in, s, s_out, 37, "per-channel row") for s in rows]
    agree_min, disagree_max, bound, inside, total, sampled = np.inf, 0.0, 0.0, 0, 0, []
    for a, b, c, z, tag in sets:
        assert rq.fast(a, b, c)
        ms = float(rq.multiplier(a, b, c))
        acc, whole = dense_ranges(ms, z)
        if not whole:
            sampled.append((float(a), float(b), float(c), z))
        want = rq.exact(acc, a, b, c, z)
        for lo in (0, z):
            est, worst = rq.estimate(acc, a, b, c, z, lo)
            same = est == np.maximum(want, np.uint8(lo))
            stands = worst >= f32(rq.GUARD)
            assert same[stands].all(), (tag, a, b, c, z, lo, acc[stands & ~same][:4])
        inside += int((~stands).sum())
        total += acc.size
        if (~same).any():
            disagree_max = max(disagree_max, float(worst[~same].max()))
        agree_min = min(agree_min, float(worst[same].min()))
        v = rq.exact_value(acc, a, b, c, z).astype(np.float64)
        e = rq.fma32(acc.astype(f32), np.broadcast_to(rq.multiplier(a, b, c), acc.shape), f32(z) - f32(0.5)).astype(np.float64)
        live = (v > -1) & (v < 256)
        bound = max(bound, float(np.abs(v - (e + 0.5))[live].max()))
    print("dense sweep: %d accumulators, %d inside the guard; %d of %d scale sets over their whole range, in windows: %s"
          % (total, inside, len(sets) - len(sampled), len(sets), sampled))
    assert len(sampled) <= 1   # (the set whose range is most of INT32)
    print("largest worst at which estimate and exact byte differ: %.4g (the guard is 2^-13 = %.4g)" % (disagree_max, rq.GUARD))
    print("smallest worst at which they still agree: %.4g" % agree_min)
    print("largest |v - (e + 0.5)| while -1 < v < 256: %.4g (csrc/i8ie_requant.h claims 9.2e-5)" % bound)
    assert disagree_max < rq.GUARD and inside >= 100
    assert bound < 9.2e-5
