"""numpy model of the requantiser's guard (csrc/i8ie_requant.h) and the operand classes that steer a contraction's epilogue
into its replay arm.  A helper module, not a conftest; tests/test_requant_host.py checks it on the CPU and
tests/test_gpu_requant_replay.py drives every replay site with it.

  exact(acc, s_in, s_w, s_out, zp, lo)      the reference's fp32 sequence (pc_pipeline.down_scale_pc) and the relu floor
  estimate(acc, s_in, s_w, s_out, zp, lo)   (byte of the estimate, distance of e to a rounding boundary), as the kernels compute them
  replays(worst, quad_axis)                 which aligned groups of four output features take the replay
  layer_class / matmul_class / attention_class   operands of the classes ALL, MIXED and EXACT-MODE (below)

The classes.  "Real" weights w' are integers in [-3, 3]; column j is quantised with the power-of-two scale
s_w[j] = 2^-t_j 2^-6, qw[j] = w' 2^t_j, t_j = 2 + (j + j/4 + j/16 + j/64) % 4 (per tensor: t_j = 3), the bias is 0, the input
bytes are zp_in + [-3, 3] ([-2, 2] from K = 512 on), s_in = 2^-2, zp_out = 128.  Every fp32 operation of both sequences is then
exact, and with
  ALL         s_out = 2^-8: C ms[j] = sum x w' is an integer, e = C ms + 127.5 sits on a rounding boundary: every value replays,
              and the estimate's own byte (ties to even) is wrong for every odd result;
  MIXED       s_out = 2^-5: C ms[j] = sum x w' / 8, one value in eight sits on a boundary, the others 1/8 or more away (a
              contraction shorter than 64 spreads sum x w' / 8 over fewer than 16 bytes: there s_out = 2^-6, one value in four);
  EXACT-MODE  ALL with s_in = 2^-103, s_out = 2^-109 (normal floats below 1e-30): the host clears `fast`, the bytes are ALL's.
A replay that reads the scale of another column lands on another power of two: all four t occur inside every aligned quad and
their order rotates between neighbouring quads, 16-column and 64-column groups."""
import numpy as np

import pc_pipeline as pcp

f32 = np.float32
GUARD = 2.0 ** -13                      # i8ie_requant_est_ok
FAST_LO, FAST_HI = 1e-30, 1e30          # i8ie_make_requant / i8ie_requant_pc_fast
CLASSES = ("ALL", "MIXED", "EXACT")
ZP_OUT = 128


# ---- the two sequences -------------------------------------------------------------------------------------------------------
def exact(acc, s_in, s_w, s_out, zp, lo=0):
    """The reference's sequence per value (s_w a scalar or one per column of the last axis), then max(., lo)."""
    s_w = np.asarray(s_w, f32)
    out = pcp.down_scale_pc(acc, f32(s_in), s_w, f32(s_out), zp)
    return np.maximum(out, np.uint8(lo))


def exact_value(acc, s_in, s_w, s_out, zp):
    """v of the same sequence, the fp32 value that the reference truncates and clamps"""
    deq = (np.asarray(acc, np.int32).astype(f32) * f32(s_in)) * np.asarray(s_w, f32)
    return (deq / f32(s_out) + f32(zp)).astype(f32)


def multiplier(s_in, s_w, s_out):
    """ms as the host computes it: the double product and quotient, rounded to float once"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (np.float64(f32(s_in)) * np.asarray(s_w, f32).astype(np.float64) / np.float64(f32(s_out))).astype(f32)


def fast(s_in, s_w, s_out):
    """whether the host lets the layer use the estimate at all (a zero column scale is allowed per channel)"""
    s_w = np.atleast_1d(np.asarray(s_w, f32))
    ms = multiplier(s_in, s_w, s_out).astype(np.float64)
    ok = lambda v: bool(np.all((v > FAST_LO) & (v < FAST_HI)))  # noqa: E731
    nz = s_w != 0 if s_w.size > 1 else np.ones(1, bool)
    return ok(np.float64(f32(s_in))) and ok(np.float64(f32(s_out))) and ok(s_w[nz].astype(np.float64)) and ok(ms[nz])


def fma32(a, b, c):
    """One correctly rounded fp32 fma of fp32 operands.  a b is exact in float64 (24 + 24 bits).  The sum p + c is formed in
    float64 with its rounding error (TwoSum, exact) and brought to round-to-odd: where the sum is inexact and its float64
    significand is even, the neighbour on the side of the error, whose significand is odd, is taken instead.  A round-to-odd
    value of 53 bits rounds to nearest-even at 24 bits exactly as the unrounded sum does (53 >= 24 + 2), so no double rounding
    occurs in the final conversion."""
    p = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, f32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(f32)


def fract32(e):
    """v_fract_f32: e - floor(e) in fp32, never 1.0 (the hardware returns the float below 1 there)"""
    e = np.asarray(e, f32)
    return np.minimum((e - np.floor(e)).astype(f32), np.nextafter(f32(1), f32(0)))


def estimate(acc, s_in, s_w, s_out, zp, lo=0):
    """(bytes, worst): byte = sat_u8(rne(max(e, lo))) with e = fma((float)C, ms, zp - 0.5), worst = |fract(e) - 0.5| per value"""
    cf = np.asarray(acc, np.int32).astype(f32)
    e = fma32(cf, np.broadcast_to(multiplier(s_in, s_w, s_out), cf.shape), f32(zp) - f32(0.5))
    worst = np.abs(fract32(e) - f32(0.5)).astype(f32)
    byte = np.clip(np.rint(np.maximum(e, f32(lo)).astype(np.float64)), 0, 255).astype(np.uint8)
    return byte, worst


def replays(worst, quad_axis=-1):
    """bool per aligned group of four consecutive output features along quad_axis (a ragged last group counts what it has):
    the group holds a value closer than 2^-13 to a rounding boundary"""
    w = np.moveaxis(np.asarray(worst, f32), quad_axis, -1)
    n = w.shape[-1]
    pad = (-n) % 4
    if pad:
        w = np.concatenate([w, np.ones(w.shape[:-1] + (pad,), f32)], axis=-1)
    return np.moveaxis(w.reshape(w.shape[:-1] + ((n + pad) // 4, 4)).min(axis=-1) < f32(GUARD), -1, quad_axis)


def value_replays(worst, quad_axis=-1):
    """replays() spread back over the values"""
    n = np.asarray(worst).shape[quad_axis]
    return np.take(np.repeat(replays(worst, quad_axis), 4, axis=quad_axis), np.arange(n), axis=quad_axis)


# ---- scale sets of the dense sweeps -------------------------------------------------------------------------------------------
# (tests/test_gpu_parity.py and tests/test_gpu_per_channel.py take theirs from here too: one definition)
# (s_in, s_w, s_out, zp_out) that put results on and next to integer boundaries, at both clamps, with huge and tiny ratios
BOUNDARY_COMBOS = [(1.0, 1.0, 1.0, 0), (1.0, 1.0, 1.0, 100), (0.5, 1.0, 0.25, 128), (1.0, 0.5, 4.0, 7),
                   (0.025, 0.0031, 0.11, 0), (0.1, 0.1, 0.01, 255), (3.0, 7.0, 0.001, 3), (1e-3, 1e-3, 10.0, 200),
                   (0.3333333, 0.1428571, 0.0476190, 64), (1.0, 1.0, 3.0, 1), (2.0, 1.0, 1.0, 254), (1.0, 1.0, 256.0, 0)]


def random_combos(rng, count=12):
    """`count` more, drawn from rng"""
    return [(float(a), float(b), float(c), int(z)) for a, b, c, z in
            zip(rng.uniform(0.001, 0.2, count), rng.uniform(0.0005, 0.01, count), rng.uniform(0.005, 0.5, count),
                rng.integers(0, 256, count))]


def sweep_combos():
    """BOUNDARY_COMBOS and 12 seeded random ones, as float32"""
    return [(f32(a), f32(b), f32(c), z) for a, b, c, z in BOUNDARY_COMBOS + random_combos(np.random.default_rng(17))]


def row_scales(n, rng, lo=1.0 / 30):
    """per-feature scales spread log-uniformly over [lo, 1] x 2e-3"""
    return (np.exp(rng.uniform(np.log(lo), 0.0, n)) * 2e-3).astype(f32)


def s_out_for(s_in, s_w, K):
    """an output scale that spreads the requantised values of a contraction of length K over the u8 range"""
    return f32(s_in * float(np.median(s_w)) * np.sqrt(K) * 40.0 / 64.0)


# ---- the classes ---------------------------------------------------------------------------------------------------------------
def column_shifts(n, per_channel):
    j = np.arange(n)
    return 2 + (j + j // 4 + j // 16 + j // 64) % 4 if per_channel else np.full(n, 3)


def mixed_shift(K):
    """MIXED divides the integer results by 2^3, below K = 64 by 2^2 (see the head of this file)"""
    return 3 if K >= 64 else 2


def class_scales(cls, n, per_channel, K, zero_cols=False):
    """dict(s_in, s_wv [n], s_w, s_out, zp_out, t [n]) of a class; zero_cols: s_wv[j] = 0 at j % 16 == 5"""
    assert cls in CLASSES
    t = column_shifts(n, per_channel)
    s_wv = np.ldexp(f32(1), -(t + 6)).astype(f32)
    if zero_cols:
        assert per_channel
        s_wv[5::16] = 0
    s_in = f32(2.0 ** -103 if cls == "EXACT" else 0.25)
    s_out = f32(2.0 ** -109) if cls == "EXACT" else f32(2.0 ** (mixed_shift(K) - 8) if cls == "MIXED" else 2.0 ** -8)
    return dict(s_in=s_in, s_wv=s_wv, s_w=f32(2.0 ** -9), s_out=s_out, zp_out=ZP_OUT, t=t)


def layer_class(cls, q_shape, w_shape, K, zp_in, per_channel, seed, zero_cols=False):
    """Operands of a layer in class `cls`: q u8 `q_shape`, qw s8 `w_shape` (output features first), qb = 0, and class_scales().
    K is the contraction length, which sets the input range."""
    rng = np.random.default_rng(seed)
    r = 2 if K >= 512 else 3
    n = w_shape[0]
    d = class_scales(cls, n, per_channel, K, zero_cols)
    assert r <= zp_in <= 255 - r
    d["q"] = (zp_in + rng.integers(-r, r + 1, q_shape)).astype(np.uint8)
    wr = rng.integers(-3, 4, w_shape)
    d["qw"] = (wr << d["t"].reshape((n,) + (1,) * (len(w_shape) - 1))).astype(np.int8)
    d["qb"] = np.zeros(n, np.int8)
    d["zp_in"], d["x"] = zp_in, None
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def layer_scale(d, per_channel):
    """the weight scale(s) that the layer of layer_class() requantises with"""
    return d["s_wv"] if per_channel else d["s_w"]


def matmul_class(cls, b, m, n, k, seed, zp_a=120, zp_b=131):
    """A [b, m, k], B [b, k, n] with bytes zp +- 4 x, x in [-3, 3]: C = 16 sum x y.  s_a = s_b = 2^-2 and s_out chosen so that
    ms = 2^-4 (ALL, EXACT: C ms = sum x y, an integer) or 2^-4 / 2^mixed_shift(k) (MIXED).  EXACT: s_a = 2^-103, s_out scaled
    alike."""
    rng = np.random.default_rng(seed)
    A = (zp_a + 4 * rng.integers(-3, 4, (b, m, k))).astype(np.uint8)
    B = (zp_b + 4 * rng.integers(-3, 4, (b, k, n))).astype(np.uint8)
    s_a = f32(2.0 ** -103 if cls == "EXACT" else 0.25)
    s_b = f32(0.25)
    ms = 2.0 ** -(4 + (mixed_shift(k) if cls == "MIXED" else 0))
    s_out = f32(float(s_a) * float(s_b) / ms)
    return dict(A=A, B=B, zp_a=zp_a, zp_b=zp_b, s_a=s_a, s_b=s_b, s_out=s_out, zp_out=ZP_OUT)


def attention_class(cls, b, heads, d, tq, tk, seed):
    """Operands of i8ie_attention_u8 whose O epilogue is in class `cls`: every k row holds zp_k, so that every score equals zp_s,
    the softmax is uniform, P = 256 / tk exactly (tk a power of two), and the second product's accumulator is
    (256 / tk) sum_j (v - zp_v) with v = zp_v + [-6, 6].  With the P scale 2^-8, ms = s_v 2^-8 / s_o = g tk / 256, so that
    C ms = g sum_j (v - zp_v): g = max(1, 64 / tk) in ALL and EXACT (an integer; about 80 % of the results stay inside the byte
    range at tk = 64 only with g = 1), g = 2^-mixed_shift(tk) in MIXED.  EXACT: s_v = 2^-103."""
    assert tk & (tk - 1) == 0 and tk <= 256
    rng = np.random.default_rng(seed)
    c = heads * d
    q = rng.integers(0, 256, (b, tq, c), dtype=np.uint8)
    k = np.full((b, tk, c), 131, np.uint8)
    v = (125 + rng.integers(-6, 7, (b, tk, c))).astype(np.uint8)
    s_v = f32(2.0 ** -103 if cls == "EXACT" else 0.25)
    g = 2.0 ** -mixed_shift(tk) if cls == "MIXED" else max(1.0, 64.0 / tk)
    ms = g * tk / 256.0
    s_o = f32(float(s_v) * 2.0 ** -8 / ms)
    qp = dict(s_q=f32(0.25), zp_q=120, s_k=f32(0.25), zp_k=131, s_v=s_v, zp_v=125, s_s=f32(0.03), zp_s=140, s_o=s_o, zp_o=ZP_OUT)
    return q, k, v, qp


def scores_class(cls, b, heads, d, tq, tk, seed):
    """Operands of i8ie_attention_u8 whose S epilogue (lo = 0, plain pack) is in class `cls`: q and k as matmul_class builds its
    operands (k = d), v is random.  EXACT: s_q = 2^-103."""
    rng = np.random.default_rng(seed)
    c = heads * d
    q = (120 + 4 * rng.integers(-3, 4, (b, tq, c))).astype(np.uint8)
    k = (131 + 4 * rng.integers(-3, 4, (b, tk, c))).astype(np.uint8)
    v = rng.integers(0, 256, (b, tk, c), dtype=np.uint8)
    s_q = f32(2.0 ** -103 if cls == "EXACT" else 0.25)
    ms = 2.0 ** -(4 + (mixed_shift(d) if cls == "MIXED" else 0))
    s_s = f32(float(s_q) * 0.25 / ms)
    qp = dict(s_q=s_q, zp_q=120, s_k=f32(0.25), zp_k=131, s_v=f32(0.04), zp_v=125, s_s=s_s, zp_s=ZP_OUT, s_o=f32(0.01), zp_o=128)
    return q, k, v, qp


# ---- what a class guarantees ---------------------------------------------------------------------------------------------------
def class_report(cls, acc, s_in, s_w, s_out, zp_out, relu, quad_axis=-1):
    """The shares the class conditions speak of, from reference accumulators (features on quad_axis)."""
    want = exact(acc, s_in, s_w, s_out, zp_out)
    est, worst = estimate(acc, s_in, s_w, s_out, zp_out, zp_out if relu else 0)
    rep = replays(worst, quad_axis)
    stands = ~value_replays(worst, quad_axis)
    floored = np.maximum(want, np.uint8(zp_out)) if relu else want
    return dict(cls=cls, quads=float(rep.mean()), inside=float(((want > 0) & (want < 255)).mean()),
                distinct=int(len(np.unique(want))), below=float((want < zp_out).mean()),
                est_ok=bool(np.array_equal(est[stands], floored[stands])), fast=fast(s_in, s_w, s_out))


def check_class(rep, relu):
    """The class conditions (conditions on the inputs, asserted before any GPU result is looked at)."""
    cls = rep["cls"]
    if cls in ("ALL", "EXACT"):
        assert rep["quads"] == 1.0, rep
    else:
        assert 0.25 <= rep["quads"] <= 0.75, rep
    assert rep["fast"] == (cls != "EXACT"), rep
    assert rep["inside"] >= 0.8 and rep["distinct"] >= 16, rep
    assert not relu or rep["below"] >= 0.1, rep
    assert rep["est_ok"], rep
