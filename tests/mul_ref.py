"""The quantized broadcast Mul restated for the tests.  A helper module, not a conftest.

The reference has no multiply; the definition is a composition of its own dequantize (src/quantize_utils.cc:38-42) and
down_scale's clamp / truncation (src/quantize_utils.cc:27-36) in IEEE fp32, one rounding per operation.  mul_u8 spells it in
numpy with an explicit float32 cast between the steps (a gate broadcasts as numpy broadcasts [n, c, 1, 1]), QP is the list of
quantisation parameter sets the exhaustive tests run over, tracer() and nontrivial() are what the network tests look at in
a spec_ref.forward (gate bytes, the floor of a relu behind a Mul), and the three new C symbols get their ctypes signatures
here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

import orc

f32 = np.float32

# the launch constants of csrc/i8ie_binary.hip: threads per block, the grid cap, pixels a lane of the gate kernel walks
THREADS, MAX_BLOCKS, WALK = 256, 256 * 8, 8


def as_gate(a, b):
    """b as numpy broadcasts it against a: a's shape, or a gate [n, c] / [n, c, 1, 1] of an [n, c, h, w] a"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape == b.shape:
        return b
    assert a.ndim == 4 and b.shape[:2] == a.shape[:2] and b.size == a.shape[0] * a.shape[1], (a.shape, b.shape)
    return b.reshape(a.shape[0], a.shape[1], 1, 1)


def mul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu=False):
    """u8 arrays -> u8 of a's shape.  Every step is one fp32 operation on float32 arrays (nothing is evaluated in double)."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    b = as_gate(a, b)
    with np.errstate(all="ignore"):
        da = (a.astype(np.int32) - np.int32(zp_a)).astype(f32)
        db = (b.astype(np.int32) - np.int32(zp_b)).astype(f32)
        fa = (da * f32(s_a)).astype(f32)
        fb = (db * f32(s_b)).astype(f32)
        p = (fa * fb).astype(f32)
        q = (p / f32(s_out)).astype(f32)
        t = (q + f32(zp_out)).astype(f32)
        inside = np.where((t >= f32(0)) & (t < f32(255)), t, f32(0))
        out = np.where(t >= f32(255), 255, np.where(t < f32(0), 0, np.trunc(inside).astype(np.int32))).astype(np.uint8)
    if relu:
        out = np.maximum(out, np.uint8(zp_out))
    return out


def _qparam_sets():
    """(name, (s_a, zp_a, s_b, zp_b, s_out, zp_out)).  With k = s_a * s_b / s_out the result is (a - zp_a)(b - zp_b) k + zp_out:
    k near 1 / 128 keeps most pairs inside [0, 255], a larger k saturates."""
    sets = []
    # the gate sets: b is a hardsigmoid's output in [0, 1] (scale 1 / 255, zero point 0) and the result keeps a's parameters
    for s, zp in ((0.05, 128), (0.02, 100), (0.11, 64), (0.007, 160), (0.3, 200)):
        sets.append(("gate_zp%d" % zp, (f32(s), zp, f32(1.0 / 255), 0, f32(s), zp)))
    sa, sb = f32(0.05), f32(0.02)
    so = f32(sa * sb * f32(128))
    for zps in ((128, 128, 128), (3, 250, 17), (0, 0, 0), (255, 255, 255), (0, 255, 128), (128, 0, 255), (255, 128, 0)):
        sets.append(("k128_zp_%d_%d_%d" % zps, (sa, zps[0], sb, zps[1], so, zps[2])))
    sets.append(("thirds", (f32(0.02), 120, f32(0.03), 131, f32(3 * 0.02 * 0.03 * 64), 64)))
    # powers of two: every product and quotient is exact, and many results sit exactly on an integer (the guard's replay)
    sets.append(("pow2_k64", (f32(2.0 ** -4), 128, f32(2.0 ** -3), 128, f32(2.0 ** -1), 128)))
    sets.append(("pow2_k256", (f32(2.0 ** -6), 100, f32(2.0 ** -7), 7, f32(2.0 ** -5), 30)))
    sets.append(("pow2_k1", (f32(0.25), 127, f32(0.5), 129, f32(0.125), 128)))
    so = f32(0.064)
    sets.append(("ratio_1_64_and_64", (so / f32(64), 7, so * f32(64), 128, f32(so * so * f32(100)), 128)))
    sets.append(("ratio_64_and_1_64", (so * f32(64), 130, so / f32(64), 200, f32(so * so * f32(100)), 9)))
    s = f32(0.05)
    sets.append(("equal_saturating", (s, 128, s, 128, s, 128)))
    rng = np.random.default_rng(20261018)
    for i in range(6):  # calibrated-looking: a range / 255 and a zero point from it
        sa, sb = (f32(v) for v in rng.uniform(0.004, 0.2, 2))
        so = f32(sa * sb * f32(rng.uniform(30, 300)))
        za, zb, zo = (int(v) for v in rng.integers(0, 256, 3))
        sets.append(("calibrated_%d" % i, (sa, za, sb, zb, so, zo)))
    sets.append(("zero_s_a", (f32(0.0), 128, f32(0.03), 100, f32(0.03), 77)))       # every product is +-0
    sets.append(("zero_s_b", (f32(0.04), 3, f32(0.0), 255, f32(0.5), 255)))
    sets.append(("negative_s_b", (f32(0.05), 128, f32(-0.02), 128, f32(0.128), 128)))
    sets.append(("denormal_s_a", (f32(1e-40), 128, f32(0.03), 128, f32(0.03), 100)))
    sets.append(("denormal_products", (f32(1e-20), 128, f32(1e-21), 128, f32(1e-40), 128)))  # P and s_out denormal, k = 0.1
    sets.append(("tiny_times_huge", (f32(1e-20), 128, f32(1e20), 128, f32(128.0), 128)))
    sets.append(("overflowing_products", (f32(1e25), 128, f32(1e12), 128, f32(1.0), 128)))   # P = +-inf or +-0
    sets.append(("huge_s_out", (f32(0.05), 128, f32(0.02), 128, f32(1e30), 200)))
    return sets


QP = _qparam_sets()
GATE_SETS = [n for n, _ in QP if n.startswith("gate_")]


def relu_follows(spec):
    """the attrs of the muls of a spec (branches included) that a relu follows directly"""
    out = set()

    def walk(ops):
        for i, op in enumerate(ops):
            if op[0] == "branch":
                walk(op[2])
            elif op[0] == "mul" and i + 1 < len(ops) and ops[i + 1][0] == "relu":
                out.add(op[1])

    walk(spec)
    return out


def tracer(spec, into):
    """a trace callback for spec_ref.forward: into[attr] = (gate bytes or None, output bytes with a directly following relu
    applied, the relu's floor or None) of every Mul of the spec"""
    floors = relu_follows(spec)

    def trace(op, out, operands):
        if op[0] == "mul":
            q, _, zp = out
            q2 = operands[1][0]
            floor = zp if op[1] in floors else None
            into[op[1]] = (q2 if q2.shape != q.shape else None, q if floor is None else orc.relu(q, zp), floor)

    return trace


# with the seeds of tests/spec_ref.py every gate of the oracle's se_tiny forward takes at least MIN_GATE_VALUES byte values and
# no Mul output has more than MAX_EDGE_SHARE of its bytes on 0, 255 or the floor of a relu behind it (tests/test_mul_host.py)
MIN_GATE_VALUES, MAX_EDGE_SHARE = 8, 0.6


def nontrivial(trace):
    """{attr: (distinct gate byte values or None, share of output bytes on 0 / 255 / the relu floor)} of a tracer()'s dict,
    asserted against the two limits"""
    out = {}
    for attr, (gate, q, floor) in trace.items():
        q = np.asarray(q, np.uint8)
        edge = (q == 0) | (q == 255)
        if floor is not None:
            edge |= q == floor
        out[attr] = (None if gate is None else int(np.unique(gate).size), float(edge.mean()))
        assert out[attr][0] is None or out[attr][0] >= MIN_GATE_VALUES, (attr, out[attr])
        assert out[attr][1] <= MAX_EDGE_SHARE, (attr, out[attr])
    return out


# ---- ctypes signatures of the mul entry points ---------------------------------------------------------------------
_P, _I, _F, _B, _L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64


def bind(lib):
    lib.i8ie_mul_u8.argtypes = [_P, _P, _P, _P, _L, _F, _B, _F, _B, _F, _B, _I]
    lib.i8ie_mul_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _F, _B, _F, _B, _F, _B, _I]
    lib.i8ie_mul_f32.argtypes = [_P, _P, _P, _P, _L, _L]
    for f in (lib.i8ie_mul_u8, lib.i8ie_mul_u8_nhwc, lib.i8ie_mul_f32):
        f.restype = _I
    return lib
