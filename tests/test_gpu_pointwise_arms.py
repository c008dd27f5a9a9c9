"""The item-width arms of the bordered NHWC pointwise entries (i8ie_add_u8_nhwc, i8ie_mul_u8_nhwc in both forms,
i8ie_lut_u8_nhwc) that are chosen by the buffers' ALIGNMENT and not by c: 4-byte items at c % 16 == 0 with buffers that are
only 4-byte aligned, 1-byte items at c % 4 == 0 with buffers that are only byte aligned.  The other tests hand these entries
64-byte aligned pointers and reach the narrower arms through c alone.  Here every base pointer lies 0, 4 or 1 bytes past a
64-byte aligned address, all buffers alike and the result alone.  Byte-exact against the numpy restatements (add_ref.add_u8,
mul_ref.mul_u8, the table itself), never against the code under test, with the guard-byte and border-ring assertions of the
test_bordered_nhwc tests.  Also: parameters at which every dword replays the exact sequence, and a denormal scale (the
estimate is off), both through the bordered entry.

The 64-bit-index instantiations of these kernels need more than 2^31 items: no small test reaches them."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import act_ref
import add_ref
import mul_ref
import pointwise_util as pu
import support

pytestmark = pytest.mark.gpu
f32 = np.float32

N, H, W = 2, 3, 5
CHANNELS = [16, 20, 3]  # 16-, 4- and 1-byte items at aligned buffers
# (a, b, out) misalignment: all buffers alike, and the result alone
SKEWS = [(0, 0, 0), (4, 4, 4), (1, 1, 1), (0, 0, 4), (0, 0, 1)]
ADD_QP = (f32(0.043), 119, f32(0.027), 131, f32(0.061), 97)
OPS = ["add", "mul", "gate"]


ctx = support.ctx_fixture(add_ref, mul_ref, act_ref)


def _at(dev, skew):
    return C.c_void_p(dev.ptr.value + pu.GUARD + skew)


def _nchw(x):
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _want(op, a, b, qp, relu):
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    if op == "add":
        return add_ref.add_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu)
    return support.nhwc(mul_ref.mul_u8(_nchw(a), zp_a, s_a, b if op == "gate" else _nchw(b), zp_b, s_b, s_out, zp_out, relu))


def _run(ctx, op, a, b, borders, flags, skews, qp, relu):
    """a: [n, h, w, c]; b: the same shape, or the gate [n, c] (op == "gate").  Returns the result's interior after checking
    that the operands, every guard byte and the result's border ring are untouched."""
    s_a, zp_a, s_b, zp_b, s_out, zp_out = qp
    n, h, w, c = a.shape
    (ba, bb, bo), (a_s8, b_s8, o_s8), (ka, kb, ko) = borders, flags, skews
    fa, _ = pu.phys(a, ba, zp_a, a_s8, ka)
    fb, _ = pu.phys(b.reshape(n, 1, 1, c) if op == "gate" else b, bb, zp_b, b_s8, kb)
    fo, oshape = pu.phys(np.zeros_like(a) + np.uint8(0xEE), bo, zp_out, o_s8, ko)  # the border as i8ie_fill_border_u8 leaves it
    da, db, do = ctx.put(fa), ctx.put(fb), ctx.put(fo)
    try:
        assert all(d.ptr.value % 64 == 0 for d in (da, db, do))
        q = (float(s_a), int(zp_a), float(s_b), int(zp_b), float(s_out), int(zp_out), 1 if relu else 0)
        if op == "add":
            abi.ck(abi.lib().i8ie_add_u8_nhwc(ctx.h, _at(da, ka), ba, a_s8, _at(db, kb), bb, b_s8, _at(do, ko), bo, o_s8, n, c, h, w, *q))
        else:
            abi.ck(abi.lib().i8ie_mul_u8_nhwc(ctx.h, _at(da, ka), ba, a_s8, _at(db, kb), bb, b_s8, 1 if op == "gate" else 0, _at(do, ko),
                                              bo, o_s8, n, c, h, w, *q))
        ga, gb, go = da.get(), db.get(), do.get()
    finally:
        for d in (da, db, do):
            d.free()
    assert np.array_equal(ga, fa) and np.array_equal(gb, fb), "operands (and their guards) must be untouched"
    return pu.interior(go, oshape, bo, zp_out, o_s8, ko)


def _operands(op, c, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (N, H, W, c), dtype=np.uint8)
    b = rng.integers(0, 256, (N, c) if op == "gate" else (N, H, W, c), dtype=np.uint8)
    return a, b


def _qp(op):
    return {"add": ADD_QP, "mul": dict(mul_ref.QP)["k128_zp_3_250_17"], "gate": dict(mul_ref.QP)["gate_zp100"]}[op]


@pytest.mark.parametrize("skews", SKEWS, ids=lambda k: "skew%d%d%d" % k)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("op", OPS)
def test_two_operand_arms(ctx, op, c, skews):
    a, b = _operands(op, c, c * 10 + sum(skews))
    qp = _qp(op)
    for i, flags in enumerate(itertools.product((0, 1), repeat=3)):
        relu = bool((i + c) % 2)
        got = _run(ctx, op, a, b, (1, 0, 1), flags, skews, qp, relu)
        assert np.array_equal(got, _want(op, a, b, qp, relu)), (flags, relu)


@pytest.mark.parametrize("skews", SKEWS, ids=lambda k: "skew%d%d%d" % k)
@pytest.mark.parametrize("c", CHANNELS)
def test_lut_arms(ctx, c, skews):
    rng = np.random.default_rng(c * 10 + sum(skews))
    q = rng.integers(0, 256, (N, H, W, c), dtype=np.uint8)
    zp_out = 13
    tab = act_ref.table("hardswish", 0.0, f32(0.04), 120, f32(0.031), zp_out)
    ki, _, ko = skews
    for i, (in_s8, out_s8) in enumerate(itertools.product((0, 1), repeat=2)):
        t = act_ref.with_relu(tab, zp_out) if (i + c) % 2 else tab  # a following relu is folded into the table
        ptr, keep = act_ref.host_table(t)
        for ib, ob in ((1, 1), (0, 1)):
            fi, _ = pu.phys(q, ib, 0x11, in_s8, ki)
            fo, oshape = pu.phys(np.zeros_like(q) + np.uint8(0xEE), ob, zp_out, out_s8, ko)
            di, do = ctx.put(fi), ctx.put(fo)
            try:
                abi.ck(abi.lib().i8ie_lut_u8_nhwc(ctx.h, _at(di, ki), ib, in_s8, _at(do, ko), ob, out_s8, N, c, H, W, ptr))
                gi, go = di.get(), do.get()
            finally:
                di.free()
                do.free()
            assert np.array_equal(gi, fi), "the input (and its guards) must be untouched"
            got = pu.interior(go, oshape, ob, zp_out, out_s8, ko)
            assert np.array_equal(got, t[q]), (in_s8, out_s8, ib, ob)
        del keep


# s_a = s_b = s_out with equal zero points.  The sum is then (a - zp) + (b - zp) + zp, an integer, at either scale; the
# product is an integer at scale 1.  An integer t makes the estimate t - 0.5, on a rounding boundary: every dword replays.
@pytest.mark.parametrize("scale", [0.05, 1.0])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("op", OPS)
def test_every_dword_replays(ctx, op, c, scale):
    a, b = _operands(op, c, 7 + c)
    qp = (f32(scale), 128, f32(scale), 128, f32(scale), 128)
    for relu, flags in ((False, (0, 0, 0)), (True, (1, 0, 1))):
        got = _run(ctx, op, a, b, (1, 0, 1), flags, (0, 0, 0), qp, relu)
        assert np.array_equal(got, _want(op, a, b, qp, relu)), (flags, relu)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("op", OPS)
def test_denormal_scale_takes_the_exact_sequence(ctx, op, c):
    a, b = _operands(op, c, 11 + c)
    qp = (f32(1e-40), 128, f32(0.03), 128, f32(0.03), 100)  # the estimate is not used: fast == 0
    for relu, flags in ((False, (0, 1, 0)), (True, (1, 0, 1))):
        got = _run(ctx, op, a, b, (1, 0, 1), flags, (0, 0, 0), qp, relu)
        assert np.array_equal(got, _want(op, a, b, qp, relu)), (flags, relu)
