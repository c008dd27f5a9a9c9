"""The fused multi-head attention on the GPU (csrc/i8ie_attention.hip).  Every comparison is bit for bit
against the numpy composition of the definition (tests/mha_ref.py over tests/attention_ref.py), never against the code under
test; the scores S, the probabilities P, the second product's accumulators and the result O are each checked through the
debug outputs, so a failure names its phase."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import attention_ref as ar
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import mha_ref as mr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL = 0xC3


ctx = support.ctx_fixture(mr)


def qp_for(d, zp=(120, 131, 125, 140, 128), s_s=0.03):
    """quantisation parameters that spread the scores of random bytes over the byte range (accumulator std ~ 5476 sqrt(d) ->
    ~40 score steps) and keep the softmax input scale where many table entries matter"""
    s = f32(np.sqrt(s_s * 40.0 / (5476.0 * np.sqrt(d))))
    return dict(s_q=s, zp_q=zp[0], s_k=s, zp_k=zp[1], s_v=f32(0.04), zp_v=zp[2], s_s=f32(s_s), zp_s=zp[3], s_o=f32(0.01), zp_o=zp[4])


def run(ctx, q, k, v, heads, qp, relu=False, s8=(False, False, False), o_s8=False, fallback=False, offsets=(0, 0, 0), packed=False,
        same_qk=False, border=None, hw=None, out_stride=None):
    """The u8 entry on host arrays q [b, tq, c], k, v [b, tk, c], laid out as asked: each operand re-biased or not and at a
    byte offset inside its allocation; packed: one [b, t, 3c] buffer; same_qk: k is q's buffer; the result plain with token
    stride out_stride (default c) or the interior of a bordered map (border, hw = (h, w)), re-biased or not.  Every output lives
    in a guarded region.  Returns (S, P, acc, O as plain bytes [b, tq, c], kernel names)."""
    b, tq, c = q.shape
    tk = k.shape[1]
    d = c // heads
    x = [np.uint8(0x80) if f else np.uint8(0) for f in s8]
    bufs = []
    if packed:
        host = np.concatenate([q ^ x[0], k ^ x[1], v ^ x[2]], axis=2)
        dev = ctx.put(np.concatenate([np.zeros(offsets[0], np.uint8), host.ravel()]))
        bufs.append(dev)
        mats = [mr.AttnMat(dev.ptr.value + offsets[0] + i * c, tq * 3 * c, 3 * c, 1 if s8[i] else 0) for i in range(3)]
    else:
        mats = []
        for i, a in enumerate((q, k, v)):
            if same_qk and i == 1:
                mats.append(mr.AttnMat(mats[0].ptr, mats[0].batch_stride, mats[0].token_stride, mats[0].s8))
                continue
            dev = ctx.put(np.concatenate([np.zeros(offsets[i], np.uint8), (a ^ x[i]).ravel()]))
            bufs.append(dev)
            mats.append(mr.mat(dev.ptr.value, a.shape[1], c, s8[i], offsets[i]))
    g = mr.AttnArgs(b=b, heads=heads, d=d, tq=tq, tk=tk, q=mats[0], k=mats[1], v=mats[2], relu=1 if relu else 0, **qp)
    if border is None:
        ots = c if out_stride is None else out_stride
        do = abi.GuardedU8(ctx, (b, tq, ots), fill=FILL)
        g.out = mr.AttnMat(do.ptr.value, tq * ots, ots, 1 if o_s8 else 0)
    else:
        h, w = hw
        do = abi.GuardedU8(ctx, (b, h + 2 * border, w + 2 * border, c), fill=FILL)
        g.out = mr.AttnMat(do.ptr.value, (h + 2 * border) * (w + 2 * border) * c, c, 1 if o_s8 else 0)
        g.out_h, g.out_w, g.out_border = h, w, border
    ds = abi.GuardedU8(ctx, (b, heads, tq, tk))
    dp = abi.GuardedU8(ctx, (b, heads, tq, tk))
    dacc = abi.GuardedU8(ctx, (b, tq, c), np.int32)
    g.scores_dbg_dev, g.probs_dbg_dev, g.acc_dbg_dev = ds.ptr.value, dp.ptr.value, dacc.ptr.value
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_attention_u8(ctx.h, C.byref(g)))
    finally:
        ctx.set_force_fallback(False)
    raw, S, P, acc = do.get(), ds.get(), dp.get(), dacc.get()
    assert do.guards_ok() and ds.guards_ok() and dp.guards_ok() and dacc.guards_ok()
    if border is None:
        O = raw[:, :, :c]
        assert (raw[:, :, c:] == FILL).all(), "the gap of a token stride above c was written"
    else:
        h, w = hw
        ring = raw.copy()
        ring[:, border:border + h, border:border + w, :] = FILL
        assert (ring == FILL).all(), "a border byte was written"
        O = raw[:, border:border + h, border:border + w, :].reshape(b, tq, c)
    O = O ^ np.uint8(0x80) if o_s8 else O
    for dv in bufs + [do, ds, dp, dacc]:
        dv.free()
    return S, P, acc, np.ascontiguousarray(O), names


def check(ctx, q, k, v, heads, qp, kernel, want=None, **kw):
    if want is None:
        want = mr.attention_u8(q, k, v, heads, relu=kw.get("relu", False), **qp)
    S, P, acc, O, names = run(ctx, q, k, v, heads, qp, **kw)
    tag = (q.shape, k.shape[1], heads, kernel, {a: b for a, b in kw.items() if a != "want"})
    assert names == {kernel: 1}, (names, tag)
    for name, got, exp in zip(("S", "P", "acc", "O"), (S, P, acc, O), want):
        assert np.array_equal(got, exp), (name, tag, np.argwhere(got != exp)[:4])
    return want


# ---- 1, 3: the grid, in attn_mfma and again under force-fallback ------------------------------------------------------------
TQS, TKS = [1, 16, 63, 64, 65, 130], [1, 15, 16, 64, 65, 200]


@pytest.mark.parametrize("d", [16, 32, 64, 80, 128])
def test_grid_mfma_and_forced_direct(ctx, d):
    """every Tq and every Tk of the lists with this d, b in {1, 3}, H in {1, 2, 3}; the re-bias flags and the relu cycle with the
    case index; the same case again under I8IE_OPT_FORCE_FALLBACK gives the same bytes"""
    rng = np.random.default_rng(d)
    spread = 0
    for i in range(6):
        b, heads, tq, tk = (1, 3)[i % 2], (1, 2, 3)[i % 3], TQS[i], TKS[(i + d // 16) % 6]
        q, k, v = support.rand_qkv(rng, b, tq, tk, heads * d)
        kw = dict(relu=bool(i & 1), s8=(bool(i & 1), bool(i & 2), bool(i & 4)), o_s8=bool(i & 2))
        want = check(ctx, q, k, v, heads, qp_for(d), "attn_mfma", **kw)
        check(ctx, q, k, v, heads, qp_for(d), "attn_direct", want=want, fallback=True, **kw)
        spread = max(spread, len(np.unique(want[3])))
        assert len(np.unique(want[0])) > min(50, tq * tk // 2)
    assert spread > 30   # the expected bytes discriminate


def test_every_tq_meets_every_tk(ctx):
    """the full Tq x Tk product at d = 16, H = 2, b = 1 (the tail rules do not depend on d)"""
    rng = np.random.default_rng(77)
    for tq, tk in itertools.product(TQS, TKS):
        q, k, v = support.rand_qkv(rng, 1, tq, tk, 32)
        check(ctx, q, k, v, 2, qp_for(16), "attn_mfma")


# ---- 2: the LDS limit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tk,kernel", [(1024, "attn_mfma"), (1025, "attn_direct")])
def test_lds_limit(ctx, tk, kernel):
    rng = np.random.default_rng(tk)
    q, k, v = support.rand_qkv(rng, 1, 65, tk, 64)
    check(ctx, q, k, v, 1, qp_for(64), kernel, relu=True)


# ---- 3: attn_direct ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 12, 17])
def test_direct_head_widths(ctx, d):
    rng = np.random.default_rng(300 + d)
    for b, heads, tq, tk in ((1, 1, 1, 1), (3, 2, 17, 33), (2, 3, 65, 70)):
        q, k, v = support.rand_qkv(rng, b, tq, tk, heads * d)
        check(ctx, q, k, v, heads, qp_for(d), "attn_direct", s8=(True, False, True), relu=bool(d & 1))


def test_direct_unaligned_pointers_and_long_rows(ctx):
    rng = np.random.default_rng(310)
    q, k, v = support.rand_qkv(rng, 2, 17, 40, 32)
    want = check(ctx, q, k, v, 2, qp_for(16), "attn_mfma")
    for offsets in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        check(ctx, q, k, v, 2, qp_for(16), "attn_direct", want=want, offsets=offsets)
    q, k, v = support.rand_qkv(rng, 1, 5, 3000, 32)
    check(ctx, q, k, v, 2, qp_for(16), "attn_direct", o_s8=True)


# ---- 4: quantisation extremes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_zero_points_and_byte_extremes(ctx, fallback):
    kernel = "attn_direct" if fallback else "attn_mfma"
    rng = np.random.default_rng(40)
    b, heads, d, tq, tk = 2, 2, 16, 20, 200
    q, k, v = support.rand_qkv(rng, b, tq, tk, heads * d)
    # every value on each of zp_q, zp_k, zp_v, zp_s, zp_o with the others central, then all at one extreme and mixed
    cases = [(128,) * 5] + [tuple(z if j == i else 128 for j in range(5)) for i in range(5) for z in (0, 255)]
    cases += [(0,) * 5, (255,) * 5, (0, 255, 0, 255, 0), (255, 0, 255, 0, 255), (0, 0, 255, 128, 255)]
    for i, zps in enumerate(cases):
        check(ctx, q, k, v, heads, qp_for(d, zp=zps), kernel, fallback=fallback, relu=bool(i & 1))
    alt = np.where(np.arange(heads * d) % 2 == 0, 0, 255).astype(np.uint8)
    for fill in (0, 255, "alt"):
        a = [np.broadcast_to(alt, x.shape).copy() if fill == "alt" else np.full_like(x, fill) for x in (q, k, v)]
        for zps in ((0, 0, 0, 0, 0), (255, 255, 255, 255, 255), (128, 3, 250, 77, 9)):
            want = check(ctx, a[0], a[1], a[2], heads, qp_for(d, zp=zps), kernel, fallback=fallback)
            assert (want[0] == want[0][0, 0, 0, 0]).all()              # a constant score row: the uniform softmax at Tk = 200
            assert (want[1] == 1).all()                                 # 256 / 200 rounds to 1
    # one dominant column: k row 7 equals the direction of q, every other k row is the zero point -> probability clamps at 255
    qd = np.full((1, 4, 16), 200, np.uint8)
    kd = np.full((1, 200, 16), 128, np.uint8)
    kd[0, 7] = 255
    vd = rng.integers(0, 256, (1, 200, 16), dtype=np.uint8)
    qp = dict(qp_for(16, zp=(128, 128, 100, 10, 128), s_s=1.0))
    want = check(ctx, qd, kd, vd, 1, qp, kernel, fallback=fallback)
    assert (want[1][0, 0, :, 7] == 255).all() and (np.delete(want[1][0, 0], 7, axis=1) == 0).all()
    # Tk = 1: every probability is 255
    q1, k1, v1 = support.rand_qkv(rng, 2, 33, 1, 32)
    want = check(ctx, q1, k1, v1, 2, qp_for(16), kernel, fallback=fallback, relu=True)
    assert (want[1] == 255).all()
    # scales that saturate the scores at both ends
    hot = dict(qp_for(d), s_q=f32(0.5), s_k=f32(0.5), s_s=f32(0.01))
    want = check(ctx, q, k, v, heads, hot, kernel, fallback=fallback)
    assert (want[0] == 0).any() and (want[0] == 255).any() and ((want[0] == 0) | (want[0] == 255)).mean() > 0.9


# ---- 5: layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_operand_and_result_layouts(ctx, fallback):
    kernel = "attn_direct" if fallback else "attn_mfma"
    rng = np.random.default_rng(50)
    b, heads, d, h, w = 2, 2, 16, 5, 7
    t, c = h * w, heads * d
    q, k, v = support.rand_qkv(rng, b, t, t, c)
    qp = qp_for(d)
    want = mr.attention_u8(q, k, v, heads, **qp)
    for s8 in itertools.product([False, True], repeat=3):
        check(ctx, q, k, v, heads, qp, kernel, want=want, fallback=fallback, s8=s8)
        check(ctx, q, k, v, heads, qp, kernel, want=want, fallback=fallback, s8=s8, packed=True)   # token stride 3c
    # q and k as the same buffer
    same = dict(qp, s_k=qp["s_q"], zp_k=qp["zp_q"])
    check(ctx, q, q, v, heads, same, kernel, fallback=fallback, same_qk=True, s8=(True, True, False))
    # the bordered result, re-biased or not, with the relu folded
    wr = mr.attention_u8(q, k, v, heads, relu=True, **qp)
    for border, o_s8 in itertools.product([1, 2], [False, True]):
        check(ctx, q, k, v, heads, qp, kernel, want=wr, fallback=fallback, relu=True, border=border, hw=(h, w), o_s8=o_s8)
    # a plain result with a token stride above c (aligned and not)
    for ots in (c + 16, c + 5):
        check(ctx, q, k, v, heads, qp, kernel, want=want, fallback=fallback, out_stride=ots)


# ---- 6: the FP32 entry ------------------------------------------------------------------------------------------------------
def test_f32_entry_is_the_composition_bit_for_bit(ctx):
    rng = np.random.default_rng(60)
    b, heads, d, tq, tk = 3, 2, 20, 5, 7
    c = heads * d
    q, k, v = (rng.normal(0, 1, (b, t, c)).astype(f32) for t in (tq, tk, tk))
    dq, dk, dv = ctx.put(q), ctx.put(k), ctx.put(v)
    do, dsc = ctx.guarded((b, tq, c)), ctx.guarded((b, heads, tq, tk))
    g = mr.AttnArgs(b=b, heads=heads, d=d, tq=tq, tk=tk, q=mr.mat(dq.ptr.value, tq, c), k=mr.mat(dk.ptr.value, tk, c),
                    v=mr.mat(dv.ptr.value, tk, c), out=mr.mat(do.ptr.value, tq, c), scores_out_dev=dsc.ptr.value)
    abi.ck(abi.lib().i8ie_attention_f32(ctx.h, C.byref(g)))
    got, ok1 = do.read()
    got_s, ok2 = dsc.read()
    assert ok1 and ok2 and abi.GuardedOut.unwritten(got) == 0 and abi.GuardedOut.unwritten(got_s) == 0
    # the composition, per head, on the same buffers through pointer offsets (elements are 4 bytes)
    ws, wo = ctx.empty((b, tq, tk), f32), ctx.guarded((b, tq, c))
    for hd in range(heads):
        off = 4 * hd * d
        s = ar.BmmArgs(b=b, m=tq, n=tk, k=d, a=ar.BmmMat(dq.ptr.value + off, tq * c, c, 1, 0),
                       bm=ar.BmmMat(dk.ptr.value + off, tk * c, 1, c, 0), out=ar.mat(ws.ptr.value, tq, tk))
        abi.ck(abi.lib().i8ie_bmm_f32(ctx.h, C.byref(s)))
        assert np.array_equal(ws.get().view(np.uint32), got_s[:, hd].view(np.uint32))
        abi.ck(abi.lib().i8ie_softmax_f32(ctx.h, ws.ptr, ws.ptr, b * tq, tk))
        o = ar.BmmArgs(b=b, m=tq, n=d, k=tk, a=ar.mat(ws.ptr.value, tq, tk), bm=ar.BmmMat(dv.ptr.value + off, tk * c, c, 1, 0),
                       out=ar.BmmMat(wo.ptr.value + off, tq * c, c, 1, 0))
        abi.ck(abi.lib().i8ie_bmm_f32(ctx.h, C.byref(o)))
    want, ok3 = wo.read()
    assert ok3 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ref_s, ref_o = mr.attention(q, k, v, heads)
    assert np.abs(got_s - ref_s).max() < 1e-4 and np.abs(got - ref_o).max() < 1e-4   # (and it is attention)
    for dv_ in (dq, dk, dv, do, dsc, ws, wo):
        dv_.free()


# ---- 7: the Python surface --------------------------------------------------------------------------------------------------
def _quant(i8ie, a, s, zp):
    return i8ie.quantize(i8ie.tensor(a), s, zp)


def test_surface_forms_shapes_and_bytes(i8ie):
    rng = np.random.default_rng(70)
    b, heads, d, h, w, tk = 2, 2, 16, 3, 4, 9
    c, t = heads * d, h * w
    qp = dict(qp_for(d), s_q=f32(0.02), s_k=f32(0.03), s_s=f32(0.05), zp_q=127, zp_k=100, zp_v=90)
    kw = dict(heads=heads, score_scale=qp["s_s"], score_zero_point=qp["zp_s"], scale=qp["s_o"], zero_point=qp["zp_o"])
    mk = lambda shape, s, zp: _quant(i8ie, rng.uniform(-3, 3, shape).astype(f32), s, zp)
    # rank 3, three tensors, cross-attention with Tq != Tk
    q3, k3, v3 = mk((b, t, c), qp["s_q"], 127), mk((b, tk, c), qp["s_k"], 100), mk((b, tk, c), qp["s_v"], 90)
    r = i8ie.attention(q3, k3, v3, **kw)
    want = mr.attention_u8(q3.numpy(), k3.numpy(), v3.numpy(), heads, **qp)[3]
    assert r.shape == (b, t, c) and r.scale == pytest.approx(0.01) and r.zero_point == 128 and np.array_equal(r.numpy(), want)
    assert np.array_equal(i8ie.relu(i8ie.attention(q3, k3, v3, **kw)).numpy(), np.maximum(want, 128))
    # rank 4 [n, c, h, w] counts as [n, h * w, c]; a rank-4 q gives a rank-4 result, whatever k and v are
    q4 = mk((b, c, h, w), qp["s_q"], 127)
    r = i8ie.attention(q4, k3, v3, **kw)
    want = mr.attention_u8(mr.tokens(q4.numpy()), k3.numpy(), v3.numpy(), heads, **qp)[3]
    assert r.shape == (b, c, h, w) and np.array_equal(r.numpy(), mr.pixels(want, h, w))
    # packed, rank 3 and rank 4: all three operands share the tensor's scale and zero point
    pq = dict(qp, s_k=qp["s_q"], s_v=qp["s_q"], zp_k=127, zp_v=127)
    p3 = mk((b, t, 3 * c), qp["s_q"], 127)
    want = mr.attention_u8(p3.numpy(), None, None, heads, **pq)[3]
    assert np.array_equal(i8ie.attention(p3, **kw).numpy(), want)
    p4 = mk((b, 3 * c, h, w), qp["s_q"], 127)
    r = i8ie.attention(p4, **kw)
    assert r.shape == (b, c, h, w)
    assert np.array_equal(r.numpy(), mr.pixels(mr.attention_u8(mr.tokens(p4.numpy()), None, None, heads, **pq)[3], h, w))
    # the layer: not converted -> RuntimeError; converted -> the same bytes
    at = i8ie.Attention(heads)
    with pytest.raises(RuntimeError):
        at(p3)
    at.set_score_qparams(qp["s_s"], qp["zp_s"])
    at.set_output_qparams(qp["s_o"], qp["zp_o"])
    at.convert()
    assert np.array_equal(at(p3).numpy(), want) and at.score_qparams() == (pytest.approx(0.05), 140)
    # the shape errors, before any launch
    for bad in (lambda: i8ie.attention(mk((b, t, 3 * c + 1), 0.1, 3), **kw), lambda: i8ie.attention(q3, k3, mk((b, tk + 1, c), 0.1, 3), **kw),
                lambda: i8ie.attention(q3, mk((b + 1, tk, c), 0.1, 3), mk((b + 1, tk, c), 0.1, 3), **kw),
                lambda: i8ie.attention(q3, k3, v3, **dict(kw, heads=3)), lambda: i8ie.attention(q3, k3, v3, **dict(kw, scale=0.0)),
                lambda: i8ie.attention(q3, k3, v3, **dict(kw, score_zero_point=256))):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(TypeError):
        i8ie.attention(q3, k3, v3, heads=heads, scale=0.1, zero_point=3)
    # FP32 tensors: rank 3 through i8ie_attention_f32, rank 4 through strides; the same numbers
    f3 = rng.normal(0, 1, (b, t, 3 * c)).astype(f32)
    g3 = i8ie.attention(i8ie.tensor(f3), heads=heads).numpy()
    assert g3.shape == (b, t, c) and np.abs(g3 - mr.attention(f3, None, None, heads)[1]).max() < 1e-4
    g4 = i8ie.attention(i8ie.tensor(mr.pixels(f3, h, w)), heads=heads).numpy()
    assert g4.shape == (b, c, h, w) and np.array_equal(mr.tokens(g4).view(np.uint32), g3.view(np.uint32))


def test_launch_counts_in_the_deferred_machinery(i8ie):
    """conv(c -> 3c) -> Attention -> conv is three launches; Attention -> relu -> padded conv is two (the relu, the border and the
    re-bias come from the attention kernel); an unbordered producer is read with no conversion launch"""
    rng = np.random.default_rng(71)
    n, c, heads, h, w = 3, 32, 2, 6, 5
    stem0, stem = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128)), support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    qkv = support.conv(i8ie, c, 3 * c, 1, 0, 2, (0.02, 127))
    proj = support.conv(i8ie, c, c, 1, 0, 3, (0.05, 125))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    at = i8ie.Attention(heads)
    at.set_score_qparams(0.04, 140)
    at.set_output_qparams(0.012, 126)
    at.convert()
    x = i8ie.relu(stem(i8ie.relu(stem0(_quant(i8ie, rng.uniform(-3, 3, (n, 3, h, w)).astype(f32), 0.025, 127)))))
    launches = support.counted(lambda: [proj(at(qkv(x)))])
    print(launches)
    assert launches.get("attn_mfma") == 1 and sum(launches.values()) == 3, launches
    p = qkv(x)
    p.data.layout()                                   # the producer has launched, unbordered
    launches = support.counted(lambda: [tail(i8ie.relu(at(p)))])
    print(launches)
    assert launches.get("attn_mfma") == 1 and sum(launches.values()) == 2, launches
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), launches
    # the bytes of the middle of the chain, from the numpy composition
    pv = p.numpy()
    qp = dict(s_q=f32(0.02), s_k=f32(0.02), s_v=f32(0.02), zp_q=127, zp_k=127, zp_v=127, s_s=f32(0.04), zp_s=140, s_o=f32(0.012), zp_o=126)
    S, P, _, O = mr.attention_u8(mr.tokens(pv), None, None, heads, **qp)
    assert len(np.unique(S)) > 30 and len(np.unique(P)) >= 16 and len(np.unique(O)) >= 16
    y = at(p)
    assert y.shape == (n, c, h, w) and np.array_equal(y.numpy(), mr.pixels(O, h, w))
    assert np.array_equal(i8ie.relu(at(qkv(x))).numpy(), np.maximum(mr.pixels(O, h, w), 126))


def test_attention_is_calibrated_like_a_layer_and_round_trips(i8ie, ctx):
    import _CXX_i8ie as cx

    rng = np.random.default_rng(72)
    b, heads, d, t = 4, 2, 8, 10
    x = rng.normal(0, 1.0, (b, t, 3 * heads * d)).astype(f32)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.attn = i8ie.Attention(heads)

    cx.set_calibration_mode("host")
    cx.set_calibration_seed(7)
    try:
        net = Net()
        net.prepare()
        got = net.attn(i8ie.tensor(x)).numpy()
        net.convert()
        ref_s, ref_o = mr.attention(x, None, None, heads)
        assert np.abs(got - ref_o).max() < 1e-4
        want_o = tuple(cx.calibrator_range([got.ravel()], 1.0))
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert net.attn.layer.is_quantized() and net.attn.output_qparams() == want_o and want_o[0] != 1.0
    # the scores the calibrator saw: the FP32 entry's scores_out_dev on the same input (bit-identical by test 6)
    c = 3 * heads * d
    dx, dsc, dout = ctx.put(x), ctx.empty((b, heads, t, t), f32), ctx.empty((b, t, heads * d), f32)
    g = mr.AttnArgs(b=b, heads=heads, d=d, tq=t, tk=t, q=mr.AttnMat(dx.ptr.value, t * c, c, 0), k=mr.AttnMat(dx.ptr.value + 4 * heads * d, t * c, c, 0),
                    v=mr.AttnMat(dx.ptr.value + 8 * heads * d, t * c, c, 0), out=mr.mat(dout.ptr.value, t, heads * d), scores_out_dev=dsc.ptr.value)
    abi.ck(abi.lib().i8ie_attention_f32(ctx.h, C.byref(g)))
    scores = dsc.get()
    assert np.abs(scores - ref_s).max() < 1e-4 and np.array_equal(dout.get().view(np.uint32), got.view(np.uint32))
    cx.set_calibration_seed(7)
    try:
        want_s = tuple(cx.calibrator_range([scores.ravel()], 1.0))
    finally:
        cx.set_calibration_seed(-1)
    s_s, zp_s = net.attn.score_qparams()
    assert (s_s, zp_s) == want_s and s_s != 1.0
    for dv in (dx, dsc, dout):
        dv.free()
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["attn.qparams", "attn.score_qparams"]
    other = Net()
    other.load_quantized(sd)
    assert other.attn.output_qparams() == net.attn.output_qparams() and other.attn.score_qparams() == net.attn.score_qparams()
    qx = _quant(i8ie, x, 0.03, 128)
    r1, r2 = net.attn(qx).numpy(), other.attn(qx).numpy()
    qp = dict(s_q=f32(0.03), s_k=f32(0.03), s_v=f32(0.03), zp_q=128, zp_k=128, zp_v=128, s_s=f32(s_s), zp_s=zp_s, s_o=f32(want_o[0]),
              zp_o=want_o[1])
    assert np.array_equal(r1, r2) and np.array_equal(r1, mr.attention_u8(qx.numpy(), None, None, heads, **qp)[3])


def test_operand_that_a_bordered_conv_consumed_first(i8ie):
    """a tensor that a padded 3x3 conv has launched with a border is then read by Attention (its storage goes back to a
    border-free buffer first), and still feeds an Add afterwards: the bytes of all three are those of the plain tensor"""
    import add_ref

    rng = np.random.default_rng(73)
    n, c, heads, h, w = 2, 16, 2, 5, 4
    stem = support.conv(i8ie, 3, 3 * c, 3, 1, 11, (0.03, 120))
    tail = support.conv(i8ie, 3 * c, 3 * c, 3, 1, 12, (0.05, 110))
    x = _quant(i8ie, rng.uniform(-3, 3, (n, 3, h, w)).astype(f32), 0.025, 127)
    plain = stem(x).numpy()
    p = stem(x)
    t = tail(p)
    t.data.layout()                                   # p has launched, bordered for the padded conv
    y = i8ie.attention(p, heads=heads, score_scale=0.05, score_zero_point=130, scale=0.02, zero_point=125)
    qp = dict(s_q=f32(0.03), s_k=f32(0.03), s_v=f32(0.03), zp_q=120, zp_k=120, zp_v=120, s_s=f32(0.05), zp_s=130, s_o=f32(0.02), zp_o=125)
    want = mr.pixels(mr.attention_u8(mr.tokens(plain), None, None, heads, **qp)[3], h, w)
    assert len(np.unique(want)) >= 16 and np.array_equal(y.numpy(), want)
    z = i8ie.add(p, t, scale=0.06, zero_point=128)
    assert np.array_equal(z.numpy(), add_ref.add_u8(plain, 120, f32(0.03), t.numpy(), 110, f32(0.05), f32(0.06), 128, relu=False))
    assert np.array_equal(p.numpy(), plain)


# ---- 8: mha_tiny (workloads.py), its expected bytes from tests/spec_ref.py ------------------------------------------------
NAME = "mha_tiny"
ATTENTIONS = ("attn1", "attn2")
TRACED = ("pool", "ln1", "qkv1", "attn1", "add1", "c2", "attn2", "add2", "gap", "fc")


def _net(per_channel):
    """nc.calibrated on the device sampler: that calibrator on score tensors too"""
    import net_cases as nc

    return nc.calibrated(NAME, per_channel, calib_images=8, mode="device")


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_mha_net_bit_exact(i8ie, batch, per_channel, tmp_path):
    """logits and every traced tensor against spec_ref.forward: eager, tensor by tensor, under force-fallback, replayed as one
    HIP graph, and from a fresh net that loaded what save_quantized() wrote"""
    import net_cases as nc
    import spec_ref as sr
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = _net(per_channel)
    both = dict(qp, **jqp)
    assert sorted(k for k in jqp if k.endswith(mr.SCORES)) == [a + mr.SCORES for a in ATTENTIONS]
    assert all(s > 0 and s != 1.0 for s, _ in both.values()), both   # everything was calibrated, the scores included
    x = wl.synthetic_input(NAME, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.network(NAME), x, qlayers, qp, jqp, per_channel, sr.traces(mr.tracer(trace, jqp), sr.keeps(TRACED, trace)))
    assert want.shape == (batch, 10) and len(np.unique(want)) > 1
    for a in ATTENTIONS:   # the expected bytes discriminate: spread scores, probabilities and results
        assert len(np.unique(trace[a + ".S"])) > 30 and len(np.unique(trace[a + ".P"])) >= 16 and len(np.unique(trace[a])) >= 16
    nc.check_bit_exact(i8ie, net, NAME, x, want, fallback=True, graph=True, reload_dir=tmp_path, expect_jqp=both)
    mine = {}
    nc.traced(i8ie, net, NAME, x, sr.keeps(TRACED, mine))
    assert sorted(mine) == sorted(TRACED) and sorted(trace) == sorted(TRACED + tuple(a + s for a in ATTENTIONS for s in (".S", ".P")))
    for k in TRACED:   # ("fc": the logits of the walk tensor by tensor)
        assert mine[k].shape == trace[k].shape and np.array_equal(mine[k], trace[k]), k


def test_mha_net_kernels_and_launches(i8ie):
    """block 1 (packed, d = 8) runs in attn_direct, block 2 (d = 16) in attn_mfma; one launch per layer, attention and Add, the
    relus, borders and re-biases folded: c1 + pool, ln1, qkv1, attn1, proj1, add1, c2, q2, k2, v2, attn2, proj2, add2, gap, fc"""
    import _CXX_i8ie as cx
    import spec_ref as sr
    from int8inferenceengine_amd import workloads as wl

    net = _net(False)[0]
    x = wl.synthetic_input(NAME, 5, seed=sr.INPUT_SEED)
    net(i8ie.tensor(x)).numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        net(i8ie.tensor(x)).numpy()
    finally:
        prof = cx.profile_stop()
    launches = support.launch_counts(prof)
    print(launches)
    assert launches.get("attn_direct") == 1 and launches.get("attn_mfma") == 1, launches
    for k in launches:
        assert not k.startswith(("bmm_", "softmax_", "rebias", "fill_border", "reborder")), launches
    # the relus behind attn / add1 / add2 are folded into their producers; the one relu launch left is c1's, whose 3-channel
    # strided conv takes the NCHW route (conv, relu, pool, one conversion), as it does without any attention in the net
    assert launches.get("relu_u8", 0) <= 1, launches
