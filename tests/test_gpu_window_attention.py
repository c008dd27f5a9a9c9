"""The windowed attention on the GPU (csrc/i8ie_attention.hip).  Every INT8 comparison is bit for bit
against tests/mha_ref.py applied to numpy-partitioned operands (tests/window_ref.py), never against the code under test; the
scores S, the probabilities P, the second product's accumulators and the result O are each checked through the debug outputs,
so a failure names its phase."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import mha_ref as mr
import support
import window_ref as wr
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL, POISON = 0xC3, 0x5A

ctx = support.ctx_fixture(wr)


def qp_for(d, zp=(120, 131, 125, 140, 128), s_s=0.03):
    """test_gpu_mha.py's choice: parameters that spread the scores of random bytes over the byte range"""
    s = f32(np.sqrt(s_s * 40.0 / (5476.0 * np.sqrt(d))))
    return dict(s_q=s, zp_q=zp[0], s_k=s, zp_k=zp[1], s_v=f32(0.04), zp_v=zp[2], s_s=f32(s_s), zp_s=zp[3], s_o=f32(0.01), zp_o=zp[4])


def rand_maps(rng, n, c, h, w):
    return tuple(rng.integers(0, 256, (n, c, h, w), dtype=np.uint8) for _ in range(3))


def run(ctx, q, k, v, heads, window, qp, relu=False, s8=(False, False, False), borders=(0, 0, 0), o_s8=False, out_border=0,
        fallback=False, packed=False, offsets=(0, 0, 0)):
    """The u8 entry on host maps [n, c, h, w], laid out as asked: each operand channels-last with a border of its own full of
    POISON, re-biased or not, at a byte offset inside its allocation; packed: one [n, h, w, 3c] buffer (one border, one
    re-bias mark); the result with its own border, re-biased or not, in a guarded buffer filled with FILL.
    Returns (S, P, acc, O as plain bytes [n, c, h, w], kernel names)."""
    n, c, h, w = q.shape
    wh, ww = wr.pair(window)
    T, nW = wh * ww, (h // wh) * (w // ww)
    bufs = []
    if packed:
        host = support.phys_nhwc(np.concatenate([q, k, v], axis=1), borders[0], POISON, s8[0])
        dev = ctx.put(np.concatenate([np.zeros(offsets[0], np.uint8), host.ravel()]))
        bufs.append(dev)
        mats = [wr.map_mat(dev.ptr.value, h, w, 3 * c, borders[0], s8[0], offsets[0] + i * c) for i in range(3)]
        borders = (borders[0],) * 3
    else:
        mats = []
        for i, a in enumerate((q, k, v)):
            host = support.phys_nhwc(a, borders[i], POISON, s8[i])
            dev = ctx.put(np.concatenate([np.zeros(offsets[i], np.uint8), host.ravel()]))
            bufs.append(dev)
            mats.append(wr.map_mat(dev.ptr.value, h, w, c, borders[i], s8[i], offsets[i]))
    g = mr.AttnArgs(b=n, heads=heads, d=c // heads, tq=T, tk=T, q=mats[0], k=mats[1], v=mats[2], relu=1 if relu else 0, **qp)
    B = out_border
    do = abi.GuardedU8(ctx, (n, h + 2 * B, w + 2 * B, c), fill=FILL)
    g.out = wr.map_mat(do.ptr.value, h, w, c, B, o_s8)
    g.out_h, g.out_w, g.out_border = h, w, B
    ds = abi.GuardedU8(ctx, (n * nW, heads, T, T))
    dp = abi.GuardedU8(ctx, (n * nW, heads, T, T))
    dacc = abi.GuardedU8(ctx, (n * nW, T, c), np.int32)
    g.scores_dbg_dev, g.probs_dbg_dev, g.acc_dbg_dev = ds.ptr.value, dp.ptr.value, dacc.ptr.value
    win = wr.AttnWindow(map_h=h, map_w=w, win_h=wh, win_w=ww, q_border=borders[0], k_border=borders[1], v_border=borders[2])
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_attention_window_u8(ctx.h, C.byref(g), C.byref(win)))
    finally:
        ctx.set_force_fallback(False)
    raw, S, P, acc = do.get(), ds.get(), dp.get(), dacc.get()
    assert do.guards_ok() and ds.guards_ok() and dp.guards_ok() and dacc.guards_ok()
    ring = raw.copy()
    ring[:, B:B + h, B:B + w, :] = FILL
    assert (ring == FILL).all(), "a border byte of the result was written"
    O = raw[:, B:B + h, B:B + w, :].transpose(0, 3, 1, 2)
    O = O ^ np.uint8(0x80) if o_s8 else O
    for dv in bufs + [do, ds, dp, dacc]:
        dv.free()
    return S, P, acc, np.ascontiguousarray(O), names


def check(ctx, q, k, v, heads, window, qp, kernel, want=None, **kw):
    if want is None:
        want = wr.attention_u8(q, k, v, heads, window, relu=kw.get("relu", False), **qp)
    S, P, acc, O, names = run(ctx, q, k, v, heads, window, qp, **kw)
    tag = (q.shape, window, heads, kernel, kw)
    assert names == {kernel: 1}, (names, tag)
    for name, got, exp in zip(("S", "P", "acc", "O"), (S, P, acc, O), want):
        assert np.array_equal(got, exp), (name, tag, np.argwhere(got != exp)[:4])
    return want


# ---- the grid ----------------------------------------------------------------------------------------------------------------
GRID = [((4, 6), (2, 3)), ((8, 8), (4, 4)), ((14, 7), (7, 7)), ((16, 8), (8, 8)), ((9, 16), (9, 8)), ((8, 8), (8, 8)), ((4, 4), (1, 1))]


@pytest.mark.parametrize("d,kernel", [(16, "attn_mfma_win"), (32, "attn_mfma_win"), (8, "attn_direct_win")])
def test_grid_both_kernels_and_forced_direct(ctx, d, kernel):
    """every (map, window) of the list with this d, crossed with images in {1, 3} and packed / unpacked operands; heads in
    {1, 2, 3}, the re-bias marks and the relu cycle with the case index; each case again under I8IE_OPT_FORCE_FALLBACK gives
    the same bytes"""
    rng = np.random.default_rng(d)
    spread, i = 0, 0
    for ((h, w), window), n, packed in itertools.product(GRID, (1, 3), (False, True)):
        i += 1
        heads = (1, 2, 3)[i % 3]
        q, k, v = rand_maps(rng, n, heads * d, h, w)
        qp = qp_for(d)
        kw = dict(relu=bool(i & 1), o_s8=bool(i & 2))
        if packed:           # one scale, zero point and re-bias mark for the three operands
            qp = dict(qp, s_k=qp["s_q"], s_v=qp["s_q"], zp_k=qp["zp_q"], zp_v=qp["zp_q"])
            kw.update(packed=True, s8=(bool(i & 4),) * 3)
        else:
            kw.update(s8=(bool(i & 2), bool(i & 4), not (i & 8)))
        want = check(ctx, q, k, v, heads, window, qp, kernel, **kw)
        check(ctx, q, k, v, heads, window, qp, "attn_direct_win", want=want, fallback=True, **kw)
        spread = max(spread, len(np.unique(want[3])))
        if window != (1, 1):
            assert len(np.unique(want[0])) > min(50, want[0].size // 4)
        else:
            assert (want[1] == 255).all()     # one key: every probability clamps at 255
    assert spread > 30   # the expected bytes discriminate


def test_the_whole_map_equals_the_global_entry(ctx):
    """window == (h, w): the bytes of i8ie_attention_u8 on the same map"""
    rng = np.random.default_rng(5)
    n, heads, d, h, w = 2, 2, 16, 8, 8
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    qp = qp_for(d)
    _, _, _, O, _ = run(ctx, q, k, v, heads, (h, w), qp)
    tq, tk, tv = (ctx.put(mr.tokens(a)) for a in (q, k, v))
    do = abi.GuardedU8(ctx, (n, h * w, heads * d), fill=FILL)
    g = mr.AttnArgs(b=n, heads=heads, d=d, tq=h * w, tk=h * w, q=mr.mat(tq.ptr.value, h * w, heads * d), k=mr.mat(tk.ptr.value, h * w, heads * d),
                    v=mr.mat(tv.ptr.value, h * w, heads * d), out=mr.mat(do.ptr.value, h * w, heads * d), **qp)
    abi.ck(abi.lib().i8ie_attention_u8(ctx.h, C.byref(g)))
    glob = do.get()
    assert do.guards_ok() and np.array_equal(O, mr.pixels(glob, h, w))
    for dv in (tq, tk, tv, do):
        dv.free()


@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_zero_points_and_byte_extremes(ctx, fallback):
    kernel = "attn_direct_win" if fallback else "attn_mfma_win"
    rng = np.random.default_rng(40)
    n, heads, d, h, w, window = 2, 2, 16, 8, 8, (4, 4)
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    cases = [tuple(z if j == i else 128 for j in range(5)) for i in range(5) for z in (0, 255)]
    cases += [(0,) * 5, (255,) * 5, (0, 255, 0, 255, 0), (255, 0, 255, 0, 255)]
    for i, zps in enumerate(cases):
        check(ctx, q, k, v, heads, window, qp_for(d, zp=zps), kernel, fallback=fallback, relu=bool(i & 1))
    for fill in (0, 255):
        a = [np.full_like(x, fill) for x in (q, k, v)]
        for zps in ((0, 0, 0, 0, 0), (255, 255, 255, 255, 255), (128, 3, 250, 77, 9)):
            want = check(ctx, a[0], a[1], a[2], heads, window, qp_for(d, zp=zps), kernel, fallback=fallback)
            assert (want[1] == 16).all()      # a constant score row: the uniform softmax, 256 / 16
    hot = dict(qp_for(d), s_q=f32(0.5), s_k=f32(0.5), s_s=f32(0.01))   # scores saturated at both ends
    want = check(ctx, q, k, v, heads, window, hot, kernel, fallback=fallback)
    assert (want[0] == 0).any() and (want[0] == 255).any()


# ---- layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_operand_and_result_layouts(ctx, fallback):
    """operands with a border of 0 or 1 full of poison that must never be read, plain and re-biased; the result with a border
    of 0 or 1, plain and re-biased, its border bytes and the guards around the buffer untouched"""
    kernel = "attn_direct_win" if fallback else "attn_mfma_win"
    rng = np.random.default_rng(50)
    n, heads, d, h, w, window = 2, 2, 16, 6, 9, (3, 3)
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    qp = qp_for(d)
    want = wr.attention_u8(q, k, v, heads, window, **qp)
    for j, borders in enumerate(itertools.product([0, 1], repeat=3)):
        s8 = (bool(j & 1), bool(j & 2), bool(j & 4))
        check(ctx, q, k, v, heads, window, qp, kernel, want=want, fallback=fallback, borders=borders, s8=s8)
        check(ctx, q, k, v, heads, window, qp, kernel, want=want, fallback=fallback, borders=borders, s8=tuple(not f for f in s8))
    pq = dict(qp, s_k=qp["s_q"], s_v=qp["s_q"], zp_k=qp["zp_q"], zp_v=qp["zp_q"])
    wp = wr.attention_u8(q, k, v, heads, window, **pq)
    for border, s8 in itertools.product([0, 1, 2], [False, True]):
        check(ctx, q, k, v, heads, window, pq, kernel, want=wp, fallback=fallback, packed=True, borders=(border,) * 3, s8=(s8,) * 3)
    wrelu = wr.attention_u8(q, k, v, heads, window, relu=True, **qp)
    for out_border, o_s8 in itertools.product([0, 1, 2], [False, True]):
        check(ctx, q, k, v, heads, window, qp, kernel, want=wrelu, fallback=fallback, relu=True, out_border=out_border, o_s8=o_s8,
              borders=(1, 0, 1))


def test_unaligned_operand_pointers_take_the_direct_kernel(ctx):
    rng = np.random.default_rng(60)
    q, k, v = rand_maps(rng, 2, 32, 8, 8)
    want = check(ctx, q, k, v, 2, (4, 4), qp_for(16), "attn_mfma_win")
    for offsets in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        check(ctx, q, k, v, 2, (4, 4), qp_for(16), "attn_direct_win", want=want, offsets=offsets)


# ---- the FP32 entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_f32_entry_is_the_f32_entry_on_partitioned_tensors(ctx, packed):
    """bit for bit: result and scores of i8ie_attention_window_f32 on NCHW maps against i8ie_attention_f32 on the tensors that
    numpy partitioned"""
    rng = np.random.default_rng(70)
    n, heads, d, h, w, window = 3, 2, 5, 6, 8, (3, 4)
    c, T, nW, hw = heads * d, 12, 4, 48
    q, k, v = (rng.normal(0, 1, (n, c, h, w)).astype(f32) for _ in range(3))
    do, dsc = ctx.guarded((n, c, h, w)), ctx.guarded((n * nW, heads, T, T))
    if packed:
        dx = ctx.put(np.concatenate([q, k, v], axis=1))
        mats = [mr.AttnMat(dx.ptr.value + 4 * i * c * hw, 3 * c * hw, hw, 0) for i in range(3)]
        bufs = [dx]
    else:
        bufs = [ctx.put(a) for a in (q, k, v)]
        mats = [mr.AttnMat(b.ptr.value, c * hw, hw, 0) for b in bufs]
    g = mr.AttnArgs(b=n, heads=heads, d=d, tq=T, tk=T, q=mats[0], k=mats[1], v=mats[2], out=mr.AttnMat(do.ptr.value, c * hw, hw, 0),
                    out_h=h, out_w=w, scores_out_dev=dsc.ptr.value)
    win = wr.AttnWindow(map_h=h, map_w=w, win_h=window[0], win_w=window[1])
    abi.ck(abi.lib().i8ie_attention_window_f32(ctx.h, C.byref(g), C.byref(win)))
    got, ok1 = do.read()
    got_s, ok2 = dsc.read()
    assert ok1 and ok2 and abi.GuardedOut.unwritten(got) == 0 and abi.GuardedOut.unwritten(got_s) == 0
    pq, pk, pv = (ctx.put(wr.part(a, window)) for a in (q, k, v))
    wo, wsc = ctx.guarded((n * nW, T, c)), ctx.guarded((n * nW, heads, T, T))
    e = mr.AttnArgs(b=n * nW, heads=heads, d=d, tq=T, tk=T, q=mr.mat(pq.ptr.value, T, c), k=mr.mat(pk.ptr.value, T, c),
                    v=mr.mat(pv.ptr.value, T, c), out=mr.mat(wo.ptr.value, T, c), scores_out_dev=wsc.ptr.value)
    abi.ck(abi.lib().i8ie_attention_f32(ctx.h, C.byref(e)))
    want, ok3 = wo.read()
    want_s, ok4 = wsc.read()
    assert ok3 and ok4 and support.same_bits(got, wr.unpart(want, window, (n, c, h, w))) and support.same_bits(got_s, want_s)
    ref_s, ref_o = wr.attention(q, k, v, heads, window)
    assert np.abs(got_s - ref_s).max() < 1e-4 and np.abs(got - ref_o).max() < 1e-4   # (and it is windowed attention)
    for dv in bufs + [do, dsc, pq, pk, pv, wo, wsc]:
        dv.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def _quant(i8ie, a, s, zp):
    return i8ie.quantize(i8ie.tensor(a), s, zp)


QP_SURF = dict(s_q=f32(0.02), s_k=f32(0.02), s_v=f32(0.02), zp_q=127, zp_k=127, zp_v=127, s_s=f32(0.04), zp_s=140, s_o=f32(0.012), zp_o=126)


def _converted(i8ie, heads, window):
    at = i8ie.Attention(heads, window=window)
    at.set_score_qparams(0.04, 140)
    at.set_output_qparams(0.012, 126)
    at.convert()
    return at


def test_surface_forms_and_bytes(i8ie):
    rng = np.random.default_rng(80)
    n, heads, d, h, w, window = 2, 2, 16, 8, 12, (4, 3)
    c = heads * d
    kw = dict(heads=heads, score_scale=0.04, score_zero_point=140, scale=0.012, zero_point=126)
    mk = lambda ch: _quant(i8ie, rng.uniform(-2.5, 2.5, (n, ch, h, w)).astype(f32), 0.02, 127)  # noqa: E731
    q, k, v, p = mk(c), mk(c), mk(c), mk(3 * c)
    want = wr.attention_u8(q.numpy(), k.numpy(), v.numpy(), heads, window, **QP_SURF)[3]
    r = i8ie.attention(q, k, v, window=window, **kw)
    assert r.shape == (n, c, h, w) and r.zero_point == 126 and np.array_equal(r.numpy(), want) and len(np.unique(want)) >= 16
    assert np.array_equal(i8ie.relu(i8ie.attention(q, k, v, window=window, **kw)).numpy(), np.maximum(want, 126))
    wantp = wr.attention_u8(p.numpy(), None, None, heads, window, **QP_SURF)[3]
    assert np.array_equal(i8ie.attention(p, window=list(window), **kw).numpy(), wantp)
    assert np.array_equal(_converted(i8ie, heads, window)(p).numpy(), wantp)
    assert np.array_equal(_converted(i8ie, heads, 4)(p).numpy(), wr.attention_u8(p.numpy(), None, None, heads, 4, **QP_SURF)[3])
    # the whole map as the window is the global form
    assert np.array_equal(i8ie.attention(p, window=(h, w), **kw).numpy(), i8ie.attention(p, **kw).numpy())
    with pytest.raises(RuntimeError):
        i8ie.Attention(heads, window=window)(p)      # not converted
    # FP32 tensors: i8ie_attention_window_f32
    f = rng.normal(0, 1, (n, 3 * c, h, w)).astype(f32)
    g = i8ie.attention(i8ie.tensor(f), heads=heads, window=window).numpy()
    assert g.shape == (n, c, h, w) and np.abs(g - wr.attention(f, None, None, heads, window)[1]).max() < 1e-4


def test_launch_counts_in_the_deferred_machinery(i8ie):
    """conv(c -> 3c) -> Attention(window) -> relu -> conv is three launches (the relu, the border and the re-bias come from the
    attention kernel); an operand that a padded conv made bordered is read with its border: no conversion launch"""
    rng = np.random.default_rng(81)
    n, c, heads, h, w, window = 3, 32, 2, 8, 8, (4, 4)
    stem0, stem = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128)), support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    qkv = support.conv(i8ie, c, 3 * c, 1, 0, 2, (0.02, 127))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    side = support.conv(i8ie, 3 * c, 8, 3, 1, 6, (0.07, 100))
    at = _converted(i8ie, heads, window)
    x = i8ie.relu(stem(i8ie.relu(stem0(_quant(i8ie, rng.uniform(-3, 3, (n, 3, h, w)).astype(f32), 0.025, 127)))))
    launches = support.counted(lambda: [tail(i8ie.relu(at(qkv(x))))])
    print(launches)
    assert launches.get("attn_mfma_win") == 1 and sum(launches.values()) == 3, launches
    support.assert_no_glue_launches(launches)
    p = qkv(x)
    s = side(p)
    s.data.layout()                                   # p has launched, bordered for the padded conv
    launches = support.counted(lambda: [tail(i8ie.relu(at(p)))])
    print(launches)
    assert launches.get("attn_mfma_win") == 1 and sum(launches.values()) == 2, launches
    support.assert_no_glue_launches(launches)
    pv = p.numpy()
    S, P, _, O = wr.attention_u8(pv, None, None, heads, window, **QP_SURF)
    assert len(np.unique(S)) > 30 and len(np.unique(P)) >= 16 and len(np.unique(O)) >= 16
    p2 = qkv(x)
    side(p2).data.layout()
    assert np.array_equal(at(p2).numpy(), O)          # the bordered operand, read in place
    assert np.array_equal(i8ie.relu(at(qkv(x))).numpy(), np.maximum(O, 126))


def test_calibration_state_dict_file_and_graph(i8ie, ctx, tmp_path):
    """while preparing the FP32 path samples the windowed scores [n * nW, H, T, T] and the result (the device observers
    against the host walk of the same arrays); convert() fixes both parameter sets; they survive the state dict and a file;
    the converted layer replays inside a HIP graph with the eager bytes"""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(82)
    n, heads, d, h, w, window = 4, 2, 16, 8, 8, (4, 4)
    c = heads * d
    x = rng.normal(0, 1.0, (n, 3 * c, h, w)).astype(f32)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.attn = i8ie.Attention(heads, window=window)

        def forward(self, t):
            return self.attn(t)

    ref_s, ref_o = wr.attention(x, None, None, heads, window)
    found = {}
    for mode in ("host", "device"):
        cx.set_calibration_mode(mode)
        cx.set_calibration_seed(7)
        try:
            net = Net()
            net.prepare()
            got = net(i8ie.tensor(x)).numpy()
            net.convert()
        finally:
            cx.set_calibration_mode("auto")
            cx.set_calibration_seed(-1)
        assert np.abs(got - ref_o).max() < 1e-4
        found[mode] = (net.attn.output_qparams(), net.attn.score_qparams())
    # the scores the calibrator saw: the windowed FP32 entry's scores_out_dev, bit-identical to the partitioned entry's
    cx.set_calibration_seed(7)
    try:
        dx, dsc, dout = ctx.put(x), ctx.empty(ref_s.shape, f32), ctx.empty((n, c, h, w), f32)
        hw = h * w
        g = mr.AttnArgs(b=n, heads=heads, d=d, tq=16, tk=16, out=mr.AttnMat(dout.ptr.value, c * hw, hw, 0), out_h=h, out_w=w,
                        scores_out_dev=dsc.ptr.value, **{m: mr.AttnMat(dx.ptr.value + 4 * i * c * hw, 3 * c * hw, hw, 0) for i, m in enumerate("qkv")})
        abi.ck(abi.lib().i8ie_attention_window_f32(ctx.h, C.byref(g), C.byref(wr.AttnWindow(map_h=h, map_w=w, win_h=4, win_w=4))))
        scores, out = dsc.get(), dout.get()
        assert scores.shape == (n * 4, heads, 16, 16) and np.abs(scores - ref_s).max() < 1e-4 and support.same_bits(out, got)
        host = (tuple(cx.calibrator_range([out.ravel()], 1.0)), tuple(cx.calibrator_range([scores.ravel()], 1.0)))
    finally:
        cx.set_calibration_seed(-1)
        for dv in (dx, dsc, dout):
            dv.free()
    # the device observers: the device sampler on its own, fed the same two arrays with the same seed
    want = tuple(tuple(cx.calibrator_device_samples([a.ravel()], 7)[2:]) for a in (out, scores))
    assert found["host"] == host and found["device"] == want and want[0][0] != 1.0 and want[1][0] != 1.0
    sd = net.quantized_state_dict()
    assert sorted(sd) == ["attn.qparams", "attn.score_qparams"]
    other = Net()
    other.load_quantized(sd)
    path = str(tmp_path / "win.npz")
    net.save_quantized(path)
    third = Net()
    third.load_quantized_file(path)
    qx = _quant(i8ie, x, 0.03, 128)
    (s_o, zp_o), (s_s, zp_s) = want
    qp = dict(s_q=f32(0.03), s_k=f32(0.03), s_v=f32(0.03), zp_q=128, zp_k=128, zp_v=128, s_s=f32(s_s), zp_s=zp_s, s_o=f32(s_o), zp_o=zp_o)
    expect = wr.attention_u8(qx.numpy(), None, None, heads, window, **qp)[3]
    for m in (net, other, third):
        assert m.attn.score_qparams() == want[1] and np.array_equal(m.forward(qx).numpy(), expect)
    gf = GraphedForward(lambda t: net.forward(i8ie.quantize(t, 0.03, 128)), i8ie.tensor(x))
    assert np.array_equal(gf().numpy(), expect) and np.array_equal(gf().numpy(), expect)


# ---- one Twins block, step by step ---------------------------------------------------------------------------------------------
def _twins_block(i8ie, c, heads, window, per_channel, seed):
    """LSA (windowed attention) + MLP, the position-encoding conv, GSA (global attention, k / v from a stride-2 conv) + MLP"""
    rng = np.random.default_rng(seed)

    class Block(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.stem = i8ie.Conv2d(3, c, 3, padding=1)
            for p, win in (("l_", window), ("g_", None)):
                setattr(self, p + "ln1", i8ie.LayerNorm(c))
                setattr(self, p + "attn", i8ie.Attention(heads, window=win))
                setattr(self, p + "proj", i8ie.Conv2d(c, c, 1))
                setattr(self, p + "add1", i8ie.Add())
                setattr(self, p + "ln2", i8ie.LayerNorm(c))
                setattr(self, p + "fc1", i8ie.Conv2d(c, 2 * c, 1))
                setattr(self, p + "act", i8ie.Activation("hardswish"))
                setattr(self, p + "fc2", i8ie.Conv2d(2 * c, c, 1))
                setattr(self, p + "add2", i8ie.Add())
            self.l_qkv = i8ie.Conv2d(c, 3 * c, 1)
            self.pos = i8ie.Conv2d(c, c, 3, padding=1, groups=c)
            self.pos_add = i8ie.Add()
            self.g_q = i8ie.Conv2d(c, c, 1)
            self.g_sr = i8ie.Conv2d(c, c, 2, stride=2)
            self.g_k = i8ie.Conv2d(c, c, 1)
            self.g_v = i8ie.Conv2d(c, c, 1)

        def steps(self, x):
            """the forward as (name, tensor) pairs, in order"""
            out = []
            keep = lambda name, t: (out.append((name, t)), t)[1]  # noqa: E731
            x = keep("stem", self.stem(x))
            y = keep("l_ln1", self.l_ln1(x))
            a = keep("l_attn", self.l_attn(keep("l_qkv", self.l_qkv(y))))
            x = keep("l_add1", self.l_add1(x, keep("l_proj", self.l_proj(a))))
            m = keep("l_fc2", self.l_fc2(keep("l_act", self.l_act(keep("l_fc1", self.l_fc1(keep("l_ln2", self.l_ln2(x))))))))
            x = keep("l_add2", self.l_add2(x, m))
            x = keep("pos_add", self.pos_add(x, keep("pos", self.pos(x))))
            y = keep("g_ln1", self.g_ln1(x))
            r = keep("g_sr", self.g_sr(y))
            a = keep("g_attn", self.g_attn(keep("g_q", self.g_q(y)), keep("g_k", self.g_k(r)), keep("g_v", self.g_v(r))))
            x = keep("g_add1", self.g_add1(x, keep("g_proj", self.g_proj(a))))
            m = keep("g_fc2", self.g_fc2(keep("g_act", self.g_act(keep("g_fc1", self.g_fc1(keep("g_ln2", self.g_ln2(x))))))))
            x = keep("g_add2", self.g_add2(x, m))
            return out

        def forward(self, x):
            return self.steps(x)[-1][1]

    net = Block()
    sd = {}
    shapes = dict(stem=(c, 3, 3, 3), l_qkv=(3 * c, c, 1, 1), l_proj=(c, c, 1, 1), l_fc1=(2 * c, c, 1, 1), l_fc2=(c, 2 * c, 1, 1), pos=(c, 1, 3, 3),
                  g_q=(c, c, 1, 1), g_sr=(c, c, 2, 2), g_k=(c, c, 1, 1), g_v=(c, c, 1, 1), g_proj=(c, c, 1, 1), g_fc1=(2 * c, c, 1, 1),
                  g_fc2=(c, 2 * c, 1, 1))
    for name, shape in shapes.items():
        fan = shape[1] * shape[2] * shape[3]
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan)).astype(f32)
        sd[name + ".bias"] = rng.uniform(-0.1, 0.1, shape[0]).astype(f32)
    for name in ("l_ln1", "l_ln2", "g_ln1", "g_ln2"):
        sd[name + ".weight"] = rng.normal(1.0, 0.2, c).astype(f32)
        sd[name + ".bias"] = rng.normal(0.0, 0.2, c).astype(f32)
    net.load(sd)
    net.prepare()
    net(i8ie.tensor(rng.uniform(-1, 1, (8, 3, 8, 8)).astype(f32)))
    net.convert(per_channel=per_channel)
    return net


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_twins_block_step_by_step(i8ie, ctx, batch, per_channel):
    """every step of the block -- windowed attention, depthwise position encoding, global attention with strided k / v, both
    MLPs (LayerNorm, 1x1 conv, hardswish, 1x1 conv), every projection and all five skips -- against the existing references
    applied to the previous steps' device bytes, eager and under force-fallback; the whole forward gives the stepwise bytes"""
    import _CXX_i8ie as cx
    import add_ref

    c, heads, window = 32, 2, (4, 4)
    net = _twins_block(i8ie, c, heads, window, per_channel, 90)
    x = i8ie.quantize(i8ie.tensor(np.random.default_rng(91).uniform(-1, 1, (batch, 3, 8, 8)).astype(f32)), 1.0 / 128, 128)
    runs = {}
    for fallback in (False, True):
        cx.force_fallback(fallback)
        try:
            runs[fallback] = {name: (t.numpy(), f32(t.scale), int(t.zero_point)) for name, t in net.steps(x)}
            whole = net.forward(x).numpy()
        finally:
            cx.force_fallback(False)
        assert np.array_equal(whole, runs[fallback]["g_add2"][0])
    got = runs[False]
    for name in got:
        assert np.array_equal(got[name][0], runs[True][name][0]), name
    # windowed attention on the packed projection's bytes
    p, s, z = got["l_qkv"]
    (s_s, zp_s), (s_o, zp_o) = net.l_attn.score_qparams(), net.l_attn.output_qparams()
    S, P, _, O = wr.attention_u8(p, None, None, heads, window, s_q=s, s_k=s, s_v=s, zp_q=z, zp_k=z, zp_v=z, s_s=f32(s_s), zp_s=zp_s,
                                 s_o=f32(s_o), zp_o=zp_o)
    assert np.array_equal(got["l_attn"][0], O) and len(np.unique(S)) > 30 and len(np.unique(P)) >= 8 and len(np.unique(O)) >= 16
    # global attention, 64 queries against the 16 keys of the stride-2 map
    (q, sq, zq), (k, sk, zk), (v, sv, zv) = got["g_q"], got["g_k"], got["g_v"]
    (s_s, zp_s), (s_o, zp_o) = net.g_attn.score_qparams(), net.g_attn.output_qparams()
    assert k.shape == (batch, c, 4, 4)
    O = mr.attention_u8(mr.tokens(q), mr.tokens(k), mr.tokens(v), heads, s_q=sq, zp_q=zq, s_k=sk, zp_k=zk, s_v=sv, zp_v=zv, s_s=f32(s_s),
                        zp_s=zp_s, s_o=f32(s_o), zp_o=zp_o)[3]
    assert np.array_equal(got["g_attn"][0], mr.pixels(O, 8, 8)) and len(np.unique(O)) >= 16
    # the five skips: behind each attention, behind each MLP, and the position encoding's
    checked = {"l_attn", "g_attn"}
    for out, a, b in (("l_add1", "stem", "l_proj"), ("l_add2", "l_add1", "l_fc2"), ("pos_add", "l_add2", "pos"),
                      ("g_add1", "pos_add", "g_proj"), ("g_add2", "g_add1", "g_fc2")):
        (xa, sa, za), (xb, sb, zb), (xo, so, zo) = got[a], got[b], got[out]
        assert np.array_equal(xo, add_ref.add_u8(xa, za, sa, xb, zb, sb, so, zo, relu=False)), out
        checked.add(out)
    # every conv: the stem, the projections, the depthwise 3x3, the stride-2 reduction and the four 1x1 convs of the MLPs
    import act_ref
    import grouped_ref as gr
    import layernorm_ref as lr

    x0 = (x.numpy(), f32(x.scale), int(x.zero_point))
    for name, src, groups, stride, pad in (("stem", None, 1, 1, 1), ("l_qkv", "l_ln1", 1, 1, 0), ("l_proj", "l_attn", 1, 1, 0),
                                           ("l_fc1", "l_ln2", 1, 1, 0), ("l_fc2", "l_act", 1, 1, 0), ("pos", "l_add2", c, 1, 1),
                                           ("g_q", "g_ln1", 1, 1, 0), ("g_sr", "g_ln1", 1, 2, 0), ("g_k", "g_sr", 1, 1, 0),
                                           ("g_v", "g_sr", 1, 1, 0), ("g_proj", "g_attn", 1, 1, 0), ("g_fc1", "g_ln2", 1, 1, 0),
                                           ("g_fc2", "g_act", 1, 1, 0)):
        L = getattr(net, name)
        xi, si, zi = x0 if src is None else got[src]
        s_out, zp_out = L.output_qparams()
        conv, ws = (gr.conv2d_grouped_pc, L.weight_scales()) if per_channel else (gr.conv2d_grouped, L.weight_scale())
        want = conv(xi, L.layer.q_weight(), L.layer.q_bias(), groups, stride, pad, si, zi, ws, f32(s_out), zp_out)[0]
        assert np.array_equal(got[name][0], want), name
        checked.add(name)
    # the four LayerNorms and the two hardswish lookups
    for name, src in (("l_ln1", "stem"), ("l_ln2", "l_add1"), ("g_ln1", "pos_add"), ("g_ln2", "g_add1")):
        L = getattr(net, name)
        xi, si, _ = got[src]
        s_out, zp_out = L.output_qparams()
        want = lr.layer_norm_u8_nchw(xi, si, L.eps, L.layer.weight(), L.layer.bias(), f32(s_out), zp_out)
        assert np.array_equal(got[name][0], want) and len(np.unique(want)) >= 16, name
        checked.add(name)
    for name, src in (("l_act", "l_fc1"), ("g_act", "g_fc1")):
        L = getattr(net, name)
        xi, si, zi = got[src]
        s_out, zp_out = L.output_qparams()
        want = act_ref.act_u8(xi, "hardswish", L.param, si, zi, f32(s_out), zp_out)
        assert np.array_equal(got[name][0], want) and len(np.unique(want)) >= 16, name
        checked.add(name)
    assert checked == set(got)   # no step of the block is left to the eager-against-fallback comparison alone
