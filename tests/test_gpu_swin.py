"""The shifted-window attention with a relative position bias on the GPU (csrc/i8ie_attention.hip).
Every INT8 comparison is bit for bit against tests/swin_ref.py, never against the code under test; the scores S, the
probabilities P, the second product's accumulators and the result O are each checked through the debug outputs, so a failure
names its phase."""
import ctypes as C

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import mha_ref as mr
import support
import swin_ref as sr
import window_ref as wr
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL, POISON = 0xC3, 0x5A

ctx = support.ctx_fixture(sr)


def qp_for(d, zp=(120, 131, 125, 140, 128), s_s=0.03):
    """test_gpu_mha.py's choice: parameters that spread the scores of random bytes over the byte range"""
    s = f32(np.sqrt(s_s * 40.0 / (5476.0 * np.sqrt(d))))
    return dict(s_q=s, zp_q=zp[0], s_k=s, zp_k=zp[1], s_v=f32(0.04), zp_v=zp[2], s_s=f32(s_s), zp_s=zp[3], s_o=f32(0.01), zp_o=zp[4])


def run(ctx, q, k, v, heads, window, shift, bias, qp, relu=False, fallback=False, packed=False, borders=(0, 0, 0), s8=False, out_border=0,
        o_s8=False, entry="i8ie_attention_swin_u8"):
    """The u8 entry on host maps [n, c, h, w]: operands channels-last with a border full of POISON (packed: one [n, h, w, 3c]
    buffer), the result with its own border in a guarded buffer full of FILL.  Returns (S, P, acc, O [n, c, h, w], names)."""
    n, c, h, w = q.shape
    (wh, ww), (sh, sw) = wr.pair(window), wr.pair(shift)
    T, nW = wh * ww, (h // wh) * (w // ww)
    if packed:
        bufs = [ctx.put(support.phys_nhwc(np.concatenate([q, k, v], axis=1), borders[0], POISON, s8))]
        mats = [wr.map_mat(bufs[0].ptr.value, h, w, 3 * c, borders[0], s8, i * c) for i in range(3)]
        borders = (borders[0],) * 3
    else:
        bufs = [ctx.put(support.phys_nhwc(a, borders[i], POISON, s8)) for i, a in enumerate((q, k, v))]
        mats = [wr.map_mat(bufs[i].ptr.value, h, w, c, borders[i], s8) for i in range(3)]
    g = mr.AttnArgs(b=n, heads=heads, d=c // heads, tq=T, tk=T, q=mats[0], k=mats[1], v=mats[2], relu=1 if relu else 0, **qp)
    B = out_border
    do = abi.GuardedU8(ctx, (n, h + 2 * B, w + 2 * B, c), fill=FILL)
    g.out = wr.map_mat(do.ptr.value, h, w, c, B, o_s8)
    g.out_h, g.out_w, g.out_border = h, w, B
    ds, dp = abi.GuardedU8(ctx, (n * nW, heads, T, T)), abi.GuardedU8(ctx, (n * nW, heads, T, T))
    dacc = abi.GuardedU8(ctx, (n * nW, T, c), np.int32)
    g.scores_dbg_dev, g.probs_dbg_dev, g.acc_dbg_dev = ds.ptr.value, dp.ptr.value, dacc.ptr.value
    win = wr.AttnWindow(map_h=h, map_w=w, win_h=wh, win_w=ww, q_border=borders[0], k_border=borders[1], v_border=borders[2])
    if bias is not None:
        bufs.append(ctx.put(sr.padded_bias(bias)))
    swin = sr.AttnSwin(sh, sw, bufs[-1].ptr.value if bias is not None else None)
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            if entry == "i8ie_attention_swin_u8":
                abi.ck(abi.lib().i8ie_attention_swin_u8(ctx.h, C.byref(g), C.byref(win), C.byref(swin)))
            else:
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


def check(ctx, q, k, v, heads, window, shift, bias, qp, kernel, want=None, **kw):
    if want is None:
        want = sr.attention_u8(q, k, v, heads, window, shift, bias, relu=kw.get("relu", False), **qp)
    S, P, acc, O, names = run(ctx, q, k, v, heads, window, shift, bias, qp, **kw)
    assert names == {kernel: 1}, names
    for name, got, exp in zip(("S", "P", "acc", "O"), (S, P, acc, O), want):
        assert np.array_equal(got, exp), (name, np.argwhere(got != exp)[:4])
    return want


def rand_maps(rng, n, c, h, w):
    return tuple(rng.integers(0, 256, (n, c, h, w), dtype=np.uint8) for _ in range(3))


def form_of(form, rng, heads, window, shift):
    """(shift, bias) of one of the three forms; the bias spans several score steps (s_s = 0.03)"""
    T = window[0] * window[1]
    bias = sr.expand_bias(rng.normal(0, 0.6, ((2 * window[0] - 1) * (2 * window[1] - 1), heads)).astype(f32), window) if form != "shift" else None
    assert bias is None or bias.shape == (heads, T, T)
    return ((0, 0) if form == "bias" else shift), bias


# n, (h, w), window, shift, d, heads, fallback, kernel
CASES = [
    (2, (8, 8), (4, 4), (2, 2), 16, 2, False, "attn_mfma_swin"),      # all four window kinds: inner, last row, last column, corner
    (1, (6, 9), (3, 3), (1, 2), 16, 1, False, "attn_mfma_swin"),      # T = 9: padded bias rows, dword tails
    (1, (14, 14), (7, 7), (3, 3), 32, 3, False, "attn_mfma_swin"),    # Swin's own T = 49
    (1, (16, 24), (8, 12), (4, 6), 16, 1, False, "attn_mfma_swin"),   # T = 96: two K tiles, two query tiles, flags across tiles
    (1, (8, 8), (4, 4), (0, 2), 16, 1, False, "attn_mfma_swin"),      # one-axis shifts
    (1, (8, 8), (4, 4), (3, 0), 16, 1, False, "attn_mfma_swin"),
    (2, (8, 8), (4, 4), (2, 2), 8, 2, False, "attn_direct_swin"),     # d % 16 != 0
    (2, (8, 8), (4, 4), (2, 2), 16, 2, True, "attn_direct_swin"),     # force-fallback
]


@pytest.mark.parametrize("form", ["shift", "bias", "both"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s-%s-d%d%s" % (c[1] + (c[2], c[3], c[4], "-fb" if c[6] else "")))
def test_bytes_of_every_phase(ctx, case, form):
    n, (h, w), window, shift, d, heads, fallback, kernel = case
    rng = np.random.default_rng(h * w + d)
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    shift, bias = form_of(form, rng, heads, window, shift)
    want = check(ctx, q, k, v, heads, window, shift, bias, qp_for(d), kernel, fallback=fallback, relu=form == "both")
    assert len(np.unique(want[0])) > 40 and len(np.unique(want[3])) > 16          # the expected bytes discriminate
    if form != "bias":
        A = np.tile(sr.allowed(h, w, window, shift), (n, 1, 1))[:, None]
        assert not A.all() and (want[1][np.broadcast_to(~A, want[1].shape)] == 0).all()


@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_extremes_of_zero_points_and_bytes(ctx, fallback):
    """Q = K = 255 against zp = 0 (the largest accumulators), with a bias that drives scores past both clamps"""
    kernel = "attn_direct_swin" if fallback else "attn_mfma_swin"
    rng = np.random.default_rng(40)
    n, heads, d, (h, w), window, shift = 1, 2, 16, (8, 8), (4, 4), (2, 2)
    q = k = np.full((n, heads * d, h, w), 255, np.uint8)
    v = rng.integers(0, 256, (n, heads * d, h, w), dtype=np.uint8)
    qp = dict(qp_for(d), zp_q=0, zp_k=0, zp_s=128)
    deq = f32(16 * 255 * 255) * qp["s_q"] * qp["s_k"]
    bias = (rng.choice([-1e4, -4.0, -1.0, 0.0, 1.0, 4.0, 1e4], (heads, 16, 16)) - deq).astype(f32)
    want = check(ctx, q, k, v, heads, window, shift, bias, qp, kernel, fallback=fallback)
    assert (want[0] == 0).any() and (want[0] == 255).any() and len(np.unique(want[0])) >= 5
    for zps in ((0,) * 5, (255,) * 5, (255, 0, 255, 0, 255)):
        check(ctx, q, k, v, heads, window, shift, bias, qp_for(d, zp=zps), kernel, fallback=fallback)


@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_packed_bordered_operands_and_bordered_result(ctx, fallback):
    """a packed 3c operand with border 0 and 1, plain and re-biased; a bordered re-biased result whose border bytes and guards
    survive (run() asserts it); poison in every operand border must never be read"""
    kernel = "attn_direct_swin" if fallback else "attn_mfma_swin"
    rng = np.random.default_rng(50)
    n, heads, d, (h, w), window, shift = 2, 2, 16, (6, 9), (3, 3), (2, 1)
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    bias = form_of("both", rng, heads, window, shift)[1]
    qp = qp_for(d)
    pq = dict(qp, s_k=qp["s_q"], s_v=qp["s_q"], zp_k=qp["zp_q"], zp_v=qp["zp_q"])
    want = sr.attention_u8(q, k, v, heads, window, shift, bias, relu=True, **pq)
    for border, s8 in ((0, False), (1, False), (1, True)):
        check(ctx, q, k, v, heads, window, shift, bias, pq, kernel, want=want, fallback=fallback, packed=True, borders=(border,) * 3, s8=s8,
              relu=True, out_border=border, o_s8=s8)
    want = sr.attention_u8(q, k, v, heads, window, shift, bias, **qp)
    check(ctx, q, k, v, heads, window, shift, bias, qp, kernel, want=want, fallback=fallback, borders=(1, 0, 1), out_border=2, o_s8=True)


def test_equivalences(ctx):
    """shift = 0 and no bias: the bytes of i8ie_attention_window_u8; the whole map as the window, unshifted, with a bias: the
    global definition plus the bias (every key allowed)"""
    rng = np.random.default_rng(60)
    n, heads, d, (h, w) = 2, 2, 16, (8, 8)
    q, k, v = rand_maps(rng, n, heads * d, h, w)
    qp = qp_for(d)
    a = run(ctx, q, k, v, heads, (4, 4), 0, None, qp)
    b = run(ctx, q, k, v, heads, (4, 4), 0, None, qp, entry="i8ie_attention_window_u8")
    assert a[4] == {"attn_mfma_win": 1} and b[4] == {"attn_mfma_win": 1}      # (by definition: the windowed instance itself)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    bias = rng.normal(0, 0.6, (heads, 64, 64)).astype(f32)
    S, P, acc, O = check(ctx, q, k, v, heads, (8, 8), 0, bias, qp, "attn_mfma_swin")
    tq, tk = mr.tokens(q), mr.tokens(k)
    for hd in range(heads):
        cs = slice(hd * d, (hd + 1) * d)
        acc1 = sr.ar.matmul_acc(tq[:, :, cs], qp["zp_q"], tk[:, :, cs], qp["zp_k"], transpose_b=True)
        Sg = sr.biased_scores(acc1, qp["s_q"], qp["s_k"], bias[hd][None], qp["s_s"], qp["zp_s"])
        assert np.array_equal(S[:, hd], Sg) and np.array_equal(P[:, hd], sr.ar.softmax_u8(Sg, qp["s_s"]))


@pytest.mark.parametrize("form", ["shift", "both"])
def test_f32_entry(ctx, form):
    """against the float64 restatement with the tolerance of test_gpu_mha.py's FP32 entry (the same composition plus one add);
    scores_out_dev holds the biased scores before masking, all finite"""
    rng = np.random.default_rng(70)
    n, heads, d, (h, w), window = 2, 2, 5, (6, 8), (3, 4)
    c, T, nW, hw = heads * d, 12, 4, 48
    shift, bias = form_of(form, rng, heads, window, (1, 3))
    q, k, v = (rng.normal(0, 1, (n, c, h, w)).astype(f32) for _ in range(3))
    bufs = [ctx.put(a) for a in (q, k, v)]
    do, dsc = ctx.guarded((n, c, h, w)), ctx.guarded((n * nW, heads, T, T))
    mats = [mr.AttnMat(b.ptr.value, c * hw, hw, 0) for b in bufs]
    g = mr.AttnArgs(b=n, heads=heads, d=d, tq=T, tk=T, q=mats[0], k=mats[1], v=mats[2], out=mr.AttnMat(do.ptr.value, c * hw, hw, 0),
                    out_h=h, out_w=w, scores_out_dev=dsc.ptr.value)
    if bias is not None:
        bufs.append(ctx.put(sr.padded_bias(bias)))
    swin = sr.AttnSwin(shift[0], shift[1], bufs[-1].ptr.value if bias is not None else None)
    abi.ck(abi.lib().i8ie_attention_swin_f32(ctx.h, C.byref(g), C.byref(wr.AttnWindow(map_h=h, map_w=w, win_h=3, win_w=4)), C.byref(swin)))
    got, ok1 = do.read()
    got_s, ok2 = dsc.read()
    assert ok1 and ok2 and abi.GuardedOut.unwritten(got) == 0 and abi.GuardedOut.unwritten(got_s) == 0 and np.isfinite(got_s).all()
    ref_s, ref_o = sr.attention(q, k, v, heads, window, shift, bias)
    assert np.abs(got_s - ref_s).max() < 1e-4 and np.abs(got - ref_o).max() < 1e-4
    assert np.abs(ref_o - wr.attention(q, k, v, heads, window)[1]).max() > 1e-2       # (the shift and the mask matter)
    for dv in bufs + [do, dsc]:
        dv.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_launch_count_and_functional_form(i8ie):
    """conv(c -> 3c) -> Attention(window, shift, bias) -> relu -> conv is three launches; the functional form with the dense
    bias gives the layer's bytes, which are the reference's"""
    rng = np.random.default_rng(81)
    n, c, heads, h, w, window, shift = 3, 32, 2, 8, 8, (4, 4), (2, 2)
    stem0, stem = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128)), support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    qkv = support.conv(i8ie, c, 3 * c, 1, 0, 2, (0.02, 127))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    table = rng.normal(0, 0.5, (49, heads)).astype(f32)
    at = i8ie.Attention(heads, window=window, shift=shift, relative_position_bias=True)
    assert (at.relative_position_bias() == 0).all()
    at.load_relative_position_bias(table)
    at.set_score_qparams(0.04, 140)
    at.set_output_qparams(0.012, 126)
    at.convert()
    x = i8ie.relu(stem(i8ie.relu(stem0(i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, 3, h, w)).astype(f32)), 0.025, 127)))))
    launches = support.counted(lambda: [tail(i8ie.relu(at(qkv(x))))])
    assert launches.get("attn_mfma_swin") == 1 and sum(launches.values()) == 3, launches
    support.assert_no_glue_launches(launches)
    p = qkv(x)
    qp = dict(s_q=f32(0.02), s_k=f32(0.02), s_v=f32(0.02), zp_q=127, zp_k=127, zp_v=127, s_s=f32(0.04), zp_s=140, s_o=f32(0.012), zp_o=126)
    O = sr.attention_u8(p.numpy(), None, None, heads, window, shift, sr.expand_bias(table, window), **qp)[3]
    assert len(np.unique(O)) >= 16 and np.array_equal(i8ie.relu(at(p)).numpy(), np.maximum(O, 126))
    got = i8ie.attention(p, heads=heads, window=window, shift=2, bias=sr.expand_bias(table, window), score_scale=0.04, score_zero_point=140,
                         scale=0.012, zero_point=126)
    assert np.array_equal(got.numpy(), O)


def test_two_swin_blocks_step_by_step(i8ie, tmp_path):
    """the example's chain -- an unshifted and a shifted block, each qkv conv -> Attention(window, shift, bias) -> projection
    -> skip: Module.load routes the tables, prepare / convert run on the device, every attention equals the reference applied to
    the previous step's device bytes, the state dict and a file keep the tables, and a HIP graph replays the eager bytes"""
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(90)
    c, heads, window = 32, 2, (4, 4)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.stem = i8ie.Conv2d(3, c, 3, padding=1)
            for p, shift in (("a_", 0), ("b_", 2)):
                setattr(self, p + "qkv", i8ie.Conv2d(c, 3 * c, 1))
                setattr(self, p + "attn", i8ie.Attention(heads, window=window, shift=shift, relative_position_bias=True))
                setattr(self, p + "proj", i8ie.Conv2d(c, c, 1))
                setattr(self, p + "add", i8ie.Add())

        def steps(self, x):
            out = {}
            x = out["stem"] = self.stem(x)
            for p in ("a_", "b_"):
                y = out[p + "qkv"] = getattr(self, p + "qkv")(x)
                y = out[p + "attn"] = getattr(self, p + "attn")(y)
                x = out[p + "add"] = getattr(self, p + "add")(x, getattr(self, p + "proj")(y))
            return out

        def forward(self, x):
            return self.steps(x)["b_add"]

    net = Net()
    sd = {}
    for name, shape in dict(stem=(c, 3, 3, 3), a_qkv=(3 * c, c, 1, 1), a_proj=(c, c, 1, 1), b_qkv=(3 * c, c, 1, 1), b_proj=(c, c, 1, 1)).items():
        fan = shape[1] * shape[2] * shape[3]
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan)).astype(f32)
        sd[name + ".bias"] = rng.uniform(-0.1, 0.1, shape[0]).astype(f32)
    tables = {p: rng.normal(0, 0.5, (49, heads)).astype(f32) for p in ("a_", "b_")}
    for p in tables:
        sd[p + "attn.relative_position_bias_table"] = tables[p]
    net.load(sd)
    net.prepare()
    net(i8ie.tensor(rng.uniform(-1, 1, (8, 3, 8, 8)).astype(f32)))
    net.convert()
    xf = i8ie.tensor(rng.uniform(-1, 1, (3, 3, 8, 8)).astype(f32))
    x = i8ie.quantize(xf, 1.0 / 128, 128)
    got = {name: (t.numpy(), f32(t.scale), int(t.zero_point)) for name, t in net.steps(x).items()}
    whole = net.forward(x).numpy()
    assert np.array_equal(whole, got["b_add"][0])
    for p, shift in (("a_", 0), ("b_", 2)):
        L = getattr(net, p + "attn")
        pk, s, z = got[p + "qkv"]
        (s_s, zp_s), (s_o, zp_o) = L.score_qparams(), L.output_qparams()
        assert s_s != 1.0 and s_o != 1.0                                    # both observers were fed
        S, P, _, O = sr.attention_u8(pk, None, None, heads, window, shift, sr.expand_bias(tables[p], window), s_q=s, s_k=s, s_v=s, zp_q=z, zp_k=z,
                                     zp_v=z, s_s=f32(s_s), zp_s=zp_s, s_o=f32(s_o), zp_o=zp_o)
        assert np.array_equal(got[p + "attn"][0], O) and len(np.unique(S)) > 30 and len(np.unique(O)) >= 16, p
    state = net.quantized_state_dict()
    assert all(state[p + "attn.relative_position_bias_table"].dtype == f32 and np.array_equal(state[p + "attn.relative_position_bias_table"], tables[p])
               for p in tables)
    other, third = Net(), Net()
    other.load_quantized(state)
    net.save_quantized(str(tmp_path / "swin.npz"))
    third.load_quantized_file(str(tmp_path / "swin.npz"))
    for m in (other, third):
        assert np.array_equal(m.b_attn.relative_position_bias(), tables["b_"]) and np.array_equal(m.forward(x).numpy(), whole)
    gf = GraphedForward(lambda t: net.forward(i8ie.quantize(t, 1.0 / 128, 128)), xf)
    assert np.array_equal(gf().numpy(), whole) and np.array_equal(gf().numpy(), whole)
