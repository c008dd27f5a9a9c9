"""CPU-side checks of the windowed attention: tests/window_ref.py partitions as the header defines and reduces to mha_ref
where it must; the header and the library carry the entries; every argument error is I8IE_ERR_ARG before any device call; the
Python surface refuses what the issue says it refuses, before any device call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
import mha_ref as mr
import support
import window_ref as wr
from support import i8ie  # noqa: F401

f32 = np.float32
QP = dict(s_q=f32(0.05), zp_q=120, s_k=f32(0.04), zp_k=131, s_v=f32(0.03), zp_v=7, s_s=f32(0.35), zp_s=140, s_o=f32(0.02), zp_o=9)

lib = support.lib_fixture(wr)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,window", [((2, 3, 4, 6), (2, 3)), ((1, 5, 14, 7), (7, 7)), ((3, 2, 9, 16), (9, 8)), ((2, 4, 6, 6), 3),
                                          ((1, 2, 4, 4), (1, 1)), ((2, 3, 5, 8), (5, 8)), ((1, 1, 6, 4), (3, 4)), ((1, 2, 4, 6), (4, 2))])
def test_part_round_trips_and_is_torchs_partition(shape, window):
    import torch

    x = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    t = wr.part(x, window)
    wh, ww = wr.pair(window)
    n, c, h, w = shape
    assert t.shape == (n * (h // wh) * (w // ww), wh * ww, c) and np.array_equal(wr.unpart(t, window, shape), x)
    # torch: unfold both spatial axes, windows to the front, pixels of a window row-major, channels last
    u = torch.from_numpy(x).unfold(2, wh, wh).unfold(3, ww, ww)          # [n, c, h / wh, w / ww, wh, ww]
    u = u.permute(0, 2, 3, 4, 5, 1).reshape(-1, wh * ww, c)
    assert np.array_equal(t, u.numpy())
    # and the view form of the same thing
    v = torch.from_numpy(x).view(n, c, h // wh, wh, w // ww, ww).permute(0, 2, 4, 3, 5, 1).reshape(-1, wh * ww, c)
    assert np.array_equal(t, v.numpy())


def test_the_whole_map_as_window_is_the_global_form():
    rng = np.random.default_rng(2)
    n, c, h, w, heads = 2, 12, 3, 5, 3
    q, k, v = (rng.integers(0, 256, (n, c, h, w), dtype=np.uint8) for _ in range(3))
    S, P, acc, O = wr.attention_u8(q, k, v, heads, (h, w), **QP)
    s, p, a, o = mr.attention_u8(mr.tokens(q), mr.tokens(k), mr.tokens(v), heads, **QP)
    assert np.array_equal(S, s) and np.array_equal(P, p) and np.array_equal(acc, a) and np.array_equal(O, mr.pixels(o, h, w))
    assert len(np.unique(S)) > 50 and len(np.unique(O)) > 20   # the expected bytes discriminate
    # packed equals unpacked, and a window is independent of its neighbours
    pq = dict(QP, s_k=QP["s_q"], s_v=QP["s_q"], zp_k=QP["zp_q"], zp_v=QP["zp_q"])
    q, k, v = (rng.integers(0, 256, (n, c, 4, 6), dtype=np.uint8) for _ in range(3))
    whole = wr.attention_u8(q, k, v, heads, (2, 3), **pq)
    for a, b in zip(whole, wr.attention_u8(np.concatenate([q, k, v], axis=1), None, None, heads, (2, 3), **pq)):
        assert np.array_equal(a, b)
    alone = mr.attention_u8(*(mr.tokens(a[1:, :, 2:4, 3:6]) for a in (q, k, v)), heads, **pq)   # image 1, window (1, 1)
    assert np.array_equal(whole[0][7:8], alone[0]) and np.array_equal(whole[3][1:, :, 2:4, 3:6], mr.pixels(alone[3], 2, 3))
    assert not np.array_equal(whole[3], mr.pixels(mr.attention_u8(mr.tokens(q), mr.tokens(k), mr.tokens(v), heads, **pq)[3], 4, 6))


def test_float_restatement_agrees_with_a_float64_torch_composition():
    """Both sides are float64 and differ only in the order of their sums: a score is a sum of d = 8 products of N(0, 1) values
    (|score| < 50 here), an output a convex combination of T = 12 values, so the difference is bounded by about
    (d + T) * 2^-52 * 50 = 2e-13; 1e-12 is asserted."""
    import torch

    rng = np.random.default_rng(3)
    n, heads, d, h, w, wh, ww = 2, 2, 8, 6, 8, 3, 4
    c = heads * d
    q, k, v = (rng.normal(0, 1, (n, c, h, w)) for _ in range(3))
    s, o = wr.attention(q.astype(f32), k.astype(f32), v.astype(f32), heads, (wh, ww))
    tq, tk, tv = (torch.from_numpy(a.astype(f32).astype(np.float64)).view(n, heads, d, h // wh, wh, w // ww, ww)
                  .permute(0, 3, 5, 1, 4, 6, 2).reshape(-1, heads, wh * ww, d) for a in (q, k, v))   # [n * nW, H, T, d]
    ts = tq @ tk.transpose(-1, -2)
    to = torch.softmax(ts, -1) @ tv                                                                   # [n * nW, H, T, d]
    to = to.view(n, h // wh, w // ww, heads, wh, ww, d).permute(0, 3, 6, 1, 4, 2, 5).reshape(n, c, h, w)
    assert s.shape == (n * 4, heads, 12, 12) and np.abs(s).max() < 50
    assert np.abs(s - ts.numpy()).max() < 1e-12 and np.abs(o - to.numpy()).max() < 1e-12


def test_reciprocal_division_is_exact_for_every_window_width():
    """the kernels' j // ww (csrc/i8ie_attention.hip, WindowRows): umulhi(j << 2, ceil(2^30 / ww)), restated in 64-bit integers,
    for every ww in 1..32768 and every token index a staged tile can ask for (j < 32768, and the 63 rows past it)"""
    j = np.arange(32768 + 64, dtype=np.uint64)
    j4 = j << np.uint64(2)
    assert int(j4.max()) < 2 ** 32
    for ww in range(1, 32769):
        m = ((1 << 30) + ww - 1) // ww
        assert m < 2 ** 32
        assert np.array_equal((j4 * np.uint64(m)) >> np.uint64(32), j // np.uint64(ww)), ww


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lib):
    names = abi.declared_symbols()
    for n in ("i8ie_attention_window_u8", "i8ie_attention_window_f32"):
        assert n in names and hasattr(lib, n)
    src = open(abi.HEADER).read()
    assert "typedef struct i8ie_attention_window" in src
    for field in ("map_h", "map_w", "win_h", "win_w", "q_border", "k_border", "v_border"):
        assert field in src


def _good():
    # 2 images of 4 x 6 pixels, H = 2, d = 4, windows of 2 x 3; the pointers are never dereferenced
    g = mr.AttnArgs(b=2, heads=2, d=4, tq=6, tk=6, q=wr.map_mat(4096, 4, 6, 8), k=wr.map_mat(8192, 4, 6, 8), v=wr.map_mat(12288, 4, 6, 8),
                    out=wr.map_mat(16384, 4, 6, 8), out_h=4, out_w=6, s_q=1.0, s_k=1.0, s_v=1.0, s_s=1.0, s_o=1.0)
    return g, wr.AttnWindow(map_h=4, map_w=6, win_h=2, win_w=3)


def _good_f32():
    # the FP32 form: NCHW, the "token" stride is the channel stride h * w = 24
    g, w = _good()
    for which in ("q", "k", "v", "out"):
        m = getattr(g, which)
        m.batch_stride, m.token_stride = 8 * 24, 24
    return g, w


def test_argument_errors_need_no_gpu(lib):
    """every argument error of both entries is I8IE_ERR_ARG before any device call (the ctx is never dereferenced)"""
    u8, f = lib.i8ie_attention_window_u8, lib.i8ie_attention_window_f32
    fake_ctx = C.create_string_buffer(512)  # (never read: each call below fails its argument check first)
    for entry, good in ((u8, _good), (f, _good_f32)):
        g, w = good()
        assert entry(None, C.byref(g), C.byref(w)) == -1
        assert entry(fake_ctx, None, C.byref(w)) == -1 and entry(fake_ctx, C.byref(g), None) == -1
        bad_g = [("b", 0), ("heads", 0), ("d", 0), ("tq", 5), ("tk", 5), ("tq", 24), ("out_h", 0), ("out_h", 2), ("out_w", 3), ("out_border", -1)]
        bad_w = [("map_h", 0), ("map_w", -6), ("win_h", 0), ("win_w", 0), ("win_h", 3), ("win_w", 4), ("win_h", 4), ("map_h", 6),
                 ("q_border", -1), ("k_border", -1), ("v_border", -1)]
        for field, value in bad_g:
            h = mr.AttnArgs.from_buffer_copy(g)
            setattr(h, field, value)
            assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1, field
            assert b"attention_window" in abi.lib().i8ie_last_error() or b"check_window" in abi.lib().i8ie_last_error()
        for field, value in bad_w:
            x = wr.AttnWindow.from_buffer_copy(w)
            setattr(x, field, value)
            assert entry(fake_ctx, C.byref(g), C.byref(x)) == -1, field
        for which in ("q", "k", "v", "out"):
            h = mr.AttnArgs.from_buffer_copy(g)
            getattr(h, which).token_stride = 7           # below heads * d = 8, and below h * w = 24
            assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1, which
            h = mr.AttnArgs.from_buffer_copy(g)
            getattr(h, which).ptr = None
            assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1, which
            h = mr.AttnArgs.from_buffer_copy(g)
            getattr(h, which).batch_stride = -1
            assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1, which
    # a border above 65535 pixels, and sizes whose product does not fit: refused, never multiplied out
    for entry, good in ((u8, _good), (f, _good_f32)):
        g, w = good()
        for field in ("q_border", "k_border", "v_border"):
            x = wr.AttnWindow.from_buffer_copy(w)
            setattr(x, field, 65536)
            assert entry(fake_ctx, C.byref(g), C.byref(x)) == -1, field
        h = mr.AttnArgs.from_buffer_copy(g)
        h.out_border = 65536
        assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1
        for b, heads, d in ((2 ** 31 - 1, 2 ** 31 - 1, 1), (2 ** 31 - 1, 1, 4), (2 ** 20, 2 ** 10, 1)):
            h = mr.AttnArgs.from_buffer_copy(g)
            h.b, h.heads, h.d = b, heads, d
            assert entry(fake_ctx, C.byref(h), C.byref(w)) == -1, (b, heads, d)
            assert b"too many query rows" in abi.lib().i8ie_last_error() or b"stride" in abi.lib().i8ie_last_error()
    # more than 32768 pixels in a window (tq == tk == win_h * win_w holds, so it is that rule which refuses)
    g, w = _good()
    g.tq = g.tk = 256 * 129
    g.out_h, g.out_w = 256, 129
    big = wr.AttnWindow(map_h=256, map_w=129, win_h=256, win_w=129)
    assert u8(fake_ctx, C.byref(g), C.byref(big)) == -1 and b"32768" in abi.lib().i8ie_last_error()
    # the u8 entry: scales, and the FP32 entry's field
    g, w = _good()
    for field, value in (("s_s", 0.0), ("s_s", -1.0), ("s_o", 0.0), ("s_o", float("nan")), ("s_q", float("inf")), ("s_k", float("nan")),
                         ("s_v", float("inf")), ("scores_out_dev", 4096)):
        h = mr.AttnArgs.from_buffer_copy(g)
        setattr(h, field, value)
        assert u8(fake_ctx, C.byref(h), C.byref(w)) == -1, field
    # the FP32 entry refuses every INT8-only field
    g, w = _good_f32()
    for field, value in (("relu", 1), ("out_border", 1), ("scores_dbg_dev", 4096), ("probs_dbg_dev", 4096), ("acc_dbg_dev", 4096)):
        h = mr.AttnArgs.from_buffer_copy(g)
        setattr(h, field, value)
        assert f(fake_ctx, C.byref(h), C.byref(w)) == -1, field
    for field in ("q_border", "k_border", "v_border"):
        x = wr.AttnWindow.from_buffer_copy(w)
        setattr(x, field, 1)
        assert f(fake_ctx, C.byref(g), C.byref(x)) == -1, field
    h = mr.AttnArgs.from_buffer_copy(g)
    h.k.s8 = 1
    assert f(fake_ctx, C.byref(h), C.byref(w)) == -1


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_window_argument_rules_come_before_any_device_call(i8ie):
    """TypeError for a window that is no int or pair of ints; RuntimeError from the shape rules; FP32 tensors made on the host
    never reach a device here"""
    import _CXX_i8ie as cx

    t = lambda *shape: i8ie.tensor(np.zeros(shape, f32))  # noqa: E731
    for bad in (2.0, "4", (2,), (2, 3, 4), (2, 3.0), [2, None], True, (True, 2), {2, 3}):
        with pytest.raises(TypeError):
            i8ie.Attention(2, window=bad)
        with pytest.raises(TypeError):
            i8ie.attention(t(1, 12, 4, 6), heads=2, window=bad)
    for ok, want in ((2, (2, 2)), ((2, 3), (2, 3)), ([4, 1], (4, 1)), (np.int64(3), (3, 3))):
        assert i8ie.Attention(2, window=ok).window == want
    assert hasattr(cx, "_attention_window") and hasattr(cx.Attention, "_set_window")
    at = i8ie.Attention(2, window=(2, 3))
    cases = [lambda: at(t(1, 4 * 6, 12)),                                  # a rank-3 operand
             lambda: at(t(1, 4, 4, 6), t(1, 24, 4), t(1, 24, 4)),         # ... among rank-4 ones
             lambda: at(t(1, 12, 4, 5)),                                   # ww does not divide w
             lambda: at(t(1, 12, 3, 6)),                                   # wh does not divide h
             lambda: at(t(1, 4, 4, 6), t(1, 4, 2, 3), t(1, 4, 2, 3)),     # k / v maps of another size
             lambda: at(t(1, 4, 4, 6), t(1, 4, 4, 6), t(1, 4, 6, 4)),
             lambda: at(t(1, 4, 4, 6), t(2, 4, 4, 6), t(2, 4, 4, 6)),     # batch
             lambda: at(t(1, 4, 4, 6), t(1, 6, 4, 6), t(1, 6, 4, 6)),     # channels differ
             lambda: at(t(1, 5, 4, 6), t(1, 5, 4, 6), t(1, 5, 4, 6)),     # c != heads * d
             lambda: at(t(1, 7, 4, 6)),                                    # packed: 7 channels are not 3 * 2 * d
             lambda: i8ie.attention(t(1, 3, 256, 129), heads=1, window=(256, 129)),   # 33024 pixels in a window
             lambda: i8ie.attention(t(1, 12, 4, 6), heads=2, window=0),
             lambda: i8ie.attention(t(1, 12, 4, 6), heads=2, window=(2, -3)),
             lambda: i8ie.Attention(2, window=(0, 2))]
    for bad in cases:
        with pytest.raises(RuntimeError):
            bad()
    for bad in (lambda: at(t(1, 4, 4, 6), t(1, 4, 4, 6)), lambda: i8ie.attention(t(1, 12, 4, 6), heads=2, window=2, scale=1.0)):
        with pytest.raises(TypeError):
            bad()
    assert "window" in i8ie.Attention.__doc__ and "window" in i8ie.attention.__doc__


def test_window_none_is_todays_attention(i8ie):
    """Attention(2) and Attention(2, window=None) are the same layer: same state, same refusals, same saved keys"""
    t = lambda *shape: i8ie.tensor(np.zeros(shape, f32))  # noqa: E731
    a, b = i8ie.Attention(2), i8ie.Attention(2, window=None)
    assert a.window is None and b.window is None and a.heads == b.heads == 2 and b.layer.heads() == 2
    assert a.output_qparams() == b.output_qparams() == (1.0, 0) and a.score_qparams() == b.score_qparams() == (1.0, 0)
    for at in (a, b):
        with pytest.raises(RuntimeError):
            at(t(1, 4, 7))                # the global form's packed rule; a rank-3 operand is not refused for its rank
        with pytest.raises(RuntimeError, match="3 \\* heads"):
            at(t(1, 7, 4, 6))
        with pytest.raises(TypeError):
            at(t(1, 4, 6), t(1, 4, 6))

    class Net(i8ie.Module):
        def __init__(self, window):
            super().__init__()
            self.attn = i8ie.Attention(2, window=window)

    sds = []
    for window in (None, (2, 2)):          # the window is a constructor argument, not state
        net = Net(window)
        net.attn.layer.load_quantized(0.25, 7, 0.5, 131)
        sds.append(net.quantized_state_dict())
        assert sorted(sds[-1]) == ["attn.qparams", "attn.score_qparams"]
    assert all(np.array_equal(sds[0][k], sds[1][k]) for k in sds[0])
    other = Net((2, 2))
    other.load_quantized(sds[0])
    assert other.attn.score_qparams() == (0.5, 131) and other.attn.window == (2, 2)
