"""The shifted-window attention without a GPU: the reference's mask against Swin's published construction and against the
wrap-flag form the kernels use, the table expansion against Swin's relative_position_index gather, the argument rules of the
C-ABI and of the Python surface, and shift = 0, bias = None against the windowed reference."""
import ctypes as C

import numpy as np
import pytest

import abi
import mha_ref as mr
import support
import swin_ref as sr
import window_ref as wr
from support import i8ie  # noqa: F401

f32 = np.float32
lib = support.lib_fixture(sr)

MASKS = [(8, 8, (4, 4), (2, 2)), (6, 9, (3, 3), (1, 2)), (14, 14, (7, 7), (3, 3)), (16, 24, (8, 12), (4, 6)), (8, 8, (4, 4), (0, 2)),
         (8, 8, (4, 4), (3, 0)), (8, 8, (4, 4), (0, 0)), (4, 12, (4, 4), (3, 1)), (8, 8, (8, 8), (5, 7))]


@pytest.mark.parametrize("h,w,window,shift", MASKS)
def test_mask_is_swins_and_is_the_wrap_flag_form(h, w, window, shift):
    """Swin's construction: region ids from the three slices per axis on an h x w image (one slice for an unshifted axis),
    partitioned into windows, masked where id_i != id_j"""
    import torch

    (wh, ww), (sh, sw) = window, shift
    slices = lambda win, s: (slice(0, -win), slice(-win, -s), slice(-s, None)) if s else (slice(None),)  # noqa: E731
    img, cnt = torch.zeros(h, w), 0
    for ys in slices(wh, sh):
        for xs in slices(ww, sw):
            img[ys, xs] = cnt
            cnt += 1
    ids = img.view(h // wh, wh, w // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)
    swin = ((ids.unsqueeze(1) - ids.unsqueeze(2)) == 0).numpy()
    got = sr.allowed(h, w, window, shift)
    assert np.array_equal(got, swin) and np.array_equal(got, sr.allowed_by_wrap(h, w, window, shift))
    assert got[:, np.arange(wh * ww), np.arange(wh * ww)].all()          # A(i) contains i
    assert (not got.all()) == (shift != (0, 0))


@pytest.mark.parametrize("wh,ww,heads", [(4, 4, 2), (3, 3, 1), (7, 7, 3), (8, 12, 2), (1, 5, 2)])
def test_relative_position_bias_is_swins_gather(lib, wh, ww, heads):
    import torch

    T, T4 = wh * ww, (wh * ww + 3) // 4 * 4
    table = np.random.default_rng(wh * ww).normal(0, 1, ((2 * wh - 1) * (2 * ww - 1), heads)).astype(f32)
    coords = torch.stack(torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    want = torch.from_numpy(table)[rel.sum(-1).view(-1)].view(T, T, heads).permute(2, 0, 1).numpy()
    out = np.full((heads, T, T4), np.nan, f32)
    assert lib.i8ie_relative_position_bias(table.ctypes.data, wh, ww, heads, out.ctypes.data) == 0
    assert support.same_bits(out[:, :, :T], want) and (out[:, :, T:] == 0).all()
    assert support.same_bits(sr.padded_bias(sr.expand_bias(table, (wh, ww))), out)
    assert lib.i8ie_relative_position_bias(None, wh, ww, heads, out.ctypes.data) == -1
    assert lib.i8ie_relative_position_bias(table.ctypes.data, 0, ww, heads, out.ctypes.data) == -1


def test_argument_errors_need_no_gpu(lib):
    """what the two entries add to the windowed rules: I8IE_ERR_ARG before any device call (the ctx is never dereferenced)"""
    fake_ctx = C.create_string_buffer(512)
    g = mr.AttnArgs(b=2, heads=2, d=4, tq=6, tk=6, q=wr.map_mat(4096, 4, 6, 8), k=wr.map_mat(8192, 4, 6, 8), v=wr.map_mat(12288, 4, 6, 8),
                    out=wr.map_mat(16384, 4, 6, 8), out_h=4, out_w=6, s_q=1.0, s_k=1.0, s_v=1.0, s_s=1.0, s_o=1.0)
    w = wr.AttnWindow(map_h=4, map_w=6, win_h=2, win_w=3)
    for entry in (lib.i8ie_attention_swin_u8, lib.i8ie_attention_swin_f32):
        if entry is lib.i8ie_attention_swin_f32:       # NCHW: the "token" stride is the channel stride h * w = 24
            for which in ("q", "k", "v", "out"):
                m = getattr(g, which)
                m.batch_stride, m.token_stride = 8 * 24, 24
        ok = sr.AttnSwin(1, 2, None)
        assert entry(None, C.byref(g), C.byref(w), C.byref(ok)) == -1 and entry(fake_ctx, C.byref(g), C.byref(w), None) == -1
        assert entry(fake_ctx, None, C.byref(w), C.byref(ok)) == -1 and entry(fake_ctx, C.byref(g), None, C.byref(ok)) == -1
        for sh, sw in ((2, 0), (0, 3), (-1, 0), (0, -1), (5, 5)):
            assert entry(fake_ctx, C.byref(g), C.byref(w), C.byref(sr.AttnSwin(sh, sw, None))) == -1, (sh, sw)
            assert b"shift" in abi.lib().i8ie_last_error()
        bad = wr.AttnWindow(map_h=4, map_w=6, win_h=3, win_w=3)                 # the windowed rules still hold
        assert entry(fake_ctx, C.byref(g), C.byref(bad), C.byref(ok)) == -1


def test_surface_argument_rules(i8ie):
    t = i8ie.tensor(np.zeros((1, 12, 4, 6), f32))
    for bad in (1.0, "1", (1,), (1, 2, 3), True, None):
        with pytest.raises(TypeError):
            i8ie.Attention(2, window=(2, 3), shift=bad)
        with pytest.raises(TypeError):
            i8ie.attention(t, heads=2, window=(2, 3), shift=bad)
    for kw in (dict(shift=1), dict(shift=(0, 1)), dict(relative_position_bias=True)):
        with pytest.raises(RuntimeError):
            i8ie.Attention(2, **kw)
    with pytest.raises(RuntimeError):
        i8ie.attention(t, heads=2, shift=1)
    with pytest.raises(RuntimeError):
        i8ie.attention(t, heads=2, bias=np.zeros((2, 6, 6), f32))
    for shift in ((2, 0), (0, 3), -1):
        with pytest.raises(RuntimeError):
            i8ie.Attention(2, window=(2, 3), shift=shift)
    assert i8ie.Attention(2, window=(2, 3), shift=1).shift == (1, 1) and i8ie.Attention(2, window=4).shift == (0, 0)
    with pytest.raises(RuntimeError):
        i8ie.Attention(2, window=(2, 3)).load_relative_position_bias(np.zeros((15, 2), f32))


def test_no_shift_and_no_bias_is_the_windowed_reference():
    rng = np.random.default_rng(3)
    q, k, v = (rng.integers(0, 256, (2, 8, 6, 9), dtype=np.uint8) for _ in range(3))
    s = f32(0.01)
    qp = dict(s_q=s, zp_q=120, s_k=s, zp_k=131, s_v=f32(0.04), zp_v=125, s_s=f32(0.03), zp_s=140, s_o=f32(0.01), zp_o=128)
    for got, want in zip(sr.attention_u8(q, k, v, 2, (3, 3), **qp), wr.attention_u8(q, k, v, 2, (3, 3), **qp)):
        assert np.array_equal(got, want)
