"""numpy restatement of the shifted-window attention with a relative position bias (include/i8ie_hip.h,
i8ie_attention_swin_u8): roll, part, per (window, head) the accumulators, the biased score sequence in np.float32, the masked
softmax through attention_ref.softmax_u8 on the allowed subsequence, the second product, unpart, roll back; Swin's table
expansion; the float64 form; the ctypes side of the descriptor.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import attention_ref as ar
import mha_ref as mr
import orc
import window_ref as wr

f32 = np.float32


def roll(x, shift, back=False):
    """[n, c, h, w] rolled by (-sh, -sw): pixel (y, x) of the result is pixel ((y + sh) % h, (x + sw) % w); back: the inverse"""
    sh, sw = wr.pair(shift)
    return np.roll(x, (sh, sw) if back else (-sh, -sw), axis=(2, 3))


def region_classes(n, win, s):
    """Swin's region class of every shifted coordinate of an axis of length n: 0 below n - win, 1 below n - s, else 2"""
    c = np.arange(n)
    return np.where(c < n - win, 0, np.where(c < n - s, 1, 2)) if s else np.zeros(n, np.int64)


def allowed(h, w, window, shift):
    """bool [nW, T, T]: query i of window (wy, wx) may attend key j iff their region classes agree on both axes"""
    (wh, ww), (sh, sw) = wr.pair(window), wr.pair(shift)
    ids = region_classes(h, wh, sh)[:, None] * 3 + region_classes(w, ww, sw)[None, :]
    t = wr.part(ids[None, None].astype(np.int64), window)[:, :, 0]          # [nW, T]
    return t[:, :, None] == t[:, None, :]


def allowed_by_wrap(h, w, window, shift):
    """the same set from the wrap flags: (ly >= ylim, lx >= xlim) of i and j are equal, ylim = wh - sh in the last window row
    and wh elsewhere, xlim likewise"""
    (wh, ww), (sh, sw) = wr.pair(window), wr.pair(shift)
    j = np.arange(wh * ww)
    out = []
    for wy in range(h // wh):
        for wx in range(w // ww):
            ylim = wh - sh if wy == h // wh - 1 else wh
            xlim = ww - sw if wx == w // ww - 1 else ww
            flags = (j // ww >= ylim) * 2 + (j % ww >= xlim)
            out.append(flags[:, None] == flags[None, :])
    return np.stack(out)


def expand_bias(table, window):
    """Swin's table [(2 wh - 1)(2 ww - 1), heads] -> B [heads, T, T]"""
    wh, ww = wr.pair(window)
    j = np.arange(wh * ww)
    ly, lx = j // ww, j % ww
    idx = (ly[:, None] - ly[None, :] + wh - 1) * (2 * ww - 1) + (lx[:, None] - lx[None, :] + ww - 1)
    return np.ascontiguousarray(np.asarray(table, f32)[idx].transpose(2, 0, 1))


def padded_bias(bias):
    """[heads, T, T] -> the C-ABI's [heads, T, roundup(T, 4)], the padding zero"""
    H, T, _ = bias.shape
    out = np.zeros((H, T, (T + 3) // 4 * 4), f32)
    out[:, :, :T] = bias
    return out


def biased_scores(acc, s_q, s_k, bias, s_s, zp_s):
    """down_scale's sequence with one more fp32 add, every step one np.float32 operation"""
    deq = (acc.astype(f32) * f32(s_q)) * f32(s_k)
    v = (deq + bias.astype(f32)) / f32(s_s) + f32(zp_s)
    return np.where(v >= 255, 255, np.where(v < 0, 0, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)


def attention_u8(q, k, v, heads, window, shift=0, bias=None, relu=False, *, s_q, zp_q, s_k, zp_k, s_v, zp_v, s_s, zp_s, s_o, zp_o):
    """q, k, v [n, c, h, w] u8 (k = v = None: q is packed).  bias: None or [heads, T, T].  Returns (S, P [n * nW, H, T, T],
    acc [n * nW, T, c], O [n, c, h, w]); S holds the biased score of every (i, j), masked or not."""
    if k is None:
        q, k, v = wr.split_packed(q)
    n, c, h, w = q.shape
    A = allowed(h, w, window, shift)
    nW = A.shape[0]
    pq, pk, pv = (wr.part(roll(a, shift), window) for a in (q, k, v))
    b, T, _ = pq.shape
    d = c // heads
    S, P = np.empty((b, heads, T, T), np.uint8), np.zeros((b, heads, T, T), np.uint8)
    acc, O = np.empty((b, T, c), np.int32), np.empty((b, T, c), np.uint8)
    for hd in range(heads):
        cs = slice(hd * d, (hd + 1) * d)
        if bias is None:
            S[:, hd] = ar.matmul_u8(pq[:, :, cs], zp_q, s_q, pk[:, :, cs], zp_k, s_k, s_s, zp_s, transpose_b=True)
        else:
            S[:, hd] = biased_scores(ar.matmul_acc(pq[:, :, cs], zp_q, pk[:, :, cs], zp_k, transpose_b=True), s_q, s_k, bias[hd][None], s_s, zp_s)
        for s in range(b):
            for i in range(T):
                idx = np.flatnonzero(A[s % nW, i])
                P[s, hd, i, idx] = ar.softmax_u8(S[s, hd, i, idx], s_s)
        acc[:, :, cs] = ar.matmul_acc(P[:, hd], 0, pv[:, :, cs], zp_v)
        o = orc.down_scale(acc[:, :, cs], mr.P_SCALE, s_v, s_o, zp_o)
        O[:, :, cs] = np.maximum(o, np.uint8(zp_o)) if relu else o
    return S, P, acc, roll(wr.unpart(O, window, q.shape), shift, back=True)


def attention(q, k, v, heads, window, shift=0, bias=None):
    """float64: (biased scores before masking [n * nW, H, T, T], out [n, c, h, w])"""
    if k is None:
        q, k, v = wr.split_packed(q)
    n, c, h, w = q.shape
    A = allowed(h, w, window, shift)
    pq, pk, pv = (np.asarray(wr.part(roll(a, shift), window), np.float64) for a in (q, k, v))
    b, T, _ = pq.shape
    d = c // heads
    qh, kh, vh = (a.reshape(b, T, heads, d).transpose(0, 2, 1, 3) for a in (pq, pk, pv))
    s = np.einsum("bhid,bhjd->bhij", qh, kh)
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[None]
    mask = np.tile(A, (n, 1, 1))[:, None]
    p = ar.softmax(np.where(mask, s, -np.inf))
    o = np.einsum("bhij,bhjd->bhid", p, vh).transpose(0, 2, 1, 3).reshape(b, T, c)
    return s, roll(wr.unpart(o, window, q.shape), shift, back=True)


# ---- ctypes ----------------------------------------------------------------------------------------------------------
class AttnSwin(C.Structure):
    """i8ie_attention_swin"""
    _fields_ = [("shift_h", C.c_int), ("shift_w", C.c_int), ("bias_dev", C.c_void_p)]


def bind(lib):
    wr.bind(lib)
    for name in ("i8ie_attention_swin_u8", "i8ie_attention_swin_f32"):
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(mr.AttnArgs), C.POINTER(wr.AttnWindow), C.POINTER(AttnSwin)]
    lib.i8ie_relative_position_bias.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib
