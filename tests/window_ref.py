"""numpy restatement of the windowed attention (include/i8ie_hip.h, i8ie_attention_window_u8): part / unpart of a map into
its non-overlapping windows, and the definition unpart(attention(part(q), part(k), part(v))) through tests/mha_ref.py, which
stays the only statement of the arithmetic.  Also the ctypes side of the window descriptor.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import mha_ref as mr

MAX_WINDOW = 32768   # pixels in a window: the second product's k


def pair(window):
    return (window, window) if isinstance(window, int) else tuple(window)


def part(x, window):
    """[n, c, h, w] -> [n * (h / wh) * (w / ww), wh * ww, c]: the window index counts (image, wy, wx), token j of a window is
    pixel (wy * wh + j // ww, wx * ww + j % ww)"""
    wh, ww = pair(window)
    n, c, h, w = x.shape
    assert h % wh == 0 and w % ww == 0
    out = np.empty((n * (h // wh) * (w // ww), wh * ww, c), x.dtype)
    s = 0
    for i in range(n):
        for wy in range(h // wh):
            for wx in range(w // ww):
                for j in range(wh * ww):
                    out[s, j] = x[i, :, wy * wh + j // ww, wx * ww + j % ww]
                s += 1
    return out


def unpart(t, window, shape):
    """the inverse of part: [n * nW, wh * ww, c] -> `shape` = (n, c, h, w)"""
    wh, ww = pair(window)
    n, c, h, w = shape
    assert t.shape == (n * (h // wh) * (w // ww), wh * ww, c)
    x = np.empty(shape, t.dtype)
    s = 0
    for i in range(n):
        for wy in range(h // wh):
            for wx in range(w // ww):
                for j in range(wh * ww):
                    x[i, :, wy * wh + j // ww, wx * ww + j % ww] = t[s, j]
                s += 1
    return x


def split_packed(qkv):
    """q, k, v of a packed [n, 3c, h, w] map: its thirds along the channel axis"""
    c = qkv.shape[1] // 3
    assert qkv.shape[1] == 3 * c
    return qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]


def attention_u8(q, k, v, heads, window, relu=False, **qp):
    """q, k, v [n, c, h, w] u8 (k = v = None: q is packed [n, 3c, h, w]).  Returns mha_ref's (S [n * nW, H, T, T],
    P [n * nW, H, T, T], acc [n * nW, T, c], O) with O moved back to [n, c, h, w]."""
    if k is None:
        q, k, v = split_packed(q)
    S, P, acc, O = mr.attention_u8(part(q, window), part(k, window), part(v, window), heads, relu=relu, **qp)
    return S, P, acc, unpart(O, window, q.shape)


def attention(q, k, v, heads, window):
    """float64: (scores [n * nW, H, T, T], out [n, c, h, w])"""
    if k is None:
        q, k, v = split_packed(q)
    s, o = mr.attention(part(q, window), part(k, window), part(v, window), heads)
    return s, unpart(o, window, q.shape)


# ---- ctypes ----------------------------------------------------------------------------------------------------------
class AttnWindow(C.Structure):
    """i8ie_attention_window"""
    _fields_ = [("map_h", C.c_int), ("map_w", C.c_int), ("win_h", C.c_int), ("win_w", C.c_int),
                ("q_border", C.c_int), ("k_border", C.c_int), ("v_border", C.c_int)]


def bind(lib):
    mr.bind(lib)
    for name in ("i8ie_attention_window_u8", "i8ie_attention_window_f32"):
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(mr.AttnArgs), C.POINTER(AttnWindow)]
    return lib


def map_mat(ptr, h, w, channels, border=0, s8=False, offset=0):
    """a channels-last map [n][h + 2B][w + 2B][channels] at ptr, columns from byte `offset`"""
    return mr.AttnMat(ptr + offset, (h + 2 * border) * (w + 2 * border) * channels, channels, 1 if s8 else 0)
