"""narrow / split / chunk / channel_shuffle / pixel_shuffle / pixel_unshuffle restated for the tests.
A helper module, not a conftest.

The reference has none of these ops.  The definitions are the ones of include/i8ie_hip.h, written as numpy index expressions
on the logical NCHW array ([m, f] rows for narrow, split and chunk too); a relu is maximum(q, zp) on the result.  The case
lists of tests/test_gpu_rearrange.py live here so that tests/test_rearrange_host.py can check, without a GPU, that every
class of case is still in them; the new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

NARROW, CHANNEL_SHUFFLE, PIXEL_SHUFFLE, PIXEL_UNSHUFFLE = 0, 1, 2, 3
KIND_NAME = {NARROW: "narrow", CHANNEL_SHUFFLE: "channel_shuffle", PIXEL_SHUFFLE: "pixel_shuffle", PIXEL_UNSHUFFLE: "pixel_unshuffle"}
MAX_FACTOR = 8


def _relu(q, relu, zp):
    return np.maximum(q, np.asarray(zp, q.dtype)) if relu else q


def narrow(x, start, length, relu=False, zp=0):
    x = np.asarray(x)
    assert x.ndim in (2, 4) and 0 <= start and 1 <= length and start + length <= x.shape[1]
    return _relu(np.ascontiguousarray(x[:, start:start + length]), relu, zp)


def split_sizes(c, sizes):
    """torch.split's rule: an int -> parts of that size, the last one smaller; a list -> itself (it must sum to c)"""
    if isinstance(sizes, (list, tuple)):
        assert sum(sizes) == c and all(s > 0 for s in sizes)
        return list(sizes)
    assert sizes > 0
    return [min(sizes, c - at) for at in range(0, c, sizes)]


def split(x, sizes):
    out, at = [], 0
    for s in split_sizes(np.asarray(x).shape[1], sizes):
        out.append(narrow(x, at, s))
        at += s
    return out


def chunk(x, chunks):
    assert chunks > 0
    return split(x, -(-np.asarray(x).shape[1] // chunks))


def channel_shuffle(x, groups, relu=False, zp=0):
    """out[:, j * g + i] = in[:, i * (c / g) + j]"""
    x = np.asarray(x)
    n, c, h, w = x.shape
    assert groups >= 1 and c % groups == 0
    cg = c // groups
    co = np.arange(c)
    return _relu(np.ascontiguousarray(x[:, (co % groups) * cg + co // groups]), relu, zp)


def pixel_shuffle(x, r, relu=False, zp=0):
    """out[n, co, h * r + i, w * r + j] = in[n, co * r * r + i * r + j, h, w]"""
    x = np.asarray(x)
    n, c, h, w = x.shape
    assert 1 <= r <= MAX_FACTOR and c % (r * r) == 0
    co, Y, X = np.arange(c // (r * r))[:, None, None], np.arange(h * r)[None, :, None], np.arange(w * r)[None, None, :]
    return _relu(np.ascontiguousarray(x[:, co * r * r + (Y % r) * r + X % r, Y // r, X // r]), relu, zp)


def pixel_unshuffle(x, r, relu=False, zp=0):
    """out[n, ci * r * r + i * r + j, y, x] = in[n, ci, y * r + i, x * r + j]"""
    x = np.asarray(x)
    n, c, h, w = x.shape
    assert 1 <= r <= MAX_FACTOR and h % r == 0 and w % r == 0
    co, Y, X = np.arange(c * r * r)[:, None, None], np.arange(h // r)[None, :, None], np.arange(w // r)[None, None, :]
    return _relu(np.ascontiguousarray(x[:, co // (r * r), Y * r + (co // r) % r, X * r + co % r]), relu, zp)


def apply(kind, x, p0, p1=0, relu=False, zp=0):
    if kind == NARROW:
        return narrow(x, p0, p1, relu, zp)
    return {CHANNEL_SHUFFLE: channel_shuffle, PIXEL_SHUFFLE: pixel_shuffle, PIXEL_UNSHUFFLE: pixel_unshuffle}[kind](x, p0, relu, zp)


def output_shape(kind, p0, p1, n, c, h, w):
    if kind == NARROW:
        return (n, p1, h, w)
    if kind == CHANNEL_SHUFFLE:
        return (n, c, h, w)
    if kind == PIXEL_SHUFFLE:
        return (n, c // (p0 * p0), h * p0, w * p0)
    return (n, c * p0 * p0, h // p0, w // p0)


def channel_bytes(shape, seed=0):
    """u8 [n, c, h, w] in which no wrong index can cancel: inside a pixel every channel position holds its own byte (channel
    ch holds ch * 37 + 11 * pixel mod 256 with 37 odd, so 256 consecutive channels differ), pixels differ by the 11 * pixel
    term, and images by a random byte"""
    n, c, h, w = shape
    ch = np.arange(c, dtype=np.int64)[None, :, None, None]
    pix = (np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :])[None, None]
    img = np.random.default_rng(seed).integers(0, 256, (n, 1, 1, 1), dtype=np.int64)
    return ((ch * 37 + pix * 11 + img) % 256).astype(np.uint8)


# ---- the case lists of tests/test_gpu_rearrange.py -----------------------------------------------------------------------------
FAST, DIRECT = "chanperm_u8_nhwc", "rearrange_u8_direct"
NARROW_KERNEL = "narrow_u8_nhwc"
NARROW_CASES = [(32, 16, 16), (32, 0, 16), (40, 4, 20), (116, 58, 58), (35, 3, 5), (16, 0, 16), (20, 19, 1),
                (24, 8, 8)]                                                                                  # (c, start, length)
NARROW_MAPS = [(1, 3, 5), (5, 3, 5), (1, 1, 1), (5, 1, 1)]                                                   # (n, h, w)
NARROW_ROWS = (5, 35)
SHUFFLE_CASES = [(32, 2), (64, 4), (48, 3), (116, 2), (20, 5), (35, 7), (16, 16), (16, 1)]                   # (c, g)
SHUFFLE_MAPS = [(1, 3, 5), (5, 3, 5)]
PIXEL_CASES = [(16, 2), (16, 4), (4, 3), (3, 2), (2, 3), (1, 8), (16, 1)]                                     # (c_out, r)
PIXEL_MAP = (2, 3)                                                                                           # pixel_shuffle's input h, w
ZPS = (0, 127, 255)
IN_BORDERS, OUT_BORDERS = (0, 1, 3), (0, 1, 2)
# one fast and one direct case per op for the layout matrix: (kind, c, p0, p1, h, w)
LAYOUT_CASES = [(NARROW, 32, 16, 16, 3, 5), (NARROW, 35, 3, 5, 3, 5),
                (CHANNEL_SHUFFLE, 32, 2, 0, 3, 5), (CHANNEL_SHUFFLE, 20, 5, 0, 3, 5),
                (PIXEL_SHUFFLE, 64, 2, 0, 2, 3), (PIXEL_SHUFFLE, 36, 3, 0, 2, 3),
                (PIXEL_UNSHUFFLE, 16, 2, 0, 4, 6), (PIXEL_UNSHUFFLE, 3, 2, 0, 4, 6)]


def narrow_item(c, start, length):
    """the item width narrow_u8_nhwc takes on 16-byte aligned buffers"""
    for v in (16, 8, 4, 2):
        if c % v == 0 and start % v == 0 and length % v == 0:
            return v
    return 1


def expected_kernel(kind, c, p0, p1=0):
    """the kernel the NHWC entry takes on 16-byte aligned buffers without the force-fallback option"""
    if kind == NARROW:
        return NARROW_KERNEL
    oc = output_shape(kind, p0, p1, 1, c, p0 * 8, p0 * 8)[1]
    return FAST if c % 16 == 0 and oc % 16 == 0 else DIRECT


# ---- ctypes signatures of the new entry points -----------------------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8


def bind(lib):
    lib.i8ie_rearrange_output_shape.argtypes = [_I] * 7 + [C.POINTER(_I)]
    lib.i8ie_rearrange_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_B]
    lib.i8ie_rearrange_u8.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_rearrange_f32.argtypes = [_P, _P, _P] + [_I] * 7
    for f in (lib.i8ie_rearrange_output_shape, lib.i8ie_rearrange_u8_nhwc, lib.i8ie_rearrange_u8, lib.i8ie_rearrange_f32):
        f.restype = _I
    return lib
