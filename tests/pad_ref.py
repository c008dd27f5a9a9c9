"""pad (constant, reflect, replicate, circular) and crop restated for the tests.  A helper module, not
a conftest.

The reference has no such op.  The definition is the index rule of include/i8ie_hip.h ("Spatial padding"), written out per
axis as a loop over the output indices -- not a call to np.pad: per axis of length L with amounts (before, after), output
index o reads input index i = o - before, and outside [0, L) the fill value (constant), -i or 2 (L - 1) - i (reflect), the
edge pixel (replicate), i + L or i - L (circular).  A relu is maximum(q, zp) on the result, fill bytes included.  The case
lists of tests/test_gpu_pad.py live here so that tests/test_pad_host.py can check, without a GPU, that every class of case is
still in them; the new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

CONSTANT, REFLECT, REPLICATE, CIRCULAR = 0, 1, 2, 3
MODES = (CONSTANT, REFLECT, REPLICATE, CIRCULAR)
MODE_NAME = {CONSTANT: "constant", REFLECT: "reflect", REPLICATE: "replicate", CIRCULAR: "circular"}
MAX_AMOUNT = 65535
f32 = np.float32


def limit(mode, L):
    """the largest amount the mode takes on an axis of length L"""
    return {CONSTANT: MAX_AMOUNT, REFLECT: L - 1, REPLICATE: MAX_AMOUNT, CIRCULAR: L}[mode]


def legal(mode, L, before, after):
    if max(abs(before), abs(after)) > MAX_AMOUNT or L + before + after < 1:
        return False
    if mode != CONSTANT and min(before, after) < 0:
        return False
    return max(before, after) <= limit(mode, L)


def axis_map(L, before, after, mode):
    """the input index every output index of one axis reads; -1 is the fill value"""
    assert legal(mode, L, before, after), (mode, L, before, after)
    src = []
    for o in range(L + before + after):
        i = o - before
        if 0 <= i < L:
            src.append(i)
        elif mode == CONSTANT:
            src.append(-1)
        elif mode == REFLECT:
            src.append(-i if i < 0 else 2 * (L - 1) - i)
        elif mode == REPLICATE:
            src.append(0 if i < 0 else L - 1)
        else:
            src.append(i + L if i < 0 else i - L)
    src = np.asarray(src, np.int64)
    assert src.min() >= -1 and src.max() < L
    return src


def apply(q, mode, l, r, t, b, fill=0, relu=False, zp=0):
    """[n, c, h, w] (any dtype; values are copied, never computed with) -> [n, c, h + t + b, w + l + r]"""
    q = np.asarray(q)
    sy, sx = axis_map(q.shape[2], t, b, mode), axis_map(q.shape[3], l, r, mode)
    out = np.ascontiguousarray(q[:, :, np.maximum(sy, 0)[:, None], np.maximum(sx, 0)[None, :]])
    out[:, :, (sy < 0)[:, None] | (sx < 0)[None, :]] = np.asarray(fill, q.dtype)
    return np.maximum(out, np.asarray(zp, q.dtype)) if relu else out


def crop(q, top, left, height, width):
    """the window as the amounts it implies"""
    h, w = np.asarray(q).shape[2:]
    assert 0 <= top and 0 <= left and height >= 1 and width >= 1 and top + height <= h and left + width <= w
    return apply(q, CONSTANT, -left, left + width - w, -top, top + height - h)


def output_shape(mode, l, r, t, b, n, c, h, w):
    assert legal(mode, w, l, r) and legal(mode, h, t, b)
    return (n, c, h + t + b, w + l + r)


def fill_byte(value, scale, zp):
    """the byte i8ie.quantize gives `value` at (scale, zp): (u8)(value / scale + zp), an fp32 divide, an fp32 add, truncation
    towards zero and the low 8 bits, no clamp (include/i8ie_hip.h, i8ie_quantize_f32_u8).  The conversion to int32 saturates
    and takes NaN to 0, as the device's does."""
    with np.errstate(all="ignore"):
        t = f32(f32(f32(value) / f32(scale)) + f32(zp))
    if np.isnan(t):
        i = 0
    elif t >= f32(2.0 ** 31):
        i = 2 ** 31 - 1
    elif t <= f32(-2.0 ** 31):
        i = -2 ** 31
    else:
        i = int(t)
    return i & 0xFF


def channel_bytes(shape, seed=0, avoid=None):
    """u8 [n, c, h, w] in which no wrong index can cancel: channel ch of pixel p of image i holds ch * 37 + p * 11 + r_i mod 256
    (37 odd: 256 consecutive channels differ; neighbouring pixels differ by 11, rows by 11 w), never the byte `avoid`"""
    n, c, h, w = shape
    ch = np.arange(c, dtype=np.int64)[None, :, None, None]
    pix = (np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :])[None, None]
    img = np.random.default_rng(seed).integers(0, 256, (n, 1, 1, 1), dtype=np.int64)
    q = ((ch * 37 + pix * 11 + img) % 256).astype(np.uint8)
    if avoid is not None:
        q[q == avoid] = avoid ^ 1
    return q


# ---- the kernels (csrc/i8ie_pad.hip) ------------------------------------------------------------------------------------------
FAST, DIRECT, FP32_KERNEL = "pad_u8_nhwc", "pad_u8_direct", "pad_f32"
THREADS, MAX_BLOCKS, WAVE = 256, 2048, 64     # kThreads, kMaxBlocks of csrc/i8ie_pointwise.h; the wave a uniform branch is taken by
MAX_LANES = THREADS * MAX_BLOCKS              # more items than this and the grid-stride loop goes round


def item_width(c, skew=0):
    """the bytes per lane pad_u8_nhwc takes: 16 / 4 / 1 by c and the misalignment of the base pointers"""
    for v in (16, 4):
        if c % v == 0 and skew % v == 0:
            return v
    return 1


def items(n, c, oh, ow, skew=0):
    return n * oh * ow * (c // item_width(c, skew))


def wave_classes(n, c, h, w, l, r, t, b, skew=0):
    """{"inner", "edge", "mixed"} -> how many waves of pad_u8_nhwc's first grid pass hold only interior items, only items
    outside the interior, or both (a lane is item v of the output in (image, oy, ox, channel item) order; a wave is 64
    consecutive lanes)"""
    per = c // item_width(c, skew)
    oh, ow = h + t + b, w + l + r
    oy, ox = np.arange(oh)[:, None], np.arange(ow)[None, :]
    inside = ((oy >= t) & (oy < t + h) & (ox >= l) & (ox < l + w)).ravel()
    lanes = np.tile(np.repeat(inside, per), n)[:MAX_LANES]
    pad = (-len(lanes)) % WAVE
    waves = np.concatenate([lanes, lanes[-1:].repeat(pad)]).reshape(-1, WAVE)
    inner, edge = waves.all(axis=1), (~waves).all(axis=1)
    return {"inner": int(inner.sum()), "edge": int(edge.sum()), "mixed": int((~inner & ~edge).sum())}


# ---- the case lists of tests/test_gpu_pad.py ------------------------------------------------------------------------------------
CHANNELS = (3, 20, 16, 48)          # byte, 4-byte and 16-byte items
BATCH = 2
ZPS = (0, 127, 255)
FILLS = (5, 200)                    # below and above the middle zero point
# (h, w, (left, right, top, bottom), modes)
GEOMETRY_CASES = [
    (5, 7, (2, 1, 3, 0), MODES),
    (4, 3, (2, 2, 3, 3), (REFLECT,)),             # L - 1 on all four sides
    (3, 4, (4, 4, 3, 3), (CIRCULAR,)),            # L on all four sides
    (1, 1, (3, 3, 3, 3), (REPLICATE,)),
    (1, 5, (3, 3, 3, 3), (REPLICATE,)),
    (5, 7, (3, 2, 0, 0), MODES),                  # one axis only
    (5, 7, (0, 0, 2, 1), MODES),
    (4, 5, (0, -4, 0, -3), (CONSTANT,)),          # crop to 1 x 1 from each corner
    (4, 5, (-4, 0, 0, -3), (CONSTANT,)),
    (4, 5, (0, -4, -3, 0), (CONSTANT,)),
    (4, 5, (-4, 0, -3, 0), (CONSTANT,)),
    (5, 7, (-1, 2, 1, -2), (CONSTANT,)),          # mixed signs
]
SEAM_MAP = (40, 40)
SEAM_CASES = [(16, 1), (16, 3), (64, 1), (64, 3)]   # (c, pad on all four sides): one and four items per pixel
IN_BORDERS, OUT_BORDERS = (0, 1, 2), (0, 1, 2)
SKEWS = (0, 4, 1)                                   # items of 16, 4 and 1 bytes at c = 16
LAYOUT_CASE = (16, 5, 7, (2, 1, 3, 0))              # (c, h, w, amounts), every mode
# (n, c, h, w, amounts, mode): just above MAX_LANES items, sizes that are no multiple of anything
WRAP_CASES = [(3, 16, 418, 419, (2, 1, 1, 2), REFLECT), (1, 3, 418, 419, (1, 0, 0, 1), CIRCULAR)]


# ---- ctypes signatures of the new entry points -----------------------------------------------------------------------------
_P, _I, _B, _F = C.c_void_p, C.c_int, C.c_uint8, C.c_float


def bind(lib):
    lib.i8ie_pad_output_shape.argtypes = [_I] * 9 + [C.POINTER(_I)]
    lib.i8ie_pad2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 9 + [_B, _I, _B]
    lib.i8ie_pad2d_u8.argtypes = [_P, _P, _P] + [_I] * 9 + [_B]
    lib.i8ie_pad2d_f32.argtypes = [_P, _P, _P] + [_I] * 9 + [_F]
    for f in (lib.i8ie_pad_output_shape, lib.i8ie_pad2d_u8_nhwc, lib.i8ie_pad2d_u8, lib.i8ie_pad2d_f32):
        f.restype = _I
    return lib
