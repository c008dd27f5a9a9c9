"""Dilated (atrous) Conv2d restated for the tests.  A helper module, not a conftest.

Nothing new is defined arithmetically: Conv2d(..., dilation=d) is the reference convolution (per group) with the kernel
inflated by zeros to side d (k - 1) + 1 -- inflate().  Zeros change neither the max-abs nor the weight sums, so the layer's
quantised weights, scales, offsets and bias are those of the compact kernel, and the expected bytes and INT32 accumulators
are grouped_ref.conv2d_grouped(_pc) on inflate(qw, d); in float64, grouped_ref.conv2d_f64 on inflated weights with the true
K = (c / groups) k k in the bound.

  inflate(w, d)          [.., k, k] -> [.., d (k - 1) + 1, d (k - 1) + 1]
  bind(lib)              ctypes signatures of the new C symbols (tests/abi.py binds the rest)
  dilated_handles(...)   inside, the helpers of tests/abi.py drive dilated handles: they are handed the INFLATED weights (so
                         that the geometry they work out is the layer's) and the patched create makes the dilated layer from
                         the compact ones
  layer_dilation(L)      the optional 8th element of a conv tuple; spec_ref.forward inflates such a layer's quantised weights
  CASES / dispatch / reference   the GPU case lists of tests/test_gpu_dilated.py, checked by tests/test_dilated_host.py"""
import collections
import contextlib
import ctypes as C

import numpy as np

import grouped_ref as gr


def inflate(w, d):
    """[..., kh, kw] -> [..., d (kh - 1) + 1, d (kw - 1) + 1] with w at the multiples of d and zeros elsewhere"""
    w = np.asarray(w)
    assert d >= 1 and w.ndim >= 2
    kh, kw = w.shape[-2:]
    out = np.zeros(w.shape[:-2] + (d * (kh - 1) + 1, d * (kw - 1) + 1), w.dtype)
    out[..., ::d, ::d] = w
    return out


def out_hw(h, w, k, s, p, d):
    e = d * (k - 1) + 1
    return (h + 2 * p - e) // s + 1, (w + 2 * p - e) // s + 1


# ---- ctypes signatures of the dilated entry points ------------------------------------------------------------------------
_P, _I, _F, _B = C.c_void_p, C.c_int, C.c_float, C.c_uint8
SYMBOLS = ["i8ie_conv2d_create_dilated", "i8ie_conv2d_create_dilated_per_channel", "i8ie_layer_dilation",
           "i8ie_conv2d_u8s8_dilated", "i8ie_conv2d_f32_dilated"]


def bind(lib):
    gr.bind(lib)
    lib.i8ie_conv2d_create_dilated.argtypes = [_P, _P, _P] + [_I] * 8 + [_F, _P]
    lib.i8ie_conv2d_create_dilated_per_channel.argtypes = [_P, _P, _P] + [_I] * 8 + [_P, _P]
    lib.i8ie_layer_dilation.argtypes = [_P, _P]
    lib.i8ie_conv2d_u8s8_dilated.argtypes = [_P, _P, _I, _I, _I, _I, _P] + [_I] * 7 + [_B, _P, _F, _F, _F, _B, _P, _P]
    lib.i8ie_conv2d_f32_dilated.argtypes = [_P, _P, _I, _I, _I, _I, _P, _P] + [_I] * 7 + [_P]
    for n in SYMBOLS:
        getattr(lib, n).restype = _I
    return lib


@contextlib.contextmanager
def dilated_handles(lib, qw, groups, dilation, scales=None):
    """Inside: lib.i8ie_conv2d_create (tests/abi.py's CDLL) makes the dilated layer of the COMPACT weights `qw`
    [kc, c/groups, k, k] -- per-channel with `scales` when given.  The helpers of tests/abi.py are to be handed
    inflate(qw, dilation): they take the output geometry from the weight's shape, and the kernel extent of a dilated layer is
    the inflated one.  The pointer and the kernel size they pass on are ignored here."""
    bind(lib)
    qw = np.ascontiguousarray(qw, np.int8)
    k = qw.shape[2]
    assert qw.shape[3] == k
    wp = qw.ctypes.data_as(C.c_void_p)
    saved = lib.i8ie_conv2d_create
    if scales is None:
        lib.i8ie_conv2d_create = lambda ctx, _qw, qb, kc, c, kh, kw, st, pad, s_w, out: lib.i8ie_conv2d_create_dilated(
            ctx, wp, qb, kc, c, k, k, st, pad, groups, dilation, s_w, out)
    else:
        sw = np.ascontiguousarray(scales, np.float32)
        p = sw.ctypes.data_as(C.c_void_p)
        lib.i8ie_conv2d_create = lambda ctx, _qw, qb, kc, c, kh, kw, st, pad, s_w, out: lib.i8ie_conv2d_create_dilated_per_channel(
            ctx, wp, qb, kc, c, k, k, st, pad, groups, dilation, p, out)
    try:
        yield
    finally:
        lib.i8ie_conv2d_create = saved


# ---- spec networks --------------------------------------------------------------------------------------------------------
def layer_dilation(L):
    return L[7] if len(L) > 7 else 1


# ---- the GPU cases --------------------------------------------------------------------------------------------------------
S_IN, ZP_IN, ZP_OUT = np.float32(0.03), 121, 37
Case = collections.namedtuple("Case", "name m c kc g k s p d h w pc force zp_in extreme")
Dispatch = collections.namedtuple("Dispatch", "kernel G dot4")
KERNELS = {"dconv_mfma", "gconv_mfma", "gconv_direct"}
DCONV_SLOTS, DCONV_TILE, DCONV_LDS = 8, 4, 64 << 10

# (m, c, kc, g, k, s, p, d, h, w): dense stride-1 layers with C % 16 == 0 and K >= 32 -- dconv_mfma's (csrc/i8ie_dconv.hip)
DENSE_S1 = [
    ("phases_unequal", (2, 32, 32, 1, 3, 1, 2, 2, 9, 11)),
    ("ragged_features_h_mod_d", (3, 16, 20, 1, 3, 1, 3, 3, 7, 8)),
    ("map_le_dilation", (2, 64, 16, 1, 3, 1, 4, 4, 4, 4)),
    ("valid_conv", (2, 32, 32, 1, 3, 1, 0, 2, 9, 9)),
    ("pad_not_multiple_of_d", (2, 32, 32, 1, 3, 1, 1, 2, 9, 9)),
    ("pad_beyond_half", (2, 32, 32, 1, 3, 1, 3, 2, 6, 6)),
    ("k5", (2, 16, 32, 1, 5, 1, 4, 2, 10, 9)),
    ("k_tail_kc80", (2, 48, 80, 1, 3, 1, 2, 2, 8, 8)),
    ("even_kernel", (2, 16, 16, 1, 2, 1, 1, 2, 7, 7)),
    ("rate6_m37", (37, 32, 16, 1, 3, 1, 6, 6, 8, 8)),
    ("chunks_c128_tiles2x3", (1, 128, 16, 1, 3, 1, 2, 2, 10, 18)),  # two channel chunks; 2 x 3 tiles per phase plane
    ("chunk_c96_kc100", (2, 96, 100, 1, 2, 1, 0, 3, 9, 9)),       # a 32-byte chunk, three of them; a second feature block of 36
]
# ... and what only the general route takes
GENERAL = [
    ("stride2", (2, 32, 32, 1, 3, 2, 2, 2, 9, 11)),
    ("c_mod16", (2, 20, 24, 1, 3, 1, 2, 2, 7, 9)),
    ("byte_gather", (2, 6, 9, 1, 3, 1, 2, 2, 7, 9)),
    ("groups2_cg48", (2, 96, 32, 2, 3, 1, 2, 2, 9, 9)),
    ("depthwise", (2, 32, 32, 32, 3, 1, 2, 2, 9, 9)),
    ("depthwise_s2", (2, 32, 32, 32, 3, 2, 2, 2, 9, 9)),
    ("lds_declines_k11", (1, 64, 16, 1, 11, 1, 10, 2, 8, 8)),      # 8 x 14 x 14 x 64 bytes of patches > 64 KiB
]


def _mk(name, t, pc=False, force=False, zp_in=ZP_IN, extreme=False):
    return Case(name + ("-pc" if pc else "-pt") + ("-forced" if force else ""), *t, pc=pc, force=force, zp_in=zp_in, extreme=extreme)


def _cases():
    out = []
    for name, t in DENSE_S1 + GENERAL:
        out += [_mk(name, t), _mk(name, t, pc=True)]
    for name, t in DENSE_S1:  # every dense case under the force-fallback option
        out += [_mk(name, t, force=True), _mk(name, t, pc=True, force=True)]
    for zp in (0, 255):  # the padding value at its ends, on both kernels
        out += [_mk("zp%d_mfma" % zp, DENSE_S1[0][1], zp_in=zp), _mk("zp%d_direct" % zp, GENERAL[4][1], pc=True, zp_in=zp)]
    out += [_mk("extreme_mfma", DENSE_S1[7][1], zp_in=0, extreme=True), _mk("extreme_direct", GENERAL[4][1], extreme=True)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
LAYOUT_CASES = ["phases_unequal-pt", "groups2_cg48-pc"]  # the layout matrix: one dense and one grouped case, kc % 16 == 0


def geom(case):
    """(Cg, Ng, Kg, OH, OW)"""
    oh, ow = out_hw(case.h, case.w, case.k, case.s, case.p, case.d)
    Cg = case.c // case.g
    return Cg, case.kc // case.g, Cg * case.k * case.k, oh, ow


def dconv_chunk(c):
    return c if c <= 64 else (64 if c % 64 == 0 else (32 if c % 32 == 0 else 16))


def dconv_takes(case):
    """i8ie_dconv_takes and the routing rule of forward_grouped restated (every buffer of the tests is 256-byte aligned)"""
    lds = DCONV_SLOTS * (case.k + DCONV_TILE - 1) ** 2 * dconv_chunk(case.c)
    return (not case.force and case.g == 1 and case.s == 1 and case.d >= 2 and case.k >= 2 and case.c % 16 == 0
            and case.c * case.k * case.k >= 32 and lds <= DCONV_LDS)


def dispatch(case):
    """dconv_mfma where it takes the layer; else the kernel the grouped launcher picks (tests/grouped_cases.dispatch restated
    on these cases; the dilation does not enter that choice)"""
    if dconv_takes(case):
        return Dispatch("dconv_mfma", None, None)
    Cg, _, Kg = geom(case)[:3]
    G = 16 if Cg % 16 == 0 else (4 if Cg % 4 == 0 else 1)
    if not case.force and Kg >= 32 and (G == 1 or case.c % G == 0):
        return Dispatch("gconv_mfma", G, None)
    return Dispatch("gconv_direct", None, Cg % 4 == 0 and case.c % 4 == 0)


_cache = {}


def reference(case):
    """operands, scales and the oracle's (out NCHW, acc) on the inflated weights, computed once per case and left unchanged.
    Scales as tests/grouped_cases.reference chooses them (s_out from the spread of the accumulators over the TRUE K)."""
    key = case._replace(name="", force=False)
    if key in _cache:
        return _cache[key]
    Cg, Ng, Kg = geom(case)[:3]
    rng = np.random.default_rng(sum(map(ord, case.name.replace("-forced", ""))))
    q = rng.integers(0, 256, (case.m, case.c, case.h, case.w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (case.kc, Cg, case.k, case.k), dtype=np.int8)
    qb = rng.integers(-127, 128, case.kc, dtype=np.int8)
    s_wv = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, case.kc)) * 2e-3).astype(np.float32)
    s_w = np.float32(np.median(s_wv))
    spread = np.sqrt(Kg * (74.0 ** 2 + (127.5 - case.zp_in) ** 2)) * 73.0
    s_out = np.float32(S_IN * float(s_w) * spread / 20.0)
    if case.extreme:  # every input byte 255, weight rows alternating 127 / -128: |acc| <= Kg * 255 * 128 < 2^31
        q[...] = 255
        qw[0::2], qw[1::2] = 127, -128
        s_out = np.float32(S_IN * float(s_w) * Kg * 255.0 * 128.0 / 100.0)
    qwi = inflate(qw, case.d)
    if case.pc:
        want, acc = gr.conv2d_grouped_pc(q, qwi, qb, case.g, case.s, case.p, S_IN, case.zp_in, s_wv, s_out, ZP_OUT)
    else:
        want, acc = gr.conv2d_grouped(q, qwi, qb, case.g, case.s, case.p, S_IN, case.zp_in, s_w, s_out, ZP_OUT)
    for a in (q, qw, qwi, qb, s_wv, want, acc):
        a.setflags(write=False)
    _cache[key] = dict(q=q, qw=qw, qwi=qwi, qb=qb, s_w=s_w, s_wv=s_wv, s_out=s_out, want=want, acc=acc)
    return _cache[key]
