"""Rectangular / anisotropic Conv2d restated for the tests.  A helper module, not a conftest.

Nothing new is defined arithmetically (include/i8ie_hip.h, i8ie_conv2d_create_rect): a layer with the geometry (kh, kw,
stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w) is the reference convolution (per group) of the kernel embedded
top-left in a square of zeros -- embed() -- at stride 1 and padding 0, on the input padded explicitly with zp_in, with rows
then subsampled by stride_h and columns by stride_w.  The square of side S is larger than the kernel's extent (eh, ew) on at
least one axis, so the explicit padding also adds the S - eh rows below and S - ew columns right that only the zeros of the
embedded kernel meet.  Zeros change neither the max-abs nor the weight sums, so scales, offsets and bias are the compact
kernel's, and the bound of the FP32 path uses the true K = (c / groups) kh kw.

  embed(w, geom)      [.., kh, kw] -> [.., S, S]
  reference(case)     operands, scales, the expected NCHW bytes and INT32 accumulators, once per case
  bind(lib)           ctypes signatures of the new C symbols
  CASES / dispatch    the GPU case lists of tests/test_gpu_rectconv.py, checked by tests/test_rectconv_host.py
  run(ctx, ...)       one forward of a rect handle with guard bytes around the output and the accumulators"""
import collections
import ctypes as C

import numpy as np

import abi
import grouped_ref as gr

Geom = collections.namedtuple("Geom", "kh kw sh sw ph pw dh dw")


class CGeom(C.Structure):
    """i8ie_conv_geom of include/i8ie_hip.h"""
    _fields_ = [(n, C.c_int) for n in ("kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "dilation_h", "dilation_w")]


def cgeom(g):
    return CGeom(*g)


def extent(g):
    return g.dh * (g.kh - 1) + 1, g.dw * (g.kw - 1) + 1


def out_hw(h, w, g):
    eh, ew = extent(g)
    return (h + 2 * g.ph - eh) // g.sh + 1, (w + 2 * g.pw - ew) // g.sw + 1


def embed(w, g):
    """[..., kh, kw] -> [..., S, S], S = max extent: w at (ky dh, kx dw), zeros elsewhere (the top-left square embedding)"""
    w = np.asarray(w)
    assert w.shape[-2:] == (g.kh, g.kw)
    eh, ew = extent(g)
    S = max(eh, ew)
    out = np.zeros(w.shape[:-2] + (S, S), w.dtype)
    out[..., 0:eh:g.dh, 0:ew:g.dw] = w
    return out


def pad_input(x, g, fill):
    """the explicit padding: (pad_h, pad_w) all round, and the rows / columns only the embedding's zeros meet"""
    eh, ew = extent(g)
    S = max(eh, ew)
    n, c, h, w = x.shape
    out = np.full((n, c, h + 2 * g.ph + S - eh, w + 2 * g.pw + S - ew), fill, x.dtype)
    out[:, :, g.ph:g.ph + h, g.pw:g.pw + w] = x
    return out


def subsample(out, acc, g):
    """rows by stride_h, columns by stride_w: of the stride-1 result [n, kc, H1, W1] and its accumulators [n, H1 W1, kc]"""
    n, kc, H1, W1 = out.shape
    o = np.ascontiguousarray(out[:, :, ::g.sh, ::g.sw])
    a = np.ascontiguousarray(acc.reshape(n, H1, W1, kc)[:, ::g.sh, ::g.sw]).reshape(n, -1, kc)
    return o, a


def conv_acc(q, qw, groups, g, zp_in):
    """INT32 sums of the definition, straight from the tap formula (no embedding): [n, oh, ow, kc] int64"""
    n, c, h, w = q.shape
    kc, Cg = qw.shape[:2]
    Ng = kc // groups
    oh, ow = out_hw(h, w, g)
    xp = np.full((n, c, h + 2 * g.ph, w + 2 * g.pw), zp_in, np.int64)
    xp[:, :, g.ph:g.ph + h, g.pw:g.pw + w] = q
    acc = np.zeros((n, oh, ow, kc), np.int64)
    for ky in range(g.kh):
        for kx in range(g.kw):
            win = xp[:, :, ky * g.dh: ky * g.dh + (oh - 1) * g.sh + 1: g.sh, kx * g.dw: kx * g.dw + (ow - 1) * g.sw + 1: g.sw]
            for gi in range(groups):
                acc[..., gi * Ng:(gi + 1) * Ng] += np.einsum("nchw,jc->nhwj", win[:, gi * Cg:(gi + 1) * Cg],
                                                             qw[gi * Ng:(gi + 1) * Ng, :, ky, kx].astype(np.int64))
    return acc


# ---- ctypes signatures ----------------------------------------------------------------------------------------------------
_P, _I, _F, _B = C.c_void_p, C.c_int, C.c_float, C.c_uint8
SYMBOLS = ["i8ie_conv2d_create_rect", "i8ie_conv2d_create_rect_per_channel", "i8ie_layer_geometry", "i8ie_conv2d_u8s8_rect",
           "i8ie_conv2d_f32_rect"]


def bind(lib):
    gr.bind(lib)
    lib.i8ie_conv2d_create_rect.argtypes = [_P, _P, _P, _I, _I, _I, _P, _F, _P]
    lib.i8ie_conv2d_create_rect_per_channel.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P, _P]
    lib.i8ie_layer_geometry.argtypes = [_P, _P]
    lib.i8ie_layer_dilation.argtypes = [_P, _P]
    lib.i8ie_conv2d_u8s8_rect.argtypes = [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _B, _P, _F, _F, _F, _B, _P, _P]
    lib.i8ie_conv2d_f32_rect.argtypes = [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]
    for n in SYMBOLS:
        getattr(lib, n).restype = _I
    return lib


# ---- the GPU cases --------------------------------------------------------------------------------------------------------
S_IN, ZP_IN, ZP_OUT = np.float32(0.03), 121, 37
Case = collections.namedtuple("Case", "name m c kc g geom h w pc force zp_in extreme")
KERNELS = {"lconv_mfma", "dconv_mfma", "gconv_mfma", "gconv_direct"}
LCONV_LDS_BUDGET = 32 << 10   # I8IE_LCONV_LDS_BUDGET of csrc/i8ie_lconv.h
LCONV_ROWS = 128
# the shortest 1 x 3 line on a 1 x 1 x W map with 16 channels whose plan, 2 lines x (W + 2) pixels x 32 bytes, is over the budget
OVER_BUDGET_W = LCONV_LDS_BUDGET // 64 - 1


def G(kh, kw, s=(1, 1), p=(0, 0), d=(1, 1)):
    return Geom(kh, kw, s[0], s[1], p[0], p[1], d[0], d[1])


# (m, c, kc, g, geom, h, w): what lconv_mfma takes (csrc/i8ie_lconv.hip)
LINES = [
    ("1x7_line17", (2, 32, 32, 1, G(1, 7, p=(0, 3)), 9, 17)),
    ("7x1_line17", (2, 32, 32, 1, G(7, 1, p=(3, 0)), 17, 9)),
    ("1x3_ragged", (3, 16, 20, 1, G(1, 3, p=(0, 1)), 7, 8)),
    ("3x1_ragged", (3, 16, 20, 1, G(3, 1, p=(1, 0)), 7, 8)),
    ("1x5_valid", (2, 32, 16, 1, G(1, 5), 6, 11)),
    ("1x3_out_longer", (2, 16, 16, 1, G(1, 3, p=(0, 2)), 5, 8)),
    ("1x7_line4", (2, 32, 16, 1, G(1, 7, p=(0, 3)), 5, 4)),
    ("7x1_m37", (37, 16, 16, 1, G(7, 1, p=(3, 0)), 5, 6)),
    ("1x3_c128", (1, 128, 16, 1, G(1, 3, p=(0, 1)), 6, 10)),
    ("3x1_c96_kc100", (2, 96, 100, 1, G(3, 1, p=(1, 0)), 9, 5)),
    ("at_lds_budget", (1, 16, 16, 1, G(1, 3, p=(0, 1)), 1, OVER_BUDGET_W - 1)),   # the longest line the plan still takes
    # padding ACROSS the line: whole output lines (rows of 1 x 3, columns of 7 x 1) lie outside the image and are all zp_in
    ("1x3_pad_across", (2, 16, 16, 1, G(1, 3, p=(1, 1)), 5, 7)),
    ("7x1_pad_across", (2, 32, 16, 1, G(7, 1, p=(3, 2)), 9, 5)),
]
# ... and what only the general route takes
GENERAL = [
    ("stride_2_1", (2, 32, 32, 1, G(3, 3, s=(2, 1), p=(1, 1)), 9, 11)),
    ("stride_1_2", (2, 32, 32, 1, G(3, 3, s=(1, 2), p=(1, 1)), 9, 11)),
    ("3x5", (2, 16, 24, 1, G(3, 5, p=(1, 2)), 8, 9)),
    ("3x3_dil_2_1", (2, 32, 16, 1, G(3, 3, p=(2, 1), d=(2, 1)), 9, 8)),
    ("3x3_pad_1_0", (2, 16, 16, 1, G(3, 3, p=(1, 0)), 7, 9)),
    ("1x7_groups2", (2, 32, 32, 2, G(1, 7, p=(0, 3)), 5, 9)),
    ("depthwise_1x5", (2, 32, 32, 32, G(1, 5, p=(0, 2)), 6, 9)),
    ("depthwise_5x1", (2, 32, 32, 32, G(5, 1, p=(2, 0)), 9, 6)),
    ("c20", (2, 20, 24, 1, G(1, 3, p=(0, 1)), 7, 9)),
    ("c6", (2, 6, 9, 1, G(3, 1, p=(1, 0)), 7, 9)),
    ("conv1d_s2_h1", (3, 16, 16, 1, G(1, 5, s=(1, 2), p=(0, 2)), 1, 19)),
    ("over_lds_budget", (1, 16, 16, 1, G(1, 3, p=(0, 1)), 1, OVER_BUDGET_W)),
]


def _mk(name, t, pc=False, force=False, zp_in=ZP_IN, extreme=False):
    return Case(name + ("-pc" if pc else "-pt") + ("-forced" if force else ""), *t, pc=pc, force=force, zp_in=zp_in, extreme=extreme)


def _cases():
    out = []
    for name, t in LINES + GENERAL:
        out += [_mk(name, t), _mk(name, t, pc=True)]
    for name, t in LINES:  # every line case under the force-fallback option
        out += [_mk(name, t, force=True), _mk(name, t, pc=True, force=True)]
    for force in (False, True):  # (the line kernel's cases, each again under the force-fallback option)
        for pc in (False, True):
            for zp in (0, 255):  # the padding value at its ends
                out += [_mk("zp%d_1x7" % zp, LINES[0][1], pc=pc, force=force, zp_in=zp),
                        _mk("zp%d_7x1" % zp, LINES[1][1], pc=pc, force=force, zp_in=zp)]
            out.append(_mk("extreme_lconv", LINES[9][1], pc=pc, force=force, zp_in=0, extreme=True))
    for pc in (False, True):
        out.append(_mk("extreme_gconv", GENERAL[2][1], pc=pc, extreme=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
LAYOUT_CASES = ["1x7_line17-pt", "1x7_groups2-pc"]  # the layout matrix: one lconv and one grouped case, kc % 16 == 0
# what the case lists must hold (tests/test_rectconv_host.py): every kernel, and every class of the issue by name
LCONV_CLASSES = ["1x7_line17", "7x1_line17", "1x3_ragged", "3x1_ragged", "1x5_valid", "1x3_out_longer", "1x7_line4", "7x1_m37", "1x3_c128",
                 "3x1_c96_kc100", "at_lds_budget", "1x3_pad_across", "7x1_pad_across", "zp0_1x7", "zp0_7x1", "zp255_1x7", "zp255_7x1",
                 "extreme_lconv"]   # each also "-forced"
CLASSES = LCONV_CLASSES + ["over_lds_budget", "stride_2_1", "stride_1_2", "3x5",
           "3x3_dil_2_1", "3x3_pad_1_0", "1x7_groups2", "depthwise_1x5", "depthwise_5x1", "c20", "c6", "conv1d_s2_h1"]


def geom_k(case):
    """(Cg, Ng, Kg, OH, OW)"""
    oh, ow = out_hw(case.h, case.w, case.geom)
    Cg = case.c // case.g
    return Cg, case.kc // case.g, Cg * case.geom.kh * case.geom.kw, oh, ow


def lconv_chunk(c):
    return c if c <= 64 else (64 if c % 64 == 0 else (32 if c % 32 == 0 else 16))


def lconv_lds(c, k, Lo):
    """i8ie_lconv_lds_bytes"""
    return ((LCONV_ROWS - 2 + Lo) // Lo + 1) * (Lo + k - 1) * (lconv_chunk(c) + 16)


def lconv_takes(case):
    """i8ie_lconv_takes and the routing rule of forward_grouped restated (every buffer of the tests is 256-byte aligned)"""
    g = case.geom
    oh, ow = out_hw(case.h, case.w, g)
    k, Lo = (g.kw, ow) if g.kh == 1 else (g.kh, oh)
    dh, dw = (1 if g.kh == 1 else g.dh), (1 if g.kw == 1 else g.dw)   # one tap on an axis has no dilation there
    return (not case.force and case.g == 1 and (g.sh, g.sw, dh, dw) == (1, 1, 1, 1) and (g.kh == 1 or g.kw == 1) and k >= 2
            and case.c % 16 == 0 and lconv_lds(case.c, k, Lo) <= LCONV_LDS_BUDGET)


def dispatch(case):
    """the name of the kernel that runs the case: lconv_mfma where it takes the layer, else the grouped launcher's choice"""
    if lconv_takes(case):
        return "lconv_mfma"
    Cg, _, Kg = geom_k(case)[:3]
    gran = 16 if Cg % 16 == 0 else (4 if Cg % 4 == 0 else 1)
    if not case.force and Kg >= 32 and (gran == 1 or case.c % gran == 0):
        return "gconv_mfma"
    return "gconv_direct"


_cache = {}


def reference(case):
    """operands, scales and the oracle's (out NCHW, acc) by the definition above, computed once per case and left unchanged.
    Scales as tests/dilated_ref.reference chooses them (s_out from the spread of the accumulators over the TRUE K)."""
    key = case._replace(name="", force=False)
    if key in _cache:
        return _cache[key]
    g = case.geom
    Cg, Ng, Kg = geom_k(case)[:3]
    rng = np.random.default_rng(sum(map(ord, case.name.replace("-forced", ""))))
    q = rng.integers(0, 256, (case.m, case.c, case.h, case.w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (case.kc, Cg, g.kh, g.kw), dtype=np.int8)
    qb = rng.integers(-127, 128, case.kc, dtype=np.int8)
    s_wv = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, case.kc)) * 2e-3).astype(np.float32)
    s_w = np.float32(np.median(s_wv))
    spread = np.sqrt(Kg * (74.0 ** 2 + (127.5 - case.zp_in) ** 2)) * 73.0
    s_out = np.float32(S_IN * float(s_w) * spread / 20.0)
    if case.extreme:  # every input byte 255, weight rows alternating 127 / -128: |acc| <= Kg * 255 * 128 < 2^31
        q[...] = 255
        qw[0::2], qw[1::2] = 127, -128
        s_out = np.float32(S_IN * float(s_w) * Kg * 255.0 * 128.0 / 100.0)
    qp, qwe = pad_input(q, g, case.zp_in), embed(qw, g)
    if case.pc:
        full, facc = gr.conv2d_grouped_pc(qp, qwe, qb, case.g, 1, 0, S_IN, case.zp_in, s_wv, s_out, ZP_OUT)
    else:
        full, facc = gr.conv2d_grouped(qp, qwe, qb, case.g, 1, 0, S_IN, case.zp_in, s_w, s_out, ZP_OUT)
    want, acc = subsample(full, facc, g)
    assert want.shape[2:] == out_hw(case.h, case.w, g)
    for a in (q, qw, qb, s_wv, want, acc):
        a.setflags(write=False)
    _cache[key] = dict(q=q, qw=qw, qb=qb, s_w=s_w, s_wv=s_wv, s_out=s_out, want=want, acc=acc)
    return _cache[key]


# ---- one forward of a rect handle -----------------------------------------------------------------------------------------
def create(ctx, case, d):
    """a handle of the case through i8ie_conv2d_create_rect(_per_channel)"""
    lib = abi.lib()
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    L, cg = C.c_void_p(), cgeom(case.geom)
    if case.pc:
        abi.ck(lib.i8ie_conv2d_create_rect_per_channel(ctx.h, P(d["qw"]), P(d["qb"]), case.kc, case.c, case.g, C.byref(cg), P(d["s_wv"]),
                                                       C.byref(L)))
    else:
        abi.ck(lib.i8ie_conv2d_create_rect(ctx.h, P(d["qw"]), P(d["qb"]), case.kc, case.c, case.g, C.byref(cg), C.c_float(d["s_w"]),
                                           C.byref(L)))
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(d["s_out"]), C.c_uint8(ZP_OUT)))
    return L


def run(ctx, case, relu, in_nhwc=False, out_nhwc=False, in_border=0, out_border=0, in_s8=False, out_s8=False, pool=None):
    """i8ie_layer_forward_fused / _pool of the case's handle, the output and the accumulators in guarded regions.  Returns a
    dict: out (NCHW), acc, names (the kernels that ran), ok (no guard byte changed), phys (the physical output, re-bias undone)"""
    lib = abi.lib()
    d = reference(case)
    oh, ow = out_hw(case.h, case.w, case.geom)
    ph, pw = (oh, ow) if pool is None else ((oh - pool[0]) // pool[1] + 1, (ow - pool[0]) // pool[1] + 1)
    ctx.set_force_fallback(case.force)
    L = None
    bufs = []
    try:
        L = create(ctx, case, d)
        phys_in = abi.Ctx.to_phys(d["q"], in_border, case.zp_in) if in_nhwc else d["q"]
        if in_s8:
            phys_in = phys_in ^ np.uint8(0x80)
        di = ctx.put(np.ascontiguousarray(phys_in))
        oshape = (case.m, ph + 2 * out_border, pw + 2 * out_border, case.kc) if out_nhwc else (case.m, case.kc, ph, pw)
        out, acc = abi.GuardedU8(ctx, oshape), abi.GuardedU8(ctx, (case.m, oh * ow, case.kc), np.int32)
        bufs = [di, out, acc]
        if out_nhwc and out_border:
            abi.ck(lib.i8ie_fill_border_u8(ctx.h, out.ptr, case.m, case.kc, ph, pw, out_border, C.c_uint8(ZP_OUT ^ (0x80 if out_s8 else 0))))
        il, ol = ((2 if in_s8 else 1) if in_nhwc else 0), ((2 if out_s8 else 1) if out_nhwc else 0)

        def forward():
            if pool is None:
                abi.ck(lib.i8ie_layer_forward_fused(L, di.ptr, il, in_border, case.m, case.h, case.w, C.c_float(S_IN), C.c_uint8(case.zp_in),
                                                    1 if relu else 0, out.ptr, ol, out_border, acc.ptr))
            else:
                abi.ck(lib.i8ie_layer_forward_pool(L, di.ptr, il, in_border, case.m, case.h, case.w, C.c_float(S_IN), C.c_uint8(case.zp_in),
                                                   1 if relu else 0, pool[0], pool[1], out.ptr, ol, out_border, acc.ptr))

        _, names = ctx.kernels_run(forward)
        phys = out.get()
        if out_s8:
            phys = phys ^ np.uint8(0x80)
        o = phys
        if out_nhwc:
            b = out_border
            o = np.ascontiguousarray((phys[:, b:-b, b:-b, :] if b else phys).transpose(0, 3, 1, 2))
        return dict(out=o, acc=acc.get(), names=names, ok=out.guards_ok() and acc.guards_ok(), phys=phys)
    finally:
        ctx.set_force_fallback(False)
        if L is not None:
            lib.i8ie_layer_destroy(L)
        for b in bufs:
            b.free()
