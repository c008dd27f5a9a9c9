"""Cases for the grouped / depthwise Conv2d kernels (csrc/i8ie_gconv.hip, PATH_G of csrc/i8ie_layer.hip), shared by
tests/test_grouped_cases_host.py and tests/test_gpu_grouped_edges.py.  A helper module, not a conftest.

  dispatch(case)     which kernel instance the launcher picks, restated from i8ie_gconv_mfma_takes,
                     i8ie_gconv_granularity and the `dot4` / `vec_out` expressions of i8ie_gconv_launch
  EDGE_CASES         named cases, each the smallest shape that reaches one edge of a kernel (tile tails in features,
                     K and pixels, borders against padding, layouts, extreme operands, the grid-stride wrap)
  fuzz_cases(n, s)   a seeded sweep over group counts, channel residues, kernels, strides, layouts and borders
  reference(case)    operands and the expected bytes / accumulators (tests/grouped_ref.py), computed once per case

Every buffer the tests hand to the library is a device allocation or a 256-byte aligned slice of the workspace, so
the alignment terms of the launcher's expressions are always true here and dispatch() depends on the shape alone.

Batches: a pixel count M = m * OH * OW that is prime (17, 31, 127) or 3 * 43 is reached with the batch, over images of
a few pixels, rather than with an image 127 pixels long; every other case keeps the batch at 1 to 3."""
import collections
import os

import numpy as np

import grouped_ref as gr

S_IN, ZP_IN, ZP_OUT = np.float32(0.03), 121, 37

Case = collections.namedtuple(
    "Case", "name m c kc groups kh kw stride pad h w in_nhwc out_nhwc ib ob pc force zp_in extreme zero_col")
Dispatch = collections.namedtuple("Dispatch", "kernel G dot4 pc vec_out")


def geom(case):
    """(Cg, Ng, Kg, OH, OW, M)"""
    oh = (case.h - case.kh + 2 * case.pad) // case.stride + 1
    ow = (case.w - case.kw + 2 * case.pad) // case.stride + 1
    Cg = case.c // case.groups
    return Cg, case.kc // case.groups, Cg * case.kh * case.kw, oh, ow, case.m * oh * ow


def granularity(Cg):
    return 16 if Cg % 16 == 0 else (4 if Cg % 4 == 0 else 1)


def dispatch(case):
    Cg, Ng, Kg = geom(case)[:3]
    G = granularity(Cg)
    vec_out = 1 if case.kc % 4 == 0 and Ng % 4 == 0 else 0
    if not case.force and Kg >= 32 and (G == 1 or case.c % G == 0):
        return Dispatch("gconv_mfma", G, None, bool(case.pc), vec_out)
    return Dispatch("gconv_direct", None, Cg % 4 == 0 and case.c % 4 == 0, bool(case.pc), vec_out)


def header_rejects(case):
    """the argument checks of layer_forward / conv_geom that a drawn shape can miss (message, or None)"""
    if case.h - case.kh + 2 * case.pad < 0 or case.w - case.kw + 2 * case.pad < 0:
        return "kernel larger than padded input"
    if (not case.in_nhwc and case.ib) or (not case.out_nhwc and case.ob):
        return "only NHWC tensors carry a border"
    return None


def _mk(name, m, c, kc, groups, k, stride, pad, h, w, lay="cc", ib=None, ob=0, pc=False, force=False, zp_in=ZP_IN,
        extreme=False, zero_col=False):
    kh, kw = (k, k) if isinstance(k, int) else k
    in_nhwc, out_nhwc = lay[0] == "h", lay[1] == "h"
    if ib is None:
        ib = pad if in_nhwc else 0
    assert groups >= 2 and c % groups == 0 and kc % groups == 0
    return Case(name, m, c, kc, groups, kh, kw, stride, pad, h, w, in_nhwc, out_nhwc, ib, ob, pc, force, zp_in, extreme,
                zero_col)


def _both(*a, **kw):
    """the case with per-tensor and with per-channel scales"""
    return [_mk(a[0] + "-pt", *a[1:], pc=False, **kw), _mk(a[0] + "-pc", *a[1:], pc=True, **kw)]


def _edge_cases():
    E = []
    # ---- gconv_mfma: instances (G x PC x vec_out), Ng, Kg and M tails.  c = groups * Cg, kc = groups * Ng ------------
    #         name                        m    c    kc  g  k  s  p  h  w
    E += _both("g1_cg6_ng3_m1",           1,   12,   6, 2, 3, 1, 0, 3, 3)            # Kg 54; the kernel is the image
    E += _both("g1_cg7_ng4_kg63_m15",     1,   14,   8, 2, 3, 1, 1, 3, 5)            # vec_out on the byte gather
    E += _both("g1_cg65_ng17_kg65_m16",   1,  130,  34, 2, 1, 1, 0, 4, 4)            # second K step holds one byte
    E += _both("g1_cg3_k5_ng20_m17",     17,    6,  40, 2, 5, 1, 2, 1, 1)            # Kg 75; a 1 x 1 image under pad 2
    E += _both("g4_cg8_kg32_ng1_m31",    31,   16,   2, 2, 2, 1, 0, 2, 2)            # the dispatch boundary for G = 4
    E += _both("g4_cg4_kg64_ng64_m32",    2,    8, 128, 2, 4, 1, 0, 7, 7)            # one full K step, 4 full fragments
    E += _both("g16_cg32_kg32_ng6_m33",   3,   64,  12, 2, 1, 1, 0, 1, 11)           # the boundary for G = 16
    E += _both("g16_cg16_kg64_ng65_m127", 127, 32, 130, 2, 2, 1, 0, 2, 2)            # second blockIdx.y: one feature
    E += _both("g16_cg32_kg128_ng72_m128", 2,  64, 144, 2, 2, 1, 0, 9, 9)            # second blockIdx.y: 8 features
    E += _both("g4_cg8_kg128_ng63_m129", 43,   16, 126, 2, 4, 1, 0, 4, 6)            # ragged last fragment, 5 waves
    # ---- gconv_direct: DOT4 x PC x vec_out, Ng 1 2 3 5 8, Kg 31 ----------------------------------------------------
    E += _both("direct_dw_ng1",           2,    4,   4, 4, 3, 1, 1, 5, 5)            # depthwise: bytes, no vec_out
    E += _both("direct_bytes_ng8_vec",    2,    6,  16, 2, 3, 1, 1, 4, 5)            # Cg 3: bytes with vec_out
    E += _both("direct_dot4_ng2",         2,    8,   4, 2, 2, 1, 0, 4, 5)            # dot4, Ng % 4 != 0
    E += _both("direct_dot4_ng8_1x5",     1,    8,  16, 2, (1, 5), 1, 2, 3, 6)       # dot4 with vec_out, rectangular
    E += _both("direct_dot4_ng3_g3",      3,   24,   9, 3, 1, 1, 0, 3, 4)            # dot4, kc % 4 != 0
    E += _both("direct_bytes_ng5_kg31",   2,   62,  10, 2, 1, 1, 0, 3, 3)            # one short of the MFMA rule
    # ---- the input border against the padding (NHWC in): ib in {0, pad - 1, pad, pad + 1} on both kernels -------------
    E += _both("mfma_ib0_pad1",           2,   16,  16, 2, 3, 1, 1, 5, 6, lay="hh", ib=0, ob=1)
    E += _both("mfma_g1_ib1_pad2",        2,    6,  16, 2, 5, 1, 2, 6, 5, lay="hc", ib=1)
    E += _both("mfma_g16_ib_eq_pad",      2,   32,  16, 2, 3, 1, 1, 5, 4, lay="hh", ib=1, ob=0)
    E += _both("mfma_g1_ib2_pad1",        2,   12,  10, 2, 3, 1, 1, 4, 6, lay="hc", ib=2)
    E += _both("direct_ib0_pad1",         2,    4,   8, 2, 3, 1, 1, 5, 4, lay="hc", ib=0)
    E += _both("direct_ib1_pad2",         2,    8,   6, 2, 2, 1, 2, 3, 4, lay="hc", ib=1)
    E += _both("direct_ib2_pad1",         2,    6,   6, 2, 3, 2, 1, 6, 5, lay="hh", ib=2, ob=0)
    # ---- geometry ------------------------------------------------------------------------------------------------
    E += _both("mfma_pad_ge_k",           1,   16,   8, 2, 2, 1, 2, 4, 3)            # windows wholly in the padding
    E += _both("direct_pad_ge_k",         2,   10,   6, 2, 1, 1, 1, 3, 4)
    E += _both("mfma_stride_gt_k",        2,   32,  24, 2, 2, 3, 1, 8, 7)
    E += _both("direct_stride_gt_k",      2,    6,   6, 3, 1, 2, 0, 5, 6)
    E += _both("mfma_1x5",                2,   16,  12, 2, (1, 5), 1, 2, 4, 6)       # Kg 40, G 4
    E += _both("mfma_3x1_g1",             2,   22,  10, 2, (3, 1), 1, 1, 5, 4)       # Kg 33, G 1
    E += _both("direct_3x1",              2,    6,   4, 2, (3, 1), 2, 1, 6, 5)
    E += _both("mfma_oh1",                2,   16,   8, 2, 3, 1, 0, 3, 9)
    E += _both("mfma_ow1",                2,   16,   8, 2, 3, 2, 0, 8, 3)
    E += _both("direct_oh1_ow1",          3,    4,   4, 2, 3, 1, 0, 3, 3)
    # ---- layouts: the four pairs on a G = 1 layer and on a direct one; out_border 0 / 1 / 2; channel residues --------
    for lay in ("cc", "ch", "hc", "hh"):
        E += _both("mfma_g1_lay_" + lay,  2,   12,  32, 2, 3, 1, 1, 5, 7, lay=lay, ob=1 if lay[1] == "h" else 0)
        E += _both("direct_lay_" + lay,   2,    6,  16, 2, 3, 2, 1, 7, 5, lay=lay, ob=1 if lay[1] == "h" else 0)
    for ob in (0, 2):
        E += _both("mfma_g4_ob%d" % ob,   2,   16,  16, 2, 3, 1, 1, 4, 5, lay="hh", ob=ob)
        E += _both("direct_ob%d" % ob,    2,    8,  16, 2, 1, 1, 0, 3, 5, lay="hh", ob=ob)
    E += _both("mfma_nhwc_out_kc6_ob0",   2,   12,   6, 2, 3, 1, 1, 4, 5, lay="ch", ob=0)    # kc % 16 != 0 (and % 4)
    E += _both("direct_nhwc_out_kc10_ob0", 2,   4,  10, 2, 3, 1, 1, 4, 5, lay="hh", ob=0)
    E += _both("mfma_nhwc_in_c12",        2,   12,   9, 3, 3, 1, 1, 5, 4, lay="hc")          # C % 16 != 0: G 4
    E += _both("mfma_nhwc_in_c14",        2,   14,   8, 2, 3, 1, 1, 5, 4, lay="hh", ob=0)    # C % 4 != 0: G 1
    E += _both("direct_nhwc_in_c9",       2,    9,   6, 3, 3, 1, 1, 4, 4, lay="hc")          # C % 4 != 0: bytes
    # ---- arithmetic ----------------------------------------------------------------------------------------------
    for zp in (0, 255):
        E += _both("mfma_zp%d_pad" % zp,  2,   12,  10, 2, 3, 1, 1, 4, 5, zp_in=zp)
        E += _both("mfma_zp%d_nhwc_ib0" % zp, 2, 32, 16, 2, 3, 1, 2, 4, 5, lay="hh", ib=0, ob=1, zp_in=zp)
        E += _both("direct_zp%d_pad" % zp, 2,   6,   4, 2, 3, 1, 1, 4, 5, zp_in=zp)
        E += _both("direct_zp%d_nhwc_ib1" % zp, 2, 8, 16, 2, 3, 1, 2, 4, 5, lay="hh", ib=1, ob=1, zp_in=zp)
    E += _both("extreme_g1",              2,   14,  12, 2, 3, 1, 1, 5, 5, zp_in=0, extreme=True)    # Kg 63
    E += _both("extreme_bytes",           2,    6,  10, 2, 3, 1, 1, 5, 5, extreme=True)             # Kg 27, !DOT4
    E += [_mk("zero_scale_mfma_ng6-pc",   2,   12,  12, 2, 3, 1, 1, 5, 5, pc=True, zero_col=True),
          _mk("zero_scale_direct_ng6-pc", 2,    8,  12, 2, 2, 1, 0, 5, 5, pc=True, zero_col=True)]
    # ---- the direct kernel's grid-stride loop wraps: items = 4225 * 1024 > 16384 * 256 ---------------------------
    E += [_mk("direct_grid_wrap-pt",      1, 1024, 1024, 1024, 1, 1, 0, 65, 65)]
    return E


EDGE_CASES = _edge_cases()
MAX_DIRECT_THREADS = 16384 * 256  # i8ie_gconv_launch caps gconv_direct at 256 * 64 blocks of 256 lanes


def direct_items(case):
    _, Ng, _, _, _, M = geom(case)
    return M * case.groups * ((Ng + 3) // 4)


def fuzz_cases(n=None, seed=None):
    """`n` drawn cases; only shapes the header rejects (or with no output pixel) are drawn again.
    fuzz_cases.rejected holds how many draws the last call threw away."""
    n = int(os.environ.get("I8IE_GCONV_FUZZ_CASES", "48")) if n is None else n
    seed = int(os.environ.get("I8IE_GCONV_FUZZ_SEED", "20261018")) if seed is None else seed
    rng = np.random.default_rng(seed)
    out, rejected = [], 0
    while len(out) < n:
        # The instance is dealt round-robin (5 kinds x per-tensor / per-channel), so that 48 cases give each of the 10
        # instances 4 or 5 of them; everything else is drawn.  Cg comes from the kind's residue class: multiples of 16,
        # other multiples of 4, the rest (odd values and 6).
        i = len(out)
        kind, pc = ("mfma16", "mfma4", "mfma1", "dot4", "bytes")[i % 5], bool((i // 5) % 2)
        Cg = int(rng.choice({"mfma16": [16, 32, 48], "mfma4": [4, 8, 12, 20], "mfma1": [3, 5, 6, 7, 9, 33],
                             "dot4": [4, 8, 16, 20], "bytes": [1, 1, 2, 3, 5, 6, 7, 9]}[kind]))
        groups = int(rng.choice([2, 3, 4, 8]))
        if Cg == 1:  # groups = C: depthwise, with or without a channel multiplier
            groups = int(rng.choice([2, 5, 16, 24]))
        Ng = int(rng.integers(1, 81))
        # kernel: square three times in four; the MFMA kinds choose among the sizes with Cg * kh * kw >= 32 (the rule of
        # i8ie_gconv_mfma_takes), so no draw is thrown away for the kind
        ks = [(a, b) for a in (1, 2, 3, 5) for b in (1, 2, 3, 5) for _ in range(9 if a == b else 1)]
        if kind.startswith("mfma"):
            ks = [k for k in ks if Cg * k[0] * k[1] >= 32]
        kh, kw = ks[int(rng.integers(0, len(ks)))]
        # the direct kernel: below the MFMA rule's 32, or forced
        force = (not kind.startswith("mfma")) and (Cg * kh * kw >= 32 or rng.integers(0, 3) == 0)
        stride = int(rng.integers(1, 4))
        pad = int(rng.integers(0, max(kh, kw) + 1))
        h, w, m = int(rng.integers(3, 18)), int(rng.integers(3, 18)), int(rng.integers(1, 6))
        lay = ("cc", "ch", "hc", "hh")[int(rng.integers(0, 4))]
        ib = int(rng.choice([0, max(pad - 1, 0), pad, pad, pad + 1])) if lay[0] == "h" else 0
        ob = int(rng.integers(0, 3)) if lay[1] == "h" else 0
        zp_in = int(rng.choice([ZP_IN, ZP_IN, 0, 255, int(rng.integers(1, 255))]))
        case = _mk("fuzz%02d" % len(out), m, groups * Cg, groups * Ng, groups, (kh, kw), stride, pad, h, w, lay=lay, ib=ib,
                   ob=ob, pc=pc, force=bool(force), zp_in=zp_in)
        if header_rejects(case) is not None or geom(case)[5] <= 0:
            rejected += 1
            continue
        out.append(case)
    fuzz_cases.rejected = rejected
    return out


_cache = {}


def reference(case):
    """operands, scales and the oracle's (out NCHW, acc) for the case's scale mode, computed once and left unchanged.
    Scales as tests/test_gpu_grouped.make chooses them, with s_out set from the spread of the accumulators
    (sqrt(Kg) * rms(x - zp_in) * 73: a uniform byte about zp_in, a uniform weight) so that the per-tensor results have
    a standard deviation of about 20 codes around zp_out rather than sitting on a clamp; the per-channel columns, whose
    scales span a factor of 30 about that median, then have between 4 and 110."""
    key = case._replace(in_nhwc=False, out_nhwc=False, ib=0, ob=0, force=False)  # (what the expected values depend on)
    if key in _cache:
        return _cache[key]
    Cg, Ng, Kg = geom(case)[:3]
    rng = np.random.default_rng(sum(map(ord, case.name)))
    q = rng.integers(0, 256, (case.m, case.c, case.h, case.w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (case.kc, Cg, case.kh, case.kw), dtype=np.int8)
    qb = rng.integers(-127, 128, case.kc, dtype=np.int8)
    s_wv = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, case.kc)) * 2e-3).astype(np.float32)
    s_w = np.float32(np.median(s_wv))
    spread = np.sqrt(Kg * (74.0 ** 2 + (127.5 - case.zp_in) ** 2)) * 73.0
    s_out = np.float32(S_IN * float(s_w) * spread / 20.0)
    if case.extreme:  # every input byte 255, weight rows alternating 127 / -128: |acc| <= Kg * 255 * 128 < 2^31
        q[...] = 255
        qw[0::2], qw[1::2] = 127, -128
        s_out = np.float32(S_IN * float(s_w) * Kg * 255.0 * 128.0 / 100.0)
    if case.zero_col:  # the last feature of group 0, in the last, partial quad of the group
        s_wv[Ng - 1] = 0.0
    if case.pc:
        want, acc = gr.conv2d_grouped_pc(q, qw, qb, case.groups, case.stride, case.pad, S_IN, case.zp_in, s_wv, s_out, ZP_OUT)
    else:
        want, acc = gr.conv2d_grouped(q, qw, qb, case.groups, case.stride, case.pad, S_IN, case.zp_in, s_w, s_out, ZP_OUT)
    for a in (q, qw, qb, s_wv, want, acc):
        a.setflags(write=False)
    _cache[key] = dict(q=q, qw=qw, qb=qb, s_w=s_w, s_wv=s_wv, s_out=s_out, want=want, acc=acc)
    return _cache[key]
