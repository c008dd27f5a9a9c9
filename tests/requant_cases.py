"""The cases of tests/test_gpu_requant_replay.py: one replay site of a contraction epilogue per entry of SITES, each run in the
classes of tests/requant_ref.py.  A helper module, not a conftest; tests/test_requant_host.py asserts the class conditions of
every case from the numpy references alone, so that the GPU file can rely on them.

A case is a case dict of tests/test_gpu_layer_routes.py (its shapes and variants come from that file's CASES, from
tests/test_gpu_pconv.py and from tests/dilated_ref.py) plus "cls", "zero" (the zero-column variant), "site" and "kernels" (the
names of which one must be in the launch map)."""
import itertools
import zlib

import numpy as np

import deconv_ref
import dilated_ref
import grouped_ref
import orc
import requant_ref as rq
import test_gpu_layer_routes as lr

NCHW, NHWC, S8 = lr.NCHW, lr.NHWC, lr.S8
V_FLIN, V_MLIN_128 = 80, 85   # I8IE_VARIANT_FLIN / _MLIN_128 of include/i8ie_hip.h
HH = dict(il=NHWC, ib=1, ol=NHWC)
# the smallest geometry of tests/test_gpu_pconv.py that variant 70 takes (K = 512, four K tiles), and the smallest dense dilated
# cases of tests/dilated_ref.py ("even_kernel"; the same with 18 features, no multiple of 4)
TC = dict(c=512, h=13, w=13, n=192, k=1, s=1, p=0, m=66, variant=70)
DC = dict(kind="gconv", c=16, h=7, w=7, n=16, k=2, s=1, p=1, dil=2)

SITES = {}   # site -> dict(kernels, cases)
CASES = {}   # id -> case


def site(tag, kernels, base, forms, pc=True):
    """The classes of requant_ref.CLASSES, per tensor and (pc) per channel, over `forms` (relu / layout / pool overrides) in
    turn, and the zero-column variant once."""
    combos = list(itertools.product(rq.CLASSES, (False, True) if pc else (False,)))
    ids = []
    for i, (cls, per_channel) in enumerate(combos + ([("ALL", True)] if pc else [])):
        zero = i == len(combos)
        form = forms[i % len(forms)]
        cs = dict(lr.DEFAULTS, **dict(base, **form))
        if "relu" not in form:
            cs["relu"] = (i // 2 + i) & 1
        cid = "%s-%s-%s%s-f%d" % (tag, cls, "pc" if per_channel else "pt", "-zero" if zero else "", i % len(forms))
        cs.update(id=cid, pc=per_channel, cls=cls, zero=zero, site=tag, kernels=tuple(kernels))
        assert cid not in CASES
        CASES[cid] = cs
        ids.append(cid)
    SITES[tag] = dict(kernels=tuple(kernels), cases=ids)


LIN = dict(kind="lin", m=3)
site("igemm_conv", ["igemm_conv_128x32"], dict(lr.A, **HH),
     [dict(ob=1), dict(ol=S8, relu=1), dict(pool=(2, 2))])
site("igemm_conv_ragged", ["igemm_conv_128x32"], dict(lr.A, n=24, ol=NHWC), [dict(), dict(pool=(2, 2), relu=1)])
site("igemm_conv_128", ["igemm_conv_128x128"], dict(lr.AP, variant=lr.V_TILED, **HH), [dict(pool=(2, 2)), dict(ol=S8, relu=1)])
site("igemm_lin", ["igemm_lin_128x32"], dict(LIN, K=32, n=32), [dict()])
site("splitk", ["splitk_reduce"], dict(LIN, K=512, n=32, variant=lr.V_TILED), [dict()])
# (n = 18, no multiple of 4: the last quad of a row has two live values, and 3 x 18 values end inside a quad)
site("splitk_ragged", ["splitk_reduce"], dict(LIN, K=512, n=18, variant=lr.V_TILED), [dict()])
site("flin", ["flin_128x16"], dict(LIN, K=1024, n=2048), [dict()])
site("flin_ragged", ["flin_128x16"], dict(LIN, K=1024, n=18, variant=V_FLIN), [dict()])
# (above 64 rows the block is 64 rows x 32 features, two wave columns: four LDS stages up to 128 rows, three above; n = 272 is no
# multiple of 32 and below the automatic feature threshold, hence the forced variant)
site("flin_64", ["flin_64x32"], dict(LIN, m=65, K=1024, n=2048), [dict()])
site("flin_64_3st", ["flin_64x32"], dict(LIN, m=129, K=1024, n=272, variant=V_FLIN), [dict()])
site("mlin", ["mlin_64x128"], dict(LIN, m=257, K=512, n=128, variant=lr.V_MLIN), [dict()])
site("mlin_128", ["mlin_128x128"], dict(LIN, m=257, K=512, n=128, variant=V_MLIN_128), [dict()])
site("pconv", ["pconv_192x192"], dict(lr.AP, **HH), [dict(), dict(ol=S8, ob=1, relu=1), dict(il=S8, ob=1)])
site("pconv_pool", ["pconv_pool_192x192"], dict(lr.AP, pool=(2, 2), **HH), [dict(), dict(il=S8, ol=S8, ob=1, relu=1)])
site("tconv", ["tconv_"], dict(TC, il=NHWC, ib=0, ol=NHWC), [dict(ob=1), dict(ol=S8, relu=1)])
site("stem", ["stem_conv"], dict(lr.B, ol=NHWC), [dict(), dict(ol=S8, relu=1), dict(f32=True), dict(f32=True, ol=S8, ob=1, relu=1)])
site("stem_pool", ["stem_conv_pool"], dict(lr.B, ol=NHWC, pool=(2, 2)),
     [dict(ob=1, relu=1), dict(f32=True, relu=0), dict(ol=S8, relu=1), dict(f32=True, relu=1)])
site("first", ["conv_smallc_wstat"], dict(lr.B, ol=NHWC, variant=lr.V_TILED),
     [dict(), dict(f32=True, ol=S8, ob=1, relu=1), dict(f32=True), dict(ol=S8, relu=1)])
site("gconv_mfma", ["gconv_mfma"], dict(lr.G2, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1), dict(il=NCHW, ib=0, ol=NCHW)])
site("gconv_direct", ["gconv_direct"], dict(lr.GD, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1), dict(il=NCHW, ib=0, ol=NCHW)])
# (depthwise: a pack holds one real column four times; two input channels per group and four features: a quad of four columns)
site("gconv_direct_ng4", ["gconv_direct"], dict(lr.GD, groups=8, n=32, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1)])
site("deconv_mfma", ["deconv_mfma"], dict(lr.T2, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1), dict(il=NCHW, ib=0, ol=NCHW)])
site("deconv_direct", ["deconv_direct"], dict(lr.TD, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1)])
site("deconv_k3", ["deconv_mfma"], dict(lr.T3, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1)])
site("dconv", ["dconv_mfma"], dict(DC, **HH), [dict(ob=1), dict(il=S8, ol=S8, relu=1), dict(il=NCHW, ib=0, ol=NCHW)])
site("dconv_ragged", ["dconv_mfma"], dict(DC, n=18), [dict()])

BMM = (2, 17, 33, 64)   # b, m, n, k of the bmm_mfma cases
ATT = (8, 2, 16, 17)     # b, heads, d, tq of the attn_mfma cases (uniform probabilities give every query row of a batch item
                        # the same result: the batch is what spreads the values)
ATT_SEED = 8


def check_case_list():
    """conditions on the case list itself: every site sees every class, relu off and on, relu with a re-biased output and
    the zero-column variant"""
    for tag, s in SITES.items():
        cases = [CASES[c] for c in s["cases"]]
        assert {c["cls"] for c in cases} == set(rq.CLASSES), tag
        assert {c["relu"] for c in cases} == {0, 1}, tag
    for group in (("igemm_conv", "igemm_conv_ragged", "igemm_conv_128"), ("pconv", "pconv_pool"), ("tconv",), ("stem", "stem_pool"),
                  ("first",), ("gconv_mfma",), ("gconv_direct", "gconv_direct_ng4"), ("deconv_mfma", "deconv_k3"), ("deconv_direct",),
                  ("dconv", "dconv_ragged")):
        cases = [CASES[c] for tag in group for c in SITES[tag]["cases"]]
        assert any(c["relu"] and c["ol"] == S8 for c in cases), group
        assert any(c["zero"] for c in cases), group
    for tag in ("igemm_lin", "splitk", "splitk_ragged", "flin", "flin_ragged", "flin_64", "flin_64_3st", "mlin", "mlin_128"):
        assert any(CASES[c]["zero"] for c in SITES[tag]["cases"]), tag


# what the sites must reach between them (the table of the issue; a name ending in "_" is a prefix)
TABLE = {
    "i8ie_igemm.hip conv": ["igemm_conv_128x32", "igemm_conv_128x128"], "i8ie_igemm.hip lin": ["igemm_lin_128x32", "splitk_reduce"],
    "i8ie_flin.hip": ["flin_64x32", "flin_128x16"], "i8ie_mlin.hip": ["mlin_64x128", "mlin_128x128"], "i8ie_pconv.hip": ["pconv_192x192", "pconv_pool_192x192"],
    "i8ie_tconv.hip": ["tconv_"], "i8ie_stem.hip": ["stem_conv", "stem_conv_pool"], "i8ie_first.hip": ["conv_smallc_wstat"],
    "i8ie_gconv.hip": ["gconv_mfma", "gconv_direct"], "i8ie_deconv.hip": ["deconv_mfma", "deconv_direct"],
    "i8ie_dconv.hip": ["dconv_mfma"], "i8ie_matmul.hip": ["bmm_mfma"], "i8ie_attention.hip": ["attn_mfma"]}


def ran(name, launch_map):
    """whether the table's `name` (a trailing "_": a prefix) is among the kernels of a launch map"""
    return any(k == name or (name.endswith("_") and k.startswith(name)) for k in launch_map)


# ---- operands and references -------------------------------------------------------------------------------------------------
def geometry(cs):
    """(input shape, weight shape, contraction length of one output value)"""
    if cs["kind"] == "lin":
        return (cs["m"], cs["K"]), (cs["n"], cs["K"]), cs["K"]
    q = (cs["m"], cs["c"], cs["h"], cs["w"])
    if cs["kind"] == "deconv":  # (the equivalent kernel; an output pixel sees ceil(k / s)^2 of its taps)
        return q, (cs["n"], cs["c"], cs["k"], cs["k"]), cs["c"] * (-(-cs["k"] // cs["s"])) ** 2
    cg = cs["c"] // cs["groups"]
    return q, (cs["n"], cg, cs["k"], cs["k"]), cg * cs["k"] ** 2


_ops, _acc = {}, {}


def operands(cs):
    """requant_ref.layer_class of the case, built once and left unchanged; an f32-input case gets x = (q - zp_in) s_in, which
    the quantize step brings back to q exactly"""
    qs, ws, K = geometry(cs)
    key = (cs["kind"], qs, ws, cs["cls"], cs["pc"], cs["zero"], cs["f32"])
    if key not in _ops:
        seed = zlib.crc32(repr((cs["kind"], qs, ws, cs["pc"])).encode())  # (one draw per layer: the classes differ in scales only)
        d = rq.layer_class(cs["cls"], qs, ws, K, 127 if cs["f32"] else 121, cs["pc"], seed, cs["zero"])
        if cs["f32"]:
            x = ((d["q"].astype(np.int32) - d["zp_in"]).astype(np.float32) * d["s_in"]).astype(np.float32)
            x.setflags(write=False)
            d["x"] = x
        _ops[key] = d
    return _ops[key]


def accumulators(cs, d):
    """INT32 accumulators of the layer from the numpy / oracle references ([m, n], or [m, oh * ow, n]); they do not depend on a
    scale (the bias is 0), so every class of a layer shares them"""
    qs, ws, _ = geometry(cs)
    key = (cs["kind"], qs, ws, cs["pc"], cs["f32"], cs.get("s"), cs.get("p"), cs["op"], cs["groups"], cs["dil"])
    if key not in _acc:
        one = np.float32(1)
        q, qw, qb, zp = d["q"], d["qw"], d["qb"], d["zp_in"]
        if cs["kind"] == "lin":
            acc = orc.linear(q, qw, qb, one, zp, one, one, 0, want_acc=True)[1]
        elif cs["kind"] == "deconv":
            acc = deconv_ref.deconv_u8(q, qw, qb, cs["s"], cs["p"], cs["op"], one, zp, one, one, 0)[1]
        else:
            acc = grouped_ref.conv2d_grouped(q, dilated_ref.inflate(qw, cs["dil"]), qb, cs["groups"], cs["s"], cs["p"], one, zp, one, one, 0)[1]
        acc.setflags(write=False)
        _acc[key] = acc
    return _acc[key]


def scales(cs, d):
    return d["s_in"], rq.layer_scale(d, cs["pc"]), d["s_out"], d["zp_out"]


def expected(cs, d, acc):
    """The physical output the case must leave: requant_ref.exact on the reference accumulators, the relu floor, the max-pool,
    layout, border and re-bias on the host"""
    s_in, s_w, s_out, zp = scales(cs, d)
    out = rq.exact(acc, s_in, s_w, s_out, zp, zp if cs["relu"] else 0)
    if cs["kind"] == "lin":
        return out
    oh, ow, _, _ = lr.out_hw(dict(cs, pool=None))
    ref = np.ascontiguousarray(out.transpose(0, 2, 1).reshape(cs["m"], cs["n"], oh, ow))
    if cs["pool"]:
        ref = orc.max_pool2d(ref, *cs["pool"])
    return lr.expected_phys(cs, ref, zp)


def report(cs, d, acc):
    s_in, s_w, s_out, zp = scales(cs, d)
    return rq.class_report(cs["cls"], acc, s_in, s_w, s_out, zp, cs["relu"])
