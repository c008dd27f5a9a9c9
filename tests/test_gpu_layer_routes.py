"""Route fingerprints of the INT8 layer forward (csrc/i8ie_layer.hip) through the C-ABI.

For every case of CASES, four things:
  (a) the output bytes equal the same layer run with I8IE_OPT_FORCE_FALLBACK from NCHW to NCHW, relu and max-pool applied
      by the separate ABI calls, brought into the case's layout, border and re-bias on the host (the force-fallback cases
      themselves: the oracle's conv2d / linear);
  (b) no guard byte around the output changed, and an output border holds zp_out (zp_out ^ 0x80 when re-biased);
  (c) the launch map (kernel name cut at '|' -> launches) of the first and of the second, warm, forward equal the recorded ones;
  (d) the answers of i8ie_layer_fuses_pool / _rebiased_io / _accepts_f32_input / _preferred_layout equal the recorded ones, and
      a query that says "folded" is not followed by a max-pool / re-bias launch of its own (implications that do not hold are
      recorded as they are, under "violations").

The recorded values are tests/golden/layer_routes.json, keyed by case id.  `python tests/test_gpu_layer_routes.py --record`
writes that file from the library as built; the pytest run only reads it, and a case without an entry fails."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np
import pytest

import abi
import support

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_routes.json")
S_IN, ZP_IN, ZP_OUT = np.float32(0.03), 121, 37
Q_SCALE, Q_ZP = np.float32(0.025), 127  # the f32-input entry quantizes with these
V_TILED, V_PCONV, V_MLIN = 11, 50, 83   # I8IE_VARIANT_TILED / _PCONV / _MLIN of include/i8ie_hip.h
NCHW, NHWC, S8 = 0, 1, 2
_P = C.c_void_p

# ---- the cases ------------------------------------------------------------------------------------------------------------
# Shapes come from the gates of the code: i8ie_flin_wants (<= 256 rows, n >= 2048, Kpad >= 1024), i8ie_mlin_wants (> 256 rows,
# Kpad >= 512, n >= 2048 unless forced), i8ie_pconv_takes (c % 32 == 0, n >= 192, >= 64 images, >= 129 output pixels per band;
# below 192 bands only when forced), i8ie_stem_supported (c <= 3, stride % 4 == 0, n in 32 / 64 / 96), i8ie_first_supported
# (n % 32 == 0), gconv_mfma (Cg * kh * kw >= 32), deconv_mfma (c * ceil(k / s)^2 >= 32).
DEFAULTS = dict(kind="conv", m=2, groups=1, op=0, il=NCHW, ib=0, ol=NCHW, ob=0, relu=0, pool=None, variant=0, force=False,
                pc=False, flat=None, offset=0, dequant=None, f32=False, dil=1)
CASES = {}


def case(cid, pc_twin=False, **kw):
    bad = set(kw) - set(DEFAULTS) - {"c", "h", "w", "n", "k", "s", "p", "K"}  # (dil: only tests/test_gpu_requant_replay.py's cases)
    assert not bad and cid not in CASES, (cid, bad)
    CASES[cid] = dict(DEFAULTS, id=cid, **kw)
    if pc_twin:
        CASES[cid + "-pc"] = dict(CASES[cid], id=cid + "-pc", pc=True)


# Linear
case("lin_smalln", kind="lin", m=3, K=32, n=10, pc_twin=True)
case("lin_smalln_dequant_null", kind="lin", m=3, K=32, n=10, dequant="null")
case("lin_dequant_n32", kind="lin", m=3, K=32, n=32, dequant="u8")
case("lin_nhwc_perm", kind="lin", m=3, K=64, n=32, flat=(16, 2, 2))
case("lin_nhwc_k20", kind="lin", m=3, K=20, n=32, flat=(5, 2, 2))
case("lin_k20", kind="lin", m=3, K=20, n=32, pc_twin=True)
case("lin_offset1", kind="lin", m=3, K=32, n=32, offset=1)
case("lin_flin", kind="lin", m=3, K=1024, n=2048)
case("lin_tiled_splitk", kind="lin", m=3, K=512, n=32, variant=V_TILED, pc_twin=True)
case("lin_257_k128", kind="lin", m=257, K=128, n=128)
case("lin_mlin", kind="lin", m=257, K=512, n=128, variant=V_MLIN)  # (K = 128 is below the kernel's four chunks)
case("lin_force_relu_k20", kind="lin", m=3, K=20, n=32, relu=1, force=True)

# Conv A, the tiled kernel: c = 16; and a shape the patch-stationary kernel takes when forced: c = 32, n = 192, 64 images
A = dict(c=16, h=8, w=8, n=16, k=3, s=1, p=1)
AP = dict(c=32, h=12, w=12, n=192, k=3, s=1, p=1, m=64, variant=V_PCONV)
case("a_cc", **A)
case("a_hh_direct", il=NHWC, ib=1, ol=NHWC, pc_twin=True, **A)
case("a_h_reborder", il=NHWC, ib=0, ol=NHWC, **A)
case("a_h_shifted", il=NHWC, ib=2, ol=NHWC, **A)
case("a_ob1", ol=NHWC, ob=1, **A)
case("a_pool_n24_h", ol=NHWC, pool=(2, 2), **dict(A, n=24))
case("a_s8out_n24_err", il=NHWC, ib=1, ol=S8, **dict(A, n=24))
case("a_pool_window_err", ol=NHWC, pool=(9, 1), **A)
case("ap_hh", il=NHWC, ib=1, ol=NHWC, **AP)
for tag, G in (("a", A), ("ap", AP)):
    case(tag + "_s8in", il=S8, ib=1, ol=NHWC, **G)
    case(tag + "_s8out", il=NHWC, ib=1, ol=S8, ob=1, **G)
    case(tag + "_s8both", il=S8, ib=1, ol=S8, **G)
    case(tag + "_pool_h", il=NHWC, ib=1, ol=NHWC, pool=(2, 2), pc_twin=True, **G)
    case(tag + "_pool_c", pool=(2, 2), **G)
    case(tag + "_pool_s8both", il=S8, ib=1, ol=S8, ob=1, pool=(2, 2), relu=1, **G)
case("ap_pool_h_tiled", il=NHWC, ib=1, ol=NHWC, pool=(2, 2), **dict(AP, variant=V_TILED))

# Conv B: c = 3, stride 4
B = dict(c=3, h=20, w=20, n=32, k=5, s=4, p=2)
case("b_c", ol=NHWC, pc_twin=True, **B)
case("b_h", il=NHWC, ol=NHWC, **B)
case("b_pool", ol=NHWC, ob=1, pool=(2, 2), relu=1, **B)
case("b_s8out", ol=S8, **B)
case("b_outc", **B)
case("b_nostem", ol=NHWC, variant=V_TILED, pc_twin=True, **B)
case("b_n16", ol=NHWC, **dict(B, n=16))
case("b_s8in", il=S8, ol=NHWC, **B)

# the f32-input entry
case("f_stem", f32=True, ol=NHWC, pc_twin=True, **B)
case("f_stem_pool", f32=True, ol=NHWC, pool=(2, 2), **B)
case("f_stem_s8", f32=True, ol=S8, ob=1, **B)
case("f_nostem", f32=True, ol=NHWC, variant=V_TILED, **B)
case("f_nostem_pool", f32=True, ol=NHWC, ob=1, pool=(2, 2), variant=V_TILED, **B)
case("f_nostem_s8", f32=True, ol=S8, ob=1, variant=V_TILED, **B)
case("f_nostem_pool_s8", f32=True, ol=S8, ob=1, pool=(2, 2), relu=1, variant=V_TILED, **B)
case("f_refuse_err", f32=True, ol=NHWC, **dict(B, n=16))

# Conv F: c = 5
F = dict(c=5, h=8, w=8, n=8, k=3, s=1, p=1)
case("f_cc", pc_twin=True, **F)
case("f_ch", ol=NHWC, ob=1, **F)
case("f_hc", il=NHWC, ib=1, **F)
case("f_hh", il=NHWC, ol=NHWC, **F)
case("f_relu", relu=1, **F)
case("f_pool", pool=(2, 2), **F)
case("f_force_path_a", il=NHWC, ib=1, ol=NHWC, relu=1, force=True, **A)

# Conv G: two groups of 16 channels (MFMA kernel), depthwise (direct kernel)
G2 = dict(kind="gconv", c=32, h=8, w=8, n=32, k=3, s=1, p=1, groups=2)
GD = dict(kind="gconv", c=16, h=8, w=8, n=16, k=3, s=1, p=1, groups=16)
# Conv T
T2 = dict(kind="deconv", c=32, h=4, w=4, n=16, k=2, s=2, p=0)
TD = dict(kind="deconv", c=16, h=4, w=4, n=16, k=2, s=2, p=0)
T3 = dict(kind="deconv", c=16, h=4, w=4, n=16, k=3, s=2, p=1, op=1)
for tag, G in (("g2", G2), ("gdw", GD), ("t_mfma", T2), ("t_direct", TD), ("t_k3", T3)):
    case(tag + "_cc", **G)
    case(tag + "_hh", il=NHWC, ib=1, ol=NHWC, ob=1, pc_twin=tag in ("g2", "gdw", "t_mfma"), **G)
    case(tag + "_s8", il=S8, ib=1, ol=S8, **G)
    case(tag + "_pool", il=NHWC, ol=NHWC, pool=(2, 2), **G)

# ---- what the recorded maps must reach ------------------------------------------------------------------------------------
LITERAL = ["linear_smalln_dot4", "splitk_reduce", "pad_rows", "im2col_u8_nchw", "relu_u8", "rebias_u8", "dequantize_u8_f32",
           "layout_nchw_to_nhwc", "layout_nhwc_to_nchw", "reborder_u8_nhwc", "maxpool_u8_nhwc", "maxpool_u8_nchw",
           "repack_smallc_u8", "conv_smallc_wstat", "quantize_repack_f32", "gconv_mfma", "gconv_direct", "deconv_mfma",
           "deconv_direct"]
ANY_OF = {  # names built at run time, as the recorder saw them, by the file that launches them
    "i8ie_flin.hip": ["flin_128x16", "flin_64x32"],
    "i8ie_gemm.hip": ["gemm_u8s8_128x32"],
    "i8ie_mlin.hip": ["mlin_64x128"],
    "i8ie_stem.hip": ["stem_conv", "stem_conv_pool"],
    "i8ie_pconv.hip": ["pconv_192x192", "pconv_pool_192x192"],
    "i8ie_igemm.hip (tiled)": ["igemm_conv_128x32", "igemm_conv_128x128", "igemm_lin_128x32"],
}


# ---- operands and references ------------------------------------------------------------------------------------------------
def out_hw(cs):
    if cs["kind"] == "deconv":
        oh, ow = ((d - 1) * cs["s"] - 2 * cs["p"] + cs["k"] + cs["op"] for d in (cs["h"], cs["w"]))
    else:
        oh, ow = ((d - cs["dil"] * (cs["k"] - 1) - 1 + 2 * cs["p"]) // cs["s"] + 1 for d in (cs["h"], cs["w"]))
    if cs["pool"]:
        pk, ps = cs["pool"]
        return oh, ow, (oh - pk) // ps + 1, (ow - pk) // ps + 1
    return oh, ow, oh, ow


_ops = {}


def operands(cs):
    """The layer's operands and scales, drawn once per layer and left unchanged.  s_out follows the accumulators' spread
    (about 20 codes of standard deviation around zp_out), as tests/deconv_ref.py chooses it."""
    lin = cs["kind"] == "lin"
    key = (cs["kind"], cs["m"], cs["n"], cs["pc"], cs["f32"]) + \
          ((cs["K"],) if lin else tuple(cs[f] for f in ("c", "h", "w", "k", "s", "p", "op", "groups")))
    if key in _ops:
        return _ops[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    n = cs["n"]
    if lin:
        q = rng.integers(0, 256, (cs["m"], cs["K"]), dtype=np.uint8)
        qw = rng.integers(-127, 128, (n, cs["K"]), dtype=np.int8)
        kred = float(cs["K"])
    else:
        q = rng.integers(0, 256, (cs["m"], cs["c"], cs["h"], cs["w"]), dtype=np.uint8)
        qw = rng.integers(-127, 128, (n, cs["c"] // cs["groups"], cs["k"], cs["k"]), dtype=np.int8)  # (deconv: the equivalent kernel)
        kred = cs["c"] // cs["groups"] * cs["k"] ** 2 / (float(cs["s"]) ** 2 if cs["kind"] == "deconv" else 1.0)
    d = dict(q=q, qw=qw, qb=rng.integers(-127, 128, n, dtype=np.int8), s_in=S_IN, zp_in=ZP_IN, x=None)
    if cs["f32"]:
        d["x"] = rng.uniform(-2.2, 2.6, q.shape).astype(np.float32)
        d["s_in"], d["zp_in"] = Q_SCALE, Q_ZP
    d["s_wv"] = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, n)) * 2e-3).astype(np.float32)
    d["s_w"] = np.float32(np.median(d["s_wv"]))
    s_ref = float(d["s_wv"].max()) if cs["pc"] else float(d["s_w"])
    spread = np.sqrt(max(kred, 1.0) * (74.0 ** 2 + (127.5 - d["zp_in"]) ** 2)) * 73.0
    d["s_out"] = np.float32(float(d["s_in"]) * s_ref * spread / 20.0)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _ops[key] = d
    return d


def create(gpu, cs, d):
    """the case's layer handle over the operands d, output qparams set (d["zp_out"] when the operands name one)"""
    import deconv_ref
    import dilated_ref
    lib = deconv_ref.bind(dilated_ref.bind(abi.lib()))
    L = C.c_void_p()
    qw, qb, sw = d["qw"].ctypes.data_as(_P), d["qb"].ctypes.data_as(_P), d["s_wv"].ctypes.data_as(_P)
    s_w, n, pc = C.c_float(d["s_w"]), cs["n"], cs["pc"]
    if cs["kind"] == "lin":
        abi.ck(lib.i8ie_linear_create_per_channel(gpu.h, qw, qb, n, cs["K"], sw, C.byref(L)) if pc else
               lib.i8ie_linear_create(gpu.h, qw, qb, n, cs["K"], s_w, C.byref(L)))
    elif cs["kind"] == "deconv":
        a = (gpu.h, qw, qb, n, cs["c"], cs["k"], cs["s"], cs["p"], cs["op"])
        abi.ck(lib.i8ie_conv_transpose2d_create_per_channel(*a, sw, C.byref(L)) if pc else
               lib.i8ie_conv_transpose2d_create(*a, s_w, C.byref(L)))
    elif cs["dil"] > 1:
        a = (gpu.h, qw, qb, n, cs["c"], cs["k"], cs["k"], cs["s"], cs["p"], cs["groups"], cs["dil"])
        abi.ck(lib.i8ie_conv2d_create_dilated_per_channel(*a, sw, C.byref(L)) if pc else
               lib.i8ie_conv2d_create_dilated(*a, s_w, C.byref(L)))
    else:
        a = (gpu.h, qw, qb, n, cs["c"], cs["k"], cs["k"], cs["s"], cs["p"], cs["groups"])
        abi.ck(lib.i8ie_conv2d_create_grouped_per_channel(*a, sw, C.byref(L)) if pc else
               lib.i8ie_conv2d_create_grouped(*a, s_w, C.byref(L)))
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(d["s_out"]), C.c_uint8(d.get("zp_out", ZP_OUT))))
    return L


_refs = {}


def reference(gpu, cs):
    """The expected result in the reference's layout ([m, n] or NCHW), relu and pool applied; computed once per (layer, relu,
    pool) and left unchanged."""
    d = operands(cs)
    key = (id(d), cs["relu"], cs["pool"], cs["force"])
    if key in _refs:
        return _refs[key]
    lib = abi.lib()
    lin = cs["kind"] == "lin"
    q = gpu.quantize(d["x"], Q_SCALE, Q_ZP) if cs["f32"] else d["q"]
    oh, ow, _, _ = out_hw(cs) if not lin else (0, 0, 0, 0)
    if cs["force"]:  # the any-geometry path is the path under test: the oracle (tests/conftest.py puts it on the path)
        import orc
        import pc_pipeline as pcp
        assert cs["kind"] in ("lin", "conv") and cs["groups"] == 1
        a = (q, d["qw"], d["qb"]) + (() if lin else (cs["s"], cs["p"])) + (d["s_in"], d["zp_in"])
        if cs["pc"]:
            ref = (pcp.linear_pc if lin else pcp.conv2d_pc)(*a, d["s_wv"], d["s_out"], ZP_OUT)[0]
        else:
            ref = (orc.linear if lin else orc.conv2d)(*a, d["s_w"], d["s_out"], ZP_OUT, want_acc=True)[0]
    else:
        L = create(gpu, cs, d)
        di = gpu.put(q)
        out = gpu.empty((cs["m"], cs["n"]) if lin else (cs["m"], cs["n"], oh, ow), np.uint8)
        gpu.set_force_fallback(True)
        try:
            abi.ck(lib.i8ie_layer_forward_fused(L, di.ptr, NCHW, 0, cs["m"], 0 if lin else cs["h"], 0 if lin else cs["w"],
                                                C.c_float(d["s_in"]), C.c_uint8(d["zp_in"]), 0, out.ptr, NCHW, 0, None))
        finally:
            gpu.set_force_fallback(False)
        ref = out.get()
        lib.i8ie_layer_destroy(L)
        di.free()
        out.free()
    if cs["relu"]:
        ref = gpu.relu(ref, ZP_OUT)
    if cs["pool"]:
        ref = gpu.max_pool2d(ref, *cs["pool"])
    ref.setflags(write=False)
    _refs[key] = ref
    return ref


def core_message(text):
    """An I8IE_REQUIRE message without the function name in front and the condition behind it."""
    text = text.split(": ", 1)[-1]
    return text[:text.rindex(" (")] if text.endswith(")") and " (" in text else text


# ---- one case through the entry point it names ------------------------------------------------------------------------------
def run(gpu, cs, d=None, want_acc=False):
    """dict(first, warm: launch maps; queries; error: [rc, message] or None; violations; phys: the output region as the call
    left it (None after an error); f32: the dequantized output of a dequant case; guards_ok).  d: the operands, operands(cs)
    when not supplied.  want_acc: the INT32 accumulators land in a guarded region of their own and come back as "acc"
    ([m, n], or [m, oh * ow, n] of the unpooled convolution); the entries of a dequant case take none."""
    lib = abi.lib()
    d = operands(cs) if d is None else d
    zp_out = d.get("zp_out", ZP_OUT)
    lin = cs["kind"] == "lin"
    m, n, il, ol, ib, ob = cs["m"], cs["n"], cs["il"], cs["ol"], cs["ib"], cs["ob"]
    pk, ps = cs["pool"] or (0, 0)
    h, w = (0, 0) if lin else (cs["h"], cs["w"])
    bufs = []
    if lin:
        phys_in = d["q"]
        if cs["flat"]:  # rows handed over as a flattened NHWC activation
            c_, h, w = cs["flat"]
            phys_in = np.ascontiguousarray(d["q"].reshape(m, c_, h, w).transpose(0, 2, 3, 1)).reshape(m, -1)
            il = NHWC
        raw = np.zeros(phys_in.size + 16, np.uint8)
        raw[cs["offset"]:cs["offset"] + phys_in.size] = phys_in.ravel()
        di = gpu.put(raw)
        in_ptr = _P(di.ptr.value + cs["offset"])
        oshape = (m, n)
    else:
        if cs["f32"]:
            phys_in = d["x"]
        else:
            phys_in = abi.Ctx.to_phys(d["q"], ib, d["zp_in"]) if il != NCHW else d["q"]
            if il == S8:
                phys_in = phys_in ^ np.uint8(0x80)
        di = gpu.put(phys_in)
        in_ptr = di.ptr
        _, _, ph, pw = out_hw(cs)
        oshape = (m, ph + 2 * ob, pw + 2 * ob, n) if ol != NCHW else (m, n, ph, pw)
    out = abi.GuardedU8(gpu, oshape)
    bufs += [di, out]
    out_f32 = None
    if cs["dequant"]:
        out_f32 = abi.GuardedU8(gpu, oshape, np.float32)
        bufs.append(out_f32)
    acc, acc_ptr = None, None
    if want_acc:
        assert not cs["dequant"]
        uh, uw, _, _ = (1, 1, 1, 1) if lin else out_hw(cs)
        acc = abi.GuardedU8(gpu, (m, n) if lin else (m, uh * uw, n), np.int32)
        acc_ptr = acc.ptr
        bufs.append(acc)
    ozp = zp_out ^ (0x80 if ol == S8 else 0)
    if ob:
        abi.ck(lib.i8ie_fill_border_u8(gpu.h, out.ptr, m, n, ph, pw, ob, C.c_uint8(ozp)))
    L = create(gpu, cs, d)
    s_in, zp_in, relu = C.c_float(d["s_in"]), C.c_uint8(d["zp_in"]), cs["relu"]

    def forward():
        if cs["dequant"]:
            return lib.i8ie_layer_forward_dequant(L, in_ptr, il, m, h, w, s_in, zp_in, relu,
                                                  None if cs["dequant"] == "null" else out.ptr, out_f32.ptr)
        if cs["f32"]:
            return lib.i8ie_layer_forward_f32_input_pool(L, in_ptr, m, h, w, s_in, zp_in, relu, pk, ps, out.ptr, ol, ob, acc_ptr)
        if cs["pool"]:
            return lib.i8ie_layer_forward_pool(L, in_ptr, il, ib, m, h, w, s_in, zp_in, relu, pk, ps, out.ptr, ol, ob, acc_ptr)
        return lib.i8ie_layer_forward_fused(L, in_ptr, il, ib, m, h, w, s_in, zp_in, relu, out.ptr, ol, ob, acc_ptr)

    res = dict(error=None, phys=None, f32=None)
    gpu.set_variant(cs["variant"])
    gpu.set_force_fallback(cs["force"])
    try:
        res["queries"] = gpu.layer_queries(L, m, h, w, pk, ps)
        for which in ("first", "warm"):
            with gpu.launch_map() as got:
                rc = forward()
            res[which] = got
            if rc != 0:
                res["error"] = [rc, core_message(lib.i8ie_last_error().decode())]
        gpu.sync()
    finally:
        gpu.set_variant(0)
        gpu.set_force_fallback(False)
    if res["error"] is None:
        res["phys"] = out.get()
        if out_f32 is not None:
            res["f32"] = out_f32.get()
        if acc is not None:
            res["acc"] = acc.get()
    res["guards_ok"] = out.guards_ok() and (out_f32 is None or out_f32.guards_ok()) and (acc is None or acc.guards_ok())
    # a query that says "folded" and a launch of its own behind it anyway
    qa, warm, bad = res["queries"], res["warm"], []
    if cs["pool"] and qa["fuses_pool"] and any(k.startswith("maxpool_") for k in warm):
        bad.append("fuses_pool")
    own = [k for k in ("rebias_u8", "reborder_u8_nhwc") if k in warm]
    if ol == S8 and il != S8 and qa["stores_s8"] and own:
        bad.append("stores_s8")
    if il == S8 and ol != S8 and qa["reads_s8"] and "rebias_u8" in warm:
        bad.append("reads_s8")
    if il == S8 and ol == S8 and qa["reads_s8"] and qa["stores_s8"] and own:
        bad.append("reads_s8+stores_s8")
    res["violations"] = bad
    lib.i8ie_layer_destroy(L)
    for b in bufs:
        b.free()
    return res


def expected_phys(cs, ref, zp_out=ZP_OUT):
    if cs["kind"] == "lin" or cs["ol"] == NCHW:
        return ref
    phys = abi.Ctx.to_phys(ref, cs["ob"], zp_out)
    return phys ^ np.uint8(0x80) if cs["ol"] == S8 else phys


RECORDED_FIELDS = ("first", "warm", "queries", "error", "violations")


gpu = support.ctx_fixture()


recorded = support.json_fixture(GOLDEN)


@pytest.mark.parametrize("cid", list(CASES))
def test_route(gpu, recorded, cid):
    cs = CASES[cid]
    assert cid in recorded, "no recorded fingerprint for this case"
    want = recorded[cid]
    got = run(gpu, cs)
    print(cid, {k: got[k] for k in RECORDED_FIELDS})
    assert got["guards_ok"], "a guard byte around the output changed"
    for field in RECORDED_FIELDS:
        assert got[field] == want[field], field
    if got["error"] is not None:
        return
    ref = reference(gpu, cs)
    if cs["dequant"]:
        assert np.array_equal(got["f32"].view(np.uint32), gpu.dequantize(ref, operands(cs)["s_out"], ZP_OUT).view(np.uint32))
        if cs["dequant"] == "null":
            return
    assert np.array_equal(got["phys"], expected_phys(cs, ref))  # (the border ring of a bordered output included)


def test_recorded_maps_reach_every_kernel(recorded):
    assert set(recorded) == set(CASES)
    seen = set()
    for r in recorded.values():
        seen.update(r["first"])
        seen.update(r["warm"])
    missing = [k for k in LITERAL if k not in seen]
    missing += [f for f, names in ANY_OF.items() if not seen.intersection(names)]
    assert not missing, (missing, sorted(seen))


def record(path):
    """Writes the fingerprints of the library as built to `path` (outputs and guards are checked on the way)."""
    gpu = abi.Ctx(0)
    rec, bad = {}, []
    for cid, cs in CASES.items():
        got = run(gpu, cs)
        rec[cid] = {k: got[k] for k in RECORDED_FIELDS}
        ok = got["guards_ok"]
        if got["error"] is None:
            ref = reference(gpu, cs)
            if cs["dequant"]:
                ok = ok and np.array_equal(got["f32"], gpu.dequantize(ref, operands(cs)["s_out"], ZP_OUT))
            if cs["dequant"] != "null":
                ok = ok and np.array_equal(got["phys"], expected_phys(cs, ref))
        print(cid, "ok" if ok else "MISMATCH", json.dumps(rec[cid]), flush=True)
        if not ok:
            bad.append(cid)
    gpu.close()
    seen = sorted({k for r in rec.values() for w in ("first", "warm") for k in r[w]})
    print("names:", seen)
    print("mismatches:", bad)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    import conftest  # noqa: F401  (puts the repository and the oracle on the path)
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python tests/test_gpu_layer_routes.py --record [FILE]")
    sys.exit(record(sys.argv[2] if len(sys.argv) == 3 else GOLDEN))
