"""ConvTranspose2d restated for the tests.  A helper module, not a conftest.

The layer is defined as the reference convolution (stride 1, padding 0) of an equivalent problem: the input with s - 1
positions inserted between neighbouring pixels and k - 1 - p (+ output_padding at the bottom / right) around it, every such
position holding zp_in (0.0 in FP32), with the kernel flipped and its channel axes swapped.  equivalent_input /
equivalent_weight build that problem in numpy and deconv_u8 / deconv_u8_pc hand it to orc.conv2d / pc_pipeline.conv2d_pc.
scatter() is the independent definition (every input pixel adds its k x k patch into the output) in float64 or exact
integers.  Also here: the ctypes signatures of the new symbols, tracer() for the up-convs' bytes in a spec_ref.forward, the
case list of the GPU tests with the launcher's dispatch restated, and the runner of a case through a handle."""
import collections
import ctypes as C

import numpy as np

import f64_ref
import orc
import pc_pipeline as pcp

f32 = np.float32


def out_hw(h, w, k, s, p, op):
    return (h - 1) * s - 2 * p + k + op, (w - 1) * s - 2 * p + k + op


def equivalent_input(x, fill, k, s, p, op):
    """x [n, c, h, w] -> x~ [n, c, (h-1) s + 1 + 2 (k-1-p) + op, ...], inserted and padded positions = fill"""
    n, c, h, w = x.shape
    lo = k - 1 - p
    assert s >= 1 and 0 <= p <= k - 1 and 0 <= op < s
    xt = np.full((n, c, (h - 1) * s + 1 + 2 * lo + op, (w - 1) * s + 1 + 2 * lo + op), fill, x.dtype)
    xt[:, :, lo:lo + (h - 1) * s + 1:s, lo:lo + (w - 1) * s + 1:s] = x
    return xt


def equivalent_weight(w):
    """torch's [in, out, k, k] -> W~ [out, in, k, k], W~[oc, ic, ky, kx] = W[ic, oc, k-1-ky, k-1-kx] (its own inverse up to
    the swap of the outer axes)"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def deconv_u8(q_in, qw_eq, qb, s, p, op, s_in, zp_in, s_w, s_out, zp_out):
    """q_in u8 [n, c, h, w], qw_eq s8 [kc, c, k, k] (the equivalent kernel) -> (out u8 NCHW, acc int32 [n, oh*ow, kc])"""
    k = qw_eq.shape[2]
    xt = equivalent_input(np.asarray(q_in, np.uint8), np.uint8(zp_in), k, s, p, op)
    return orc.conv2d(xt, np.asarray(qw_eq, np.int8), np.asarray(qb, np.int8), 1, 0, s_in, zp_in, s_w, s_out, zp_out, want_acc=True)


def deconv_u8_pc(q_in, qw_eq, qb, s, p, op, s_in, zp_in, s_wv, s_out, zp_out):
    k = qw_eq.shape[2]
    xt = equivalent_input(np.asarray(q_in, np.uint8), np.uint8(zp_in), k, s, p, op)
    return pcp.conv2d_pc(xt, np.asarray(qw_eq, np.int8), np.asarray(qb, np.int8), 1, 0, s_in, zp_in, np.asarray(s_wv, f32), s_out, zp_out)


def scatter(x, w, b, s, p, op, dtype=np.float64):
    """the transposed convolution by its definition: x [n, c, h, w], w [c, kc, k, k] (torch), b [kc]"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    n, c, h, wd = x.shape
    kc, k = w.shape[1], w.shape[2]
    oh, ow = out_hw(h, wd, k, s, p, op)
    full = np.zeros((n, kc, (h - 1) * s + k + op, (wd - 1) * s + k + op), dtype)
    for ky in range(k):
        for kx in range(k):
            full[:, :, ky:ky + (h - 1) * s + 1:s, kx:kx + (wd - 1) * s + 1:s] += np.einsum("nchw,cj->njhw", x, w[:, :, ky, kx])
    return full[:, :, p:p + oh, p:p + ow] + np.asarray(b, dtype).reshape(1, -1, 1, 1)


def scatter_mag(x, w, b, s, p, op):
    return scatter(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64)), s, p, op)


def equivalent_f64(x, w, b, s, p, op):
    """the same through the equivalent problem and f64_ref.conv2d"""
    k = w.shape[2]
    return f64_ref.conv2d(equivalent_input(np.asarray(x, np.float64), 0.0, k, s, p, op), equivalent_weight(np.asarray(w, np.float64)),
                          np.asarray(b, np.float64), 1, 0)


# ---- spec networks -----------------------------------------------------------------------------------------------------
def tracer(layers, into):
    """a trace callback for spec_ref.forward: into[attr] = the output bytes of every "deconv" layer"""
    def trace(op, out, operands):
        if op[0] == "layer" and layers[op[1]][0] == "deconv":
            into[op[1]] = out[0]

    return trace


# ---- ctypes signatures of the new entry points -----------------------------------------------------------------------------
_P, _I, _F, _B = C.c_void_p, C.c_int, C.c_float, C.c_uint8


def bind(lib):
    lib.i8ie_conv_transpose2d_create.argtypes = [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P]
    lib.i8ie_conv_transpose2d_create_per_channel.argtypes = [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]
    lib.i8ie_conv_transpose2d_u8s8.argtypes = [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _B, _P, _F, _F, _F, _B, _P, _P]
    lib.i8ie_conv_transpose2d_f32.argtypes = [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P]
    for f in (lib.i8ie_conv_transpose2d_create, lib.i8ie_conv_transpose2d_create_per_channel, lib.i8ie_conv_transpose2d_u8s8,
              lib.i8ie_conv_transpose2d_f32):
        f.restype = _I
    return lib


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------------
S_IN, ZP_IN, ZP_OUT = f32(0.03), 121, 37

Case = collections.namedtuple("Case", "name m c kc k s p op h w in_nhwc out_nhwc ib ob pc force zp_in extreme zero_col classes")
Dispatch = collections.namedtuple("Dispatch", "kernel G dot4 pc vec_out nph")


def taps(k, s, r):
    return (k - r + s - 1) // s if r < k else 0


def geom(case):
    """(OH, OW, K of the equivalent matrix, the longest phase K, cells of the input-grid tiling)"""
    oh, ow = out_hw(case.h, case.w, case.k, case.s, case.p, case.op)
    T = taps(case.k, case.s, 0)
    cells = case.m * ((oh - 1 + case.p) // case.s + 1) * ((ow - 1 + case.p) // case.s + 1)
    return oh, ow, case.c * case.k * case.k, case.c * T * T, cells


def dispatch(case):
    """i8ie_deconv_mfma_takes and the `dot4` / `vec_out` / k == s == 2 expressions of i8ie_deconv_launch, restated (every
    buffer of the tests is an allocation of its own: the alignment terms are true)"""
    G = 16 if case.c % 16 == 0 else (4 if case.c % 4 == 0 else 1)
    vec_out = 1 if case.kc % 4 == 0 else 0
    if not case.force and geom(case)[3] >= 32:
        return Dispatch("deconv_mfma", G, None, bool(case.pc), vec_out, 4 if case.k == 2 and case.s == 2 else 1)
    return Dispatch("deconv_direct", None, case.c % 4 == 0, bool(case.pc), vec_out, None)


def _mk(name, m, c, kc, geo, h, w, lay="cc", ib=0, ob=0, pc=False, force=False, zp_in=ZP_IN, extreme=False, zero_col=False,
        classes=()):
    k, s, p, op = geo
    return Case(name, m, c, kc, k, s, p, op, h, w, lay[0] == "h", lay[1] == "h", ib, ob, pc, force, zp_in, extreme, zero_col,
                tuple(classes))


def _both(name, *a, **kw):
    return [_mk(name + "-pt", *a, pc=False, **kw), _mk(name + "-pc", *a, pc=True, **kw)]


# the geometries the issue names, (k, s, p, op)
GEOMETRIES = [(2, 2, 0, 0), (3, 2, 1, 1), (4, 2, 1, 0), (3, 1, 1, 0), (1, 2, 0, 1), (5, 3, 2, 2), (3, 2, 0, 0), (3, 3, 2, 0),
              (2, 2, 0, 1)]


def _cases():
    E = []
    #           name                 m   c   kc  (k, s, p, op)   h  w
    # ---- geometry, each on deconv_mfma (the direct kernel takes them again under force-fallback) -------------------------
    E += _both("geo_k2s2",           2,  32, 16, (2, 2, 0, 0),   3, 4, classes=["geo", "in32", "phk32", "out16"])
    E += _both("geo_k3s2p1op1",      2,  16, 17, (3, 2, 1, 1),   3, 4, classes=["geo", "in16", "phk64", "out17"])
    E += _both("geo_k4s2p1",         2,   8,  3, (4, 2, 1, 0),   4, 3, classes=["geo", "out3"])
    E += _both("geo_k3s1p1",         2,   4, 16, (3, 1, 1, 0),   4, 5, classes=["geo", "in4", "single_phase"])
    E += _both("geo_k1s2op1",        2,  32,  8, (1, 2, 0, 1),   3, 3, classes=["geo", "empty_phase"])
    E += _both("geo_k5s3p2op2",      1,   8, 16, (5, 3, 2, 2),   3, 4, classes=["geo"])
    E += _both("geo_k3s2",           2,  20, 12, (3, 2, 0, 0),   3, 3, classes=["geo", "in20"])
    E += _both("geo_k3s3p2",         2,  32,  4, (3, 3, 2, 0),   3, 4, classes=["geo", "p_eq_k1"])
    E += _both("geo_k2s2op1",        2,  64,  1, (2, 2, 0, 1),   2, 3, classes=["geo", "in64", "out1", "op_eq_s1"])
    # ---- channels: in 1 3 (direct / byte gather), 65; phase K 31 63 65 128; out 63 64 65 --------------------------------
    E += _both("in1_direct",         2,   1,  5, (3, 1, 1, 0),   4, 4, classes=["in1"])
    E += _both("in3_k4_bytes",       2,   3, 16, (4, 1, 1, 0),   4, 5, classes=["in3"])
    E += _both("phk31_direct",       2,  31,  8, (2, 2, 0, 0),   3, 3, classes=["phk31"])
    E += _both("phk63_in7",          2,   7, 63, (3, 1, 1, 0),   3, 4, classes=["phk63", "out63"])
    E += _both("phk65_in65",         2,  65, 64, (2, 2, 0, 0),   2, 3, classes=["phk65", "in65", "out64"])
    E += _both("phk128_out65",       1,  32, 65, (4, 2, 1, 0),   3, 3, classes=["phk128", "out65"])
    E += _both("direct_dot4_in4",    2,   4,  6, (2, 2, 0, 0),   3, 4, classes=["direct_dot4"])
    E += _both("direct_k1s2",        2,   8,  7, (1, 2, 0, 1),   3, 2, classes=["direct_empty_phase"])
    # ---- tiles: 1 x 1, 1 x W, H x 1 inputs; 1, 15-17 and 127-129 cells across image boundaries --------------------------
    E += _both("tile_1x1_cells1",    1,  32, 16, (2, 2, 0, 0),   1, 1, classes=["in1x1", "cells1"])
    E += _both("tile_1xw_cells15",   5,  32,  8, (2, 2, 0, 0),   1, 3, classes=["in1xw", "cells15"])
    E += _both("tile_cells16",       4,  32,  8, (2, 2, 0, 0),   2, 2, classes=["cells16"])
    E += _both("tile_cells17",      17,  32,  8, (2, 2, 0, 0),   1, 1, classes=["cells17"])
    E += _both("tile_hx1",           2,  32,  8, (2, 2, 0, 0),   4, 1, classes=["inhx1"])
    E += _both("tile_cells127",    127,  32,  4, (2, 2, 0, 0),   1, 1, classes=["cells127"])
    E += _both("tile_cells128",     32,  32,  4, (2, 2, 0, 0),   2, 2, classes=["cells128"])
    E += _both("tile_cells129",     43,  32,  4, (2, 2, 0, 0),   1, 3, classes=["cells129"])
    E += _both("tile_k3s2_ragged",  43,  16,  4, (3, 2, 1, 1),   1, 3, classes=["ragged_phase_loop"])
    # ---- layouts -------------------------------------------------------------------------------------------------------
    for lay in ("cc", "ch", "hc", "hh"):
        E += _both("lay_" + lay,     2,  16, 16, (3, 2, 1, 1),   3, 3, lay=lay, ob=1 if lay[1] == "h" else 0, classes=["lay_" + lay])
    for ib in (0, 1, 2):
        E += _both("ib%d" % ib,      2,  32, 16, (2, 2, 0, 0),   3, 2, lay="hc", ib=ib, classes=["ib%d" % ib])
    for ob in (0, 1, 2):
        E += _both("ob%d" % ob,      2,   8, 12, (4, 2, 1, 0),   2, 3, lay="ch", ob=ob, classes=["ob%d" % ob])
    # ---- values ----------------------------------------------------------------------------------------------------------
    E += _both("zp0",                2,  16,  8, (3, 2, 1, 1),   3, 3, zp_in=0, classes=["zp0"])
    E += _both("zp255",              2,  16,  8, (3, 2, 0, 0),   3, 3, zp_in=255, classes=["zp255"])
    E += _both("extreme",            1,  64,  8, (4, 2, 1, 0),   3, 3, extreme=True, classes=["extreme"])
    E += [_mk("zero_scale_row-pc",   2,  32,  7, (2, 2, 0, 0),   3, 3, pc=True, zero_col=True, classes=["zero_col"])]
    return E


CASES = _cases()
CLASSES = (["geo", "single_phase", "empty_phase", "p_eq_k1", "op_eq_s1", "direct_dot4", "direct_empty_phase", "extreme", "zero_col",
            "zp0", "zp255", "in1x1", "in1xw", "inhx1", "ragged_phase_loop"]
           + ["in%d" % c for c in (1, 3, 4, 16, 20, 64, 65)] + ["phk%d" % k for k in (31, 32, 63, 64, 65, 128)]
           + ["out%d" % n for n in (1, 3, 16, 17, 63, 64, 65)] + ["cells%d" % n for n in (1, 15, 16, 17, 127, 128, 129)]
           + ["lay_" + l for l in ("cc", "ch", "hc", "hh")] + ["ib0", "ib1", "ib2", "ob0", "ob1", "ob2"])

_cache = {}


def reference(case):
    """operands (the weight in torch's layout and as the equivalent matrix), scales and the oracle's (out NCHW, acc), computed
    once per case and left unchanged.  s_out follows the accumulators' spread as tests/grouped_cases.py chooses it, with the
    average number of real taps of an output pixel, c k^2 / s^2 (at least 1), in the place of K: about 20 codes of standard
    deviation around zp_out per tensor, and for the column with the largest weight scale per channel."""
    key = case._replace(in_nhwc=False, out_nhwc=False, ib=0, ob=0, force=False, classes=())
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(sum(map(ord, case.name.rsplit("-", 1)[0])))
    q = rng.integers(0, 256, (case.m, case.c, case.h, case.w), dtype=np.uint8)
    wt = rng.integers(-127, 128, (case.c, case.kc, case.k, case.k), dtype=np.int8)  # torch's layout
    qb = rng.integers(-127, 128, case.kc, dtype=np.int8)
    s_wv = (np.exp(rng.uniform(np.log(1.0 / 30), 0.0, case.kc)) * 2e-3).astype(f32)
    s_w = f32(np.median(s_wv))
    kreal = max(case.c * case.k * case.k / float(case.s * case.s), 1.0)
    spread = np.sqrt(kreal * (74.0 ** 2 + (127.5 - case.zp_in) ** 2)) * 73.0
    s_ref = float(s_wv.max()) if case.pc else float(s_w)  # (per channel: the widest column gets the 20 codes)
    s_out = f32(S_IN * s_ref * spread / 20.0)
    if case.extreme:  # every input byte 255, weight rows alternating 127 / -128: at most 30 codes either side of zp_out
        q[...] = 255
        wt[:, 0::2], wt[:, 1::2] = 127, -128
        s_out = f32(S_IN * s_ref * kreal * 255.0 * 128.0 / 30.0)
    if case.zero_col:
        s_wv[case.kc - 1] = 0.0
    qw = equivalent_weight(wt)
    if case.pc:
        want, acc = deconv_u8_pc(q, qw, qb, case.s, case.p, case.op, S_IN, case.zp_in, s_wv, s_out, ZP_OUT)
    else:
        want, acc = deconv_u8(q, qw, qb, case.s, case.p, case.op, S_IN, case.zp_in, s_w, s_out, ZP_OUT)
    for a in (q, wt, qw, qb, s_wv, want, acc):
        a.setflags(write=False)
    _cache[key] = dict(q=q, wt=wt, qw=qw, qb=qb, s_w=s_w, s_wv=s_wv, s_out=s_out, want=want, acc=acc)
    return _cache[key]


def create(lib, ctx, d, case):
    """a transposed handle of the case (per-channel with the case's scales when case.pc), output qparams set"""
    L = C.c_void_p()
    import abi
    qw, qb = np.ascontiguousarray(d["qw"]), np.ascontiguousarray(d["qb"])
    if case.pc:
        sw = np.ascontiguousarray(d["s_wv"], f32)
        abi.ck(lib.i8ie_conv_transpose2d_create_per_channel(ctx.h, qw.ctypes.data_as(_P), qb.ctypes.data_as(_P), case.kc, case.c, case.k,
                                                            case.s, case.p, case.op, sw.ctypes.data_as(_P), C.byref(L)))
    else:
        abi.ck(lib.i8ie_conv_transpose2d_create(ctx.h, qw.ctypes.data_as(_P), qb.ctypes.data_as(_P), case.kc, case.c, case.k, case.s,
                                                case.p, case.op, C.c_float(d["s_w"]), C.byref(L)))
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(d["s_out"]), C.c_uint8(ZP_OUT)))
    return L


def run_handle(ctx, case, relu, pool=None, in_s8=False, out_s8=False, **over):
    """the case through i8ie_layer_forward_fused (or _pool) on a transposed handle, output and accumulators in guarded
    regions.  Returns dict(out NCHW, acc, phys (the whole physical output, a re-bias undone), ok (no guard byte changed),
    names (kernels launched))."""
    import abi
    lib = bind(abi.lib())
    d = reference(case)
    c = case._replace(**over) if over else case
    oh, ow = geom(c)[:2]
    ph, pw = (oh, ow) if pool is None else ((oh - pool[0]) // pool[1] + 1, (ow - pool[0]) // pool[1] + 1)
    ctx.set_force_fallback(c.force)
    L = create(lib, ctx, d, c)
    phys_in = abi.Ctx.to_phys(d["q"], c.ib, c.zp_in) if c.in_nhwc else d["q"]
    if in_s8:
        phys_in = phys_in ^ np.uint8(0x80)
    di = ctx.put(np.ascontiguousarray(phys_in))
    oshape = (c.m, ph + 2 * c.ob, pw + 2 * c.ob, c.kc) if c.out_nhwc else (c.m, c.kc, ph, pw)
    out, acc = abi.GuardedU8(ctx, oshape), abi.GuardedU8(ctx, (c.m, oh * ow, c.kc), np.int32)
    if c.out_nhwc and c.ob:
        abi.ck(lib.i8ie_fill_border_u8(ctx.h, out.ptr, c.m, c.kc, ph, pw, c.ob, C.c_uint8(ZP_OUT ^ (0x80 if out_s8 else 0))))
    il = (2 if in_s8 else 1) if c.in_nhwc else 0
    ol = (2 if out_s8 else 1) if c.out_nhwc else 0
    names = []
    abi.ck(lib.i8ie_profile_start(ctx.h, 0))
    try:
        if pool is None:
            abi.ck(lib.i8ie_layer_forward_fused(L, di.ptr, il, c.ib, c.m, c.h, c.w, C.c_float(S_IN), C.c_uint8(c.zp_in), 1 if relu else 0,
                                                out.ptr, ol, c.ob, acc.ptr))
        else:
            abi.ck(lib.i8ie_layer_forward_pool(L, di.ptr, il, c.ib, c.m, c.h, c.w, C.c_float(S_IN), C.c_uint8(c.zp_in), 1 if relu else 0,
                                               pool[0], pool[1], out.ptr, ol, c.ob, acc.ptr))
    finally:
        ents, cnt = (abi.ProfEntry * 64)(), C.c_int(0)
        abi.ck(lib.i8ie_profile_stop(ctx.h, ents, 64, C.byref(cnt)))
        names.extend(ents[i].name.decode().split("|")[0] for i in range(cnt.value))
        ctx.set_force_fallback(False)
    try:
        phys = out.get()
        if out_s8:
            phys = phys ^ np.uint8(0x80)
        o = phys
        if c.out_nhwc:
            b = c.ob
            o = np.ascontiguousarray((phys[:, b:-b, b:-b, :] if b else phys).transpose(0, 3, 1, 2))
        return dict(out=o, acc=acc.get(), phys=phys, ok=out.guards_ok() and acc.guards_ok(), names=names)
    finally:
        lib.i8ie_layer_destroy(L)
        for bb in (di, out, acc):
            bb.free()
