"""Quantized channel concatenation restated for the tests.  A helper module, not a conftest.

The reference has no concat; the definition is a composition of its own dequantize (src/quantize_utils.cc:38-42) and
down_scale's clamp / truncation (src/quantize_utils.cc:27-36) in IEEE fp32, one rounding per operation, plus the copy rule:
an input whose (scale bits, zero point) equal the result's is not touched.  cat_u8 spells it in numpy with an explicit float32
cast between the steps, and the three new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32
MAX_INPUTS = 8


def same_qparams(s_i, zp_i, s_out, zp_out):
    """the copy rule's condition: equal scale BITS (so -0.0 != 0.0 and a NaN equals itself) and equal zero points"""
    return np.array(s_i, f32).view(np.uint32) == np.array(s_out, f32).view(np.uint32) and int(zp_i) == int(zp_out)


def requant_u8(q, s_i, zp_i, s_out, zp_out):
    """the literal sequence on one u8 array (no copy rule, no relu): every step one fp32 operation on float32 arrays"""
    q = np.asarray(q, np.uint8)
    with np.errstate(all="ignore"):
        d = (q.astype(np.int32) - np.int32(zp_i)).astype(f32)
        f = (d * f32(s_i)).astype(f32)
        t = (f / f32(s_out)).astype(f32)
        t = (t + f32(zp_out)).astype(f32)
        inside = np.where((t >= f32(0)) & (t < f32(255)), t, f32(0))
        return np.where(t >= f32(255), 255, np.where(t < f32(0), 0, np.trunc(inside).astype(np.int32))).astype(np.uint8)


def cat_u8(inputs, s_out, zp_out, relu=False):
    """inputs: list of (q u8 [n, c_i, h, w] or [m, f_i], s_i, zp_i) -> u8, joined along axis 1"""
    assert 1 <= len(inputs) <= MAX_INPUTS
    parts = []
    for q, s_i, zp_i in inputs:
        q = np.asarray(q, np.uint8)
        parts.append(q.copy() if same_qparams(s_i, zp_i, s_out, zp_out) else requant_u8(q, s_i, zp_i, s_out, zp_out))
    out = np.concatenate(parts, axis=1)
    if relu:
        out = np.maximum(out, np.uint8(zp_out))
    return out


# ---- ctypes signatures of the concat entry points ------------------------------------------------------------------
_P, _I, _F, _B, _L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64


def bind(lib):
    lib.i8ie_concat_u8.argtypes = [_P, _I, _P, _P, _P, _P, _P, _L, _F, _B, _I]
    lib.i8ie_concat_u8_nhwc.argtypes = [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _B, _I]
    lib.i8ie_concat_f32.argtypes = [_P, _I, _P, _P, _P, _L]
    for f in (lib.i8ie_concat_u8, lib.i8ie_concat_u8_nhwc, lib.i8ie_concat_f32):
        f.restype = _I
    return lib


def ptrs(values):
    """a host array of k device addresses (c_void_p objects or ints)"""
    return (C.c_void_p * len(values))(*[v.value if isinstance(v, C.c_void_p) else v for v in values])


def arr(ctype, values):
    return (ctype * len(values))(*values)


def concat_u8(lib, ctx_h, in_ptrs, lens, s_in, zp_in, out_ptr, outer, s_out, zp_out, relu):
    k = len(in_ptrs)
    return lib.i8ie_concat_u8(ctx_h, k, ptrs(in_ptrs), arr(C.c_int64, lens), arr(C.c_float, [float(s) for s in s_in]),
                              arr(C.c_uint8, [int(z) for z in zp_in]), out_ptr, outer, float(s_out), int(zp_out), 1 if relu else 0)


def concat_u8_nhwc(lib, ctx_h, in_ptrs, c_in, b_in, s8_in, s_in, zp_in, out_ptr, out_border, out_s8, n, h, w, s_out, zp_out, relu):
    k = len(in_ptrs)
    return lib.i8ie_concat_u8_nhwc(ctx_h, k, ptrs(in_ptrs), arr(C.c_int, c_in), arr(C.c_int, b_in), arr(C.c_int, s8_in),
                                   arr(C.c_float, [float(s) for s in s_in]), arr(C.c_uint8, [int(z) for z in zp_in]), out_ptr,
                                   out_border, out_s8, n, h, w, float(s_out), int(zp_out), 1 if relu else 0)


def concat_f32(lib, ctx_h, in_ptrs, lens, out_ptr, outer):
    return lib.i8ie_concat_f32(ctx_h, len(in_ptrs), ptrs(in_ptrs), arr(C.c_int64, lens), out_ptr, outer)
