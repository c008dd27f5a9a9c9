"""The quantized residual Add restated for the tests.  A helper module, not a conftest.

The reference has no add; the definition is a composition of its own dequantize (src/quantize_utils.cc:38-42) and
down_scale's clamp / truncation (src/quantize_utils.cc:27-36) in IEEE fp32, one rounding per operation.  add_u8 spells it
in numpy with an explicit float32 cast between the steps, and the three new C symbols get their ctypes signatures here
(tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32


def add_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu=False):
    """u8 arrays of one shape -> u8.  Every step is one fp32 operation on float32 arrays (nothing is evaluated in double)."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.shape == b.shape
    with np.errstate(all="ignore"):
        da = (a.astype(np.int32) - np.int32(zp_a)).astype(f32)
        db = (b.astype(np.int32) - np.int32(zp_b)).astype(f32)
        fa = (da * f32(s_a)).astype(f32)
        fb = (db * f32(s_b)).astype(f32)
        s = (fa + fb).astype(f32)
        q = (s / f32(s_out)).astype(f32)
        t = (q + f32(zp_out)).astype(f32)
        inside = np.where((t >= f32(0)) & (t < f32(255)), t, f32(0))
        out = np.where(t >= f32(255), 255, np.where(t < f32(0), 0, np.trunc(inside).astype(np.int32))).astype(np.uint8)
    if relu:
        out = np.maximum(out, np.uint8(zp_out))
    return out


# ---- ctypes signatures of the add entry points ---------------------------------------------------------------------
_P, _I, _F, _B, _L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64


def bind(lib):
    lib.i8ie_add_u8.argtypes = [_P, _P, _P, _P, _L, _F, _B, _F, _B, _F, _B, _I]
    lib.i8ie_add_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _F, _B, _F, _B, _F, _B, _I]
    lib.i8ie_add_f32.argtypes = [_P, _P, _P, _P, _L]
    for f in (lib.i8ie_add_u8, lib.i8ie_add_u8_nhwc, lib.i8ie_add_f32):
        f.restype = _I
    return lib
