"""Table-driven quantized activations restated for the tests.  A helper module, not a conftest.

The reference's one non-linearity is relu; every other activation is defined in include/i8ie_hip.h as a 256-entry table built
from the reference's own dequantize (src/quantize_utils.cc:38-42) and down_scale's clamp / truncation (:27-36) around f, IEEE
fp32 with one rounding per operation.  act_f32 and table spell that in numpy with an explicit float32 cast between the steps
(sigmoid and tanh through Python's math.exp / math.tanh in float64, the libm the host code calls, then one rounding to
float32), nontrivial() holds the limits the network tests put on the Activations' expected bytes, and the four new C symbols
get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
KINDS = {"relu6": 0, "leaky_relu": 1, "hardsigmoid": 2, "hardswish": 3, "sigmoid": 4, "tanh": 5}

# the launch constants of csrc/i8ie_lut.hip: threads per block, the grid cap, bytes per lane of the widest item
THREADS, MAX_BLOCKS, VEC = 256, 256 * 8, 16


def act_f32(kind, x, param=0.0):
    """f on a float32 array -> float32 array; every step one fp32 operation (sigmoid / tanh: float64 libm, one rounding)"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        if kind == "relu6":
            v = np.where(x > f32(0), x, f32(0)).astype(f32)
            return np.where(v < f32(6), v, f32(6)).astype(f32)
        if kind == "leaky_relu":
            return np.where(x >= f32(0), x, (x * f32(param)).astype(f32)).astype(f32)
        if kind in ("hardsigmoid", "hardswish"):
            v = (x + f32(3)).astype(f32)
            v = np.where(v > f32(0), v, f32(0)).astype(f32)
            h = np.where(v < f32(6), v, f32(6)).astype(f32)
            if kind == "hardsigmoid":
                return (h / f32(6)).astype(f32)
            return ((x * h).astype(f32) / f32(6)).astype(f32)
        if kind == "sigmoid":
            return np.array([f32(1.0 / (1.0 + _exp(-float(v)))) for v in x.ravel()], f32).reshape(x.shape)
        if kind == "tanh":
            return np.array([f32(math.tanh(float(v))) for v in x.ravel()], f32).reshape(x.shape)
    raise ValueError(kind)


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:  # (libm returns +inf there; Python raises)
        return math.inf


def act_f64(kind, x, param=0.0):
    """the real-valued function in float64 (the yardstick of the FP32 entry's sigmoid / tanh, and of spec_ref.fp32_qparams)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if kind == "relu6":
            return np.clip(x, 0.0, 6.0)
        if kind == "leaky_relu":
            return np.where(x >= 0, x, x * np.float64(f32(param)))
        if kind == "hardsigmoid":
            return np.clip(x + 3.0, 0.0, 6.0) / 6.0
        if kind == "hardswish":
            return x * np.clip(x + 3.0, 0.0, 6.0) / 6.0
        if kind == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        return np.tanh(x)


def table(kind, param, s_in, zp_in, s_out, zp_out):
    """uint8[256]: the definition of include/i8ie_hip.h for every input byte"""
    a = np.arange(256, dtype=np.int32)
    with np.errstate(all="ignore"):
        x = ((a - np.int32(zp_in)).astype(f32) * f32(s_in)).astype(f32)
        y = act_f32(kind, x, param)
        t = (y / f32(s_out)).astype(f32)
        t = (t + f32(zp_out)).astype(f32)
        inside = np.where((t >= f32(0)) & (t < f32(255)), t, f32(0))
        return np.where(t >= f32(255), 255, np.where(t < f32(0), 0, np.trunc(inside).astype(np.int32))).astype(np.uint8)


def with_relu(tab, zp_out):
    """a following relu folded into a table"""
    return np.maximum(np.asarray(tab, np.uint8), np.uint8(zp_out))


def act_u8(q, kind, param, s_in, zp_in, s_out, zp_out, relu=False):
    t = table(kind, param, s_in, zp_in, s_out, zp_out)
    return (with_relu(t, zp_out) if relu else t)[np.asarray(q, np.uint8)]


def act_of(op):
    """(kind, param) of an ("act", attr, kind[, param]) op; leaky_relu's default slope is 0.01"""
    return op[2], f32(op[3] if len(op) > 3 else (0.01 if op[2] == "leaky_relu" else 0.0))


# with the seeds of tests/spec_ref.py every Activation's oracle output takes at least MIN_DISTINCT byte values and no value
# holds more than MAX_SHARE of its bytes (tests/test_act_host.py)
MIN_DISTINCT, MAX_SHARE = 16, 0.9


def nontrivial(trace):
    """{attr: (distinct byte values, largest share of one value)} of the Activations' traced bytes, asserted against the two limits"""
    out = {}
    for attr, q in trace.items():
        counts = np.bincount(np.asarray(q, np.uint8).ravel(), minlength=256)
        out[attr] = (int((counts > 0).sum()), float(counts.max()) / q.size)
        assert out[attr][0] >= MIN_DISTINCT and out[attr][1] <= MAX_SHARE, (attr, out[attr])
    return out


# ---- ctypes signatures of the new entry points ---------------------------------------------------------------------
_P, _I, _F, _B, _L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64


def bind(lib):
    lib.i8ie_activation_table.argtypes = [_I, _F, _F, _B, _F, _B, _P]
    lib.i8ie_lut_u8.argtypes = [_P, _P, _P, _L, _P]
    lib.i8ie_lut_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]
    lib.i8ie_activation_f32.argtypes = [_P, _I, _F, _P, _P, _L]
    for f in (lib.i8ie_activation_table, lib.i8ie_lut_u8, lib.i8ie_lut_u8_nhwc, lib.i8ie_activation_f32):
        f.restype = _I
    return lib


def c_table(lib, kind, param, s_in, zp_in, s_out, zp_out):
    """(rc, uint8[256]) of i8ie_activation_table; kind by name or by code"""
    out = np.zeros(256, np.uint8)
    rc = lib.i8ie_activation_table(KINDS.get(kind, kind), float(param), float(s_in), int(zp_in), float(s_out), int(zp_out),
                                   out.ctypes.data_as(C.c_void_p))
    return rc, out


def host_table(tab):
    tab = np.ascontiguousarray(tab, np.uint8)
    assert tab.shape == (256,)
    return tab.ctypes.data_as(C.c_void_p), tab  # (the array is returned to keep it alive over the call)
