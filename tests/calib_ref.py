"""Histogram calibration restated in numpy, independently of csrc/i8ie_calib_hist.hip (the definition: include/i8ie_hip.h,
"Histogram calibration"): the observer (exact min / max, the non-finite count, 2048 bins of width 2^e, the fold when e
grows), the three range methods and the reference's last step from a range to (scale, zero_point).  Every result is exact:
the tests compare counts, exponents, ranges and parameters for equality, never within a tolerance."""
import ctypes as C
import math

import numpy as np

f32, f64 = np.float32, np.float64
BINS = 2048
MIN_EXP = -100
METHODS = {"minmax": 0, "percentile": 1, "mse": 2}   # I8IE_CALIB_*
TINY = f32(2.0 ** -126)


# ---- the observer ---------------------------------------------------------------------------------------------------------
def exponent_for(absmax):
    """the smallest integer e >= -100 with absmax < 1024 * 2^e, strictly"""
    if absmax == 0:
        return MIN_EXP
    m, x = math.frexp(float(absmax))   # absmax = m * 2^x, 0.5 <= m < 1: 2^(x-1) <= absmax < 2^x
    return max(MIN_EXP, x - 10)


def bin_index(x, e):
    """bins of canonical finite float32 values: floor of the exact product, in float64"""
    return np.floor(np.asarray(x, f32).astype(f64) * 2.0 ** -e).astype(np.int64) + BINS // 2


def fold(counts, d):
    """d folds: old bin i goes to 512 + i // 2, counts add"""
    for _ in range(min(d, 12)):   # (after 11 folds only bins 1023 and 1024 are occupied, and a fold leaves them in place)
        out = np.zeros(BINS, np.uint64)
        np.add.at(out, BINS // 4 + np.arange(BINS) // 2, counts)
        counts = out
    return counts


class Observer:
    def __init__(self):
        self.min, self.max = f32(np.inf), f32(-np.inf)
        self.nonfinite = 0
        self.exponent = MIN_EXP
        self.counts = np.zeros(BINS, np.uint64)

    def observe(self, x):
        x = np.ascontiguousarray(x, f32).reshape(-1)
        finite = np.isfinite(x)
        self.nonfinite += int((~finite).sum())
        v = x[finite]
        v = np.where(np.abs(v) < TINY, f32(0), v)   # a denormal or a zero of either sign counts as +0
        if v.size == 0:
            return self
        self.min, self.max = f32(min(self.min, v.min())), f32(max(self.max, v.max()))
        e = exponent_for(max(abs(float(self.min)), abs(float(self.max))))
        self.counts = fold(self.counts, e - self.exponent)
        self.exponent = e
        idx = bin_index(v, e)
        assert idx.min() >= 0 and idx.max() < BINS
        self.counts = self.counts + np.bincount(idx, minlength=BINS).astype(np.uint64)
        return self

    def state(self):
        return {"exponent": self.exponent, "counts": self.counts.copy(), "min": float(self.min), "max": float(self.max),
                "nonfinite": self.nonfinite}


def observed(*chunks):
    o = Observer()
    for c in chunks:
        o.observe(c)
    return o.state()


def same_state(got, want):
    return (got["exponent"] == want["exponent"] and got["nonfinite"] == want["nonfinite"]
            and f32(got["min"]).tobytes() == f32(want["min"]).tobytes() and f32(got["max"]).tobytes() == f32(want["max"]).tobytes()
            and got["counts"].dtype == np.uint64 and np.array_equal(got["counts"], want["counts"]))


# ---- range -> (scale, zero_point): the reference's last step (src/calibrator.cc:31-36) ---------------------------------------
def qparams(lo, hi):
    lo, hi = f32(min(f32(lo), f32(0))), f32(max(f32(hi), f32(0)))
    num = f32(255) * (f32(0) - lo)                       # int * float: a float product
    den = f64(f32(hi - lo)) + 1e-09                      # float difference, then the double constant
    zp = int(f64(num) / den) & 0xFF
    scale = f32(hi - lo) / f32(255) if zp == 0 else (f32(0) - lo) / f32(zp)
    if scale == 0:
        scale = f32(1)
    return f32(scale), zp


# ---- the range methods ------------------------------------------------------------------------------------------------------
def _empty(st):
    return int(st["counts"].sum()) == 0


def minmax_range(st):
    return (f32(0), f32(0)) if _empty(st) else (f32(st["min"]), f32(st["max"]))


def percentile_range(st, p):
    assert 50 < p <= 100
    if _empty(st):
        return f32(0), f32(0)
    h = [int(c) for c in st["counts"]]
    k = int(math.floor((1.0 - p / 100.0) * float(sum(h))))
    w = 2.0 ** st["exponent"]
    cum, i = 0, 0
    while True:
        cum += h[i]
        if cum > k:
            break
        i += 1
    cum, j = 0, BINS - 1
    while True:
        cum += h[j]
        if cum > k:
            break
        j -= 1
    lower, upper = (i - 1024) * w, (j - 1023) * w
    lo = f32(lower) if lower > float(st["min"]) else f32(st["min"])
    hi = f32(upper) if upper < float(st["max"]) else f32(st["max"])
    return lo, hi


def mse_error(st, scale, zp):
    """E = sum_i h_i * (c_i - d(c_i))^2 in ascending i, accumulated sequentially in float64 (np.cumsum adds in order)"""
    h = st["counts"]
    keep = h != 0
    c = (np.arange(BINS, dtype=f64) - 1023.5) * 2.0 ** st["exponent"]
    s, z = f64(f32(scale)), f64(zp)
    q = np.minimum(255.0, np.maximum(0.0, np.trunc(c / s + z)))
    r = c - (q - z) * s
    terms = (h.astype(f64) * (r * r))[keep]
    return float(np.cumsum(terms)[-1]) if terms.size else 0.0


def mse_candidates(st):
    lo0, hi0 = f32(min(f32(st["min"]), f32(0))), f32(max(f32(st["max"]), f32(0)))
    return [(j, f32(f64(lo0) * f64(j) / 64.0), f32(f64(hi0) * f64(j) / 64.0)) for j in range(16, 65)]


def mse_range(st, want_j=False):
    if _empty(st):
        return (f32(0), f32(0), None) if want_j else (f32(0), f32(0))
    best = None
    for j, lo, hi in mse_candidates(st):
        err = mse_error(st, *qparams(lo, hi))
        if best is None or err <= best[0]:   # ties go to the larger j
            best = (err, j, lo, hi)
    return (best[2], best[3], best[1]) if want_j else (best[2], best[3])


def range_of(st, method, p=99.99):
    if method == "minmax":
        return minmax_range(st)
    if method == "percentile":
        return percentile_range(st, p)
    assert method == "mse"
    return mse_range(st)


def result_of(st, method, p=99.99):
    """(scale, zero_point, lo, hi) as Layer.calibration_range returns it"""
    lo, hi = range_of(st, method, p)
    s, z = qparams(lo, hi)
    return float(s), z, float(lo), float(hi)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
class Header(C.Structure):
    """i8ie_calib_hist_header"""
    _fields_ = [("min", C.c_float), ("max", C.c_float), ("exponent", C.c_int32), ("scratch", C.c_uint32 * 3), ("nonfinite", C.c_uint64)]


SYMBOLS = ["i8ie_calib_hist_state_bytes", "i8ie_calib_hist_reset", "i8ie_calib_hist_observe_f32", "i8ie_calib_hist_read",
           "i8ie_calib_range_qparams", "i8ie_calib_hist_range"]
_P = C.c_void_p


def bind(lib):
    lib.i8ie_calib_hist_state_bytes.argtypes, lib.i8ie_calib_hist_state_bytes.restype = [], C.c_size_t
    lib.i8ie_calib_hist_reset.argtypes = [_P, _P]
    lib.i8ie_calib_hist_observe_f32.argtypes = [_P, _P, C.c_int64, _P]
    lib.i8ie_calib_hist_read.argtypes = [_P, _P, C.POINTER(Header), _P]
    lib.i8ie_calib_range_qparams.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    lib.i8ie_calib_range_qparams.restype = None
    lib.i8ie_calib_hist_range.argtypes = [C.POINTER(Header), _P, C.c_int, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for n in ("i8ie_calib_hist_reset", "i8ie_calib_hist_observe_f32", "i8ie_calib_hist_read", "i8ie_calib_hist_range"):
        getattr(lib, n).restype = C.c_int
    return lib


def header_of(st):
    return Header(min=float(st["min"]), max=float(st["max"]), exponent=int(st["exponent"]), nonfinite=int(st["nonfinite"]))


def lib_range(lib, st, method, p=99.99):
    """(rc, lo, hi) of i8ie_calib_hist_range on a state dict"""
    h, lo, hi = header_of(st), C.c_float(), C.c_float()
    counts = np.ascontiguousarray(st["counts"], np.uint64)
    rc = lib.i8ie_calib_hist_range(C.byref(h), counts.ctypes.data_as(_P), METHODS[method], C.c_double(p), C.byref(lo), C.byref(hi))
    return rc, f32(lo.value), f32(hi.value)


def lib_qparams(lib, lo, hi):
    s, z = C.c_float(), C.c_uint8()
    lib.i8ie_calib_range_qparams(C.c_float(lo), C.c_float(hi), C.byref(s), C.byref(z))
    return f32(s.value), int(z.value)
