"""Position embedding with an optional class token restated for the tests (include/i8ie_hip.h, i8ie_posembed_u8_nhwc; DESIGN.md
section 8v).  A helper module, not a conftest.  Every step is one np.float32 operation, in the order the header writes them; the
three new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

f32 = np.float32
WALK = 8  # I8IE_POSEMBED_WALK: images a lane of the nhwc kernel walks, at most
FULL_GRID = 512  # units below which the kernel halves its walk (csrc/i8ie_posembed.hip)
THREADS, MAX_BLOCKS = 256, 256 * 8  # the launch constants of csrc/i8ie_pointwise.h


def table(P, cls=None):
    """E [T', c] float32: P, the class token added into row 0 (one fp32 add)"""
    E = np.array(P, f32, copy=True)
    if cls is not None:
        E[0] = (np.asarray(cls, f32) + E[0]).astype(f32)
    return E


def tokens_of(q):
    """[n, c, h, w] -> [n, T, c]: token j is pixel (j // w, j % w)"""
    n, c, h, w = q.shape
    return q.reshape(n, c, h * w).transpose(0, 2, 1)


def posembed_u8(q, E, class_token, s_in, zp_in, s_out, zp_out, relu=False):
    """uint8 [n, c, h, w] -> uint8 [n, c, h, w], or [n, c, 1, T + 1] with a class token"""
    n, c, h, w = q.shape
    with np.errstate(all="ignore"):
        fa = ((tokens_of(q).astype(np.int32) - np.int32(zp_in)).astype(f32) * f32(s_in)).astype(f32)
        if class_token:
            fa = np.concatenate([np.zeros((n, 1, c), f32), fa], 1)
        j = (fa + np.asarray(E, f32)[None]).astype(f32)
        t = (j / f32(s_out)).astype(f32)
        t = (t + f32(zp_out)).astype(f32)
        inside = np.where((t >= f32(0)) & (t < f32(255)), t, f32(0))
        out = np.where(t >= f32(255), 255, np.where(t < f32(0), 0, np.trunc(inside).astype(np.int32))).astype(np.uint8)
    if relu:
        out = np.maximum(out, np.uint8(zp_out))
    out = out.transpose(0, 2, 1)
    return np.ascontiguousarray(out.reshape(n, c, 1, h * w + 1) if class_token else out.reshape(n, c, h, w))


def posembed_f32(x, E, class_token):
    """float32 [n, c, h, w] -> x + E in fp32; the class column is E[0] itself"""
    n, c, h, w = x.shape
    E = np.asarray(E, f32)
    tok = tokens_of(np.asarray(x, f32))
    if class_token:
        out = np.concatenate([np.broadcast_to(E[:1][None], (n, 1, c)), (tok + E[None, 1:]).astype(f32)], 1)
        return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(n, c, 1, h * w + 1))
    return np.ascontiguousarray((tok + E[None]).astype(f32).transpose(0, 2, 1).reshape(n, c, h, w))


def real_and_bound(q, P, cls, s_in, zp_in, s_out, zp_out):
    """(y*, B) of the header in float64, in the layout posembed_u8 returns: y* from a float64 cat + add of the dequantised tokens,
    the class token and the table, B = 1.01 * 2^-24 * (|Fa| + 3 |X| + |y*|)"""
    n, c, h, w = q.shape
    fa = (tokens_of(q).astype(np.float64) - float(zp_in)) * float(f32(s_in))
    if cls is not None:
        seq = np.concatenate([np.broadcast_to(np.asarray(cls, np.float64)[None, None], (n, 1, c)), fa], 1)
        fa = np.concatenate([np.zeros((n, 1, c)), fa], 1)
    else:
        seq = fa
    X = (seq + np.asarray(P, np.float64)[None]) / float(f32(s_out))
    y = X + float(zp_out)
    B = 1.01 * 2.0 ** -24 * (np.abs(fa / float(f32(s_out))) + 3 * np.abs(X) + np.abs(y))
    shape = (n, c, 1, h * w + 1) if cls is not None else (n, c, h, w)
    return y.transpose(0, 2, 1).reshape(shape), B.transpose(0, 2, 1).reshape(shape)


# (s_in, zp_in, s_out, zp_out, table spread, saturating entries): ordinary scales, zp 0 and 255, table entries that saturate
# either way, a tiny and a huge s_out with a table of their magnitude (not ordinary scales: they take the exact sequence), and a
# negative s_in
SETS = {
    "ordinary": (f32(0.05), 128, f32(0.04), 120, 1.0, ()),
    "zp0": (f32(0.02), 0, f32(0.031), 0, 0.5, ()),
    "zp255": (f32(0.11), 255, f32(0.09), 255, 4.0, ()),
    "saturating": (f32(0.03), 90, f32(0.025), 30, 1.0, (1e9, -1e9, 3e38, -3e38)),
    "tiny_s_out": (f32(2e-37), 128, f32(1e-36), 7, 4e-35, (1.0, -1.0)),
    "huge_s_out": (f32(0.05), 128, f32(1e32), 100, 4e33, (3e38, -3e38)),
    "negative_s_in": (f32(-0.07), 100, f32(0.06), 128, 1.0, ()),
}


def make_table(name, tokens, c, class_token, seed=0):
    """(P [tokens, c], cls [c] or None) of a parameter set: normal entries of the set's spread, the saturating ones planted"""
    spread, extra = SETS[name][4], SETS[name][5]
    rng = np.random.default_rng(1000 + seed + 7 * tokens + c)
    P = rng.normal(0, spread, (tokens, c)).astype(f32)
    flat = P.reshape(-1)
    for i, v in enumerate(extra):
        flat[(3 + 5 * i) % flat.size] = f32(v)
    cls = rng.normal(0, spread, c).astype(f32) if class_token else None
    return P, cls


# ---- ctypes signatures of the new entry points ---------------------------------------------------------------------
_P, _I, _F, _B = C.c_void_p, C.c_int, C.c_float, C.c_uint8


def bind(lib):
    lib.i8ie_posembed_table.argtypes = [_P, _P, _I, _I, _P]
    lib.i8ie_posembed_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _F, _B, _F, _B, _I]
    lib.i8ie_posembed_f32.argtypes = [_P, _P, _P, _I, _I, _I, _I, _I, _P]
    for f in (lib.i8ie_posembed_table, lib.i8ie_posembed_u8_nhwc, lib.i8ie_posembed_f32):
        f.restype = _I
    return lib


def c_table(lib, P, cls):
    """(rc, E) of i8ie_posembed_table"""
    P = np.ascontiguousarray(P, f32)
    E = np.zeros_like(P)
    c = None if cls is None else np.ascontiguousarray(cls, f32)
    rc = lib.i8ie_posembed_table(P.ctypes.data_as(_P), None if c is None else c.ctypes.data_as(_P), P.shape[0], P.shape[1], E.ctypes.data_as(_P))
    return rc, E
