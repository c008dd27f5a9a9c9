"""Grouped / depthwise Conv2d restated for the tests.  A helper module, not a conftest.

A grouped convolution is `groups` independent reference convolutions over channel slices that share the layer's
(s_in, zp_in, s_w, s_out, zp_out): the expected bytes and accumulators are orc.conv2d (per-channel layers:
pc_pipeline.conv2d_pc) per group, concatenated on the channel axis.  The same composition in float64 over
f64_ref.conv2d pins the FP32 path.  The new C symbols get their ctypes signatures here (tests/abi.py binds the rest)."""
import contextlib
import ctypes as C

import numpy as np

import f64_ref
import orc
import pc_pipeline as pcp


def _split(q_in, qw, groups):
    c, kc = q_in.shape[1], qw.shape[0]
    assert groups >= 1 and c % groups == 0 and kc % groups == 0 and qw.shape[1] == c // groups
    return c // groups, kc // groups


def conv2d_grouped(q_in, qw, qb, groups, stride, pad, s_in, zp_in, s_w, s_out, zp_out):
    """q_in u8 [n, c, h, w], qw s8 [kc, c/groups, kh, kw], qb s8 [kc] -> (out u8 NCHW, acc int32 [n, oh*ow, kc])."""
    q_in, qw, qb = np.asarray(q_in, np.uint8), np.asarray(qw, np.int8), np.asarray(qb, np.int8)
    Cg, Ng = _split(q_in, qw, groups)
    outs, accs = [], []
    for g in range(groups):
        o, a = orc.conv2d(q_in[:, g * Cg:(g + 1) * Cg], qw[g * Ng:(g + 1) * Ng], qb[g * Ng:(g + 1) * Ng], stride, pad,
                          s_in, zp_in, s_w, s_out, zp_out, want_acc=True)
        outs.append(o)
        accs.append(a)
    return np.concatenate(outs, axis=1), np.concatenate(accs, axis=2)


def conv2d_grouped_pc(q_in, qw, qb, groups, stride, pad, s_in, zp_in, s_w, s_out, zp_out):
    """the same with one weight scale per output feature, s_w float32 [kc]"""
    q_in, qw, qb = np.asarray(q_in, np.uint8), np.asarray(qw, np.int8), np.asarray(qb, np.int8)
    s_w = np.asarray(s_w, np.float32)
    Cg, Ng = _split(q_in, qw, groups)
    outs, accs = [], []
    for g in range(groups):
        o, a = pcp.conv2d_pc(q_in[:, g * Cg:(g + 1) * Cg], qw[g * Ng:(g + 1) * Ng], qb[g * Ng:(g + 1) * Ng], stride, pad,
                             s_in, zp_in, s_w[g * Ng:(g + 1) * Ng], s_out, zp_out)
        outs.append(o)
        accs.append(a)
    return np.concatenate(outs, axis=1), np.concatenate(accs, axis=2)


def block_diagonal(w, groups):
    """[kc, c/groups, kh, kw] -> the dense [kc, c, kh, kw] weight that is zero outside each group's block"""
    w = np.asarray(w)
    kc, Cg = w.shape[:2]
    Ng = kc // groups
    d = np.zeros((kc, Cg * groups) + w.shape[2:], w.dtype)
    for g in range(groups):
        d[g * Ng:(g + 1) * Ng, g * Cg:(g + 1) * Cg] = w[g * Ng:(g + 1) * Ng]
    return d


def conv2d_f64(x, w, b, groups, stride, pad):
    """float64 grouped conv over f64_ref.conv2d: x [n, c, h, w], w [kc, c/groups, kh, kw], b [kc]"""
    Cg, Ng = x.shape[1] // groups, w.shape[0] // groups
    return np.concatenate([f64_ref.conv2d(x[:, g * Cg:(g + 1) * Cg], w[g * Ng:(g + 1) * Ng], b[g * Ng:(g + 1) * Ng], stride, pad)
                           for g in range(groups)], axis=1)


def conv2d_f64_mag(x, w, b, groups, stride, pad):
    return conv2d_f64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64)),
                      groups, stride, pad)


def layer_groups(L):
    return L[6] if len(L) > 6 else 1


# ---- ctypes signatures of the grouped entry points --------------------------------------------------------------
_P, _I, _F, _B = C.c_void_p, C.c_int, C.c_float, C.c_uint8


def bind(lib):
    lib.i8ie_conv2d_create_grouped.argtypes = [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P]
    lib.i8ie_conv2d_create_grouped_per_channel.argtypes = [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]
    lib.i8ie_layer_groups.argtypes = [_P, _P]
    lib.i8ie_conv2d_u8s8_grouped.argtypes = [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _B, _P, _F, _F, _F, _B, _P, _P]
    lib.i8ie_conv2d_f32_grouped.argtypes = [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]
    for f in (lib.i8ie_conv2d_create_grouped, lib.i8ie_conv2d_create_grouped_per_channel, lib.i8ie_layer_groups,
              lib.i8ie_conv2d_u8s8_grouped, lib.i8ie_conv2d_f32_grouped):
        f.restype = _I
    return lib


@contextlib.contextmanager
def grouped_handles(lib, groups, scales=None):
    """Inside: lib.i8ie_conv2d_create (tests/abi.py's CDLL) makes a grouped layer -- per-channel with `scales` when
    given -- so that the layout / pool / profile helpers of tests/abi.py drive grouped handles unchanged (they take c
    from the input and [kc, c/groups, kh, kw] weights as they come)."""
    bind(lib)
    saved = lib.i8ie_conv2d_create
    if scales is None:
        lib.i8ie_conv2d_create = lambda ctx, qw, qb, kc, c, kh, kw, st, pad, s_w, out: lib.i8ie_conv2d_create_grouped(
            ctx, qw, qb, kc, c, kh, kw, st, pad, groups, s_w, out)
    else:
        sw = np.ascontiguousarray(scales, np.float32)
        p = sw.ctypes.data_as(C.c_void_p)
        lib.i8ie_conv2d_create = lambda ctx, qw, qb, kc, c, kh, kw, st, pad, s_w, out: lib.i8ie_conv2d_create_grouped_per_channel(
            ctx, qw, qb, kc, c, kh, kw, st, pad, groups, p, out)
    try:
        yield
    finally:
        lib.i8ie_conv2d_create = saved
