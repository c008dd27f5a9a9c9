"""Quantized average pooling restated for the tests.  A helper module, not a conftest.

The reference has no average pool.  Everything but the reduction follows its max_pool2d<u8_t> (src/functional.cc:36-64):
NCHW, window kh x kw, one stride, floor output size, no padding, the input's (scale, zero_point) carried through.
avg_pool2d_u8 is the integer definition q = (S + n // 2) // n in int64, avg_pool2d_f32 the FP32 one (fp32 sum in window
order, rows outer and columns inner, then one fp32 division), avg_pool2d_f64 the float64 mean the FP32 kernel is bounded
against.  forward() walks a residual spec with the two new ops over the oracle, and the three new C symbols get their
ctypes signatures here (tests/abi.py binds the rest)."""
import ctypes as C

import numpy as np

import add_ref as ar
import grouped_ref as gr
import orc
import pc_pipeline as pcp
import pipeline

f32 = np.float32


def out_hw(h, w, kh, kw, s):
    assert 0 < kh <= h and 0 < kw <= w and s > 0
    return (h - kh) // s + 1, (w - kw) // s + 1


def _windows(x, kh, kw, s):
    """the kh * kw strided views of x [n, c, h, w], window rows outer and columns inner"""
    oh, ow = out_hw(x.shape[2], x.shape[3], kh, kw, s)
    for m in range(kh):
        for l in range(kw):
            yield x[:, :, m:m + (oh - 1) * s + 1:s, l:l + (ow - 1) * s + 1:s]


def avg_pool2d_u8(q, kh, kw, s, relu=False, zp=0):
    """u8 [n, c, h, w] -> u8 [n, c, oh, ow]: (S + n // 2) // n with S the exact window sum, then max(q, zp) if relu."""
    q = np.asarray(q, np.uint8)
    n = kh * kw
    assert n <= 65536
    S = None
    for v in _windows(q.astype(np.int64), kh, kw, s):
        S = v.copy() if S is None else S + v
    out = (S + n // 2) // n
    assert out.min() >= 0 and out.max() <= 255
    if relu:
        out = np.maximum(out, int(zp))
    return out.astype(np.uint8)


def global_avg_pool2d_u8(q, relu=False, zp=0):
    return avg_pool2d_u8(q, q.shape[2], q.shape[3], 1, relu, zp)


def avg_pool2d_f32(x, kh, kw, s):
    """float32 in, float32 out: every step one fp32 operation"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        acc = None
        for v in _windows(x, kh, kw, s):
            acc = (f32(0) + v).astype(f32) if acc is None else (acc + v).astype(f32)
        return (acc / f32(kh * kw)).astype(f32)


def avg_pool2d_f64(x, kh, kw, s):
    """(mean, mean of |x|) of every window in float64"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        tot = sum(_windows(x, kh, kw, s))
        mag = sum(_windows(np.abs(x), kh, kw, s))
    return tot / (kh * kw), mag / (kh * kw)


def forward(networks_entry, x, qlayers, out_qparams, add_qparams, per_channel=False):
    """add_ref.forward with ("avgpool", k, s) and ("gap",).  Returns float32 logits."""
    layers, spec, _ = networks_entry

    def run(ops, cur, saved):
        q, s, zp = cur
        for op in ops:
            if op[0] == "layer":
                L = layers[op[1]]
                qw, qb, s_w = qlayers[op[1]]
                s_out, zp_out = out_qparams[op[1]]
                s_out = f32(s_out)
                if L[0] == "conv":
                    f = gr.conv2d_grouped_pc if per_channel else gr.conv2d_grouped
                    q, _ = f(q, qw, qb, gr.layer_groups(L), L[4], L[5], s, zp, s_w, s_out, zp_out)
                elif per_channel:
                    q, _, _ = pcp.linear_pc(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_out, zp_out)
                else:
                    q, _, _ = orc.linear(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_out, zp_out)
                s, zp = s_out, int(zp_out)
            elif op[0] == "relu":
                q = orc.relu(q, zp)
            elif op[0] == "pool":
                q = orc.max_pool2d(q, op[1], op[2])
            elif op[0] == "avgpool":
                q = avg_pool2d_u8(q, op[1], op[1], op[2])
            elif op[0] == "gap":
                q = global_avg_pool2d_u8(q)
            elif op[0] == "save":
                saved[op[1]] = (q, s, zp)
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                q2, s2, zp2 = saved[op[2]]
                s_out, zp_out = add_qparams[op[1]]
                q = ar.add_u8(q, zp, s, q2, zp2, s2, f32(s_out), int(zp_out), relu=False)
                s, zp = f32(s_out), int(zp_out)
            else:
                q = q.reshape(-1, op[1])
        return q, s, zp

    q0 = orc.quantize(x, pipeline.INPUT_SCALE, pipeline.INPUT_ZP)
    q, s, zp = run(spec, (q0, pipeline.INPUT_SCALE, pipeline.INPUT_ZP), {})
    return orc.dequantize(q, s, zp)


# ---- ctypes signatures of the average-pool entry points ------------------------------------------------------------
_P, _I, _B = C.c_void_p, C.c_int, C.c_uint8


def bind(lib):
    lib.i8ie_avgpool2d_u8.argtypes = [_P, _P, _P] + [_I] * 7
    lib.i8ie_avgpool2d_u8_nhwc.argtypes = [_P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_B]
    lib.i8ie_avgpool2d_f32.argtypes = [_P, _P, _P] + [_I] * 7
    for f in (lib.i8ie_avgpool2d_u8, lib.i8ie_avgpool2d_u8_nhwc, lib.i8ie_avgpool2d_f32):
        f.restype = _I
    return lib
