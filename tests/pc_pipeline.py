"""Per-output-channel weight quantization, restated for the tests ("Per-channel weight scales").

The expected bytes come from the oracle's own contractions: orc.conv2d(..., want_acc=True) and orc.linear(...) return
accumulators that do not depend on s_w, and the per-column requantiser below is the oracle's down_scale with column
j's own scale, written as the same IEEE fp32 sequence in numpy (no contraction: numpy rounds every operation)."""
import contextlib
import ctypes as C

import numpy as np

import orc
import pipeline


def quantize_weight_pc(w, b):
    """a_j = max(max_k |w[j,k]|, |b[j]|); s_w[j] = a_j / 127 (1 when a_j == 0); q = clamp(rint(x / s_w[j]), +-127)."""
    w = np.ascontiguousarray(w, np.float32)
    rows = w.shape[0]
    w2 = w.reshape(rows, -1)
    b = np.zeros(rows, np.float32) if b is None else np.ascontiguousarray(b, np.float32)
    a = np.maximum(np.abs(w2).max(axis=1), np.abs(b)).astype(np.float32)
    s = np.where(a == 0, np.float32(1), a / np.float32(127)).astype(np.float32)
    qw = np.clip(np.rint(w2 / s[:, None]), -127, 127).astype(np.int8).reshape(w.shape)
    qb = np.clip(np.rint(b / s), -127, 127).astype(np.int8)
    return qw, qb, s


def down_scale_pc(acc, sa, s_w, sc, zp):
    """src/quantize_utils.cc:27-36 per column: acc [..., n] int32, s_w [n]."""
    acc = np.asarray(acc, np.int32)
    deq = (acc.astype(np.float32) * np.float32(sa)) * np.asarray(s_w, np.float32)
    q = deq / np.float32(sc) + np.float32(zp)
    out = np.where(q >= 255, 255, np.where(q < 0, 0, np.trunc(np.clip(q, 0, 255))))
    return out.astype(np.uint8)


def conv2d_pc(q_in, qw, qb, stride, pad, s_in, zp_in, s_w, s_out, zp_out):
    """(out u8 NCHW, acc int32 [n, oh*ow, kc])"""
    _, acc = orc.conv2d(q_in, qw, qb, stride, pad, s_in, zp_in, np.float32(1), s_out, zp_out, want_acc=True)
    n, kc = q_in.shape[0], qw.shape[0]
    oh = (q_in.shape[2] - qw.shape[2] + 2 * pad) // stride + 1
    ow = (q_in.shape[3] - qw.shape[3] + 2 * pad) // stride + 1
    out = down_scale_pc(acc, s_in, s_w, s_out, zp_out)  # [n, oh*ow, kc]
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(n, kc, oh, ow)), acc


def linear_pc(q_in, qw, qb, s_in, zp_in, s_w, s_out, zp_out):
    """(out u8 [m, n], acc before the bias step, acc after it)"""
    _, a0, a1 = orc.linear(q_in, qw, qb, s_in, zp_in, np.float32(1), s_out, zp_out, want_acc=True)
    return down_scale_pc(a1, s_in, s_w, s_out, zp_out), a0, a1


def quantize_layers_pc(networks_entry, state_dict):
    return {attr: quantize_weight_pc(state_dict[attr + ".weight"], state_dict[attr + ".bias"]) for attr in networks_entry[0]}


def forward_pc(networks_entry, x, qlayers, out_qparams):
    """pipeline.forward with per-channel layers: {attr: (qw, qb, s_w[n])}."""
    layers, spec, _ = networks_entry
    q = orc.quantize(x, pipeline.INPUT_SCALE, pipeline.INPUT_ZP)
    s, zp = pipeline.INPUT_SCALE, pipeline.INPUT_ZP
    for op in spec:
        if op[0] == "layer":
            L = layers[op[1]]
            qw, qb, s_w = qlayers[op[1]]
            s_out, zp_out = out_qparams[op[1]]
            s_out = np.float32(s_out)
            if L[0] == "conv":
                q, _ = conv2d_pc(q, qw, qb, L[4], L[5], s, zp, s_w, s_out, zp_out)
            else:
                q, _, _ = linear_pc(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_out, zp_out)
            s, zp = s_out, int(zp_out)
        elif op[0] == "relu":
            q = orc.relu(q, zp)
        elif op[0] == "pool":
            q = orc.max_pool2d(q, op[1], op[2])
        else:
            q = q.reshape(-1, op[1])
    return orc.dequantize(q, s, zp)


@contextlib.contextmanager
def per_channel_handles(lib, scales):
    """Inside: the per-tensor create calls of `lib` (tests/abi.py's CDLL) make per-channel layers with `scales`
    instead (their s_w argument is ignored), so that the layout / pool / profile helpers of tests/abi.py drive the
    per-channel handles unchanged."""
    sw = np.ascontiguousarray(scales, np.float32)
    p = sw.ctypes.data_as(C.c_void_p)
    saved = (lib.i8ie_linear_create, lib.i8ie_conv2d_create)
    lin_pc, conv_pc = lib.i8ie_linear_create_per_channel, lib.i8ie_conv2d_create_per_channel
    lib.i8ie_linear_create = lambda ctx, qw, qb, n, k, s_w, out: lin_pc(ctx, qw, qb, n, k, p, out)
    lib.i8ie_conv2d_create = lambda ctx, qw, qb, kc, c, kh, kw, st, pad, s_w, out: conv_pc(ctx, qw, qb, kc, c, kh, kw, st, pad, p, out)
    try:
        yield
    finally:
        lib.i8ie_linear_create, lib.i8ie_conv2d_create = saved
