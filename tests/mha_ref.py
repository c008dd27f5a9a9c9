"""numpy restatement of the fused multi-head attention (include/i8ie_hip.h, i8ie_attention_u8): per head exactly the
composition attention_ref.matmul_u8 -> softmax_u8 -> matmul_acc / down_scale, the float64 form, and the ctypes side of the
descriptor.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import attention_ref as ar
import orc

MAX_TK = 32768
STRIP_MAX_TK = 1024   # key tokens up to here can take attn_mfma (csrc/i8ie_attention.hip)
P_SCALE = np.float32(1.0 / 256)


def split_packed(qkv):
    """q, k, v of a packed [b, t, 3c] array: its thirds along the last axis"""
    c = qkv.shape[2] // 3
    assert qkv.shape[2] == 3 * c
    return qkv[:, :, :c], qkv[:, :, c:2 * c], qkv[:, :, 2 * c:]


def attention_u8(q, k, v, heads, s_q, zp_q, s_k, zp_k, s_v, zp_v, s_s, zp_s, s_o, zp_o, relu=False):
    """q [b, tq, c], k, v [b, tk, c] u8, c = heads * d; k = v = None: q is packed [b, t, 3c].
    Returns (S [b, H, tq, tk] u8, P [b, H, tq, tk] u8, acc [b, tq, c] int32, O [b, tq, c] u8)."""
    if k is None:
        q, k, v = split_packed(q)
    b, tq, c = q.shape
    tk = k.shape[1]
    assert c % heads == 0 and k.shape == (b, tk, c) and v.shape == (b, tk, c) and tk <= MAX_TK
    d = c // heads
    S = np.empty((b, heads, tq, tk), np.uint8)
    P = np.empty((b, heads, tq, tk), np.uint8)
    acc = np.empty((b, tq, c), np.int32)
    O = np.empty((b, tq, c), np.uint8)
    for h in range(heads):
        cs = slice(h * d, (h + 1) * d)
        S[:, h] = ar.matmul_u8(q[:, :, cs], zp_q, s_q, k[:, :, cs], zp_k, s_k, s_s, zp_s, transpose_b=True)
        P[:, h] = ar.softmax_u8(S[:, h], s_s)
        acc[:, :, cs] = ar.matmul_acc(P[:, h], 0, v[:, :, cs], zp_v)
        o = orc.down_scale(acc[:, :, cs], P_SCALE, s_v, s_o, zp_o)
        O[:, :, cs] = np.maximum(o, np.uint8(zp_o)) if relu else o
    return S, P, acc, O


def attention(q, k, v, heads):
    """float64: (scores [b, H, tq, tk], out [b, tq, c])"""
    if k is None:
        q, k, v = split_packed(q)
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    b, tq, c = q.shape
    d = c // heads
    qh, kh, vh = (a.reshape(a.shape[0], a.shape[1], heads, d).transpose(0, 2, 1, 3) for a in (q, k, v))
    s = np.einsum("bhid,bhjd->bhij", qh, kh)
    o = np.einsum("bhij,bhjd->bhid", ar.softmax(s), vh)
    return s, o.transpose(0, 2, 1, 3).reshape(b, tq, c)


def tokens(x):
    """[n, c, h, w] as the token matrix [n, h * w, c]"""
    n, c, h, w = x.shape
    return np.ascontiguousarray(x.reshape(n, c, h * w).transpose(0, 2, 1))


def pixels(t, h, w):
    """[n, h * w, c] back to [n, c, h, w]"""
    n, _, c = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 1).reshape(n, c, h, w))


# ---- the ("attention", attr, heads[, tag_k, tag_v]) op of a workloads spec --------------------------------------------------
SCORES = ".scores"   # attr + SCORES: the key of an Attention's score (scale, zero_point) in a table of join parameters


def attend_u8(operands, heads, score_qp, s_o, zp_o):
    """attention_u8 on spec_ref operands, each (bytes [n, c, h, w], scale, zp): one packed tensor, or q, k, v"""
    t = [tokens(a[0]) for a in operands]
    q, k, v = operands * 3 if len(operands) == 1 else operands
    return attention_u8(t[0], *(t[1:] or (None, None)), heads, q[1], q[2], k[1], k[2], v[1], v[2],
                        np.float32(score_qp[0]), int(score_qp[1]), s_o, zp_o)


def tracer(into, join_qparams):
    """a trace callback for spec_ref.forward: into[attr] = the output bytes of every Attention, and into[attr + ".S"] /
    into[attr + ".P"] = its scores and probabilities [n, heads, tq, tk], from the operands (where the caller has them) and
    join_qparams[attr + SCORES]"""
    def trace(op, out, operands):
        if op[0] == "attention":
            into[op[1]] = out[0]
            if operands is not None:
                into[op[1] + ".S"], into[op[1] + ".P"] = attend_u8(operands, op[2], join_qparams[op[1] + SCORES], out[1], out[2])[:2]

    return trace


# ---- ctypes ----------------------------------------------------------------------------------------------------------
class AttnMat(C.Structure):
    """i8ie_attn_mat"""
    _fields_ = [("ptr", C.c_void_p), ("batch_stride", C.c_int64), ("token_stride", C.c_int64), ("s8", C.c_int)]


class AttnArgs(C.Structure):
    """i8ie_attention_args"""
    _fields_ = [("b", C.c_int), ("heads", C.c_int), ("d", C.c_int), ("tq", C.c_int), ("tk", C.c_int),
                ("q", AttnMat), ("k", AttnMat), ("v", AttnMat), ("out", AttnMat),
                ("out_h", C.c_int), ("out_w", C.c_int), ("out_border", C.c_int),
                ("s_q", C.c_float), ("s_k", C.c_float), ("s_v", C.c_float), ("s_s", C.c_float), ("s_o", C.c_float),
                ("zp_q", C.c_uint8), ("zp_k", C.c_uint8), ("zp_v", C.c_uint8), ("zp_s", C.c_uint8), ("zp_o", C.c_uint8),
                ("relu", C.c_int), ("scores_dbg_dev", C.c_void_p), ("probs_dbg_dev", C.c_void_p),
                ("acc_dbg_dev", C.c_void_p), ("scores_out_dev", C.c_void_p)]


def bind(lib):
    ar.bind(lib)
    lib.i8ie_attention_u8.argtypes = [C.c_void_p, C.POINTER(AttnArgs)]
    lib.i8ie_attention_f32.argtypes = [C.c_void_p, C.POINTER(AttnArgs)]
    return lib


def mat(ptr, tokens_, channels, s8=False, offset=0):
    """a dense [b, tokens, channels] array at ptr + offset"""
    return AttnMat(ptr + offset, tokens_ * channels, channels, 1 if s8 else 0)
