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


# ---- the test network of tests/test_gpu_mha.py and its numpy walk ----------------------------------------------------------
# 3x32x32 -> conv 3x3 s2, relu, max-pool 2/2 (8x8, t = 64) -> [LayerNorm, packed 1x1 conv 16 -> 48, Attention(2) at d = 8,
# 1x1 conv] + skip -> relu, conv 3x3 s2 with padding (4x4, t = 16) -> [three 1x1 convs, Attention(2) at d = 16, 1x1 conv] + skip
# -> relu, global average pool, fc.  Layers in workloads' notation: ("conv", in, out, k, stride, pad), ("ln", c), ("fc", in, out).
NET_INPUT = (3, 32, 32)
NET_HEADS = 2
NET_LAYERS = {
    "c1": ("conv", 3, 16, 3, 2, 1), "ln1": ("ln", 16), "qkv1": ("conv", 16, 48, 1, 1, 0), "proj1": ("conv", 16, 16, 1, 1, 0),
    "c2": ("conv", 16, 32, 3, 2, 1), "q2": ("conv", 32, 32, 1, 1, 0), "k2": ("conv", 32, 32, 1, 1, 0), "v2": ("conv", 32, 32, 1, 1, 0),
    "proj2": ("conv", 32, 32, 1, 1, 0), "fc": ("fc", 32, 10)}
NET_JOINS = ("attn1", "add1", "attn2", "add2")          # the modules without weights: output_qparams() beside the layers
NET_ATTENTIONS = ("attn1", "attn2")                     # ... of which these have score_qparams() too
NET_TRACED = ("pool", "ln1", "qkv1", "attn1", "add1", "c2", "attn2", "add2", "gap")
WEIGHT_SEED, CALIB_SEED, INPUT_SEED = 42, 99, 5
INPUT_SCALE, INPUT_ZP = np.float32(0.025), 127


def net_state_dict(seed=WEIGHT_SEED):
    """He-uniform weights and U(-1, 1) / sqrt(fan_in) biases, gamma from U(0.5, 1.5), beta from U(-0.3, 0.3).  The 1 / sqrt(d)
    of scaled-dot-product attention is folded into the query projections: the first 16 filters of qkv1, and q2."""
    rng = np.random.default_rng(seed)
    sd = {}
    for attr, L in NET_LAYERS.items():
        if L[0] == "ln":
            sd[attr + ".weight"] = rng.uniform(0.5, 1.5, L[1]).astype(np.float32)
            sd[attr + ".bias"] = rng.uniform(-0.3, 0.3, L[1]).astype(np.float32)
            continue
        shape = (L[2], L[1], L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
        fan_in = int(np.prod(shape[1:]))
        fold = np.ones(shape[0], np.float64)
        if attr == "qkv1":
            fold[:16] = 1.0 / np.sqrt(16 // NET_HEADS)
        elif attr == "q2":
            fold[:] = 1.0 / np.sqrt(32 // NET_HEADS)
        w = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)
        sd[attr + ".weight"] = (w * fold.reshape((-1,) + (1,) * (len(shape) - 1))).astype(np.float32)
        sd[attr + ".bias"] = (rng.uniform(-1, 1, shape[0]) / np.sqrt(fan_in) * fold).astype(np.float32)
    return sd


def net_input(batch, seed=INPUT_SEED):
    """normalised-image-like input, inside quantize()'s no-wrap window for INPUT_SCALE / INPUT_ZP"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (batch,) + NET_INPUT).astype(np.float32)
    a = rng.uniform(0.2, 1.0, (batch, NET_INPUT[0], 1, 1)).astype(np.float32)
    return ((u * a - np.float32(0.45)) / np.float32(0.226)).astype(np.float32)


def net_quantize_layers(state_dict, per_channel=False):
    """convert()'s weight rules; a LayerNorm keeps its float32 (gamma, beta)"""
    import pc_pipeline as pcp

    rule = pcp.quantize_weight_pc if per_channel else orc.quantize_weight
    out = {}
    for attr, L in NET_LAYERS.items():
        w, b = state_dict[attr + ".weight"], state_dict[attr + ".bias"]
        out[attr] = (w, b) if L[0] == "ln" else tuple(rule(w, b))
    return out


def net_forward(x, qlayers, qp, score_qp, per_channel=False, trace=None):
    """float32 logits of the test network.  qlayers: net_quantize_layers(); qp: {attr: (scale, zp)} of NET_LAYERS and NET_JOINS;
    score_qp: the same of the scores of NET_ATTENTIONS.  trace: a dict that receives the bytes of NET_TRACED, and of each
    attention its scores and probabilities as attr + ".S" and attr + ".P"."""
    import add_ref
    import avgpool_ref as apr
    import grouped_ref as gr
    import layernorm_ref as lnr
    import pc_pipeline as pcp

    def out_of(table, attr):
        s, zp = table[attr]
        return np.float32(s), int(zp)

    def layer(attr, cur):
        (q, s, zp), L, (s_o, zp_o) = cur, NET_LAYERS[attr], out_of(qp, attr)
        if L[0] == "ln":
            return (lnr.layer_norm_any(q, s, np.float32(1e-5), qlayers[attr][0], qlayers[attr][1], s_o, zp_o), s_o, zp_o)
        qw, qb, s_w = qlayers[attr]
        if L[0] == "conv":
            f = gr.conv2d_grouped_pc if per_channel else gr.conv2d_grouped
            return (f(q, qw, qb, 1, L[4], L[5], s, zp, s_w, s_o, zp_o)[0], s_o, zp_o)
        f = pcp.linear_pc if per_channel else orc.linear
        return (f(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_o, zp_o)[0], s_o, zp_o)

    def attend(attr, q, k, v):
        """q, k, v: (bytes [n, c, h, w], scale, zp), or k = v = None for the packed form"""
        (s_s, zp_s), (s_o, zp_o) = out_of(score_qp, attr), out_of(qp, attr)
        k, v = (q, q) if k is None else (k, v)
        packed = k is q
        S, P, _, O = attention_u8(tokens(q[0]), None if packed else tokens(k[0]), None if packed else tokens(v[0]), NET_HEADS,
                                  q[1], q[2], k[1], k[2], v[1], v[2], s_s, zp_s, s_o, zp_o)
        keep(attr + ".S", S)
        keep(attr + ".P", P)
        return (pixels(O, q[0].shape[2], q[0].shape[3]), s_o, zp_o)

    def add(attr, a, b):
        s_o, zp_o = out_of(qp, attr)
        return (add_ref.add_u8(a[0], a[2], a[1], b[0], b[2], b[1], s_o, zp_o, relu=False), s_o, zp_o)

    def relu(cur):
        return (orc.relu(cur[0], cur[2]), cur[1], cur[2])

    def keep(name, q):
        if trace is not None:
            trace[name] = q

    def kept(name, cur):
        keep(name, cur[0])
        return cur

    cur = (orc.quantize(x, INPUT_SCALE, INPUT_ZP), INPUT_SCALE, INPUT_ZP)
    cur = relu(layer("c1", cur))
    cur = kept("pool", (orc.max_pool2d(cur[0], 2, 2), cur[1], cur[2]))
    y = kept("qkv1", layer("qkv1", kept("ln1", layer("ln1", cur))))
    y = kept("attn1", attend("attn1", y, None, None))
    cur = kept("add1", add("add1", layer("proj1", y), cur))
    cur = kept("c2", layer("c2", relu(cur)))
    y = kept("attn2", attend("attn2", layer("q2", cur), layer("k2", cur), layer("v2", cur)))
    cur = kept("add2", add("add2", layer("proj2", y), cur))
    cur = relu(cur)
    cur = kept("gap", (apr.global_avg_pool2d_u8(cur[0]), cur[1], cur[2]))
    return orc.dequantize(*layer("fc", cur))


def net_fp32_qparams(state_dict, x):
    """Stand-in for calibration without a GPU (spec_ref.fp32_qparams' method): a float64 forward over the FP32 weights; the
    range of every layer, join and score tensor gives its (scale, zero_point).  Returns (qp, score_qp)."""
    import f64_ref
    import grouped_ref as gr
    import layernorm_ref as lnr
    import spec_ref as sr

    qp, sq = {}, {}

    def note(table, attr, v):
        table[attr] = sr.range_qparams(v.min(), v.max())
        return v

    def layer(attr, v):
        L = NET_LAYERS[attr]
        w, b = state_dict[attr + ".weight"].astype(np.float64), state_dict[attr + ".bias"].astype(np.float64)
        if L[0] == "ln":
            return note(qp, attr, np.ascontiguousarray(np.moveaxis(lnr.layer_norm_f64(np.moveaxis(v, 1, -1), w, b, 1e-5), -1, 1)))
        if L[0] == "conv":
            return note(qp, attr, gr.conv2d_f64(v, w, b, 1, L[4], L[5]))
        return note(qp, attr, f64_ref.linear(v.reshape(v.shape[0], -1), w, b))

    def attend(attr, q, k, v):
        s, o = attention(tokens(q), None if k is None else tokens(k), None if v is None else tokens(v), NET_HEADS)
        note(sq, attr, s)
        return note(qp, attr, pixels(o, q.shape[2], q.shape[3]))

    v = np.maximum(layer("c1", np.asarray(x, np.float64)), 0.0)
    v = f64_ref.max_pool2d(v, 2, 2)
    y = attend("attn1", layer("qkv1", layer("ln1", v)), None, None)
    v = note(qp, "add1", layer("proj1", y) + v)
    v = layer("c2", np.maximum(v, 0.0))
    y = attend("attn2", layer("q2", v), layer("k2", v), layer("v2", v))
    v = note(qp, "add2", layer("proj2", y) + v)
    layer("fc", np.maximum(v, 0.0).mean(axis=(2, 3)))
    return qp, sq
