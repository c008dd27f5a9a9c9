"""numpy restatement of the quantized batched matmul and softmax (include/i8ie_hip.h, i8ie_bmm_u8 / i8ie_softmax_u8), the
float64 references of their FP32 forms, and the ctypes side of the two descriptors.  A helper, not a conftest."""
import ctypes as C

import numpy as np

import orc

MAX_K = 32768
SOFTMAX_WAVE_MAX_L = 1024   # rows up to here take the one-wave-per-row kernel (csrc/i8ie_softmax.hip)


# ---- matmul ----------------------------------------------------------------------------------------------------------
def logical(a, b, transpose_a=False, transpose_b=False):
    """the operands as [b, m, k] and [b, k, n] (rank 4 counts as [n, c, h * w])"""
    a = np.asarray(a).reshape(a.shape[0], a.shape[1], -1)
    b = np.asarray(b).reshape(b.shape[0], b.shape[1], -1)
    if transpose_a:
        a = a.transpose(0, 2, 1)
    if transpose_b:
        b = b.transpose(0, 2, 1)
    assert a.shape[0] == b.shape[0] and a.shape[2] == b.shape[1]
    return a, b


def matmul_acc(a, zp_a, b, zp_b, transpose_a=False, transpose_b=False):
    """C[b,i,j] = sum_k (a - zp_a)(b - zp_b), exact (int64 einsum), asserted to fit int32"""
    a, b = logical(a, b, transpose_a, transpose_b)
    acc = np.einsum("bik,bkj->bij", a.astype(np.int64) - int(zp_a), b.astype(np.int64) - int(zp_b))
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return acc.astype(np.int32)


def matmul_u8(a, zp_a, s_a, b, zp_b, s_b, s_out, zp_out, relu=False, transpose_a=False, transpose_b=False):
    acc = matmul_acc(a, zp_a, b, zp_b, transpose_a, transpose_b)
    q = orc.down_scale(acc, s_a, s_b, s_out, zp_out)
    return np.maximum(q, np.uint8(zp_out)) if relu else q


def result_shape(a_shape, b_shape, transpose_a=False, transpose_b=False):
    """the Python surface's shape rule"""
    m = int(np.prod(a_shape[2:])) if transpose_a else a_shape[1]
    n = b_shape[1] if transpose_b else int(np.prod(b_shape[2:]))
    if len(a_shape) == 4 and not transpose_a and n == a_shape[2] * a_shape[3]:
        return (a_shape[0], m, a_shape[2], a_shape[3])
    return (a_shape[0], m, n)


def matmul(a, b, transpose_a=False, transpose_b=False):
    """float64 product and magnitude sum_k |a||b| of float operands"""
    a, b = logical(a, b, transpose_a, transpose_b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.einsum("bik,bkj->bij", a, b), np.einsum("bik,bkj->bij", np.abs(a), np.abs(b))


# ---- softmax ---------------------------------------------------------------------------------------------------------
def softmax_table(s):
    """E[d] = floor(65536 exp(-s d) + 0.5) in double, s taken as the float32 it travels as"""
    d = np.arange(256, dtype=np.float64)
    return np.floor(65536.0 * np.exp(-np.float64(np.float32(s)) * d) + 0.5).astype(np.uint32)


def softmax_u8(x, s):
    """over the last axis; the result carries scale 1/256, zero point 0.  Every intermediate is asserted below 2^32."""
    x = np.asarray(x, np.uint8)
    E = softmax_table(s).astype(np.uint64)
    d = x.max(axis=-1, keepdims=True).astype(np.int64) - x.astype(np.int64)
    e = E[d]
    S = e.sum(axis=-1, keepdims=True)
    num = e * np.uint64(256) + S // np.uint64(2)
    assert S.min() >= 65536 and S.max() < 2 ** 32 and num.max() < 2 ** 32
    return np.minimum(num // S, np.uint64(255)).astype(np.uint8)


def softmax(x):
    """float64, over the last axis"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_u8_bound(L):
    """|q - 256 softmax| <= 0.5 (rounding of q) + 256 (L + 1) / 131072 (L table entries and E itself, each rounded by at most
    1/2 against S >= 65536).  That bounds the unclamped quotient, which can be 256; the byte is min(255, .), so compare against
    min(256 softmax, 255): a quotient of 256 means 256 softmax > 255, and both sides then sit at 255."""
    return 0.5 + 256.0 * (L + 1) / 131072.0


# ---- ctypes ----------------------------------------------------------------------------------------------------------
class BmmMat(C.Structure):
    """i8ie_bmm_mat"""
    _fields_ = [("ptr", C.c_void_p), ("batch_stride", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("s8", C.c_int)]


class BmmArgs(C.Structure):
    """i8ie_bmm_args"""
    _fields_ = [("b", C.c_int), ("m", C.c_int), ("n", C.c_int), ("k", C.c_int), ("a", BmmMat), ("bm", BmmMat),
                ("out", BmmMat), ("out_pix_axis", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
                ("out_border", C.c_int), ("s_a", C.c_float), ("s_b", C.c_float), ("s_out", C.c_float),
                ("zp_a", C.c_uint8), ("zp_b", C.c_uint8), ("zp_out", C.c_uint8), ("relu", C.c_int),
                ("acc_dbg_dev", C.c_void_p)]


def bind(lib):
    lib.i8ie_bmm_u8.argtypes = [C.c_void_p, C.POINTER(BmmArgs)]
    lib.i8ie_bmm_f32.argtypes = [C.c_void_p, C.POINTER(BmmArgs)]
    lib.i8ie_softmax_table.argtypes = [C.c_float, C.c_void_p]
    lib.i8ie_softmax_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float]
    lib.i8ie_softmax_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    return lib


def mat(ptr, rows, cols, transposed=False, s8=False, offset=0):
    """the [rows, cols] matrix per batch item of a dense array; transposed: the array holds [cols, rows]"""
    return BmmMat(ptr + offset, rows * cols, 1 if transposed else cols, rows if transposed else 1, 1 if s8 else 0)


# ---- the numpy composition of NonLocalNet (int8inferenceengine_amd/nonlocal_net.py) ----------------------------------------
INPUT_SCALE, INPUT_ZP = np.float32(0.025), 127
# weights, calibration batch and input of the "tiny" tests, GPU and host: tests/test_attention_host.py checks that with
# them the expected bytes discriminate (more than one logit, spread softmax bytes, few saturated scores)
WEIGHT_SEED, CALIB_SEED, INPUT_SEED = 42, 99, 5


def _layer(L, cur, qlayer, s_out, zp_out, per_channel):
    import grouped_ref as gr
    import pc_pipeline as pcp

    (q, s, zp), (qw, qb, s_w) = cur, qlayer
    if L[0] == "conv":
        f = gr.conv2d_grouped_pc if per_channel else gr.conv2d_grouped
        return f(q, qw, qb, 1, L[4], L[5], s, zp, s_w, s_out, zp_out)[0]
    f = pcp.linear_pc if per_channel else orc.linear
    return f(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_out, zp_out)[0]


def nonlocal_forward(entry, x, qlayers, qp, jqp, per_channel=False, trace=None):
    """float32 logits of a NonLocalNet plan.  entry: nonlocal_net.CONFIGS[config]; qlayers: {attr: (qw, qb, s_w)}; qp / jqp:
    {attr: (scale, zp)} of the layers / of the MatMuls and Adds.  trace: a dict that receives, per block prefix p,
    p + "scores", p + "softmax" and p + "block" (the Add's result) as bytes."""
    import add_ref
    import avgpool_ref as apr

    layers, spec, _ = entry

    def out_of(table, attr):
        s, zp = table[attr]
        return np.float32(s), int(zp)

    def layer(attr, cur):
        s_out, zp_out = out_of(qp, attr)
        return (_layer(layers[attr], cur, qlayers[attr], s_out, zp_out, per_channel), s_out, zp_out)

    def block(p, cur):
        th, ph, g = layer(p + "theta", cur), layer(p + "phi", cur), layer(p + "g", cur)
        s1, z1 = out_of(jqp, p + "mm1")
        scores = matmul_u8(th[0], th[2], th[1], ph[0], ph[2], ph[1], s1, z1, transpose_a=True)
        prob = softmax_u8(scores, s1)
        s2, z2 = out_of(jqp, p + "mm2")
        y = matmul_u8(g[0], g[2], g[1], prob, 0, np.float32(1.0 / 256), s2, z2, transpose_b=True)
        y = y.reshape(result_shape(g[0].shape, prob.shape, False, True))
        z = layer(p + "out", (y, s2, z2))
        s3, z3 = out_of(jqp, p + "add")
        out = add_ref.add_u8(z[0], z[2], z[1], cur[0], cur[2], cur[1], s3, z3, relu=False)
        if trace is not None:
            trace[p + "scores"], trace[p + "softmax"], trace[p + "block"] = scores, prob, out
        return (out, s3, z3)

    def run(ops, cur, saved):
        for op in ops:
            q, s, zp = cur
            if op[0] == "layer":
                cur = layer(op[1], cur)
            elif op[0] == "relu":
                cur = (orc.relu(q, zp), s, zp)
            elif op[0] == "pool":
                cur = (orc.max_pool2d(q, op[1], op[2]), s, zp)
            elif op[0] == "gap":
                cur = (apr.global_avg_pool2d_u8(q), s, zp)
            elif op[0] == "save":
                saved[op[1]] = cur
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                q2, s2, zp2 = saved[op[2]]
                s_o, z_o = out_of(jqp, op[1])
                cur = (add_ref.add_u8(q, zp, s, q2, zp2, s2, s_o, z_o, relu=False), s_o, z_o)
            elif op[0] == "flatten":
                cur = (q.reshape(-1, op[1]), s, zp)
            elif op[0] == "nonlocal":
                cur = block(op[1], cur)
            else:
                raise ValueError("attention_ref.nonlocal_forward: op %r" % (op,))
        return cur

    q0 = orc.quantize(x, INPUT_SCALE, INPUT_ZP)
    return orc.dequantize(*run(spec, (q0, INPUT_SCALE, INPUT_ZP), {}))


def nonlocal_quantize_layers(entry, state_dict, per_channel=False):
    """convert()'s weight rules, as spec_ref.quantize_layers applies them"""
    import pc_pipeline as pcp

    rule = pcp.quantize_weight_pc if per_channel else orc.quantize_weight
    return {a: tuple(rule(state_dict[a + ".weight"], state_dict[a + ".bias"])) for a in entry[0]}


def nonlocal_fp32_qparams(entry, state_dict, x):
    """Stand-in for calibration without a GPU (spec_ref.fp32_qparams' method): a float64 forward over the FP32 weights; the
    output range of every layer, MatMul and Add gives its (scale, zero_point) by the calibrator's rule.  Returns (qp, jqp)."""
    import f64_ref
    import grouped_ref as gr
    import spec_ref as sr

    layers, spec, _ = entry
    qp, jqp = {}, {}

    def layer(attr, v):
        L = layers[attr]
        w, b = state_dict[attr + ".weight"].astype(np.float64), state_dict[attr + ".bias"].astype(np.float64)
        v = gr.conv2d_f64(v, w, b, 1, L[4], L[5]) if L[0] == "conv" else f64_ref.linear(v.reshape(v.shape[0], -1), w, b)
        qp[attr] = sr.range_qparams(v.min(), v.max())
        return v

    def joined(attr, v):
        jqp[attr] = sr.range_qparams(v.min(), v.max())
        return v

    def run(ops, v, saved):
        for op in ops:
            if op[0] == "layer":
                v = layer(op[1], v)
            elif op[0] == "relu":
                v = np.maximum(v, 0.0)
            elif op[0] == "pool":
                v = f64_ref.max_pool2d(v, op[1], op[2])
            elif op[0] == "gap":
                v = v.mean(axis=(2, 3), keepdims=True)
            elif op[0] == "save":
                saved[op[1]] = v
            elif op[0] == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                v = joined(op[1], v + saved[op[2]])
            elif op[0] == "flatten":
                v = v.reshape(-1, op[1])
            elif op[0] == "nonlocal":
                p = op[1]
                th, ph, g = layer(p + "theta", v), layer(p + "phi", v), layer(p + "g", v)
                s = joined(p + "mm1", matmul(th, ph, transpose_a=True)[0])
                y = joined(p + "mm2", matmul(g, softmax(s), transpose_b=True)[0]).reshape(g.shape)
                v = joined(p + "add", layer(p + "out", y) + v)
        return v

    run(spec, np.asarray(x, np.float64), {})
    return qp, jqp
