"""numpy restatement of the quantized batched matmul and softmax (include/i8ie_hip.h, i8ie_bmm_u8 / i8ie_softmax_u8), the
float64 references of their FP32 forms, the ctypes side of the two descriptors, and the trace adapter of the attention
networks (tests/spec_ref.py composes them).  A helper, not a conftest."""
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


def tracer(into):
    """a trace callback for spec_ref.forward: of every attention block of prefix p, into[p + "scores"] (the bytes of its first
    MatMul, p + "mm1"), into[p + "softmax"] (of the softmax behind it) and into[p + "block"] (of its Add, p + "add")"""
    at = {"p": None}

    def trace(op, out, operands):
        if op[0] == "matmul" and op[1].endswith("mm1"):
            at["p"] = op[1][:-3]
            into[at["p"] + "scores"] = out[0]
        elif op[0] == "softmax":
            into[at["p"] + "softmax"] = out[0]
        elif op[0] == "add" and at["p"] is not None and op[1] == at["p"] + "add":
            into[at["p"] + "block"] = out[0]

    return trace
