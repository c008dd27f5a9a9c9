"""Shared by tests/golden/make_golden_layers.py and the tests that read its fixtures (a helper module, not a
conftest): how a case's operands are obtained.

A case of ref_conv2d_u8.npz / ref_linear_u8.npz either stores its operands (`q_in`, `w`, `b`) or, where they would
not fit the size limit of a committed file, stores `redraw` (a numpy seed) and `operands_sha256`: the operands are
then redrawn from the seed and must hash to the stored digest, so a changed random stream is caught instead of
compared (the scheme of mkl_gemm_seed9.npz).  The kernel-sized cases of ref_kernel_digests.json are redrawn the same
way and store their results as digests too."""
import hashlib

import numpy as np

from synth import he_weights


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def redraw(seed, in_shape, w_shape):
    """(q_in u8, w f32, b f32) of a redrawn case, in this order from one generator."""
    rng = np.random.default_rng(int(seed))
    w, b = he_weights(rng, tuple(int(d) for d in w_shape))
    q_in = rng.integers(0, 256, tuple(int(d) for d in in_shape), dtype=np.uint8)
    return q_in, w, b


def conv_shapes(geom):
    n, c, h, w, kc, k, stride, pad = (int(v) for v in geom)
    return (n, c, h, w), (kc, c, k, k)


def operands(case, kind):
    """(q_in, w, b) of a fixture case: stored, or redrawn and checked against the stored digest."""
    if "redraw" not in case:
        return case["q_in"], case["w"], case["b"]
    if kind == "conv":
        in_shape, w_shape = conv_shapes(case["geom"])
    else:
        m, k, n = (int(v) for v in case["geom"])
        in_shape, w_shape = (m, k), (n, k)
    q_in, w, b = redraw(int(case["redraw"]), in_shape, w_shape)
    assert sha(q_in, w, b) == str(case["operands_sha256"]), "the random stream changed: operands are not the fixture's"
    return q_in, w, b


def qparams(case):
    """(s_in f32, zp_in, s_out f32, zp_out) of a conv / linear case."""
    return (np.float32(case["s_in"]), int(case["zp"][0]), np.float32(case["s_out"]), int(case["zp"][1]))


def range_qparams(lo, hi):
    """The calibrator's rule (src/calibrator.cc:24-37 at quantile 1) on a real-valued range: the generator's
    stand-in for calibration.  Its result is stored in the fixture; nothing recomputes it."""
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    if hi - lo < 1e-12:
        return np.float32(1.0), 0
    zp = int(255 * (0 - lo) / (hi - lo))
    scale = (hi - lo) / 255 if zp == 0 else (0 - lo) / zp
    return np.float32(scale), zp


def provider_gemm(A, B, oc):
    """cblas_gemm_s8u8s32 of oracle/libgemm_provider.so (our plain-C provider, oracle/gemm_provider.c) with the
    reference's argument pattern: A u8 [M, K], B s8 [N, K], oc s32 [N] -> C s32 [M, N]."""
    import ctypes as C
    import os

    import orc

    path = os.path.join(os.path.dirname(os.path.abspath(orc.__file__)), "libgemm_provider.so")
    if not os.path.exists(path):
        orc.build()
    lib = C.CDLL(path)
    A, B, oc = np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.int8), np.ascontiguousarray(oc, np.int32)
    (M, K), N = A.shape, B.shape[0]
    out = np.empty((M, N), np.int32)
    lib.cblas_gemm_s8u8s32(101, 111, 112, 171, C.c_int(M), C.c_int(N), C.c_int(K), C.c_float(1.0),
                           A.ctypes.data_as(C.c_void_p), C.c_int(K), C.c_int8(0), B.ctypes.data_as(C.c_void_p), C.c_int(K),
                           C.c_int8(0), C.c_float(0.0), out.ctypes.data_as(C.c_void_p), C.c_int(N),
                           oc.ctypes.data_as(C.c_void_p))
    return out


MKL_SEED9_SHAPES = ((17, 363, 20), (40, 4096, 10), (3, 800, 500))  # (M, K, N), tests/golden/make_golden_mkl.py


def check_gemm_against_mkl(gemm, load_cases):
    """`gemm` reproduces every committed MKL result (mkl_gemm_s8u8s32.npz, mkl_gemm_seed9.npz) bit for bit.
    Returns the number of cases compared."""
    n = 0
    for c in load_cases("mkl_gemm_s8u8s32.npz"):
        assert np.array_equal(gemm(c["A"], c["B"], c["oc"]), c["C"])
        n += 1
    rng = np.random.default_rng(9)
    stored = load_cases("mkl_gemm_seed9.npz")
    assert len(stored) == len(MKL_SEED9_SHAPES)
    for (M, K, N), want in zip(MKL_SEED9_SHAPES, stored):
        A = rng.integers(0, 256, (M, K), dtype=np.uint8)
        B = rng.integers(-128, 128, (N, K), dtype=np.int8)
        oc = rng.integers(-50000, 50000, N).astype(np.int32)
        assert sha(A, B, oc) == str(want["operands_sha256"])
        assert np.array_equal(gemm(A, B, oc), want["C"])
        n += 1
    return n
