"""The quantized batched matmul and softmax on the GPU (csrc/i8ie_matmul.hip, csrc/i8ie_softmax.hip).
Every comparison is against the numpy restatement of the definition (tests/attention_ref.py), never against the code under
test: accumulators and every output byte of both matmul kernels over a grid of shapes, transpose forms, re-biased operands,
zero points and byte extremes; the bordered NHWC result with guard bytes; the softmax in both forms, its edge rows and in
place; the FP32 entries against float64; the Python surface (shapes, layouts, launch counts, calibration, save / load)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import attention_ref as ar
import f64_ref
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = [(False, False), (True, False), (False, True), (True, True)]
QP = (f32(0.02), f32(0.03), f32(0.21), 117)   # s_a, s_b, s_out, zp_out: spreads random accumulators over the byte range


ctx = support.ctx_fixture(ar)


SENTINEL = 0xA5   # the bytes between the rows and the batch items of a pitched matrix


def _pitched(phys, pitch=None):
    """phys [b, R, C] (C the contiguous axis) inside a larger allocation.  pitch: (row pitch, batch pitch), None for the
    compact value of either; batch pitch 0 keeps one matrix, which every batch item reads (phys must repeat it).
    Returns (flat bytes with SENTINEL in every gap, the index of phys[i, r, c] in it, row pitch, batch pitch)."""
    b, R, C = phys.shape
    rp, bp = pitch or (None, None)
    rp = C if rp is None else rp
    bp = R * rp if bp is None else bp
    assert rp >= C and (bp == 0 or bp >= (R - 1) * rp + C)
    nb = b if bp else 1
    assert bp or (phys == phys[:1]).all()
    idx = np.arange(nb)[:, None, None] * bp + np.arange(R)[None, :, None] * rp + np.arange(C)[None, None, :]
    flat = np.full((nb - 1) * bp + (R - 1) * rp + C, SENTINEL, np.uint8)
    flat[idx] = phys[:nb]
    return flat, idx, rp, bp


def _mat(ptr, rp, bp, transposed, s8, offset=0):
    """the descriptor of a pitched matrix: the logical rows are the physical ones, or with `transposed` the physical columns"""
    return ar.BmmMat(ptr + offset, bp, 1 if transposed else rp, rp if transposed else 1, 1 if s8 else 0)


def _bmm(ctx, A, zp_a, B, zp_b, ta=False, tb=False, relu=False, a_s8=False, b_s8=False, o_s8=False, qp=QP, fallback=False,
         offsets=(0, 0, 0), out_t=False, pitch_a=None, pitch_b=None, pitch_o=None):
    """A [b, m, k], B [b, k, n] logical.  The operands are laid out as asked (transposed, re-biased, at a byte offset inside
    their allocation, with a row pitch and a batch pitch -- _pitched), the result and the accumulators land in guarded
    regions; the gaps of a pitched result are asserted untouched.  Returns (out [b, m, n] plain bytes, acc [b, m, n], kernel
    names)."""
    bb, m, k = A.shape
    n = B.shape[2]
    s_a, s_b, s_out, zp_out = qp
    pa = np.ascontiguousarray(A.transpose(0, 2, 1)) if ta else np.ascontiguousarray(A)
    pb = np.ascontiguousarray(B.transpose(0, 2, 1)) if tb else np.ascontiguousarray(B)
    pa = pa ^ np.uint8(0x80) if a_s8 else pa
    pb = pb ^ np.uint8(0x80) if b_s8 else pb
    oa, ob, oo = offsets
    (fa, _, rpa, bpa), (fb, _, rpb, bpb) = _pitched(pa, pitch_a), _pitched(pb, pitch_b)
    fo, io, rpo, bpo = _pitched(np.zeros((bb, n, m) if out_t else (bb, m, n), np.uint8), pitch_o)
    fo[:] = SENTINEL
    da = ctx.put(np.concatenate([np.zeros(oa, np.uint8), fa]))
    db = ctx.put(np.concatenate([np.zeros(ob, np.uint8), fb]))
    do = abi.GuardedU8(ctx, (fo.size + oo,))
    before = np.concatenate([np.full(oo, SENTINEL, np.uint8), fo])
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, do.ptr, before.ctypes.data_as(C.c_void_p), C.c_size_t(before.nbytes)))
    dacc = abi.GuardedU8(ctx, (bb, m, n), np.int32)
    g = ar.BmmArgs(b=bb, m=m, n=n, k=k, a=_mat(da.ptr.value, rpa, bpa, ta, a_s8, oa), bm=_mat(db.ptr.value, rpb, bpb, tb, b_s8, ob),
                   out=_mat(do.ptr.value, rpo, bpo, out_t, o_s8, oo), s_a=s_a, s_b=s_b, s_out=s_out, zp_a=zp_a, zp_b=zp_b,
                   zp_out=zp_out, relu=1 if relu else 0, acc_dbg_dev=dacc.ptr.value)
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_bmm_u8(ctx.h, C.byref(g)))
    finally:
        ctx.set_force_fallback(False)
    raw = do.get().ravel()
    written = np.zeros(raw.size, bool)
    written[io.ravel() + oo] = True
    assert (raw[~written] == SENTINEL).all(), "a byte between the result's rows or batch items was written"
    out = raw[io + oo].transpose(0, 2, 1) if out_t else raw[io + oo]
    out = out ^ np.uint8(0x80) if o_s8 else out
    acc = dacc.get()
    assert do.guards_ok() and dacc.guards_ok()
    for d in (da, db, do, dacc):
        d.free()
    return np.ascontiguousarray(out), acc, names


def _check(ctx, A, zp_a, B, zp_b, kernel=None, **kw):
    out, acc, names = _bmm(ctx, A, zp_a, B, zp_b, **kw)
    qp = kw.get("qp", QP)
    want_acc = ar.matmul_acc(A, zp_a, B, zp_b)
    want = ar.matmul_u8(A, zp_a, qp[0], B, zp_b, qp[1], qp[2], qp[3], kw.get("relu", False))
    tag = (A.shape, B.shape[2], zp_a, zp_b, kw)
    assert np.array_equal(acc, want_acc), tag
    assert np.array_equal(out, want), tag
    if kernel is not None:
        assert names == {kernel: 1}, (names, tag)
    return want


@pytest.mark.parametrize("ta,tb", FORMS, ids=["nn", "tn", "nt", "tt"])
def test_matmul_grid(ctx, ta, tb):
    """every (m, n, k, b) of the grid in this transpose form; k < 16 takes bmm_direct, everything else bmm_mfma; the
    re-biased flags, the relu, the zero points and a transposed result cycle with the case index"""
    rng = np.random.default_rng(1 + 2 * ta + tb)
    zps = [0, 1, 127, 128, 255]
    spread = 0
    for i, (m, n, k, bb) in enumerate(itertools.product([1, 15, 16, 17, 65], [1, 15, 16, 17, 65], [1, 3, 15, 16, 63, 64, 65, 130], [1, 3])):
        A = rng.integers(0, 256, (bb, m, k), dtype=np.uint8)
        B = rng.integers(0, 256, (bb, k, n), dtype=np.uint8)
        want = _check(ctx, A, zps[i % 5], B, zps[(i // 5) % 5], kernel="bmm_direct" if k < 16 else "bmm_mfma", ta=ta, tb=tb,
                      a_s8=bool(i & 1), b_s8=bool(i & 2), o_s8=bool(i & 4), relu=bool(i & 8), out_t=bool(i & 16))
        spread = max(spread, len(np.unique(want)))
    assert spread > 100   # the expected bytes discriminate


@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
def test_matmul_zero_points_and_byte_extremes(ctx, fallback):
    rng = np.random.default_rng(5)
    kernel = "bmm_direct" if fallback else "bmm_mfma"
    A = rng.integers(0, 256, (2, 17, 65), dtype=np.uint8)
    B = rng.integers(0, 256, (2, 65, 33), dtype=np.uint8)
    for zp_a, zp_b in itertools.product([0, 1, 127, 128, 255], repeat=2):
        for s8 in (False, True):
            _check(ctx, A, zp_a, B, zp_b, kernel=kernel, fallback=fallback, a_s8=s8, b_s8=not s8, tb=True)
    wide = (f32(0.01), f32(0.01), f32(30.0), 128)
    for va, vb in itertools.product([0, 255], repeat=2):
        for zp_a, zp_b in ((0, 0), (255, 255), (0, 255), (128, 1)):
            _check(ctx, np.full_like(A, va), zp_a, np.full_like(B, vb), zp_b, kernel=kernel, fallback=fallback, qp=wide, ta=True)


@pytest.mark.parametrize("value,zp", [(255, 0), (0, 255)], ids=["all255_zp0", "all0_zp255"])
def test_matmul_largest_accumulator(ctx, value, zp):
    """k = 32768, m = n = 16: C = 255 * 255 * 32768 everywhere, the largest value an accumulator can take"""
    A = np.full((1, 16, ar.MAX_K), value, np.uint8)
    B = np.full((1, ar.MAX_K, 16), value, np.uint8)
    qp = (f32(1e-3), f32(1e-3), f32(10.0), 3)
    out, acc, names = _bmm(ctx, A, zp, B, zp, tb=True, qp=qp)
    assert names == {"bmm_mfma": 1} and (acc == 255 * 255 * ar.MAX_K).all()
    assert np.array_equal(out, ar.matmul_u8(A, zp, qp[0], B, zp, qp[1], qp[2], qp[3]))
    assert 3 < int(out[0, 0, 0]) < 255


def test_matmul_unaligned_pointers_take_the_direct_kernel(ctx):
    rng = np.random.default_rng(6)
    A = rng.integers(0, 256, (2, 17, 64), dtype=np.uint8)
    B = rng.integers(0, 256, (2, 64, 20), dtype=np.uint8)
    _check(ctx, A, 3, B, 200, kernel="bmm_mfma")
    for offsets in ((1, 0, 0), (0, 4, 0), (0, 0, 8), (3, 5, 7)):
        _check(ctx, A, 3, B, 200, kernel="bmm_direct", offsets=offsets, relu=True)


def _up16(v):
    return (v + 15) // 16 * 16


def _pitches(R, Cn):
    """the pitch cases of a physical [R, Cn] operand: a) row pitch = extent + 16, batch pitch a multiple of 16; A) the same
    with the extent rounded up to 16 first, so that both pitches are multiples of 16 at every extent (the 16-byte loads of a
    K-contiguous operand under a real pitch); b) both multiples of 16 but for 4 more bytes per batch item (op_vec must drop
    to the 4-byte loads); c) row pitch = extent + 4; C) a multiple of 4 above it (4-byte loads at every extent, the K-strided
    operand's widest); d) row pitch = extent + 1 (byte loads)"""
    up4 = (Cn + 3) // 4 * 4
    return {"a": (Cn + 16, _up16(R * (Cn + 16)) + 16), "A": (_up16(Cn) + 16, _up16(R * (_up16(Cn) + 16)) + 16),
            "b": (_up16(Cn) + 16, _up16(R * (_up16(Cn) + 16)) + 4), "c": (Cn + 4, None), "C": (up4 + 4, R * (up4 + 4) + 4),
            "d": (Cn + 1, None)}


@pytest.mark.parametrize("ta,tb", FORMS, ids=["nn", "tn", "nt", "tt"])
def test_matmul_strided_and_broadcast_operands(ctx, ta, tb):
    """each operand, K-contiguous or K-strided by the transpose form, inside a larger allocation under the six pitch cases of
    _pitches, as a broadcast (batch_stride == 0 on A, on B, on both), and the result under a row pitch of n + 4 and n + 3
    (dword and byte stores): accumulators, bytes and the untouched gaps, in bmm_mfma and again in bmm_direct.  k = 20, 36
    and 68 are multiples of 4 and not of 16: the 4-byte arm of stage_tile with a K tail."""
    rng = np.random.default_rng(21 + 2 * ta + tb)
    bb = 3
    for i, (m, n, k) in enumerate(itertools.product([17, 65], [17, 65], [20, 36, 64, 68, 130])):
        A = rng.integers(0, 256, (bb, m, k), dtype=np.uint8)
        B = rng.integers(0, 256, (bb, k, n), dtype=np.uint8)
        A1, B1 = np.repeat(A[:1], bb, axis=0), np.repeat(B[:1], bb, axis=0)
        pa, pb = _pitches(*((k, m) if ta else (m, k))), _pitches(*((n, k) if tb else (k, n)))
        runs = [(A, B, {"pitch_a": pa[c]}) for c in "aAbcCd"] + [(A, B, {"pitch_b": pb[c]}) for c in "aAbcCd"]
        runs += [(A, B, {"pitch_a": pa["c"], "pitch_b": pb["a"], "pitch_o": (n + 4, None)}), (A, B, {"pitch_o": (n + 3, None)}),
                 (A, B, {"pitch_o": (m + 4, _up16(n * (m + 4)) + 4), "out_t": True})]
        runs += [(A1, B, {"pitch_a": (None, 0)}), (A, B1, {"pitch_b": (None, 0)}), (A1, B1, {"pitch_a": (None, 0), "pitch_b": (None, 0)}),
                 (A1, B, {"pitch_a": (pa["d"][0], 0), "pitch_b": pb["b"]})]
        for j, (a, b_, kw) in enumerate(runs):
            flags = dict(a_s8=bool((i + j) & 1), b_s8=bool((i + j) & 2), o_s8=bool((i + j) & 4), relu=bool((i + j) & 8))
            for fallback in (False, True):
                _check(ctx, a, (120, 128, 131, 3, 250)[j % 5], b_, (131, 117, 128, 250)[i % 4], kernel="bmm_direct" if fallback else "bmm_mfma", ta=ta,
                       tb=tb, fallback=fallback, **flags, **kw)


def test_matmul_refuses_a_broadcast_result(ctx):
    """batch_stride == 0 on the result with b > 1: the batch items would share their bytes (include/i8ie_hip.h)"""
    buf = ctx.put(np.zeros(4096, np.uint8))
    p = buf.ptr.value
    g = ar.BmmArgs(b=2, m=4, n=4, k=16, a=ar.mat(p, 4, 16), bm=ar.mat(p, 16, 4), out=ar.BmmMat(p + 2048, 0, 4, 1, 0), s_a=1.0,
                   s_b=1.0, s_out=1.0)
    with ctx.launch_map() as names:
        assert abi.lib().i8ie_bmm_u8(ctx.h, C.byref(g)) == -1
        assert abi.lib().i8ie_bmm_f32(ctx.h, C.byref(g)) == -1
        g.b = 1
        abi.ck(abi.lib().i8ie_bmm_u8(ctx.h, C.byref(g)))
    assert names == {"bmm_mfma": 1}
    buf.free()


@pytest.mark.parametrize("fallback", [False, True], ids=["mfma", "forced_direct"])
@pytest.mark.parametrize("axis", [1, 2])
def test_matmul_bordered_rebiased_nhwc_result(ctx, axis, fallback):
    """the result as the interior of [b, h + 2B, w + 2B, c], re-biased, with the relu folded in: only the interior is written"""
    rng = np.random.default_rng(9 + axis)
    bb, c, h, w, k, border = 3, 20, 5, 7, 40, 2
    m, n = (h * w, c) if axis == 1 else (c, h * w)
    A = rng.integers(0, 256, (bb, m, k), dtype=np.uint8)
    B = rng.integers(0, 256, (bb, k, n), dtype=np.uint8)
    s_a, s_b, s_out, zp_out = QP
    want = ar.matmul_u8(A, 120, s_a, B, 131, s_b, s_out, zp_out, True)          # [b, m, n]
    want_pix = want if axis == 1 else want.transpose(0, 2, 1)                    # [b, h * w, c]
    phys = np.full((bb, h + 2 * border, w + 2 * border, c), zp_out ^ 0x80, np.uint8)
    expect = phys.copy()
    expect[:, border:-border, border:-border, :] = want_pix.reshape(bb, h, w, c) ^ np.uint8(0x80)
    da, db = ctx.put(A), ctx.put(B)
    do = abi.GuardedU8(ctx, phys.shape)
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, do.ptr, phys.ctypes.data_as(C.c_void_p), C.c_size_t(phys.nbytes)))
    img = phys[0].size
    out = ar.BmmMat(do.ptr.value, img, c if axis == 1 else 1, 1 if axis == 1 else c, 1)
    g = ar.BmmArgs(b=bb, m=m, n=n, k=k, a=ar.mat(da.ptr.value, m, k), bm=ar.mat(db.ptr.value, k, n), out=out, out_pix_axis=axis,
                   out_h=h, out_w=w, out_border=border, s_a=s_a, s_b=s_b, s_out=s_out, zp_a=120, zp_b=131, zp_out=zp_out, relu=1)
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_bmm_u8(ctx.h, C.byref(g)))
    finally:
        ctx.set_force_fallback(False)
    got = do.get()
    assert do.guards_ok() and names == {"bmm_direct" if fallback else "bmm_mfma": 1}
    assert np.array_equal(got, expect)
    for d in (da, db, do):
        d.free()


def test_matmul_argument_errors_launch_nothing(ctx):
    buf = ctx.put(np.zeros(4096, np.uint8))
    p = buf.ptr.value
    good = ar.BmmArgs(b=2, m=4, n=4, k=16, a=ar.mat(p, 4, 16), bm=ar.mat(p, 16, 4), out=ar.mat(p + 2048, 4, 4), s_a=1.0, s_b=1.0,
                      s_out=1.0)

    def rc(**kw):
        h = ar.BmmArgs.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    bad = [rc(k=ar.MAX_K + 1), rc(b=0), rc(s_out=0.0), rc(s_out=-2.0), rc(s_b=float("nan"))]
    h = rc()
    h.bm.row_stride, h.bm.col_stride = 4, 16
    bad.append(h)
    h = rc()
    h.out.ptr = None
    bad.append(h)
    with ctx.launch_map() as names:
        for h in bad:
            assert abi.lib().i8ie_bmm_u8(ctx.h, C.byref(h)) == -1
    assert names == {}
    # the Python surface refuses a batch mismatch (the descriptor has one b) and k above the limit before any launch
    import i8ie

    q = i8ie.quantize(i8ie.tensor(np.zeros((2, 4, 16), f32)), 0.1, 3)
    q3 = i8ie.quantize(i8ie.tensor(np.zeros((3, 16, 4), f32)), 0.1, 3)
    with pytest.raises(RuntimeError):
        i8ie.matmul(q, q3, 0.1, 3)
    big = i8ie.quantize(i8ie.tensor(np.zeros((1, 1, ar.MAX_K + 1), f32)), 0.1, 3)
    with pytest.raises(RuntimeError, match="32768"):
        i8ie.matmul(big, big, 0.1, 3, transpose_b=True)
    buf.free()


# ---- softmax -----------------------------------------------------------------------------------------------------------
def _softmax(ctx, x, s, in_place=False, offset=0):
    rows, L = x.shape
    di = abi.GuardedU8(ctx, (rows * L + offset,))
    host = np.concatenate([np.zeros(offset, np.uint8), x.ravel()])
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, di.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
    do = di if in_place else abi.GuardedU8(ctx, (rows * L + offset,))
    with ctx.launch_map() as names:
        abi.ck(abi.lib().i8ie_softmax_u8(ctx.h, di.ptr.value + offset, do.ptr.value + offset, rows, L, float(s)))
    got = do.get()[offset:].reshape(rows, L)
    assert do.guards_ok() and di.guards_ok()
    assert names == {"softmax_u8_wave" if L <= ar.SOFTMAX_WAVE_MAX_L else "softmax_u8_block": 1}, names
    di.free()
    if not in_place:
        do.free()
    return got


@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1027])
def test_softmax_rows(ctx, L):
    rng = np.random.default_rng(40 + L)
    for rows, s in zip(itertools.cycle([1, 3, 67]), [1.0 / 256, 0.01, 0.05, 0.3, 1.0, 0.05]):
        x = rng.integers(0, 256, (rows, L), dtype=np.uint8)
        if s == 0.3:
            x = (rng.integers(0, 24, (rows, L)) + 100).astype(np.uint8)   # close values: many entries share the mass
        x[0] = 91                                                         # an all-equal row
        if rows > 1:
            x[1] = 3
            x[1, L // 2] = 255                                            # one dominant entry (the 255 clamp)
        want = ar.softmax_u8(x, s)
        for in_place, offset in ((False, 0), (True, 0), (False, 1)):
            got = _softmax(ctx, x, s, in_place, offset)
            assert np.array_equal(got, want), (L, rows, s, in_place, offset, np.argwhere(got != want)[:4])


def test_softmax_every_distance_and_remainder_edges(ctx):
    # rows that hold every d in 0..255, in the wave form (twice over) and in the block form
    for L in (256, 512, 1280):
        x = np.stack([np.roll(np.arange(L) % 256, r) for r in (0, 1, 77)]).astype(np.uint8)
        for s in (1.0 / 256, 0.01, 0.05):
            assert np.array_equal(_softmax(ctx, x, s), ar.softmax_u8(x, s)), (L, s)
    # (E 256 + S / 2) mod S == 0: 16 entries at the max and 3 at distance 176, s = 0.01; == S - 1: [mx, mx - 2], s = 1 / 256
    for s, row, rem in ((0.01, [200] * 16 + [24] * 3, 0), (1.0 / 256, [9, 7], -1)):
        x = np.array([row], np.uint8)
        E = ar.softmax_table(s).astype(np.int64)
        S = int(E[x.max() - x.astype(np.int64)].sum())
        assert (int(E[0]) * 256 + S // 2) % S == (0 if rem == 0 else S - 1)
        assert np.array_equal(_softmax(ctx, x, s), ar.softmax_u8(x, s))


# ---- FP32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", FORMS, ids=["nn", "tn", "nt", "tt"])
def test_bmm_f32_against_float64(ctx, ta, tb):
    rng = np.random.default_rng(60)
    for bb, m, n, k in ((1, 1, 1, 1), (3, 17, 33, 65), (2, 64, 5, 300)):
        A = rng.normal(0, 1.5, (bb, m, k)).astype(f32)
        B = rng.normal(0.2, 1.0, (bb, k, n)).astype(f32)
        pa = np.ascontiguousarray(A.transpose(0, 2, 1)) if ta else A
        pb = np.ascontiguousarray(B.transpose(0, 2, 1)) if tb else B
        da, db, do = ctx.put(pa), ctx.put(pb), ctx.guarded((bb, m, n))
        g = ar.BmmArgs(b=bb, m=m, n=n, k=k, a=ar.mat(da.ptr.value, m, k, ta), bm=ar.mat(db.ptr.value, k, n, tb),
                       out=ar.mat(do.ptr.value, m, n))
        abi.ck(abi.lib().i8ie_bmm_f32(ctx.h, C.byref(g)))
        got, ok = do.read()
        want, mag = ar.matmul(A, B)
        assert ok and abi.GuardedOut.unwritten(got) == 0
        err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, k)
        assert (err <= bound).all(), (bb, m, n, k, float((err / np.maximum(bound, 1e-300)).max()))
        for d in (da, db, do):
            d.free()


@pytest.mark.parametrize("case", ["pitched", "broadcast"])
def test_bmm_f32_pitched_and_broadcast_against_float64(ctx, case):
    """i8ie_bmm_f32 under the stride contract of the u8 entry: every matrix under a row and a batch pitch (A given [b, k, m]),
    or A as one matrix against the batch; the gaps of the result stay as they were"""
    rng = np.random.default_rng(61)
    bb, m, n, k = 3, 17, 33, 65
    A = rng.normal(0, 1.5, (1 if case == "broadcast" else bb, m, k)).astype(f32)
    B = rng.normal(0.2, 1.0, (bb, k, n)).astype(f32)
    (rpa, bpa), (rpb, bpb), (rpo, bpo) = ((m + 3, k * (m + 3) + 5), (n + 1, k * (n + 1) + 2), (n + 2, m * (n + 2) + 7)) \
        if case == "pitched" else ((k, 0), (n, k * n), (n, m * n))
    pa = np.ascontiguousarray(A.transpose(0, 2, 1)) if case == "pitched" else A
    ia = np.arange(pa.shape[0])[:, None, None] * bpa + np.arange(pa.shape[1])[None, :, None] * rpa + np.arange(pa.shape[2])
    fa, fb = np.full(int(ia.max()) + 1, np.nan, f32), np.full(bb * bpb, np.nan, f32)
    ib = np.arange(bb)[:, None, None] * bpb + np.arange(k)[None, :, None] * rpb + np.arange(n)
    io = np.arange(bb)[:, None, None] * bpo + np.arange(m)[None, :, None] * rpo + np.arange(n)
    fa[ia], fb[ib] = pa, B
    da, db, do = ctx.put(fa), ctx.put(fb), ctx.guarded((bb * bpo,))
    a_mat = ar.BmmMat(da.ptr.value, bpa, 1, rpa, 0) if case == "pitched" else ar.BmmMat(da.ptr.value, 0, rpa, 1, 0)
    g = ar.BmmArgs(b=bb, m=m, n=n, k=k, a=a_mat, bm=ar.BmmMat(db.ptr.value, bpb, rpb, 1, 0), out=ar.BmmMat(do.ptr.value, bpo, rpo, 1, 0))
    abi.ck(abi.lib().i8ie_bmm_f32(ctx.h, C.byref(g)))
    raw, ok = do.read()
    got = raw[io]
    want, mag = ar.matmul(np.repeat(A, bb // A.shape[0], axis=0), B)
    assert ok and abi.GuardedOut.unwritten(got) == 0 and abi.GuardedOut.unwritten(raw) == raw.size - got.size
    err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, k)
    assert (err <= bound).all(), (case, float((err / np.maximum(bound, 1e-300)).max()))
    for d in (da, db, do):
        d.free()


@pytest.mark.parametrize("L", [1, 2, 17, 64, 257, 1027])
def test_softmax_f32_against_float64(ctx, L):
    rng = np.random.default_rng(70 + L)
    x = rng.normal(0, 4, (5, L)).astype(f32)
    x[1] = 2.5
    di, do = ctx.put(x), ctx.guarded(x.shape)
    abi.ck(abi.lib().i8ie_softmax_f32(ctx.h, di.ptr, do.ptr, 5, L))
    got, ok = do.read()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    err = np.abs(got.astype(np.float64) - ar.softmax(x)).max()
    print("softmax_f32 L=%d: max abs error %.3g, bound %.3g" % (L, err, (L + 8) * 2.0 ** -23))
    assert err <= (L + 8) * 2.0 ** -23
    di.free(); do.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_surface_shapes_and_errors(i8ie):
    rng = np.random.default_rng(80)
    a3 = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 5, 12)).astype(f32)), 0.025, 127)
    b3 = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 12, 7)).astype(f32)), 0.03, 100)
    a4 = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 5, 3, 4)).astype(f32)), 0.025, 127)
    b12 = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 12, 12)).astype(f32)), 0.03, 100)
    av, bv, a4v, b12v = a3.numpy(), b3.numpy(), a4.numpy(), b12.numpy()
    r = i8ie.matmul(a3, b3, 0.2, 120)
    assert r.shape == (2, 5, 7) and r.scale == pytest.approx(0.2) and r.zero_point == 120
    assert np.array_equal(r.numpy(), ar.matmul_u8(av, 127, f32(0.025), bv, 100, f32(0.03), f32(0.2), 120))
    r = i8ie.relu(i8ie.matmul(b3, a3, scale=0.2, zero_point=120, transpose_a=True, transpose_b=True))   # [7, 12] . [12, 5]
    assert r.shape == (2, 7, 5)
    assert np.array_equal(r.numpy(), ar.matmul_u8(bv, 100, f32(0.03), av, 127, f32(0.025), f32(0.2), 120, True, True, True))
    # rank 4 counts as [n, c, h * w]; a rank-4 untransposed `a` with n == h * w gives a rank-4 result
    r = i8ie.matmul(a4, b12, 0.2, 120)
    assert r.shape == (2, 5, 3, 4)
    assert np.array_equal(r.numpy().reshape(2, 5, 12), ar.matmul_u8(a4v, 127, f32(0.025), b12v, 100, f32(0.03), f32(0.2), 120))
    assert i8ie.matmul(a4, b3, 0.2, 120).shape == (2, 5, 7)
    assert i8ie.matmul(a4, a4, 0.2, 120, transpose_a=True).shape == (2, 12, 12)
    for bad in (lambda: i8ie.matmul(a3, a3, 0.2, 120), lambda: i8ie.matmul(a3, b3.reshape(1, 24, 7), 0.2, 120),
                lambda: i8ie.matmul(a3.reshape(10, 12), b3, 0.2, 120), lambda: i8ie.matmul(a3, b3, 0.0, 1),
                lambda: i8ie.matmul(a3, b3, 0.2, 256), lambda: i8ie.MatMul()(a3, b3)):
        with pytest.raises(RuntimeError):
            bad()
    for kw in ({}, {"scale": 0.2}, {"zero_point": 3}):
        with pytest.raises(TypeError):
            i8ie.matmul(a3, b3, **kw)
    # softmax: a plain tensor with scale 1/256, zero point 0, over the last axis
    p = i8ie.softmax(a3)
    assert p.shape == (2, 5, 12) and p.scale == pytest.approx(1 / 256) and p.zero_point == 0
    assert np.array_equal(p.numpy(), ar.softmax_u8(av, f32(0.025)))
    # FP32 tensors
    fa, fb = rng.normal(0, 1, (2, 5, 12)).astype(f32), rng.normal(0, 1, (2, 12, 7)).astype(f32)
    got = i8ie.matmul(i8ie.tensor(fa), i8ie.tensor(fb)).numpy()
    want, mag = ar.matmul(fa, fb)
    assert got.shape == (2, 5, 7) and (np.abs(got - want) <= f64_ref.dot_bound(mag, 12)).all()
    got = i8ie.softmax(i8ie.tensor(fa)).numpy()
    assert np.abs(got - ar.softmax(fa)).max() <= 20 * 2.0 ** -23


def test_nonlocal_block_bytes_layouts_and_launch_counts(i8ie):
    """a non-local block on a conv activation in the engine's layout: theta, phi, g are 1x1 projections, s = mm(theta, phi,
    transpose_a), p = softmax(s), y = mm(g, p, transpose_b), then a padded 3x3 conv on relu(y) (a bordered consumer).  After
    convert() the three attention ops are three launches, each projection conv is one, and nothing converts a layout,
    re-biases or fills a border in between."""
    rng = np.random.default_rng(90)
    n, c, d, h, w = 3, 16, 16, 6, 5
    # (two convs: the second one's result is an activation in the engine's layout, as in tests/test_gpu_mul.py)
    stem0, stem = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128)), support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    theta, phi, gp = (support.conv(i8ie, c, d, 1, 0, sd, (0.06, 125 + sd)) for sd in (2, 3, 4))
    tail = support.conv(i8ie, d, 16, 3, 1, 5, (0.07, 100))
    mm1, mm2 = i8ie.MatMul(transpose_a=True), i8ie.MatMul(transpose_b=True)
    mm1.set_output_qparams(0.6, 150)
    mm1.convert()
    mm2.set_output_qparams(0.06, 128)
    mm2.convert()
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, 3, h, w)).astype(f32)), 0.025, 127)
    x = i8ie.relu(stem(i8ie.relu(stem0(q))))

    def block():
        s = mm1(theta(x), phi(x))
        p = i8ie.softmax(s)
        return [tail(i8ie.relu(mm2(gp(x), p)))]

    launches = support.counted(block)
    print(launches)
    assert launches.get("bmm_mfma", 0) + launches.get("bmm_direct", 0) == 2 and launches.get("softmax_u8_wave", 0) == 1
    assert sum(launches.values()) == 3 + 4, launches   # + theta, phi, g and the tail conv, one launch each
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), launches
    # the bytes, from the numpy composition
    xv = x.numpy()
    tv, pv, gv = (support.conv_ref(L, xv, 0.05, 120) for L in (theta, phi, gp))
    sv = ar.matmul_u8(tv, 127, f32(0.06), pv, 128, f32(0.06), f32(0.6), 150, transpose_a=True)
    assert sv.shape == (n, h * w, h * w) and ((sv == 0) | (sv == 255)).mean() < 0.05
    smv = ar.softmax_u8(sv, f32(0.6))
    assert len(np.unique(smv)) >= 16
    yv = ar.matmul_u8(gv, 129, f32(0.06), smv, 0, f32(1 / 256), f32(0.06), 128, True, transpose_b=True).reshape(n, d, h, w)
    assert len(np.unique(yv)) >= 16
    want = support.conv_ref(tail, yv, 0.06, 128, pad=1)
    s = mm1(theta(x), phi(x))
    assert s.shape == (n, h * w, h * w) and np.array_equal(s.numpy(), sv)
    y = mm2(gp(x), i8ie.softmax(s))
    assert y.shape == (n, d, h, w) and np.array_equal(i8ie.relu(y).numpy(), yv)
    assert np.array_equal(block()[0].numpy(), want)


def test_matmul_is_calibrated_like_a_layer_and_round_trips(i8ie):
    import _CXX_i8ie as cx

    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, (5, 8, 10)).astype(f32)
    b = rng.normal(0.0, 1.0, (5, 6, 10)).astype(f32)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.mm1 = i8ie.MatMul(transpose_b=True)

    cx.set_calibration_mode("host")
    cx.set_calibration_seed(7)
    try:
        net = Net()
        net.prepare()
        got = net.mm1(i8ie.tensor(a), i8ie.tensor(b)).numpy()
        net.convert()
        want = tuple(cx.calibrator_range([got.ravel()], 1.0))
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    ref, mag = ar.matmul(a, b, transpose_b=True)
    assert got.shape == (5, 8, 6) and (np.abs(got - ref) <= f64_ref.dot_bound(mag, 10)).all()
    assert net.mm1.layer.is_quantized() and net.mm1.output_qparams() == want and want[0] != 1.0
    sd = net.quantized_state_dict()
    assert list(sd) == ["mm1.qparams"]
    other = Net()
    other.load_quantized(sd)
    assert other.mm1.output_qparams() == net.mm1.output_qparams()
    qa = i8ie.quantize(i8ie.tensor(a), 0.05, 120)
    qb = i8ie.quantize(i8ie.tensor(b), 0.04, 128)
    r1, r2 = net.mm1(qa, qb).numpy(), other.mm1(qa, qb).numpy()
    s_o, zp_o = want
    assert np.array_equal(r1, r2)
    assert np.array_equal(r1, ar.matmul_u8(qa.numpy(), 120, f32(0.05), qb.numpy(), 128, f32(0.04), f32(s_o), zp_o, transpose_b=True))


# ---- nonlocal_tiny ----------------------------------------------------------------------------------------------------------
NAME = "nonlocal_tiny"


def _case(per_channel, batch):
    """(net, jqp, x, expected logits, the reference's traced tensors) with spec_ref's seeds"""
    import net_cases as nc
    import spec_ref as sr
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = nc.calibrated(NAME, per_channel, calib_images=8)
    x = wl.synthetic_input(NAME, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.network(NAME), x, qlayers, qp, jqp, per_channel, ar.tracer(trace))
    return net, jqp, x, want, trace


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_nonlocal_tiny_bit_exact(i8ie, batch, per_channel):
    import net_cases as nc

    net, jqp, x, want, trace = _case(per_channel, batch)
    assert all(s > 0 and s != 1.0 for s, _ in jqp.values()), jqp   # the MatMuls and Adds were calibrated
    assert want.shape == (batch, 10) and len(np.unique(want)) > 1
    nc.check_bit_exact(i8ie, net, NAME, x, want, fallback=True)
    mine = {}
    nc.traced(i8ie, net, NAME, x, ar.tracer(mine))
    assert sorted(mine) == sorted(trace) and len(trace) == 6
    for k in trace:
        assert mine[k].shape == trace[k].shape and np.array_equal(mine[k], trace[k]), k


def test_nonlocal_tiny_kernels_graph_replay_and_reload(i8ie, tmp_path):
    """block A's products run in bmm_mfma, block B's first one (k = 12) in bmm_direct; the forward replayed as one HIP graph
    and a fresh net loaded from the saved quantized state give the expected bytes"""
    import _CXX_i8ie as cx
    import net_cases as nc

    net, jqp, x, want, _ = _case(False, 5)
    nc.check_bit_exact(i8ie, net, NAME, x, want, graph=True, reload_dir=tmp_path, expect_jqp=jqp)
    cx.synchronize()
    cx.profile_start()
    try:
        net(i8ie.tensor(x)).numpy()
    finally:
        prof = cx.profile_stop()
    launches = {}
    for k, v in prof.items():
        launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0]
    print(launches)
    assert launches.get("bmm_mfma") == 3 and launches.get("bmm_direct") == 1 and launches.get("softmax_u8_wave") == 2, launches
