"""The requantiser's replay arm in every contraction epilogue (csrc/i8ie_requant.h and its call sites), on the GPU.

Every case of tests/requant_cases.py runs a layer through the route helpers of tests/test_gpu_layer_routes.py with operands of
one class of tests/requant_ref.py -- ALL (every output dword replays the exact sequence, and the estimate's own byte would be
wrong for every odd result), MIXED (estimate and replay meet inside one launch) and EXACT-MODE (scales below 1e-30: the host
clears `fast`) -- per tensor and per channel, with and without ReLU, bordered and re-biased outputs, pooled forms, and a zero
scale column.  bmm_mfma and both epilogues of attn_mfma get the same classes from their operands.  The expected bytes are
requant_ref.exact on the numpy references' accumulators, never a result of the library; the class conditions are asserted from
those references before any GPU result is looked at (tests/test_requant_host.py asserts them on the CPU too); every case
asserts through the launch map that the kernel it is for ran.  The last tests sweep contiguous accumulators through the guard
arithmetic of a per-channel tiled Linear and of bmm_mfma."""
import ctypes as C

import numpy as np
import pytest

import abi
import attention_ref as ar
import mha_ref as mr
import requant_cases as rc
import requant_ref as rq
import support
import test_gpu_attention as tga
import test_gpu_layer_routes as lr
import test_gpu_mha as tgm

pytestmark = pytest.mark.gpu
f32 = np.float32
SEEN = {}   # case id -> launch map, for test_every_kernel_of_the_table_ran


gpu = support.ctx_fixture(mr)


# ---- the layer sites ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(rc.CASES))
def test_layer_site(gpu, cid):
    cs = rc.CASES[cid]
    d = rc.operands(cs)
    acc = rc.accumulators(cs, d)
    rep = rc.report(cs, d, acc)
    print(cid, rep)
    rq.check_class(rep, cs["relu"])
    want = rc.expected(cs, d, acc)
    # without the accumulator pointer, the instantiation every network runs, and with it (stem, pconv, tconv, first and igemm
    # compile a form of their own for it, under the same kernel name)
    for want_acc in (False, True):
        got = lr.run(gpu, cs, d, want_acc=want_acc)
        print(cid, want_acc, got["warm"], got["error"])
        assert got["error"] is None, got["error"]
        SEEN[cid] = dict(got["first"], **got["warm"])
        for which in ("first", "warm"):
            assert any(rc.ran(k, got[which]) for k in cs["kernels"]), (cs["kernels"], got[which])
        assert got["guards_ok"], "a guard byte around the output or the accumulators changed"
        if want_acc:
            assert np.array_equal(got["acc"], acc), "accumulators"
        bad = np.argwhere(got["phys"] != want)
        assert bad.size == 0, (want_acc, len(bad), bad[:4].tolist(), got["phys"][tuple(bad[0])], want[tuple(bad[0])])
    if cs["zero"]:   # a zero scale column always replays and holds zp_out
        cols = np.flatnonzero(d["s_wv"] == 0)
        assert cols.size and (cols % 4 != 0).all()
        assert (rq.exact(acc, *rc.scales(cs, d))[..., cols] == d["zp_out"]).all()


def test_every_site_sees_relu_rebias_and_zero_column():
    rc.check_case_list()


# ---- bmm_mfma ------------------------------------------------------------------------------------------------------------------
BMM = rc.BMM


def _bmm_bordered(gpu, o, relu):
    """the result as the re-biased interior of a bordered NHWC map, m = h w pixels of n channels (as
    test_gpu_attention.test_matmul_bordered_rebiased_nhwc_result lays it out); returns (plain bytes [b, m, n], launch map)"""
    bb, m, n, k = BMM
    h, w, border = m, 1, 2
    zp = o["zp_out"]
    phys = np.full((bb, h + 2 * border, w + 2 * border, n), zp ^ 0x80, np.uint8)
    da, db = gpu.put(o["A"]), gpu.put(o["B"])
    do = abi.GuardedU8(gpu, phys.shape)
    abi.ck(abi.lib().i8ie_memcpy_h2d(gpu.h, do.ptr, phys.ctypes.data_as(C.c_void_p), C.c_size_t(phys.nbytes)))
    out = ar.BmmMat(do.ptr.value, phys[0].size, n, 1, 1)
    g = ar.BmmArgs(b=bb, m=m, n=n, k=k, a=ar.mat(da.ptr.value, m, k), bm=ar.mat(db.ptr.value, k, n), out=out, out_pix_axis=1,
                   out_h=h, out_w=w, out_border=border, s_a=o["s_a"], s_b=o["s_b"], s_out=o["s_out"], zp_a=o["zp_a"],
                   zp_b=o["zp_b"], zp_out=zp, relu=1 if relu else 0)
    with gpu.launch_map() as names:
        abi.ck(abi.lib().i8ie_bmm_u8(gpu.h, C.byref(g)))
    got = do.get()
    assert do.guards_ok()
    ring = got.copy()
    ring[:, border:-border, border:-border, :] = zp ^ 0x80
    assert (ring == (zp ^ 0x80)).all(), "a border byte was written"
    for dv in (da, db, do):
        dv.free()
    return (got[:, border:-border, border:-border, :] ^ np.uint8(0x80)).reshape(bb, m, n), names


@pytest.mark.parametrize("form", ["plain", "transposed", "bordered"])
@pytest.mark.parametrize("cls", rq.CLASSES)
def test_bmm_site(gpu, cls, form):
    i = rq.CLASSES.index(cls) + ["plain", "transposed", "bordered"].index(form)
    relu = bool(i & 1) or form == "bordered"
    o = rq.matmul_class(cls, *BMM, seed=31)
    acc = ar.matmul_acc(o["A"], o["zp_a"], o["B"], o["zp_b"])
    rep = rq.class_report(cls, acc, o["s_a"], o["s_b"], o["s_out"], o["zp_out"], relu)
    print(cls, form, rep)
    rq.check_class(rep, relu)
    want = rq.exact(acc, o["s_a"], o["s_b"], o["s_out"], o["zp_out"], o["zp_out"] if relu else 0)
    if form == "bordered":
        got, names = _bmm_bordered(gpu, o, relu)
    else:
        got, gacc, names = tga._bmm(gpu, o["A"], o["zp_a"], o["B"], o["zp_b"], relu=relu, o_s8=form == "transposed",
                                    out_t=form == "transposed", qp=(o["s_a"], o["s_b"], o["s_out"], o["zp_out"]))
        assert np.array_equal(gacc, acc)
    SEEN["bmm-%s-%s" % (cls, form)] = names
    assert names == {"bmm_mfma": 1}, names
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- attn_mfma: the S and the O epilogue -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tk", [16, 64])
@pytest.mark.parametrize("which", ["S", "O"])
@pytest.mark.parametrize("cls", rq.CLASSES)
def test_attention_site(gpu, cls, which, tk):
    b, heads, d, tq = rc.ATT
    i = rq.CLASSES.index(cls) + (tk == 64)
    relu, o_s8 = bool(i & 1), bool(i & 1)
    q, k, v, qp = (rq.scores_class if which == "S" else rq.attention_class)(cls, b, heads, d, tq, tk, seed=rc.ATT_SEED + tk)
    want = mr.attention_u8(q, k, v, heads, relu=relu, **qp)
    S, P, acc, O = want
    if which == "S":   # the scores of every head: lo = 0, the plain pack; features along tk
        sacc = np.stack([ar.matmul_acc(q[:, :, h * d:(h + 1) * d], qp["zp_q"], k[:, :, h * d:(h + 1) * d], qp["zp_k"], transpose_b=True)
                         for h in range(heads)], axis=1)
        rep = rq.class_report(cls, sacc, qp["s_q"], qp["s_k"], qp["s_s"], qp["zp_s"], False)
        assert np.array_equal(S, rq.exact(sacc, qp["s_q"], qp["s_k"], qp["s_s"], qp["zp_s"]))
    else:
        assert (P == 256 // tk).all()
        rep = rq.class_report(cls, acc, mr.P_SCALE, qp["s_v"], qp["s_o"], qp["zp_o"], relu)
        assert np.array_equal(O, rq.exact(acc, mr.P_SCALE, qp["s_v"], qp["s_o"], qp["zp_o"], qp["zp_o"] if relu else 0))
    print(cls, which, tk, rep)
    rq.check_class(rep, relu and which == "O")
    tgm.check(gpu, q, k, v, heads, qp, "attn_mfma", want=want, relu=relu, o_s8=o_s8)
    SEEN["attn-%s-%s-%d" % (cls, which, tk)] = {"attn_mfma": 1}


# ---- the guard arithmetic over contiguous accumulators -------------------------------------------------------------------------
ROWS = 127 * 256   # accumulators 0 .. 32511 and their negatives


def _sweep_rows(k):
    r = np.arange(ROWS)
    q = np.zeros((ROWS, k), np.uint8)
    q[:, 0], q[:, 1] = r % 127, r // 127
    return q


@pytest.fixture(scope="module")
def sweep_combos():
    return rq.sweep_combos()


def test_guard_sweep_per_channel_tiled_linear(gpu, sweep_combos):
    """rows are base-127 digits, the columns' weights (+-1, +-127, 0 ...), zp_in = 0: column j's accumulators are the integers
    0 .. 32511 (j even) or their negatives; column j requantises with s_w * (a per-column factor from row_scales)"""
    K, n = 32, 32
    q = _sweep_rows(K)
    qw = np.zeros((n, K), np.int8)
    qw[0::2, 0], qw[0::2, 1], qw[1::2, 0], qw[1::2, 1] = 1, 127, -1, -127
    acc = orc_linear_acc(q, qw)
    assert np.array_equal(acc[:, 0], np.arange(ROWS)) and np.array_equal(acc[:, 1], -np.arange(ROWS))
    cs = dict(lr.DEFAULTS, kind="lin", m=ROWS, K=K, n=n, variant=lr.V_TILED, pc=True, id="sweep")
    spread = (rq.row_scales(n, np.random.default_rng(3)) / f32(2e-3)).astype(f32)   # in (1/30, 1]
    replayed, jobs = 0, []
    for s_in, s_w, s_out, zp in sweep_combos:
        s_wv = (f32(s_w) * spread).astype(f32)
        s_wv[0:2] = f32(s_w)
        _, worst = rq.estimate(acc, s_in, s_wv, s_out, zp)
        replayed += int((worst < f32(rq.GUARD)).sum()) if rq.fast(s_in, s_wv, s_out) else 0
        jobs.append((dict(q=q, qw=qw, qb=np.zeros(n, np.int8), s_in=f32(s_in), zp_in=0, x=None, s_wv=s_wv, s_w=f32(s_w),
                          s_out=f32(s_out), zp_out=zp), rq.exact(acc, s_in, s_wv, s_out, zp)))
    print("values inside the guard over the sweep:", replayed)
    assert replayed >= 100
    for d, want in jobs:
        got = lr.run(gpu, cs, d)
        assert got["error"] is None and got["guards_ok"]
        assert rc.ran("igemm_lin_128x32", got["warm"]), got["warm"]
        assert np.array_equal(got["phys"], want), (d["s_in"], d["s_w"], d["s_out"], d["zp_out"], np.argwhere(got["phys"] != want)[:4])


def orc_linear_acc(q, qw):
    import orc
    return orc.linear(q, qw, np.zeros(qw.shape[0], np.int8), f32(1), 0, f32(1), f32(1), 0, want_acc=True)[1]


def test_guard_sweep_bmm(gpu, sweep_combos):
    """A's rows are the same digits (zp_a = 0), B's columns hold zp_b +- 1, zp_b +- 127 with zp_b = 128"""
    k, n = 16, 16
    A = _sweep_rows(k)[None]
    B = np.full((1, k, n), 128, np.uint8)
    B[0, 0, 0::2], B[0, 1, 0::2], B[0, 0, 1::2], B[0, 1, 1::2] = 129, 255, 127, 1
    acc = ar.matmul_acc(A, 0, B, 128)
    assert np.array_equal(acc[0, :, 0], np.arange(ROWS)) and np.array_equal(acc[0, :, 1], -np.arange(ROWS))
    replayed = 0
    for s_a, s_b, s_out, zp in sweep_combos:
        _, worst = rq.estimate(acc, s_a, s_b, s_out, zp)
        replayed += int((worst < f32(rq.GUARD)).sum())
    print("values inside the guard over the sweep:", replayed)
    assert replayed >= 100
    for i, (s_a, s_b, s_out, zp) in enumerate(sweep_combos):
        relu = bool(i & 1)
        got, gacc, names = tga._bmm(gpu, A, 0, B, 128, relu=relu, qp=(f32(s_a), f32(s_b), f32(s_out), zp))
        assert names == {"bmm_mfma": 1}, names
        assert np.array_equal(gacc, acc)
        want = rq.exact(acc, s_a, s_b, s_out, zp, zp if relu else 0)
        assert np.array_equal(got, want), (s_a, s_b, s_out, zp, np.argwhere(got != want)[:4])


# ---- every kernel of the table ran in some case ---------------------------------------------------------------------------------
def test_every_kernel_of_the_table_ran(gpu):
    """over the launch maps the cases above collected; a case that did not run in this session (a partial run) is run here for
    its map alone"""
    for cid, cs in rc.CASES.items():
        if cid not in SEEN:
            got = lr.run(gpu, cs, rc.operands(cs))
            SEEN[cid] = dict(got["first"], **got["warm"])
    if not any(k.startswith("bmm-") for k in SEEN):
        o = rq.matmul_class("ALL", *BMM, seed=31)
        SEEN["bmm-"] = tga._bmm(gpu, o["A"], o["zp_a"], o["B"], o["zp_b"], qp=(o["s_a"], o["s_b"], o["s_out"], o["zp_out"]))[2]
    if not any(k.startswith("attn-") for k in SEEN):
        q, k, v, qp = rq.attention_class("ALL", *rc.ATT, 16, seed=23)
        SEEN["attn-"] = tgm.run(gpu, q, k, v, 2, qp)[4]
    seen = {}
    for m in SEEN.values():
        seen.update(m)
    missing = [(f, name) for f, names in rc.TABLE.items() for name in names if not rc.ran(name, seen)]
    assert not missing, (missing, sorted(seen))
