"""Rectangular Conv2d on the GPU: every case of tests/rectconv_ref.py through a handle of
i8ie_conv2d_create_rect(_per_channel) -- the kernel that ran against rectconv_ref.dispatch(), the INT32 accumulators and every
byte of the physical output with guard bytes, against the oracle on the embedded kernel, with and without ReLU; the layout
matrix; the handle's answers; equal pairs against the dilated entry; the stateless and the FP32 entry; the Python surface."""
import ctypes as C
import zlib

import numpy as np
import pytest

import abi
import concat_ref as cr
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import padpool_ref as pp
import rectconv_ref as rr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32

ctx = support.ctx_fixture(rr)


@pytest.mark.parametrize("case", rr.CASES, ids=[c.name for c in rr.CASES])
def test_case(ctx, case):
    d = rr.reference(case)
    kernel = rr.dispatch(case)
    for relu in (False, True):
        want = np.maximum(d["want"], np.uint8(rr.ZP_OUT)) if relu else d["want"]
        r = rr.run(ctx, case, relu)
        tag = "%s relu=%d" % (case.name, relu)
        print(tag, sorted(r["names"]))
        assert rr.KERNELS & set(r["names"]) == {kernel}, (tag, r["names"])
        assert np.array_equal(r["acc"], d["acc"]), tag + ": accumulators"
        assert np.array_equal(r["out"], want), tag
        assert r["ok"], tag + ": a byte outside the output or the accumulators was written"


@pytest.mark.parametrize("name", rr.LAYOUT_CASES)
def test_layout_matrix(ctx, name):
    case = rr.BY_NAME[name]
    d = rr.reference(case)
    relu_want = np.maximum(d["want"], np.uint8(rr.ZP_OUT))
    lays = [dict(in_nhwc=False, out_nhwc=False)]
    for ib in (0, 1, 3):
        for ob in (0, 1):
            lays.append(dict(in_nhwc=True, out_nhwc=True, in_border=ib, out_border=ob))
    lays += [dict(in_nhwc=True, out_nhwc=False, in_border=1), dict(in_nhwc=False, out_nhwc=True, out_border=1),
             dict(in_nhwc=True, out_nhwc=True, in_border=1, out_border=1, in_s8=True),
             dict(in_nhwc=True, out_nhwc=True, in_border=0, out_border=1, out_s8=True),
             dict(in_nhwc=True, out_nhwc=True, in_border=3, out_border=0, in_s8=True, out_s8=True)]
    for kw in lays:
        r = rr.run(ctx, case, True, **kw)
        assert rr.KERNELS & set(r["names"]) == {rr.dispatch(case)}, (kw, r["names"])
        assert np.array_equal(r["acc"], d["acc"]) and np.array_equal(r["out"], relu_want) and r["ok"], kw
        if kw["out_nhwc"]:
            assert np.array_equal(r["phys"], abi.Ctx.to_phys(relu_want, kw.get("out_border", 0), rr.ZP_OUT)), kw
    # a following max-pool through the peel passes, plain and re-biased
    pooled = orc.max_pool2d(relu_want, 2, 2)
    for kw in (dict(in_nhwc=True, out_nhwc=True, in_border=1, out_border=1), dict(in_nhwc=False, out_nhwc=False),
               dict(in_nhwc=True, out_nhwc=True, in_border=0, out_border=1, out_s8=True)):
        r = rr.run(ctx, case, True, pool=(2, 2), **kw)
        assert rr.KERNELS & set(r["names"]) == {rr.dispatch(case)}, (kw, r["names"])
        assert np.array_equal(r["acc"], d["acc"]) and np.array_equal(r["out"], pooled) and r["ok"], kw


def _geometry(L):
    g = rr.CGeom()
    abi.ck(abi.lib().i8ie_layer_geometry(L, C.byref(g)))
    return tuple(getattr(g, n) for n, _ in rr.CGeom._fields_)


def test_handle_answers(ctx):
    lib = abi.lib()
    for name in ("1x7_line17-pt", "3x3_dil_2_1-pc", "stride_2_1-pt"):
        case = rr.BY_NAME[name]
        L = rr.create(ctx, case, rr.reference(case))
        pad, dil = C.c_int(-1), C.c_int(-1)
        abi.ck(lib.i8ie_layer_padding(L, C.byref(pad)))
        rc = lib.i8ie_layer_dilation(L, C.byref(dil))
        text = lib.i8ie_last_error()
        q = ctx.layer_queries(L, 2, case.h, case.w, 2, 2)
        geom = _geometry(L)
        lib.i8ie_layer_destroy(L)
        assert pad.value == 0 and geom == tuple(case.geom)
        assert q == dict(fuses_pool=0, reads_s8=0, stores_s8=0, accepts_f32=0, preferred_layout=1), q
        if case.geom.dh != case.geom.dw:
            assert rc == -1 and b"i8ie_layer_geometry" in text
        else:
            assert rc == 0 and dil.value == case.geom.dh
    # a square handle of an old entry answers with equal pairs
    case = rr.BY_NAME["1x7_line17-pt"]
    d = rr.reference(case)
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    qw = np.zeros((16, 32, 3, 3), np.int8)
    L = C.c_void_p()
    abi.ck(lib.i8ie_conv2d_create(ctx.h, P(qw), P(d["qb"]), 16, 32, 3, 3, 2, 1, C.c_float(0.01), C.byref(L)))
    geom = _geometry(L)
    lib.i8ie_layer_destroy(L)
    assert geom == (3, 3, 2, 2, 1, 1, 1, 1)


def _forward_names(ctx, create, q, s_out, h, w, oshape):
    lib = abi.lib()
    L = C.c_void_p()
    create(L)
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(s_out), C.c_uint8(37)))
    di, out = ctx.put(q), ctx.empty(oshape, np.uint8)
    try:
        _, names = ctx.kernels_run(lambda: abi.ck(lib.i8ie_layer_forward(L, di.ptr, q.shape[0], h, w, C.c_float(0.03), C.c_uint8(121),
                                                                         out.ptr, None)))
        return out.get(), sorted(names)
    finally:
        lib.i8ie_layer_destroy(L)
        di.free()
        out.free()


@pytest.mark.parametrize("k,s,p,d,g,c", [(3, 1, 1, 1, 1, 32), (3, 2, 1, 1, 1, 32), (3, 1, 2, 2, 1, 32), (3, 1, 1, 1, 2, 32), (1, 1, 0, 3, 1, 32),
                                        (3, 1, 1, 1, 1, 6)])
def test_equal_pairs_are_the_dilated_entry(ctx, k, s, p, d, g, c):
    """all four pairs equal through the new entry: the kernels and the bytes of i8ie_conv2d_create_dilated"""
    lib = abi.lib()
    rng = np.random.default_rng(k * 100 + s * 10 + d + g)
    kc, h, w = 16, 9, 11
    q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (kc, c // g, k, k), dtype=np.int8)
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    geom = rr.cgeom(rr.G(k, k, (s, s), (p, p), (d, d)))
    oh, ow = rr.out_hw(h, w, rr.G(k, k, (s, s), (p, p), (d, d)))
    s_out = f32(0.03 * 0.002 * np.sqrt(c // g * k * k) * 74 * 73 / 20)
    new = lambda L: abi.ck(lib.i8ie_conv2d_create_rect(ctx.h, P(qw), P(qb), kc, c, g, C.byref(geom), C.c_float(0.002), C.byref(L)))  # noqa: E731
    old = lambda L: abi.ck(lib.i8ie_conv2d_create_dilated(ctx.h, P(qw), P(qb), kc, c, k, k, s, p, g, d, C.c_float(0.002), C.byref(L)))  # noqa: E731
    a, na = _forward_names(ctx, new, q, s_out, h, w, (2, kc, oh, ow))
    b, nb = _forward_names(ctx, old, q, s_out, h, w, (2, kc, oh, ow))
    print(na)
    assert na == nb and "lconv_mfma" not in na and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["1x7_line17-pt", "c6-pt", "depthwise_5x1-pt", "conv1d_s2_h1-pt"])
def test_stateless(ctx, name):
    case = rr.BY_NAME[name]
    d = rr.reference(case)
    _, _, Kg, oh, ow = rr.geom_k(case)
    lib = abi.lib()
    di, dw, db = ctx.put(d["q"]), ctx.put(d["qw"]), ctx.put(d["qb"])
    oc = ctx.empty((case.kc,), np.int32)
    out, acc = abi.GuardedU8(ctx, (case.m, case.kc, oh, ow)), abi.GuardedU8(ctx, (case.m, oh * ow, case.kc), np.int32)
    geom = rr.cgeom(case.geom)
    try:
        abi.ck(lib.i8ie_conv_offsets(ctx.h, dw.ptr, db.ptr, case.kc, Kg, C.c_float(rr.S_IN), C.c_uint8(case.zp_in), oc.ptr))
        abi.ck(lib.i8ie_conv2d_u8s8_rect(ctx.h, di.ptr, case.m, case.c, case.h, case.w, dw.ptr, case.kc, case.g, C.byref(geom), case.zp_in,
                                         oc.ptr, rr.S_IN, d["s_w"], d["s_out"], rr.ZP_OUT, out.ptr, acc.ptr))
        got, gacc = out.get(), acc.get()
        ok = out.guards_ok() and acc.guards_ok()
    finally:
        for b in (di, dw, db, oc, out, acc):
            b.free()
    assert ok and np.array_equal(gacc, d["acc"]) and np.array_equal(got, d["want"])


# ---- FP32 -----------------------------------------------------------------------------------------------------------------
def _f32(ctx, x, w, b, g, geom, dilated_entry=False):
    lib = abi.lib()
    n, c, h, wd = x.shape
    kc = w.shape[0]
    oh, ow = rr.out_hw(h, wd, geom)
    di, dw, db, o = ctx.put(x), ctx.put(w), ctx.put(b), ctx.guarded((n, kc, oh, ow))
    cg = rr.cgeom(geom)
    try:
        if dilated_entry:
            abi.ck(lib.i8ie_conv2d_f32_dilated(ctx.h, di.ptr, n, c, h, wd, dw.ptr, db.ptr, kc, geom.kh, geom.kw, geom.sh, geom.ph, g, geom.dh,
                                               o.ptr))
        else:
            abi.ck(lib.i8ie_conv2d_f32_rect(ctx.h, di.ptr, n, c, h, wd, dw.ptr, db.ptr, kc, g, C.byref(cg), o.ptr))
        return o.read()
    finally:
        for t in (di, dw, db, o):
            t.free()


F32_CASES = [t for _, t in rr.LINES[:4] + rr.LINES[5:7] + rr.GENERAL[:-1]]


@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("t", F32_CASES, ids=[n for n, _ in rr.LINES[:4] + rr.LINES[5:7] + rr.GENERAL[:-1]])
def test_conv2d_f32_rect(ctx, t, cls):
    m, c, kc, g, geom, h, w = t
    rng = np.random.default_rng(zlib.crc32((repr(t) + cls).encode()))
    xs, ws = (m, c, h, w), (kc, c // g, geom.kh, geom.kw)
    if cls == "exact":
        x, wt, b = (rng.integers(-8, 9, xs).astype(f32), rng.integers(-8, 9, ws).astype(f32), rng.integers(-64, 65, kc).astype(f32))
    else:
        x, wt, b = (rng.uniform(-1, 1, xs).astype(f32), rng.uniform(-1, 1, ws).astype(f32), rng.uniform(-1, 1, kc).astype(f32))
    got, ok = _f32(ctx, x, wt, b, g, geom)
    xp, we = rr.pad_input(x, geom, 0.0), rr.embed(wt, geom)
    want = gr.conv2d_f64(xp, we, b, g, 1, 0)[:, :, ::geom.sh, ::geom.sw]
    assert ok and got.shape == want.shape and abi.GuardedOut.unwritten(got) == 0
    if cls == "exact":
        assert np.abs(want).max() < 2.0 ** 24 and np.array_equal(got.view(np.uint32), (want + 0.0).astype(f32).view(np.uint32))
    else:
        mag = gr.conv2d_f64_mag(xp, we, b, g, 1, 0)[:, :, ::geom.sh, ::geom.sw]
        err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, (c // g) * geom.kh * geom.kw)  # (the true K)
        assert np.all(err <= bound), float(np.nanmax(err / bound))


@pytest.mark.parametrize("g", [1, 2])
def test_conv2d_f32_equal_pairs_is_the_dilated_entry(ctx, g):
    rng = np.random.default_rng(g)
    x, wt, b = rng.uniform(-1, 1, (2, 12, 9, 7)).astype(f32), rng.uniform(-1, 1, (10, 12 // g, 3, 3)).astype(f32), rng.uniform(-1, 1, 10).astype(f32)
    geom = rr.G(3, 3, (2, 2), (2, 2), (2, 2))
    a, oka = _f32(ctx, x, wt, b, g, geom)
    c, okc = _f32(ctx, x, wt, b, g, geom, dilated_entry=True)
    assert oka and okc and np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def _conv(i8ie, cin, cout, k, pad, seed, qp, per_channel=False):
    rng = np.random.default_rng(seed)
    L = i8ie.Conv2d(cin, cout, k, padding=pad)
    kh, kw = (k, k) if isinstance(k, int) else k
    L.load_weight((rng.uniform(-1, 1, (cout, cin, kh, kw)) * np.sqrt(6.0 / (cin * kh * kw))).astype(f32))
    L.load_bias(rng.uniform(-0.1, 0.1, cout).astype(f32))
    if qp is not None:
        L.set_output_qparams(*qp)
        L.convert(per_channel)
    return L


def _expect(L, q, s_in, zp_in, relu=True):
    """the bytes a converted Conv2d must give on the bytes q: the oracle on the embedded kernel"""
    gd = L.geometry()
    geom = rr.G(*gd["kernel_size"], s=gd["stride"], p=gd["padding"], d=gd["dilation"])
    s_out, zp_out = L.output_qparams()
    qp, we = rr.pad_input(q, geom, zp_in), rr.embed(L.layer.q_weight(), geom)
    if L.is_per_channel():
        full, _ = gr.conv2d_grouped_pc(qp, we, L.layer.q_bias(), L.groups(), 1, 0, f32(s_in), zp_in, L.weight_scales(), f32(s_out), zp_out)
    else:
        full, _ = gr.conv2d_grouped(qp, we, L.layer.q_bias(), L.groups(), 1, 0, f32(s_in), zp_in, L.weight_scale(), f32(s_out), zp_out)
    out = np.ascontiguousarray(full[:, :, ::geom.sh, ::geom.sw])
    return np.maximum(out, np.uint8(zp_out)) if relu else out


def test_1x7_relu_7x1_is_two_launches(i8ie):
    """an activation in the engine's layout -> Conv2d(1x7) -> relu -> Conv2d(7x1) -> relu: two launches of lconv_mfma, no border,
    fill, layout or relu pass, and the oracle's bytes"""
    q = support.activation(i8ie, 9)
    assert q.data.layout() == 1  # NHWC
    a = _conv(i8ie, 16, 32, (1, 7), (0, 3), 5, (0.04, 110))
    b = _conv(i8ie, 32, 16, (7, 1), (3, 0), 6, (0.05, 120), per_channel=True)
    assert type(a.layer).__name__ == "_Conv2dRect"
    first, again, launches = support.counted_forward(lambda: i8ie.relu(b(i8ie.relu(a(q)))))
    assert launches == {"lconv_mfma": 2}, launches
    mid = _expect(a, q.numpy(), q.scale, q.zero_point)
    want = _expect(b, mid, 0.04, 110)
    assert np.array_equal(first, want) and np.array_equal(again, want) and want.shape == (2, 16, 9, 9)


class _InceptionC:
    """a hand-built Inception-C block at 17 x 17: 1x1 | 1x7 -> 7x1 | 7x1 -> 1x7 -> 7x1 -> 1x7 | avg_pool(3, 1, 1) -> 1x1, joined"""
    CONVS = [("b1", 32, 32, 1, 0), ("b7a", 32, 16, 1, 0), ("b7b", 16, 16, (1, 7), (0, 3)), ("b7c", 16, 32, (7, 1), (3, 0)),
             ("d7a", 32, 16, 1, 0), ("d7b", 16, 16, (7, 1), (3, 0)), ("d7c", 16, 16, (1, 7), (0, 3)), ("d7d", 16, 16, (7, 1), (3, 0)),
             ("d7e", 16, 32, (1, 7), (0, 3)), ("bp", 32, 32, 1, 0)]

    @staticmethod
    def build(i8ie):
        class Net(i8ie.Module):
            def __init__(self):
                super().__init__()
                self.stem = _conv(i8ie, 3, 32, 3, 1, 40, None)
                for i, (name, cin, cout, k, pad) in enumerate(_InceptionC.CONVS):
                    setattr(self, name, _conv(i8ie, cin, cout, k, pad, 41 + i, None))
                self.cat = i8ie.Concat()

            def steps(self, x, see=lambda *a: None):
                r = i8ie.relu

                def conv(name, t):
                    y = r(getattr(self, name)(t))
                    see(name, t, y)
                    return y

                x = conv("stem", x)
                b1 = conv("b1", x)
                b7 = conv("b7c", conv("b7b", conv("b7a", x)))
                d7 = conv("d7e", conv("d7d", conv("d7c", conv("d7b", conv("d7a", x)))))
                pooled = i8ie.avg_pool2d(x, 3, 1, padding=1)
                see("pool", x, pooled)
                bp = conv("bp", pooled)
                y = self.cat([b1, b7, d7, bp])
                see("cat", [b1, b7, d7, bp], y)
                return y

            def forward(self, x):
                return self.steps(x)

        return Net()


def test_inception_c_block_step_by_step(i8ie, tmp_path):
    """calibrate, convert, then every step of the block bit for bit; a save / load round trip; a HIP-graph replay"""
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(11)
    net = _InceptionC.build(i8ie)
    xs = rng.uniform(-2, 2, (4, 3, 17, 17)).astype(f32)
    net.prepare()
    net(i8ie.tensor(xs))   # FP32 through i8ie_conv2d_f32_rect, sampled by the calibrator
    net.convert()
    x = rng.uniform(-2, 2, (2, 3, 17, 17)).astype(f32)
    seen = []

    def see(name, t, y):
        if name == "cat":
            want = cr.cat_u8([(b.numpy(), b.scale, b.zero_point) for b in t], y.scale, y.zero_point)
        elif name == "pool":
            want = pp.avg_pool2d_u8(t.numpy(), 3, 1, 1, zp=t.zero_point)
        else:
            want = _expect(getattr(net, name), t.numpy(), t.scale, t.zero_point)
        got = y.numpy()
        assert np.array_equal(got, want), name
        seen.append((name, len(np.unique(got))))

    from i8ie import module

    qx = i8ie.quantize(i8ie.tensor(x), module.INPUT_SCALE, module.INPUT_ZERO_POINT)   # (what a converted Module does to its input)
    last = net.steps(qx, see)
    stepped = i8ie.dequantize(last).numpy()   # (a converted Module dequantizes its result)
    assert len(seen) == 13 and stepped.shape == (2, 128, 17, 17) and last.numpy().dtype == np.uint8
    assert all(n > 8 for _, n in seen), seen   # (no step's map is saturated)
    whole = net(i8ie.tensor(x)).numpy()
    assert support.same_bits(whole, stepped)
    assert [net.b7b.geometry()["kernel_size"], net.d7b.geometry()["padding"]] == [(1, 7), (3, 0)]
    # save / load
    path = str(tmp_path / "inc.npz")
    net.save_quantized(path)
    fresh = _InceptionC.build(i8ie)
    fresh.load_quantized_file(path)
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), stepped)
    # a HIP-graph replay
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert support.same_bits(g().numpy(), stepped)
