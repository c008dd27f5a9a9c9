"""The quantized GroupNorm on the GPU (csrc/i8ie_groupnorm.hip).  Every byte is compared against the numpy
restatement of the definition (tests/groupnorm_ref.py), never against the code under test: every group shape through the form
its sizes select and through the direct form, the LDS budget's edge, the split form's chunks, the statistics extremes, the
bordered / re-biased layouts with guard bytes in all three forms, the FP32 entry against float64, and the Python surface
(shapes, launch counts, calibration, save / load, graph replay)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import groupnorm_ref as gn
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import spec_ref as sr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
QP = support.NORM_QP   # s_in, s_out, zp_out, eps
# (C, G): cg = 1 (InstanceNorm), 2, 4, 10, 16, 32, G = 1, and two channel counts that are no multiple of 16 (direct)
GROUPS = [(32, 32), (64, 32), (16, 4), (160, 16), (64, 4), (64, 2), (48, 1), (320, 32), (20, 5), (35, 7)]
MAPS = [(1, 1), (3, 5), (8, 8), (7, 9)]


ctx = support.ctx_fixture(gn)


def _images(rng, n, Cn, h, w):
    """n images of distinct content: uniform bytes, a narrow image, a ramp over channels"""
    q = rng.integers(0, 256, (n, Cn, h, w), dtype=np.uint8)
    if n > 1:
        q[1] = (rng.integers(0, 9, (Cn, h, w)) + 60).astype(np.uint8)
    if n > 2:
        q[2] = ((np.arange(Cn).reshape(Cn, 1, 1) * 5 + rng.integers(0, 40, (Cn, h, w))) % 256).astype(np.uint8)
    return q


def _run(ctx, q, G, dg, db, qp=QP, relu=False, fallback=False, bi=0, bo=0, in_s8=0, out_s8=0, in_place=False, rng=None):
    """one call of i8ie_groupnorm_u8_nhwc on [n, C, h, w] bytes; returns the interior as NCHW.  Checks the guard bytes of both
    buffers, that the input and the result's border are untouched, and which kernels ran.  ws is filled with 0xFF."""
    n, Cn, h, w = q.shape
    s_in, _, zp_out, eps = qp
    rng = rng or np.random.default_rng(0)
    phys_in = rng.integers(0, 256, (n, h + 2 * bi, w + 2 * bi, Cn), dtype=np.uint8)   # a garbage border: it is never read
    phys_in[:, bi:bi + h, bi:bi + w, :] = q.transpose(0, 2, 3, 1) ^ np.uint8(0x80 if in_s8 else 0)
    di = abi.GuardedU8(ctx, phys_in.shape)
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, di.ptr, phys_in.ctypes.data_as(C.c_void_p), C.c_size_t(phys_in.nbytes)))
    if in_place:
        assert bi == bo and in_s8 == out_s8
        do, phys_out = di, phys_in
    else:
        ring = np.uint8(zp_out ^ (0x80 if out_s8 else 0))
        phys_out = np.full((n, h + 2 * bo, w + 2 * bo, Cn), ring, np.uint8)   # as i8ie_fill_border_u8 leaves it
        do = abi.GuardedU8(ctx, phys_out.shape)
        abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, do.ptr, phys_out.ctypes.data_as(C.c_void_p), C.c_size_t(phys_out.nbytes)))
    nbytes = abi.lib().i8ie_groupnorm_workspace_bytes(n, Cn, G, h, w)
    assert nbytes == gn.workspace_bytes(n, Cn, G, h, w)
    ws = abi.GuardedU8(ctx, (max(nbytes, 16),), fill=0xFF)
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_groupnorm_u8_nhwc(ctx.h, di.ptr, bi, in_s8, do.ptr, bo, out_s8, n, Cn, G, h, w, dg.ptr, db.ptr, s_in, eps,
                                                   1 if relu else 0, zp_out, ws.ptr if nbytes else None))
    finally:
        ctx.set_force_fallback(False)
    got = do.get()
    ws.get()
    assert do.guards_ok() and di.guards_ok() and ws.guards_ok()
    assert names == gn.kernels(Cn, h, w, fallback), (names, q.shape, fallback)
    if not in_place:
        assert np.array_equal(di.get(), phys_in)
        do.free()
    outside = got.copy()
    outside[:, bo:bo + h, bo:bo + w, :] = phys_out[:, bo:bo + h, bo:bo + w, :]
    assert np.array_equal(outside, phys_out)   # nothing but the interior was written
    di.free(); ws.free()
    return np.ascontiguousarray((got[:, bo:bo + h, bo:bo + w, :] ^ np.uint8(0x80 if out_s8 else 0)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("Cn,G", GROUPS)
def test_group_shapes_image_form_and_forced_fallback(ctx, Cn, G):
    """n = 3 images of distinct content (a mix-up of images or groups changes bytes), every map, relu on / off, in place"""
    rng = np.random.default_rng(500 + Cn + G)
    gamma, beta, dg, db = support.norm_params(ctx, Cn, Cn)
    spread = set()
    for h, w in MAPS:
        assert gn.form(Cn, h, w) == ("direct" if Cn % 16 else "image")
        q = _images(rng, 3, Cn, h, w)
        for relu in (False, True):
            want = gn.group_norm_u8(q, G, QP[0], QP[3], gamma, beta, QP[1], QP[2], relu)
            spread |= set(np.unique(want).tolist())
            for fallback, in_place in ((False, False), (True, False), (False, True)):
                got = _run(ctx, q, G, dg, db, relu=relu, fallback=fallback, in_place=in_place)
                assert np.array_equal(got, want), (Cn, G, h, w, relu, fallback, in_place, np.argwhere(got != want)[:4])
    assert len(spread) > 40
    dg.free(); db.free()


# (C, G, h, w, n): the LDS budget's edge (the same C, one pixel row apart), then split-form shapes whose pixel count is no
# multiple of the chunk, with more chunks than one: cg = 2 (byte units), 10 (byte units, C / 16 no power of two), 4 (dword
# units), 16 (item units)
SPLIT = [(64, 32, 48, 32, 3), (64, 32, 49, 32, 3), (64, 32, 56, 56, 2), (160, 16, 25, 25, 2), (128, 32, 28, 28, 2), (256, 16, 20, 20, 2)]


@pytest.mark.parametrize("Cn,G,h,w,n", SPLIT)
def test_lds_budget_edge_and_split_form(ctx, Cn, G, h, w, n):
    edge = (Cn, h, w) == (64, 48, 32)
    assert gn.form(Cn, h, w) == ("image" if edge else "split") and (edge or gn.chunks(Cn, h, w) > 1)
    assert edge or (h * w) % max(1, gn.CHUNK_BYTES // Cn) != 0
    assert not edge or h * w * Cn == gn.IMAGE_BYTES
    rng = np.random.default_rng(Cn + h)
    gamma, beta, dg, db = support.norm_params(ctx, Cn, Cn + 1)
    q = _images(rng, n, Cn, h, w)
    for relu in (False, True):
        want = gn.group_norm_u8(q, G, QP[0], QP[3], gamma, beta, QP[1], QP[2], relu)
        assert len(np.unique(want)) > 40
        for fallback, in_place in ((False, False), (True, False), (False, True)):
            got = _run(ctx, q, G, dg, db, relu=relu, fallback=fallback, in_place=in_place)
            assert np.array_equal(got, want), (relu, fallback, in_place, np.argwhere(got != want)[:4])
    dg.free(); db.free()


@pytest.mark.parametrize("Cn,G", [(16, 1), (32, 2)], ids=["image", "split"])
def test_statistics_extremes_on_the_device(ctx, Cn, G):
    """N = 65536 in both 16-byte forms and in the direct one"""
    assert gn.form(Cn, 64, 64) == ("image" if Cn == 16 else "split")
    for name, q in gn.extreme_images(Cn, G):
        for qp in (QP, (f32(0.1), f32(0.05), 100, f32(1e-6))):
            gamma, beta, dg, db = support.norm_params(ctx, Cn, 7 + Cn, qp)
            want = gn.group_norm_u8(q, G, qp[0], qp[3], gamma, beta, qp[1], qp[2])
            for fallback in (False, True):
                got = _run(ctx, q, G, dg, db, qp=qp, fallback=fallback)
                assert np.array_equal(got, want), (name, fallback, np.argwhere(got != want)[:4])
            dg.free(); db.free()


@pytest.mark.parametrize("Cn,G,h,w,n,fallback", [(32, 8, 3, 5, 2, False), (64, 32, 49, 32, 1, False), (20, 5, 3, 5, 2, False),
                                                 (32, 8, 3, 5, 2, True)], ids=["image", "split", "direct", "fallback"])
def test_layout_matrix_borders_rebias_relu_in_place_and_guards(ctx, Cn, G, h, w, n, fallback):
    rng = np.random.default_rng(40 + Cn)
    s_in, s_out, zp_out, eps = QP
    gamma, beta, dg, db = support.norm_params(ctx, Cn, Cn)
    q = _images(rng, n, Cn, h, w)
    want = {relu: gn.group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out, bool(relu)) for relu in (0, 1)}
    for bi, bo, in_s8, out_s8, relu in itertools.product((0, 1, 2), (0, 1, 3), (0, 1), (0, 1), (0, 1)):
        got = _run(ctx, q, G, dg, db, relu=bool(relu), fallback=fallback, bi=bi, bo=bo, in_s8=in_s8, out_s8=out_s8, rng=rng)
        assert np.array_equal(got, want[relu]), (bi, bo, in_s8, out_s8, relu, np.argwhere(got != want[relu])[:4])
        if bi == bo and in_s8 == out_s8:
            got = _run(ctx, q, G, dg, db, relu=bool(relu), fallback=fallback, bi=bi, bo=bo, in_s8=in_s8, out_s8=out_s8, in_place=True, rng=rng)
            assert np.array_equal(got, want[relu]), ("in place", bi, in_s8, relu)
    dg.free(); db.free()


def test_argument_errors_launch_nothing(ctx):
    buf = ctx.put(np.zeros(8192, np.uint8))
    p = buf.ptr.value
    with ctx.launch_map() as names:
        for Cn, G, h, w, s_in, eps, ws in ((0, 1, 2, 2, 0.1, 1e-5, p), (16, 3, 2, 2, 0.1, 1e-5, p), (16, 1, 64, 65, 0.1, 1e-5, p),
                                           (16, 4, 2, 2, 0.0, 1e-5, p), (16, 4, 2, 2, 0.1, float("inf"), p), (64, 32, 56, 56, 0.1, 1e-5, None)):
            assert abi.lib().i8ie_groupnorm_u8_nhwc(ctx.h, p, 0, 0, p, 0, 0, 1, Cn, G, h, w, p + 1024, p + 2048, s_in, eps, 0, 0, ws) == -1
        assert abi.lib().i8ie_groupnorm_u8_nhwc(ctx.h, None, 0, 0, p, 0, 0, 1, 16, 4, 2, 2, p + 1024, p + 2048, 0.1, 1e-5, 0, 0, p) == -1
        assert abi.lib().i8ie_groupnorm_u8_nhwc(ctx.h, p, -1, 0, p, 0, 0, 1, 16, 4, 2, 2, p + 1024, p + 2048, 0.1, 1e-5, 0, 0, p) == -1
    assert names == {}
    buf.free()


@pytest.mark.parametrize("Cn,G,h,w", [(6, 3, 1, 1), (15, 5, 3, 7), (16, 1, 64, 64)], ids=["N2", "N63", "N65536"])
def test_f32_against_float64(ctx, Cn, G, h, w):
    """bound: groupnorm_ref.group_norm_f32_bound, derived from N and the roundings of the fp32 sequence"""
    rng = np.random.default_rng(70 + Cn)
    x = rng.normal(0.3, 2.0, (2, Cn, h, w)).astype(f32)
    x[1, :Cn // G] = 2.5   # a constant row: var = 0, out = beta
    gamma, beta = rng.normal(1, 0.5, Cn).astype(f32), rng.normal(0, 0.5, Cn).astype(f32)
    dg, db = ctx.put(gamma), ctx.put(beta)
    di, do = ctx.put(x), ctx.guarded(x.shape)
    with ctx.launch_map() as names:
        abi.ck(abi.lib().i8ie_groupnorm_f32(ctx.h, di.ptr, do.ptr, 2, Cn, G, h * w, dg.ptr, db.ptr, 1e-5))
    got, ok = do.read()
    assert ok and abi.GuardedOut.unwritten(got) == 0 and names == {"groupnorm_f32": 1}
    err = np.abs(got.astype(np.float64) - gn.group_norm_f64(x, G, gamma, beta, 1e-5))
    bound = gn.group_norm_f32_bound(x, G, gamma, beta, 1e-5)
    print("groupnorm_f32 N=%d: max err %.3g, max err / bound %.3g" % ((Cn // G) * h * w, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(got[1, :Cn // G], np.broadcast_to(beta[:Cn // G].reshape(-1, 1, 1), (Cn // G, h, w)))
    for d in (di, do, dg, db):
        d.free()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def _gn(i8ie, groups, c, seed, qp, eps=1e-5):
    rng = np.random.default_rng(seed)
    L = i8ie.GroupNorm(groups, c, eps)
    w, b = rng.uniform(0.5, 1.5, c).astype(f32), rng.uniform(-0.3, 0.3, c).astype(f32)
    L.load_weight(w)
    L.load_bias(b)
    L.set_output_qparams(*qp)
    L.convert()
    return L, w, b


def test_surface_shapes_and_errors(i8ie):
    rng = np.random.default_rng(80)
    w, b = rng.uniform(0.5, 1.5, 12).astype(f32), rng.uniform(-0.3, 0.3, 12).astype(f32)
    for shape in ((2, 12, 3, 4), (5, 12)):
        xf = rng.uniform(-3, 3, shape).astype(f32)
        q = i8ie.quantize(i8ie.tensor(xf), 0.025, 127)
        qv = q.numpy()
        r = i8ie.relu(i8ie.group_norm(q, 3, w, b, 1e-5, 0.02, 120))
        assert r.shape == shape and r.scale == pytest.approx(0.02) and r.zero_point == 120
        assert np.array_equal(r.numpy(), gn.group_norm_u8(qv, 3, f32(0.025), f32(1e-5), w, b, f32(0.02), 120, True)), shape
        r = i8ie.group_norm(q, 12, scale=0.02, zero_point=120)   # weight, bias default to ones, zeros; InstanceNorm
        assert np.array_equal(r.numpy(), gn.group_norm_u8(qv, 12, f32(0.025), f32(1e-5), np.ones(12, f32), np.zeros(12, f32), f32(0.02), 120))
        layer, lw, lb = _gn(i8ie, 1, 12, 4, (0.03, 131))
        assert np.array_equal(layer(q).numpy(), gn.group_norm_u8(qv, 1, f32(0.025), f32(1e-5), lw, lb, f32(0.03), 131))
        got = i8ie.group_norm(i8ie.tensor(xf), 3, w, b).numpy()
        assert got.shape == shape
        assert (np.abs(got - gn.group_norm_f64(xf, 3, w, b, 1e-5).reshape(shape)) <= gn.group_norm_f32_bound(xf, 3, w, b, 1e-5).reshape(shape)).all()
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 12, 3, 4)).astype(f32)), 0.025, 127)
    g = i8ie.GroupNorm(3, 12)
    g10, _, _ = _gn(i8ie, 2, 10, 1, (0.02, 1))
    bad = [lambda: g(q),                                                     # not converted
           lambda: g10(q),                                                   # c != num_channels
           lambda: i8ie.group_norm(q.reshape(-1), 1, None, None, 1e-5, 0.02, 1),              # rank 1
           lambda: i8ie.group_norm(q.reshape(2, 12, 12), 3, None, None, 1e-5, 0.02, 1),       # rank 3
           lambda: i8ie.group_norm(q.reshape(1, 2, 12, 3, 4), 1, None, None, 1e-5, 0.02, 1),  # rank 5
           lambda: i8ie.group_norm(q, 5, w, b, 1e-5, 0.02, 1),               # C % G
           lambda: i8ie.group_norm(q, 3, w[:11], b, 1e-5, 0.02, 1),
           lambda: i8ie.group_norm(q, 3, w, b, 0.0, 0.02, 1),
           lambda: i8ie.group_norm(q, 3, w, b, 1e-5, 0.0, 1),
           lambda: i8ie.group_norm(q, 3, w, b, 1e-5, 0.02, 256)]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    for kw in ({}, {"scale": 0.2}, {"zero_point": 3}):
        with pytest.raises(TypeError):
            i8ie.group_norm(q, 3, w, b, **kw)


@pytest.mark.parametrize("h,w,form", [(6, 5, "image"), (80, 80, "split")])
def test_launch_counts_borders_and_bytes(i8ie, h, w, form):
    """conv -> GN -> relu -> padded conv is three launches in the image form and four in the split form (the GN reads the conv's
    NHWC result as it lies and writes the border and re-bias the next conv asks for); nothing converts a layout, re-biases,
    applies a relu or fills a border in between"""
    rng = np.random.default_rng(90)
    n, c = 2, 16
    assert gn.form(c, h, w) == form
    stem0 = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128))
    stem1 = support.conv(i8ie, c, c, 3, 1, 11, (0.05, 128))
    stem = support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    g, gam, bet = _gn(i8ie, 4, c, 2, (0.02, 125))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, 3, h, w)).astype(f32)), 0.025, 127)
    x = i8ie.relu(stem1(i8ie.relu(stem0(q))))

    launches = support.counted(lambda: [tail(i8ie.relu(g(stem(x))))])
    print(launches)
    mine = {k: v for k, v in launches.items() if k.startswith("groupnorm")}
    assert mine == gn.kernels(c, h, w) and sum(launches.values()) == (3 if form == "image" else 4), launches
    for k in launches:
        assert not k.startswith(("relu_u8", "rebias", "fill_border", "reborder", "layout_")), launches
    xv = x.numpy()
    yv = support.conv_ref(stem, xv, 0.05, 128, pad=1)
    lv = gn.group_norm_u8(yv, 4, f32(0.05), f32(1e-5), gam, bet, f32(0.02), 125)
    assert len(np.unique(lv)) > 40
    assert np.array_equal(g(stem(x)).numpy(), lv)
    assert np.array_equal(tail(i8ie.relu(g(stem(x)))).numpy(), support.conv_ref(tail, np.maximum(lv, 125), 0.02, 125, pad=1))
    # an NCHW input (user-made) goes through one layout conversion
    qn = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, c, h, w)).astype(f32)), 0.025, 127)
    assert np.array_equal(g(qn).numpy(), gn.group_norm_u8(qn.numpy(), 4, f32(0.025), f32(1e-5), gam, bet, f32(0.02), 125))


@pytest.mark.parametrize("shape,groups", [((5, 20, 4, 3), 5), ((2, 16, 80, 80), 4)], ids=["direct", "split"])
def test_calibrated_like_a_layer_round_trips_and_replays(i8ie, tmp_path, shape, groups):
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    c = shape[1]
    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, shape).astype(f32)
    w, b = rng.uniform(0.5, 1.5, c).astype(f32), rng.uniform(-0.3, 0.3, c).astype(f32)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.gn1 = i8ie.GroupNorm(groups, c)

        def forward(self, x):
            return self.gn1(x)

    cx.set_calibration_mode("host")
    cx.set_calibration_seed(7)
    try:
        net = Net()
        net.load({"gn1.weight": w, "gn1.bias": b})
        net.prepare()
        got = net(i8ie.tensor(a)).numpy()
        net.convert(per_channel=True)   # (accepted and ignored)
        want = tuple(cx.calibrator_range([got.ravel()], 1.0))
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert (np.abs(got - gn.group_norm_f64(a, groups, w, b, 1e-5)) <= gn.group_norm_f32_bound(a, groups, w, b, 1e-5)).all()
    assert net.gn1.layer.is_quantized() and net.gn1.output_qparams() == want and want[0] != 1.0 and not net.gn1.is_per_channel()
    sd = net.quantized_state_dict()
    assert list(sd) == ["gn1.weight", "gn1.bias", "gn1.qparams"]
    assert sd["gn1.weight"].dtype == np.float32 and np.array_equal(sd["gn1.weight"], w) and np.array_equal(sd["gn1.bias"], b)
    assert sd["gn1.qparams"].tolist() == [0.0, want[0], float(want[1])]
    path = str(tmp_path / "gn.npz")
    net.save_quantized(path)
    other = Net()
    other.load_quantized_file(path)
    assert other.gn1.output_qparams() == want and other.is_quant
    x = rng.normal(0.2, 1.5, shape).astype(f32)
    r1, r2 = net(i8ie.tensor(x)).numpy(), other(i8ie.tensor(x)).numpy()
    qx = orc.quantize(x, sr.pipeline.INPUT_SCALE, sr.pipeline.INPUT_ZP)
    ref = orc.dequantize(gn.group_norm_u8(qx, groups, sr.pipeline.INPUT_SCALE, f32(1e-5), w, b, f32(want[0]), want[1]), f32(want[0]), want[1])
    assert np.array_equal(r1.view(np.uint32), ref.view(np.uint32)) and np.array_equal(r2.view(np.uint32), ref.view(np.uint32))
    # set_output_qparams on a converted layer re-derives g and b
    other.gn1.set_output_qparams(0.05, 99)
    ref2 = orc.dequantize(gn.group_norm_u8(qx, groups, sr.pipeline.INPUT_SCALE, f32(1e-5), w, b, f32(0.05), 99), f32(0.05), 99)
    assert np.array_equal(other(i8ie.tensor(x)).numpy().view(np.uint32), ref2.view(np.uint32))
    g = GraphedForward(net, i8ie.tensor(x).prefetch())   # (the split form takes its workspace inside the capture)
    for _ in range(2):
        assert np.array_equal(g().numpy().view(np.uint32), ref.view(np.uint32))


def test_calibration_on_the_device(i8ie):
    """the device sampler sees the GroupNorm's FP32 result like a layer's: its (scale, zero_point) is close to the host
    sampler's (the two draw different samples; the closeness asked is tests/test_gpu_calibration_device.py's)"""
    import _CXX_i8ie as cx

    rng = np.random.default_rng(5)
    a = rng.normal(0.2, 1.5, (4, 16, 6, 6)).astype(f32)
    got = {}
    for mode in ("host", "device"):
        cx.set_calibration_mode(mode)
        cx.set_calibration_seed(11)
        try:
            g = i8ie.GroupNorm(4, 16)
            g.prepare()
            g(i8ie.tensor(a)).numpy()
            g.convert()
        finally:
            cx.set_calibration_mode("auto")
            cx.set_calibration_seed(-1)
        assert g.layer.is_quantized()
        got[mode] = g.output_qparams()
    (sh, zh), (sd, zd) = got["host"], got["device"]
    assert sh != 1.0 and sd != 1.0 and 0.5 < sd / sh < 2.0 and abs(int(zd) - int(zh)) <= 64, got


# ---- groupnorm_tiny (workloads.py), its expected bytes from tests/spec_ref.py ---------------------------------------------
NAME = "groupnorm_tiny"
GROUPNORMS = ("a_gn1", "a_gn2", "d_gn", "b_gn1", "b_gn2", "s_gn")
TRACED = ("pool",) + GROUPNORMS + ("a_add", "b_add", "s_sig", "s_mul", "s_c", "s_attn", "s_add", "gap", "fc")


def _net(per_channel):
    """nc.calibrated on the device sampler, as tests/test_gpu_mha.py's network"""
    import net_cases as nc

    return nc.calibrated(NAME, per_channel, calib_images=8, mode="device")


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_gn_net_bit_exact(i8ie, batch, per_channel, tmp_path):
    """logits and every traced tensor against spec_ref.forward: eager, tensor by tensor, under force-fallback, replayed as one
    HIP graph, and from a fresh net that loaded what save_quantized() wrote"""
    import net_cases as nc
    from int8inferenceengine_amd import workloads as wl

    net, qlayers, qp, jqp = _net(per_channel)
    both = dict(qp, **jqp)
    assert "s_attn" + sr.mhr.SCORES in jqp and all(s > 0 and s != 1.0 for s, _ in both.values()), both   # everything was calibrated
    x = wl.synthetic_input(NAME, batch, seed=sr.INPUT_SEED)
    trace = {}
    want = sr.forward(wl.network(NAME), x, qlayers, qp, jqp, per_channel, sr.keeps(TRACED, trace))
    assert want.shape == (batch, 10) and len(np.unique(want)) > 1
    for k in GROUPNORMS:   # the expected bytes discriminate
        assert len(np.unique(trace[k])) >= 32 and ((trace[k] == 0) | (trace[k] == 255)).mean() < 0.05, k
    nc.check_bit_exact(i8ie, net, NAME, x, want, fallback=True, graph=True, reload_dir=tmp_path, expect_jqp=both)
    mine = {}
    nc.traced(i8ie, net, NAME, x, sr.keeps(TRACED, mine))
    assert sorted(mine) == sorted(TRACED) == sorted(trace)
    for k in TRACED:   # ("fc": the logits of the walk tensor by tensor)
        assert mine[k].shape == trace[k].shape and np.array_equal(mine[k], trace[k]), k


def test_gn_net_kernels_and_launches(i8ie):
    """the two GroupNorms of 16 channels run in the image form and the four of 20 channels in the direct form, one launch
    each, with the relus behind them folded in (the one relu launch left is c1's NCHW route).  The launches between the
    20-channel layers belong to the existing operand machinery, which tests/test_gpu_operand_rules.py pins."""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd import workloads as wl

    net = _net(False)[0]
    x = wl.synthetic_input(NAME, 5, seed=sr.INPUT_SEED)
    net(i8ie.tensor(x)).numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        net(i8ie.tensor(x)).numpy()
    finally:
        prof = cx.profile_stop()
    launches = support.launch_counts(prof)
    print(launches)
    assert launches.get("groupnorm_u8_image") == 2 and launches.get("groupnorm_u8_direct") == 4, launches
    assert launches.get("relu_u8", 0) <= 1, launches
