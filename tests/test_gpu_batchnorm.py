"""The quantized inference BatchNorm on the GPU (csrc/i8ie_batchnorm.hip).  Expected bytes always come from
the numpy restatement of the definition (tests/batchnorm_ref.py), never from the code under test, and every physical byte is
compared, with guard bytes around the buffers and poisoned result borders that must come back intact: every byte value per
channel through both kernels, values on truncation boundaries, the tiling edges of the walking kernel, the bordered / re-biased
layout matrix, the flat entry, the FP32 entry against float64, and the Python surface (launch counts, calibration, save / load,
graph replay, the fold end to end, a hand-built dense block)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import avgpool_ref as apr
import batchnorm_ref as bn
import concat_ref as ccr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
POISON = 0x3C   # a result border as nobody's zero point leaves it: it must come back intact

ctx = support.ctx_fixture(bn)


def _nhwc(ctx, q, g, b, s_in, zp_in, zp_out, relu=False, ib=0, in_s8=0, ob=0, out_s8=0, fallback=False, expect_rc=0):
    """i8ie_batchnorm_u8_nhwc on q [n, C, h, w]: the input border is garbage, the result border POISON; -> [n, C, h, w]"""
    n, Cn, h, w = q.shape
    rng = np.random.default_rng(Cn + h)
    phys_in = rng.integers(0, 256, (n, h + 2 * ib, w + 2 * ib, Cn), dtype=np.uint8)   # a garbage border: it is never read
    phys_in[:, ib:ib + h, ib:ib + w, :] = q.transpose(0, 2, 3, 1) ^ np.uint8(0x80 if in_s8 else 0)
    phys_out = np.full((n, h + 2 * ob, w + 2 * ob, Cn), POISON, np.uint8)
    di, do = abi.GuardedU8(ctx, phys_in.shape), abi.GuardedU8(ctx, phys_out.shape)
    dg, db = ctx.put(np.ascontiguousarray(g, f32)), ctx.put(np.ascontiguousarray(b, f32))
    for d, host in ((di, phys_in), (do, phys_out)):
        abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, d.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
    ctx.set_force_fallback(fallback)
    try:
        with ctx.launch_map() as names:
            rc = abi.lib().i8ie_batchnorm_u8_nhwc(ctx.h, di.ptr, ib, in_s8, do.ptr, ob, out_s8, n, Cn, h, w, dg.ptr, db.ptr, s_in, zp_in,
                                                  1 if relu else 0, zp_out)
    finally:
        ctx.set_force_fallback(False)
    got = do.get()
    assert do.guards_ok() and di.guards_ok() and np.array_equal(di.get(), phys_in)
    for d in (di, do, dg, db):
        d.free()
    assert rc == expect_rc, abi.lib().i8ie_last_error()
    if rc != 0:
        assert names == {} and (got == POISON).all()
        return None
    assert names == {"batchnorm_u8_direct" if fallback else "batchnorm_u8_nhwc": 1}, names
    ring = got.copy()
    ring[:, ob:ob + h, ob:ob + w, :] = POISON
    assert (ring == POISON).all()   # only the interior was written
    return np.ascontiguousarray((got[:, ob:ob + h, ob:ob + w, :] ^ np.uint8(0x80 if out_s8 else 0)).transpose(0, 3, 1, 2))


# ---- 1. every byte, every channel form, both kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", bn.EXHAUSTIVE_C)
def test_every_byte_per_channel_through_both_kernels(ctx, Cn):
    q = support.byte_image(Cn)
    spread = set()
    for i, (s_in, zp_in, s_out, zp_out, eps, what) in enumerate(bn.PARAM_SETS):
        gamma, beta, mean, var = bn.case_params(Cn, 10 * Cn + i, what)
        g, b = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
        for relu in (False, True):
            want = bn.batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, relu)
            spread |= set(np.unique(want).tolist())
            for fallback in (False, True):
                got = _nhwc(ctx, q, g, b, s_in, zp_in, zp_out, relu, fallback=fallback)
                assert np.array_equal(got, want), (Cn, what, relu, fallback, np.argwhere(got != want)[:4])
    assert len(spread) > 100


def test_values_on_truncation_boundaries(ctx):
    """s_in = 0.5, g = 2 and an integer b: every v is an exact integer, so every byte lies on a truncation boundary; then
    b = integer - 2^-10, just below it"""
    Cn = 20
    q = support.byte_image(Cn)
    rng = np.random.default_rng(3)
    g = np.full(Cn, 2.0, f32)
    g[1::3] = -2.0
    whole = rng.integers(-120, 300, Cn).astype(f32)
    spread = set()
    for b in (whole, (whole - f32(2.0 ** -10)).astype(f32)):
        for zp_in, zp_out, relu in ((100, 90, False), (0, 255, True), (255, 0, True), (17, 130, True)):
            want = bn.bytes_of(q, f32(0.5), zp_in, g, b, zp_out, relu)
            v = bn.batch_norm_v(q, f32(0.5), zp_in, g, b)
            if b is whole:
                assert np.array_equal(v, np.rint(v))
            spread |= set(np.unique(want).tolist())
            for fallback in (False, True):
                got = _nhwc(ctx, q, g, b, f32(0.5), zp_in, zp_out, relu, fallback=fallback)
                assert np.array_equal(got, want), (zp_in, zp_out, relu, fallback, np.argwhere(got != want)[:4])
    assert len(spread) > 200   # (a relu at zp_out = 255 leaves one value; the other cases spread)


# ---- 2. tiling edges ----------------------------------------------------------------------------------------------------------
def _hw(pixels):
    for w in (7, 5, 3, 2):
        if pixels % w == 0:
            return pixels // w, w
    return 1, pixels


def _case(ctx, rng, n, Cn, h, w, qp=bn.PARAM_SETS[0], **kw):
    s_in, zp_in, s_out, zp_out, eps, what = qp
    gamma, beta, mean, var = bn.case_params(Cn, Cn + h, what)
    g, b = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
    q = rng.integers(0, 256, (n, Cn, h, w), dtype=np.uint8)
    want = bn.batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, kw.get("relu", False))
    got = _nhwc(ctx, q, g, b, s_in, zp_in, zp_out, **kw)
    assert np.array_equal(got, want), (n, Cn, h, w, kw, np.argwhere(got != want)[:4])
    return want


@pytest.mark.parametrize("Cn", [16, 20, 3, 4096 + 16])
def test_pixel_run_edges(ctx, Cn):
    """h * w at -1 / 0 / +1 around the pixels a block covers (its rows times the lane's walk) and around twice that, one and
    three images, a bordered result"""
    run = bn.pixel_run(Cn)
    assert run == {16: 2048, 20: 408, 3: 680, 4112: 8}[Cn] and bn.WALK == 8 and bn.item_width(Cn) in bn.ITEM_WIDTHS
    rng = np.random.default_rng(Cn)
    for pixels in sorted({run - 1, run, run + 1, 2 * run - 1, 2 * run, 2 * run + 1}):
        h, w = _hw(pixels)
        for n in (1, 3):
            _case(ctx, rng, n, Cn, h, w, ib=1, ob=1, relu=bool(n == 3))


def test_channel_limits_and_a_grid_that_wraps(ctx):
    rng = np.random.default_rng(8)
    q = rng.integers(0, 256, (1, 16400, 1, 1), dtype=np.uint8)
    assert _nhwc(ctx, q, np.ones(16400, f32), np.ones(16400, f32), f32(0.1), 3, 4, expect_rc=-1) is None   # refused, nothing launched
    for fallback in (False, True):
        _case(ctx, rng, 1, 16384, 1, 1, fallback=fallback)   # 1024 items of one pixel: four channel chunks
    # more (image, channel chunk, pixel tile) units than the grid has blocks: a block takes a second unit
    n = bn.MAX_BLOCKS + 52
    want = _case(ctx, rng, n, 16, 1, 1)
    assert len(np.unique(want)) > 100
    _case(ctx, rng, n, 3, 2, 1, ob=1)


# ---- 3. the layout matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [16, 20])
def test_layout_matrix(ctx, Cn):
    rng = np.random.default_rng(Cn)
    for i, (ib, in_s8, ob, out_s8) in enumerate(itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1))):
        for fallback in (False, True):
            _case(ctx, rng, 2, Cn, 3, 5, bn.PARAM_SETS[i % len(bn.PARAM_SETS)], ib=ib, in_s8=in_s8, ob=ob, out_s8=out_s8, relu=bool(i % 2),
                  fallback=fallback)


def test_nhwc_in_place(ctx):
    Cn, n, h, w = 20, 2, 5, 3
    s_in, zp_in, s_out, zp_out, eps, what = bn.PARAM_SETS[0]
    gamma, beta, mean, var = bn.case_params(Cn, 4, what)
    g, b = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
    q = np.random.default_rng(2).integers(0, 256, (n, Cn, h, w), dtype=np.uint8)
    phys = support.phys_nhwc(q, 1, POISON, False)
    d = abi.GuardedU8(ctx, phys.shape)
    dg, db = ctx.put(g), ctx.put(b)
    abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, d.ptr, phys.ctypes.data_as(C.c_void_p), C.c_size_t(phys.nbytes)))
    abi.ck(abi.lib().i8ie_batchnorm_u8_nhwc(ctx.h, d.ptr, 1, 0, d.ptr, 1, 0, n, Cn, h, w, dg.ptr, db.ptr, s_in, zp_in, 1, zp_out))
    want = support.phys_nhwc(bn.batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, True), 1, POISON, False)
    assert np.array_equal(d.get(), want) and d.guards_ok()
    for x in (d, dg, db):
        x.free()


# ---- 4. the flat entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 20), (3, 20, 4, 5), (2, 17, 3, 3), (300, 1)], ids=str)
def test_flat_entry(ctx, shape):
    """inner = 1 ([m, C] rows) and inner = h * w (an NCHW tensor in one launch), aligned and offset by one byte, in place"""
    Cn = shape[1]
    inner = int(np.prod(shape[2:], dtype=np.int64))
    rows = shape[0] * inner
    s_in, zp_in, s_out, zp_out, eps, what = bn.PARAM_SETS[2]
    gamma, beta, mean, var = bn.case_params(Cn, 6, what)
    g, b = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
    dg, db = ctx.put(g), ctx.put(b)
    q = np.random.default_rng(Cn).integers(0, 256, shape, dtype=np.uint8)
    for relu, offset, in_place in itertools.product((False, True), (0, 1), (False, True)):
        want = bn.batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, relu)
        di = abi.GuardedU8(ctx, (q.size + offset,))
        host = np.concatenate([np.zeros(offset, np.uint8), q.ravel()])
        abi.ck(abi.lib().i8ie_memcpy_h2d(ctx.h, di.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
        do = di if in_place else abi.GuardedU8(ctx, (q.size + offset,))
        with ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_batchnorm_u8(ctx.h, di.ptr.value + offset, do.ptr.value + offset, rows, Cn, inner, dg.ptr, db.ptr, s_in, zp_in,
                                              1 if relu else 0, zp_out))
        raw = do.get()
        assert do.guards_ok() and di.guards_ok() and names == {"batchnorm_u8_direct": 1}, names
        assert (raw[:offset] == (0 if in_place else 0xC3)).all()   # the byte in front of an offset result is untouched
        assert np.array_equal(raw[offset:].reshape(shape), want), (shape, relu, offset, in_place)
        di.free()
        if not in_place:
            do.free()
    dg.free(); db.free()


# ---- 5. FP32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 20, 4, 5), (7, 33), (2, 1, 3, 3)], ids=str)
def test_f32_against_float64(ctx, shape):
    """bound: batchnorm_ref.batch_norm_f32_bound, from the roundings of the fp32 sequence (f64_ref.gamma); the sequence itself
    bit for bit"""
    Cn = shape[1]
    inner = int(np.prod(shape[2:], dtype=np.int64))
    rng = np.random.default_rng(70 + Cn)
    x = rng.normal(0.3, 2.0, shape).astype(f32)
    gamma, beta, mean, var = bn.random_params(rng, Cn)
    var[0] = 0.0
    ds = [ctx.put(v) for v in (gamma, beta, mean, var)]
    di, do = ctx.put(x), ctx.guarded(shape)
    abi.ck(abi.lib().i8ie_batchnorm_f32(ctx.h, di.ptr, do.ptr, shape[0] * inner, Cn, inner, *[d.ptr for d in ds], 1e-5))
    got, ok = do.read()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    err = np.abs(got.astype(f64) - bn.batch_norm_f64(x, gamma, beta, mean, var, 1e-5))
    bound = bn.batch_norm_f32_bound(x, gamma, beta, mean, var, 1e-5)
    print("batchnorm_f32 %s: max err %.3g, max err / bound %.3g" % (shape, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert support.same_bits(got, bn.batch_norm_f32(x, gamma, beta, mean, var, 1e-5))
    for d in ds + [di, do]:
        d.free()


# ---- 6. the Python surface ----------------------------------------------------------------------------------------------------
def _bn_layer(i8ie, c, seed, qp=None, eps=1e-5):
    gamma, beta, mean, var = bn.random_params(np.random.default_rng(seed), c)
    L = i8ie.BatchNorm2d(c, eps)
    L.load_weight(gamma)
    L.load_bias(beta)
    L.load_running_mean(mean)
    L.load_running_var(var)
    if qp is not None:
        L.set_output_qparams(*qp)
        L.convert()
    return L, (gamma, beta, mean, var)


def _ref(q, s_in, zp_in, params, qp, relu=False, eps=1e-5):
    return bn.batch_norm_u8(q, f32(s_in), zp_in, *params, f32(eps), f32(qp[0]), qp[1], relu)


def test_functional_forms_and_shapes(i8ie):
    rng = np.random.default_rng(80)
    gamma, beta, mean, var = params = bn.random_params(rng, 12)
    for shape in ((2, 12, 3, 4), (5, 12)):
        xf = rng.uniform(-3, 3, shape).astype(f32)
        q = i8ie.quantize(i8ie.tensor(xf), 0.025, 127)   # a user-made tensor, in reference order: the flat entry
        qv = q.numpy()
        r = i8ie.relu(i8ie.batch_norm(q, mean, var, gamma, beta, 1e-5, 0.02, 120))
        assert r.shape == shape and r.scale == pytest.approx(0.02) and r.zero_point == 120
        assert np.array_equal(r.numpy(), _ref(qv, 0.025, 127, params, (0.02, 120), True)), shape
        r = i8ie.batch_norm(q, mean, var, scale=0.02, zero_point=120)   # weight, bias default to ones, zeros
        assert np.array_equal(r.numpy(), _ref(qv, 0.025, 127, (np.ones(12, f32), np.zeros(12, f32), mean, var), (0.02, 120)))
        got = i8ie.batch_norm(i8ie.tensor(xf), mean, var, gamma, beta).numpy()
        assert support.same_bits(got, bn.batch_norm_f32(xf, gamma, beta, mean, var, 1e-5))
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (2, 12, 3, 4)).astype(f32)), 0.025, 127)
    B11, _ = _bn_layer(i8ie, 11, 1, (0.02, 1))
    bad = [lambda: i8ie.BatchNorm2d(12)(q),                                   # not converted
           lambda: B11(q),                                                    # c != num_features
           lambda: i8ie.batch_norm(q.reshape(-1), None, None, scale=0.02, zero_point=1),          # rank 1
           lambda: i8ie.batch_norm(q.reshape(2, 12, 12), None, None, scale=0.02, zero_point=1),   # rank 3
           lambda: i8ie.batch_norm(q, mean[:11], var, scale=0.02, zero_point=1),
           lambda: i8ie.batch_norm(q, mean, -var, scale=0.02, zero_point=1),                      # var < 0
           lambda: i8ie.batch_norm(q, mean, var, eps=0.0, scale=0.02, zero_point=1),
           lambda: i8ie.batch_norm(q, mean, var, scale=0.0, zero_point=1),
           lambda: i8ie.batch_norm(q, mean, var, scale=0.02, zero_point=256)]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    for kw in ({}, {"scale": 0.2}, {"zero_point": 3}):
        with pytest.raises(TypeError):
            i8ie.batch_norm(q, mean, var, **kw)


def test_launch_counts_and_bytes(i8ie):
    """conv -> bn -> relu -> conv is three launches (the BatchNorm reads the conv's NHWC result as it lies, takes the relu in and
    writes the border and re-bias the next conv asks for), two with the BatchNorm folded; one BatchNorm feeding two convs is
    three; concat -> bn -> relu -> conv is three; nothing converts a layout, re-biases or fills a border in between"""
    rng = np.random.default_rng(90)
    n, c, h, w = 3, 16, 6, 5   # (16 channels: the convs keep the engine's NHWC layout, as in tests/test_gpu_layernorm.py)
    stem0 = support.conv(i8ie, 3, c, 3, 1, 9, (0.05, 128))
    stem1 = support.conv(i8ie, c, c, 3, 1, 11, (0.05, 128))
    stem = support.conv(i8ie, c, c, 3, 1, 1, (0.05, 120))
    B, params = _bn_layer(i8ie, c, 2, (0.02, 125))
    tail = support.conv(i8ie, c, 16, 3, 1, 5, (0.07, 100))
    proj = [support.conv(i8ie, c, 16, 1, 0, sd, (0.06, 120 + sd)) for sd in (3, 4)]
    q = i8ie.quantize(i8ie.tensor(rng.uniform(-3, 3, (n, 3, h, w)).astype(f32)), 0.025, 127)
    x = i8ie.relu(stem1(i8ie.relu(stem0(q))))

    own, others, launches = support.split_launches(support.counted(lambda: [tail(i8ie.relu(B(stem(x))))]), "batchnorm_u8")
    assert launches.get("batchnorm_u8_nhwc") == 1 and (own, others) == (1, 2), launches
    y = stem(x)
    own, others, launches = support.split_launches(support.counted(lambda: (lambda t: [p(t) for p in proj])(B(y))), "batchnorm_u8")
    assert launches.get("batchnorm_u8_nhwc") == 1 and (own, others) == (1, 2), launches
    # folded: the BatchNorm is the identity, conv -> bn -> relu -> conv stays two launches
    folded_conv = i8ie.Conv2d(c, c, 3, padding=1)
    wr = np.random.default_rng(1)
    wf, bf = (wr.uniform(-1, 1, (c, c, 3, 3)) * np.sqrt(6.0 / (c * 9))).astype(f32), wr.uniform(-0.1, 0.1, c).astype(f32)
    folded_conv.load_weight(wf)
    folded_conv.load_bias(bf)
    Bf, pf = _bn_layer(i8ie, c, 2)
    i8ie.fold_batchnorm(folded_conv, Bf)
    folded_conv.set_output_qparams(0.05, 120)
    folded_conv.convert()
    own, others, launches = support.split_launches(support.counted(lambda: [tail(i8ie.relu(Bf(folded_conv(x))))]), "batchnorm_u8")
    assert (own, others) == (0, 2), launches
    # concat -> bn -> relu -> conv
    cat = i8ie.Concat()
    cat.set_output_qparams(0.05, 124)
    cat.convert()
    B32, p32 = _bn_layer(i8ie, 2 * c, 6, (0.03, 110))
    tail32 = support.conv(i8ie, 2 * c, 16, 3, 1, 7, (0.07, 100))
    x2 = i8ie.relu(stem(x))
    own, others, launches = support.split_launches(support.counted(lambda: [tail32(i8ie.relu(B32(cat([x, x2]))))]), "batchnorm_u8")
    assert launches.get("batchnorm_u8_nhwc") == 1 and (own, others) == (1, 2), launches
    # the bytes
    xv = x.numpy()
    yv = support.conv_ref(stem, xv, 0.05, 128, pad=1)
    bv = _ref(yv, 0.05, 120, params, (0.02, 125))
    assert len(np.unique(bv)) > 40 and np.array_equal(B(stem(x)).numpy(), bv)
    assert np.array_equal(tail(i8ie.relu(B(stem(x)))).numpy(), support.conv_ref(tail, np.maximum(bv, 125), 0.02, 125, pad=1))
    t = B(y)
    for p in proj:
        assert np.array_equal(p(t).numpy(), support.conv_ref(p, bv, 0.02, 125))
    cv = ccr.cat_u8([(xv, f32(0.05), 128), (np.maximum(yv, 120), f32(0.05), 120)], f32(0.05), 124)
    b32 = _ref(cv, 0.05, 124, p32, (0.03, 110), True)
    assert np.array_equal(tail32(i8ie.relu(B32(cat([x, x2])))).numpy(), support.conv_ref(tail32, b32, 0.03, 110, pad=1))


def test_calibration_on_the_device(i8ie):
    """prepare() / convert() with the device sampler: it sees the BatchNorm's FP32 result like a layer's, and the sampled output
    fixes (s_out, zp_out) close to the host sampler's (the two draw different samples; the closeness asked is
    tests/test_gpu_groupnorm.py's); the converted layer then gives the restatement's bytes for the parameters it took"""
    import _CXX_i8ie as cx

    rng = np.random.default_rng(5)
    a = rng.normal(0.2, 1.5, (4, 16, 6, 6)).astype(f32)
    got = {}
    for mode in ("host", "device"):
        cx.set_calibration_mode(mode)
        cx.set_calibration_seed(11)
        try:
            B, params = _bn_layer(i8ie, 16, 4)
            B.prepare()
            assert B.layer._is_preparing()
            B(i8ie.tensor(a)).numpy()
            B.convert()
        finally:
            cx.set_calibration_mode("auto")
            cx.set_calibration_seed(-1)
        assert B.layer.is_quantized() and not B.layer._is_preparing()
        got[mode] = B.output_qparams()
    (sh, zh), (sd, zd) = got["host"], got["device"]
    assert sh != 1.0 and sd != 1.0 and 0.5 < sd / sh < 2.0 and abs(int(zd) - int(zh)) <= 64, got
    q = i8ie.quantize(i8ie.tensor(a), 0.025, 127)
    assert np.array_equal(B(q).numpy(), _ref(q.numpy(), 0.025, 127, params, (sd, zd)))


def test_calibrated_like_a_layer_round_trips_and_replays(i8ie, tmp_path):
    import _CXX_i8ie as cx
    import orc
    import spec_ref as sr
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(8)
    a = rng.normal(0.2, 1.5, (5, 20, 4, 3)).astype(f32)
    gamma, beta, mean, var = params = bn.random_params(rng, 20)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.bn1 = i8ie.BatchNorm2d(20)

        def forward(self, x):
            return self.bn1(x)

    cx.set_calibration_mode("host")
    cx.set_calibration_seed(7)
    try:
        net = Net()
        net.load({"bn1.weight": gamma, "bn1.bias": beta, "bn1.running_mean": mean, "bn1.running_var": var, "bn1.num_batches_tracked": 3})
        net.prepare()
        got = net(i8ie.tensor(a)).numpy()
        net.convert()
        want = tuple(cx.calibrator_range([got.ravel()], 1.0))
    finally:
        cx.set_calibration_mode("auto")
        cx.set_calibration_seed(-1)
    assert support.same_bits(got, bn.batch_norm_f32(a, gamma, beta, mean, var, 1e-5))
    assert net.bn1.layer.is_quantized() and net.bn1.output_qparams() == want and want[0] != 1.0
    sd = net.quantized_state_dict()
    assert list(sd) == ["bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.qparams"]
    assert all(sd["bn1." + k].dtype == np.float32 for k in ("weight", "bias", "running_mean", "running_var"))
    assert np.array_equal(sd["bn1.running_var"], var) and sd["bn1.qparams"].tolist() == [0.0, want[0], float(want[1])]
    path = str(tmp_path / "bn.npz")
    net.save_quantized(path)
    other = Net()
    other.load_quantized_file(path)
    assert other.bn1.output_qparams() == want and other.is_quant and not other.bn1.is_folded()
    x = rng.normal(0.2, 1.5, (5, 20, 4, 3)).astype(f32)
    r1, r2 = net(i8ie.tensor(x)).numpy(), other(i8ie.tensor(x)).numpy()
    qx = orc.quantize(x, sr.pipeline.INPUT_SCALE, sr.pipeline.INPUT_ZP)
    ref = orc.dequantize(_ref(qx, sr.pipeline.INPUT_SCALE, sr.pipeline.INPUT_ZP, params, want), f32(want[0]), want[1])
    assert support.same_bits(r1, ref) and support.same_bits(r2, ref)
    other.load_quantized_file(path)   # a state that carries the BatchNorm clears a folded mark
    other.bn1._folded = True
    other.load_quantized_file(path)
    assert not other.bn1.is_folded() and support.same_bits(other(i8ie.tensor(x)).numpy(), ref)
    other.bn1.set_output_qparams(0.05, 99)   # on a converted layer: g and b are made again
    ref2 = orc.dequantize(_ref(qx, sr.pipeline.INPUT_SCALE, sr.pipeline.INPUT_ZP, params, (0.05, 99)), f32(0.05), 99)
    assert support.same_bits(other(i8ie.tensor(x)).numpy(), ref2)
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert support.same_bits(g().numpy(), ref)


# ---- 7. the fold, end to end ------------------------------------------------------------------------------------------------------
def _fold_net(i8ie, with_bn):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.c1 = i8ie.Conv2d(3, 16, 3, padding=1)
            self.c2 = i8ie.Conv2d(16, 20, 1)
            self.fc = i8ie.Linear(20, 10)
            if with_bn:
                self.bn1, self.bn2, self.bn3 = i8ie.BatchNorm2d(16), i8ie.BatchNorm2d(20), i8ie.BatchNorm2d(10)

        def forward(self, x):
            bn1, bn2, bn3 = (self.bn1, self.bn2, self.bn3) if with_bn else (lambda t: t,) * 3
            x = i8ie.relu(bn1(self.c1(x)))
            x = i8ie.relu(bn2(self.c2(x)))
            return bn3(self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 20)))

    return Net()


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
def test_fold_end_to_end(i8ie, per_channel, tmp_path):
    """every BatchNorm folded (the last one a BatchNorm1d on [n, c] rows behind the Linear): bit for bit the same net built
    without BatchNorms and loaded with the restatement's pre-folded weights, under the same explicit output qparams"""
    rng = np.random.default_rng(31)
    shapes = {"c1": (16, 3, 3, 3), "c2": (20, 16, 1, 1), "fc": (10, 20)}
    sd, folded = {}, {}
    for i, (name, bname) in enumerate((("c1", "bn1"), ("c2", "bn2"), ("fc", "bn3"))):
        shp = shapes[name]
        w = (rng.uniform(-1, 1, shp) * np.sqrt(6.0 / np.prod(shp[1:]))).astype(f32)
        b = rng.uniform(-0.1, 0.1, shp[0]).astype(f32)
        gamma, beta, mean, var = bn.random_params(rng, shp[0])
        sd.update({name + ".weight": w, name + ".bias": b, bname + ".weight": gamma, bname + ".bias": beta, bname + ".running_mean": mean,
                   bname + ".running_var": var, bname + ".num_batches_tracked": 5})
        folded[name + ".weight"], folded[name + ".bias"] = bn.fold(w, b, gamma, beta, mean, var, 1e-5)
    qps = {"c1": (0.04, 120), "c2": (0.03, 110), "fc": (0.05, 128)}
    nets = []
    for with_bn in (True, False):
        net = _fold_net(i8ie, with_bn)
        net.load(sd if with_bn else folded)
        if with_bn:
            net.fold_batchnorm([("c1", "bn1"), ("c2", "bn2"), ("fc", "bn3")])
        for k, qp in qps.items():
            getattr(net, k).set_output_qparams(*qp)
        net.convert(per_channel)
        nets.append(net)
    x = rng.uniform(-3, 3, (4, 3, 8, 8)).astype(f32)
    a, b = nets[0](i8ie.tensor(x)).numpy(), nets[1](i8ie.tensor(x)).numpy()
    assert a.shape == (4, 10) and len(np.unique(a)) > 10 and support.same_bits(a, b)
    launches = support.counted(lambda: [nets[0](i8ie.tensor(x))])   # (a 3-channel stem: layout conversions are legitimate here)
    assert launches and not [k for k in launches if k.startswith("batchnorm")], launches
    # a folded model saves no BatchNorm key, and a fresh model that loads the file marks its BatchNorms folded
    keys = list(nets[0].quantized_state_dict())
    assert not [k for k in keys if k.startswith("bn")] and sorted(keys) == sorted(nets[1].quantized_state_dict())
    path = str(tmp_path / "folded.npz")
    nets[0].save_quantized(path)
    fresh = _fold_net(i8ie, True)
    fresh.load_quantized_file(path)
    assert fresh.bn1.is_folded() and fresh.bn2.is_folded() and fresh.bn3.is_folded()
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), a)


# ---- 8. a hand-built dense block ----------------------------------------------------------------------------------------------------
def test_dense_block_step_by_step(i8ie):
    """two DenseNet layers and a transition at 12 -> 20 -> 28 channels on 8 x 8: concat -> bn -> relu -> 1x1 -> bn (folded) ->
    relu -> 3x3 -> concat -> ... -> bn -> relu -> 1x1 -> avg_pool2d, every intermediate tensor against the numpy composition of
    the restatements; eager, under force-fallback and as a replayed graph"""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(17)

    def folded_conv(cin, cout, k, pad, seed, qp):
        r = np.random.default_rng(seed)
        L = i8ie.Conv2d(cin, cout, k, padding=pad)
        L.load_weight((r.uniform(-1, 1, (cout, cin, k, k)) * np.sqrt(6.0 / (cin * k * k))).astype(f32))
        L.load_bias(r.uniform(-0.1, 0.1, cout).astype(f32))
        B, _ = _bn_layer(i8ie, cout, seed + 100)
        i8ie.fold_batchnorm(L, B)
        L.set_output_qparams(*qp)
        L.convert()
        return L, B

    def concat(qp):
        L = i8ie.Concat()
        L.set_output_qparams(*qp)
        L.convert()
        return L

    sa, sb = support.conv(i8ie, 3, 8, 3, 1, 1, (0.05, 128)), support.conv(i8ie, 3, 4, 3, 1, 2, (0.04, 120))
    cats = [concat((0.05, 126)), concat((0.05, 125)), concat((0.05, 124))]
    bns = [_bn_layer(i8ie, c, 20 + c, (0.03, 100 + c)) for c in (12, 20, 28)]
    bott = [folded_conv(12, 16, 1, 0, 3, (0.04, 118)), folded_conv(20, 16, 1, 0, 4, (0.04, 119))]
    grow = [support.conv(i8ie, 16, 8, 3, 1, 5, (0.05, 121)), support.conv(i8ie, 16, 8, 3, 1, 6, (0.05, 122))]
    trans = support.conv(i8ie, 28, 14, 1, 0, 7, (0.06, 123))
    x = rng.uniform(-3, 3, (2, 3, 8, 8)).astype(f32)

    def forward(xt, keep=None):
        keep = {} if keep is None else keep
        q = i8ie.quantize(xt, 0.025, 127)
        keep["a"], keep["b"] = i8ie.relu(sa(q)), i8ie.relu(sb(q))
        t = keep["cat0"] = cats[0]([keep["a"], keep["b"]])
        for i in range(2):
            u = keep["bn%d" % i] = i8ie.relu(bns[i][0](t))
            u = keep["bott%d" % i] = i8ie.relu(bott[i][1](bott[i][0](u)))
            u = keep["grow%d" % i] = grow[i](u)
            t = keep["cat%d" % (i + 1)] = cats[i + 1]([t, u])
        u = keep["bn2"] = i8ie.relu(bns[2][0](t))
        u = keep["trans"] = trans(u)
        keep["out"] = i8ie.avg_pool2d(u, 2)
        return keep["out"]

    import orc
    qx = orc.quantize(x, f32(0.025), 127)
    want = {}
    want["a"] = np.maximum(support.conv_ref(sa, qx, 0.025, 127, pad=1), 128)
    want["b"] = np.maximum(support.conv_ref(sb, qx, 0.025, 127, pad=1), 120)
    t, tqp = ccr.cat_u8([(want["a"], f32(0.05), 128), (want["b"], f32(0.04), 120)], f32(0.05), 126), (0.05, 126)
    want["cat0"] = t
    for i in range(2):
        qp = bns[i][0].output_qparams()
        u = want["bn%d" % i] = _ref(t, tqp[0], tqp[1], bns[i][1], qp, True)
        bqp = bott[i][0].output_qparams()
        u = want["bott%d" % i] = np.maximum(support.conv_ref(bott[i][0], u, qp[0], qp[1]), bqp[1])
        gqp = grow[i].output_qparams()
        u = want["grow%d" % i] = support.conv_ref(grow[i], u, bqp[0], bqp[1], pad=1)
        nqp = cats[i + 1].output_qparams()
        t = want["cat%d" % (i + 1)] = ccr.cat_u8([(t, f32(tqp[0]), tqp[1]), (u, f32(gqp[0]), gqp[1])], f32(nqp[0]), nqp[1])
        tqp = nqp
    qp = bns[2][0].output_qparams()
    u = want["bn2"] = _ref(t, tqp[0], tqp[1], bns[2][1], qp, True)
    u = want["trans"] = support.conv_ref(trans, u, qp[0], qp[1])
    want["out"] = apr.avg_pool2d_u8(u, 2, 2, 2)
    assert want["out"].shape == (2, 14, 4, 4) and all(len(np.unique(want[k])) > 30 for k in ("bn0", "bn1", "bn2", "out"))

    def check(tag):
        keep = {}
        forward(i8ie.tensor(x), keep)
        for k, v in want.items():
            got = keep[k].numpy()
            assert got.shape == v.shape and np.array_equal(got, v), (tag, k, np.argwhere(got != v)[:4])

    check("eager")
    assert np.array_equal(forward(i8ie.tensor(x)).numpy(), want["out"])   # nothing observed on the way: the deferred path
    cx.force_fallback(True)
    try:
        check("force_fallback")
    finally:
        cx.force_fallback(False)
    g = GraphedForward(forward, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy(), want["out"])
