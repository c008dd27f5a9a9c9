"""Quantized upsampling on the GPU (csrc/i8ie_upsample.hip).  Every comparison is against the numpy
restatement of the definition (tests/upsample_ref.py), never against the code under test: every rounding case through both
u8 entries, the edges where the clamps act, the bordered / re-biased layout matrix with guard bands and sentinel borders, a
shape that wraps the grid, the FP32 entry, the Python surface with launch counts, and the two networks end to end."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import abi
import f64_ref
import grouped_ref as gr
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import net_cases as nc
import pointwise_util as pu
import spec_ref as sr
import support
from support import i8ie  # noqa: F401
import upsample_ref as ur

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = [ur.NEAREST, ur.BILINEAR]
MODE_NAME = {ur.NEAREST: "nearest", ur.BILINEAR: "bilinear"}
KERNEL = {ur.NEAREST: "upsample_nearest_u8_nhwc", ur.BILINEAR: "upsample_bilinear_u8_nhwc"}


ctx = support.ctx_fixture(ur)


def _assert_same(got, want, tag):
    """bit equality, with the first few places that differ in the message"""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, "%d of %d differ" % (len(bad), want.size),
                           [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
    return True


def _nchw(ctx, q, fh, fw, mode):
    n, c, h, w = q.shape
    di, do = ctx.put(q), abi.GuardedU8(ctx, (n, c, h * fh, w * fw), fill=0xEE)
    try:
        abi.ck(abi.lib().i8ie_upsample2d_u8(ctx.h, di.ptr, do.ptr, n, c, h, w, fh, fw, mode))
        got = do.get()
        assert do.guards_ok(), "a byte outside the NCHW result was written"
        return got
    finally:
        di.free()
        do.free()


def _nhwc(ctx, q, fh, fw, mode, relu=False, zp=0, ib=0, ob=0, in_s8=0, out_s8=0, in_fill=0xC7, out_fill=0x3C):
    """q NCHW logical -> the NHWC entry's result, NCHW logical again.  The input's border holds in_fill (not the zero point, not
    the edge pixel: a kernel that read it would blend it in); the output's border holds out_fill and, like the guard bytes
    around both buffers, must come back untouched (pointwise_util.interior asserts it)."""
    n, c, h, w = q.shape
    x = np.ascontiguousarray(q.transpose(0, 2, 3, 1))
    fi, _ = pu.phys(x, ib, in_fill, in_s8)
    fo, oshape = pu.phys(np.full((n, h * fh, w * fw, c), 0xEE, np.uint8), ob, out_fill, out_s8)
    di, do = ctx.put(fi), ctx.put(fo)
    try:
        abi.ck(abi.lib().i8ie_upsample2d_u8_nhwc(ctx.h, C.c_void_p(di.ptr.value + pu.GUARD), ib, in_s8, C.c_void_p(do.ptr.value + pu.GUARD),
                                                 ob, out_s8, n, c, h, w, fh, fw, mode, 1 if relu else 0, zp))
        gi, go = di.get(), do.get()
    finally:
        di.free()
        do.free()
    assert np.array_equal(gi, fi), "the input (and its guards) must be untouched"
    return np.ascontiguousarray(pu.interior(go, oshape, ob, out_fill, out_s8).transpose(0, 3, 1, 2))


# ---- 1. every rounding case --------------------------------------------------------------------------------------------
def _rounding_data():
    """random bytes [2, 16, 5, 5] (seed 0), all 0, all 255 and a 0 / 255 checkerboard, one image each behind the two random ones"""
    rnd = np.random.default_rng(0).integers(0, 256, (2, 16, 5, 5), dtype=np.uint8)
    cb = np.zeros((1, 16, 5, 5), np.uint8)
    cb[:, :, 0::2, 1::2] = 255
    cb[:, :, 1::2, 0::2] = 255
    return np.concatenate([rnd, np.zeros((1, 16, 5, 5), np.uint8), np.full((1, 16, 5, 5), 255, np.uint8), cb])


def _reachable_residues(fh, fw):
    """the residues S mod D any bytes can reach: at one output position S is an integer combination of its four weight
    products with coefficients 0 ... 255, i.e. (255 >= D / g - 1) every multiple of g = gcd(products, D); the union over the
    positions of an axis of length 3, which has every (w0, w1) pair of the rule"""
    D = 4 * fh * fw
    _, _, wy0, wy1 = ur.taps(3, fh)
    _, _, wx0, wx1 = ur.taps(3, fw)
    out = set()
    for a0, a1 in zip(wy0, wy1):
        for b0, b1 in zip(wx0, wx1):
            g = D
            for p in (a0 * b0, a1 * b0, a0 * b1, a1 * b1):
                g = math.gcd(g, int(p))
            out |= set(range(0, D, g))
    return out


ROUNDING = [(1, 1), (2, 2), (3, 3), (4, 4), (8, 8), (2, 3), (3, 2)]


def test_reachable_residue_counts():
    assert len(_reachable_residues(2, 2)) == 16 and len(_reachable_residues(4, 4)) == 64 and len(_reachable_residues(8, 8)) == 256
    assert _reachable_residues(3, 3) == set(range(0, 36, 4))


@pytest.mark.parametrize("fh,fw", ROUNDING, ids=["%dx%d" % f for f in ROUNDING])
def test_every_rounding_case(ctx, fh, fw):
    """the restatement's own data reaches every reachable residue S mod D (ties, S mod D == D / 2, among them wherever they are
    reachable); both u8 entries give the restatement's bytes on it, in both modes"""
    q = _rounding_data()
    S, D = ur.bilinear_sd(q, fh, fw)
    reached, reachable = set(np.unique(S % D).tolist()), _reachable_residues(fh, fw)
    print("%dx%d: D = %d, %d of %d reachable residues, ties %s" % (fh, fw, D, len(reached), len(reachable), D // 2 in reached))
    assert reached == reachable
    assert (D // 2 in reached) == (D // 2 in reachable)
    for mode in MODES:
        want = ur.upsample_u8(q, fh, fw, mode)
        assert _assert_same(_nchw(ctx, q, fh, fw, mode), want, (fh, fw, mode, "nchw"))
        assert _assert_same(_nhwc(ctx, q, fh, fw, mode), want, (fh, fw, mode, "nhwc"))
        for zp in (0, 128, 255):
            assert _assert_same(_nhwc(ctx, q, fh, fw, mode, True, zp), ur.upsample_u8(q, fh, fw, mode, True, zp), (fh, fw, mode, zp))


# ---- 2. edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 20, 16, 48])
def test_edges(ctx, c):
    """h, w in {1, 2, 3} in every combination (at 1 both clamps of an axis act at once), one image and three, every item width"""
    rng = np.random.default_rng(c)
    for n, h, w in itertools.product((1, 3), (1, 2, 3), (1, 2, 3)):
        q = rng.integers(0, 256, (n, c, h, w), dtype=np.uint8)
        for (fh, fw), mode in itertools.product([(2, 2), (3, 4), (8, 1)], MODES):
            want = ur.upsample_u8(q, fh, fw, mode)
            assert _assert_same(_nhwc(ctx, q, fh, fw, mode, ib=1, ob=1), want, (n, c, h, w, fh, fw, mode, "nhwc"))
            assert _assert_same(_nchw(ctx, q, fh, fw, mode), want, (n, c, h, w, fh, fw, mode, "nchw"))


# ---- 3. the layout matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 20, 16, 48])
def test_layout_matrix(ctx, c):
    rng = np.random.default_rng(100 + c)
    q = rng.integers(0, 256, (2, c, 3, 4), dtype=np.uint8)
    q[0, :, 0, :], q[1, :, :, 0] = 255, 0
    for fh, fw in [(2, 2), (2, 3)]:
        for mode in MODES:
            for relu, zp in [(False, 0), (True, 0), (True, 128), (True, 255)]:
                want = ur.upsample_u8(q, fh, fw, mode, relu, zp)
                for ib, ob, in_s8, out_s8 in itertools.product((0, 1, 2), (0, 1, 2), (0, 1), (0, 1)):
                    got = _nhwc(ctx, q, fh, fw, mode, relu, zp, ib, ob, in_s8, out_s8)
                    assert _assert_same(got, want, (c, fh, fw, mode, relu, zp, ib, ob, in_s8, out_s8))


# ---- 4. a grid that wraps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 20, 33, 17), (3, 20, 191, 187)], ids=["3x20x33x17", "3x20x191x187"])
def test_many_blocks(ctx, shape):
    """[3, 20, 191, 187]: 535 755 four-channel items, more than the 2048 x 256 lanes of the largest grid, so the grid-stride
    loop goes round; both shapes have sizes that are no multiple of anything"""
    q = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
    if shape[2] == 191:
        assert shape[0] * shape[2] * shape[3] * (shape[1] // 4) > 2048 * 256
    for mode in MODES:
        want = ur.upsample_u8(q, 2, 2, mode, True, 100)
        assert _assert_same(_nhwc(ctx, q, 2, 2, mode, True, 100, ib=1, ob=1, out_s8=1), want, (mode, "nhwc"))
        assert _assert_same(_nchw(ctx, q, 2, 2, mode), ur.upsample_u8(q, 2, 2, mode), (mode, "nchw"))


# ---- 5. FP32 -----------------------------------------------------------------------------------------------------------
def _f32(ctx, x, fh, fw, mode):
    n, c, h, w = x.shape
    di, do = ctx.put(x), ctx.guarded((n, c, h * fh, w * fw))
    try:
        abi.ck(abi.lib().i8ie_upsample2d_f32(ctx.h, di.ptr, do.ptr, n, c, h, w, fh, fw, mode))
        got, ok = do.read()
    finally:
        di.free()
        do.free()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    return got


@pytest.mark.parametrize("fh,fw", [(1, 1), (2, 2), (3, 3), (4, 4), (8, 8), (2, 3), (3, 2)])
def test_fp32(ctx, fh, fw):
    """nearest copies bits.  Bilinear against S / D in float64 within 16 * 2^-24 * max|window|: each axis weight carries 2
    roundings (the division and 1 - l), each blend 3 more (2 products and an add), so a row blend is off by at most
    5 * 2^-24 M and the column blend of two of them by at most 10 * 2^-24 M; 16 leaves slack.  It is also the FP32 sequence
    of include/i8ie_hip.h bit for bit."""
    rng = np.random.default_rng(10 * fh + fw)
    x = (rng.standard_normal((2, 5, 3, 4)) * np.exp(rng.uniform(-3, 3, (2, 5, 3, 4)))).astype(f32)
    near = _f32(ctx, x, fh, fw, ur.NEAREST)
    assert np.array_equal(near.view(np.uint32), ur.nearest(x, fh, fw).view(np.uint32))
    got = _f32(ctx, x, fh, fw, ur.BILINEAR)
    val, mag = ur.bilinear_f64(x, fh, fw)
    err, bound = np.abs(got.astype(np.float64) - val), 16 * 2.0 ** -24 * mag
    print("fp32 %dx%d: worst err / bound = %.3g" % (fh, fw, float((err / bound).max())))
    assert got.dtype == f32 and np.all(err <= bound)
    assert np.array_equal(got.view(np.uint32), ur.upsample_f32(x, fh, fw, ur.BILINEAR).view(np.uint32))


# ---- 6. argument errors of the C entries ---------------------------------------------------------------------------------
def test_c_entry_argument_errors(ctx):
    lib = abi.lib()
    buf = ctx.put(np.zeros(4096, np.uint8))
    try:
        p, h = buf.ptr, ctx.h
        bad = [lib.i8ie_upsample2d_u8(h, None, p, 1, 4, 2, 2, 2, 2, 0), lib.i8ie_upsample2d_u8(h, p, None, 1, 4, 2, 2, 2, 2, 0),
               lib.i8ie_upsample2d_u8(h, p, p, 0, 4, 2, 2, 2, 2, 0), lib.i8ie_upsample2d_u8(h, p, p, 1, 4, 2, 2, 0, 2, 0),
               lib.i8ie_upsample2d_u8(h, p, p, 1, 4, 2, 2, 2, 9, 1), lib.i8ie_upsample2d_u8(h, p, p, 1, 4, 2, 2, 2, 2, 2),
               lib.i8ie_upsample2d_f32(h, p, p, 1, 4, 2, -1, 2, 2, 0), lib.i8ie_upsample2d_f32(h, p, p, 1, 4, 2, 2, 2, 2, -1),
               lib.i8ie_upsample2d_f32(h, p, p, 1, 4, 2, 2, 9, 2, 1),
               lib.i8ie_upsample2d_u8_nhwc(h, p, -1, 0, p, 0, 0, 1, 4, 2, 2, 2, 2, 0, 0, 0),
               lib.i8ie_upsample2d_u8_nhwc(h, p, 0, 0, p, -1, 0, 1, 4, 2, 2, 2, 2, 0, 0, 0),
               lib.i8ie_upsample2d_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 2, 2, 3, 0, 0),
               lib.i8ie_upsample2d_u8_nhwc(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 0, 2, 1, 0, 0),
               lib.i8ie_upsample2d_u8_nhwc(h, p, 0, 0, None, 0, 0, 1, 4, 2, 2, 2, 2, 1, 0, 0)]
        assert bad == [-1] * len(bad), bad
        assert (buf.get() == 0).all()
    finally:
        buf.free()


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------
FOREIGN = ("relu_u8", "rebias", "fill_border", "reborder", "layout_", "upsample_u8_nchw")


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_conv_upsample_relu_conv_is_three_launches(i8ie, mode):
    """conv -> upsample -> relu -> conv(3x3 pad 1): one launch each; the relu folds into the upsample, whose kernel writes the
    border and the bytes the second conv asks for"""
    q = support.activation(i8ie)
    conv0, conv_c = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120))
    first, got, launches = support.counted_forward(lambda: conv_c(i8ie.relu(i8ie.upsample(conv0(q), 2, mode))))
    mid = i8ie.relu(i8ie.upsample(conv0(q), 2, mode))
    assert mid.shape == (2, 16, 16, 16) and mid.scale == pytest.approx(0.04) and mid.zero_point == 110
    assert np.array_equal(mid.numpy(), ur.upsample_u8(conv0(q).numpy(), 2, 2, mode, True, 110))
    assert got.shape == (2, 16, 16, 16) and np.array_equal(got, conv_c(mid).numpy()) and np.array_equal(first, got)
    assert launches.get(KERNEL[ur.MODES[mode]], 0) == 1 and sum(launches.values()) == 3, launches
    for k in launches:
        assert not k.startswith(FOREIGN), launches
    assert q.data.layout() == 1  # NHWC


def test_upsample_into_add_with_bordered_skip(i8ie):
    """the step of a feature pyramid: x = relu(conv0(..)) is made bordered for the stride-2 conv below it and read by the Add
    as it lies; upsample and add are one launch each; nothing converts, re-biases or fills"""
    import add_ref as ar

    q = support.activation(i8ie, 16)
    conv0, conv_d = support.conv(i8ie, 16, 16, 3, 1, 1, (0.04, 110)), support.conv(i8ie, 16, 16, 3, 1, 2, (0.05, 120), stride=2)
    add = i8ie.Add()
    add.set_output_qparams(0.07, 100)
    add.convert()

    def forward():
        x = i8ie.relu(conv0(q))
        return i8ie.relu(add(i8ie.upsample(i8ie.relu(conv_d(x)), 2, "nearest"), x))

    first, got, launches = support.counted_forward(forward)
    xv = i8ie.relu(conv0(q)).numpy()
    dv = i8ie.relu(conv_d(i8ie.relu(conv0(q)))).numpy()
    want = ar.add_u8(ur.upsample_u8(dv, 2, 2, "nearest"), 120, f32(0.05), xv, 110, f32(0.04), f32(0.07), 100, True)
    assert got.shape == (2, 16, 16, 16) and np.array_equal(got, want) and np.array_equal(first, want)
    assert launches.get("upsample_nearest_u8_nhwc", 0) == 1, launches
    assert sum(v for k, v in launches.items() if k.startswith("add_u8")) == 1, launches
    assert sum(launches.values()) == 4, launches  # conv0, conv_d, the upsample, the add
    for k in launches:
        assert not k.startswith(FOREIGN), launches


def test_surface_user_tensor_qparams_and_errors(i8ie):
    rng = np.random.default_rng(12)
    x = rng.uniform(-3, 3, (2, 5, 3, 4)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), 0.025, 127)  # a user-made tensor: NCHW bytes
    qv = q.numpy()
    for factor, mode in [(2, "nearest"), (2, "bilinear"), ((2, 3), "bilinear"), ((3, 1), "nearest"), (8, "bilinear")]:
        fh, fw = ur.factors(factor)
        r = i8ie.upsample(q, factor, mode)
        assert r.shape == (2, 5, 3 * fh, 4 * fw) and r.scale == pytest.approx(0.025) and r.zero_point == 127
        assert np.array_equal(r.numpy(), ur.upsample_u8(qv, fh, fw, mode)), (factor, mode)
        r = i8ie.relu(i8ie.upsample(q, factor, mode))
        assert np.array_equal(r.numpy(), ur.upsample_u8(qv, fh, fw, mode, True, 127)), (factor, mode)
    assert np.array_equal(i8ie.upsample(q, 2).numpy(), ur.upsample_u8(qv, 2, 2, "nearest"))  # the default mode
    t = i8ie.tensor(x)
    assert np.array_equal(i8ie.upsample(t, (2, 3)).numpy().view(np.uint32), ur.nearest(x, 2, 3).view(np.uint32))
    assert np.array_equal(i8ie.upsample(t, (2, 3), "bilinear").numpy().view(np.uint32), ur.upsample_f32(x, 2, 3, "bilinear").view(np.uint32))
    for bad in (lambda: i8ie.upsample(q, 0), lambda: i8ie.upsample(q, 9, "bilinear"), lambda: i8ie.upsample(q, (2, -1)),
                lambda: i8ie.upsample(q, 2, "bicubic"), lambda: i8ie.upsample(q.reshape(2, -1), 2)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(TypeError):
        i8ie.upsample(q, 1.5)


# ---- 8. the networks ---------------------------------------------------------------------------------------------------
_WANT = {}


def _want(name, batch, per_channel):
    from int8inferenceengine_amd import workloads as wl

    if (name, batch, per_channel) not in _WANT:
        net, qlayers, qp, jqp = nc.calibrated(name, per_channel, calib_images=8)
        x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
        trace = []
        want = sr.forward(wl.NETWORKS[name], x, qlayers, qp, jqp, per_channel, ur.tracer(trace))
        _WANT[(name, batch, per_channel)] = (x, want, trace)
    return _WANT[(name, batch, per_channel)]


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [2, 9])
@pytest.mark.parametrize("name", ["upsample_tiny", "unet_bilinear_cifar"])
def test_networks_bit_exact(i8ie, name, batch, per_channel):
    net = nc.calibrated(name, per_channel, calib_images=8)[0]
    x, want, trace = _want(name, batch, per_channel)
    assert len(trace) == (5 if name == "upsample_tiny" else 3)
    print([(op[1:], len(np.unique(q))) for op, q in trace])
    assert all(len(np.unique(q)) > 30 for _, q in trace)  # (the upsampled tensors are not saturated)
    assert want.shape == ((batch, 10, 32, 48) if name == "upsample_tiny" else (batch, 10, 32, 32))
    # (upsample_tiny also captured and replayed as one HIP graph)
    nc.check_bit_exact(i8ie, net, name, x, want, graph=name == "upsample_tiny")


def test_fp32_upsample_tiny_layer_by_layer(i8ie):
    """Before convert(): walk the spec by hand with the FP32 ops, every op fed the product's own previous output -- convs
    inside f64_ref.dot_bound of the float64 result, the upsamples as test_fp32 has them, relu / pool / add / concat
    bit-identical; then net(x) in one call equals the walked result bit for bit."""
    from int8inferenceengine_amd import workloads as wl

    name = "upsample_tiny"
    layers, spec, _ = wl.NETWORKS[name]
    sd = wl.synthetic_state_dict(name)
    net = wl.build(name)
    net.load(sd)
    x = wl.synthetic_input(name, 3, seed=5)
    seen = []

    def walk(ops, t, saved):
        for op in ops:
            prev = t.numpy()
            if op[0] == "layer":
                L, w, b = layers[op[1]], sd[op[1] + ".weight"], sd[op[1] + ".bias"]
                t = getattr(net, op[1])(t)
                got = t.numpy()
                want, mag = gr.conv2d_f64(prev, w, b, 1, L[4], L[5]), gr.conv2d_f64_mag(prev, w, b, 1, L[4], L[5])
                err, bound = np.abs(got.astype(np.float64) - want), f64_ref.dot_bound(mag, L[1] * L[3] * L[3])
                assert got.dtype == f32 and got.shape == want.shape and np.all(err <= bound), (op, float(np.nanmax(err / bound)))
            elif op[0] == "relu":
                t = i8ie.relu(t)
                assert support.bits_equal(t.numpy(), f64_ref.relu(prev)), op
            elif op[0] == "pool":
                t = i8ie.max_pool2d(t, op[1], op[2])
                assert support.bits_equal(t.numpy(), f64_ref.max_pool2d(prev.astype(np.float64), op[1], op[2])), op
            elif op[0] == "upsample":
                fh, fw = ur.factors(op[1])
                t = i8ie.upsample(t, op[1], op[2])
                got = t.numpy()
                seen.append(op)
                if op[2] == "nearest":
                    assert support.bits_equal(got, ur.nearest(prev, fh, fw)), op
                else:
                    val, mag = ur.bilinear_f64(prev, fh, fw)
                    assert got.shape == val.shape and np.all(np.abs(got.astype(np.float64) - val) <= 16 * 2.0 ** -24 * mag), op
                    assert support.bits_equal(got, ur.upsample_f32(prev, fh, fw, "bilinear")), op
            elif op[0] == "save":
                saved[op[1]] = t
            elif op[0] == "branch":
                saved[op[1]] = walk(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                other = saved[op[2]].numpy()
                t = getattr(net, op[1])(t, saved[op[2]])
                assert support.bits_equal(t.numpy(), (prev + other).astype(f32)), op
            elif op[0] == "concat":
                others = [saved[tag].numpy() for tag in op[2]]
                t = getattr(net, op[1])([t] + [saved[tag] for tag in op[2]])
                assert support.bits_equal(t.numpy(), np.concatenate([prev] + others, axis=1)), op
            else:
                raise AssertionError(op)
        return t

    walked = walk(spec, i8ie.tensor(x), {}).numpy()
    assert walked.shape == (3, 10, 32, 48) and len(seen) == 5
    assert support.bits_equal(net(i8ie.tensor(x)).numpy(), walked)
