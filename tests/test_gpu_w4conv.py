"""4-bit weights for k x k Conv2d on the GPU (csrc/i8ie_w4conv.hip): both instances of w4conv_mfma and w4conv_direct bit for bit
against the oracle's accumulators requantised per column (tests/pc_pipeline.py: conv2d_pc) on the unpacked integers -- every
geometry the kernel addresses differently, channels of half an MFMA, one, and a tap that spans two chunks, feature-tile tails,
maps on either side of the instance switch, every layout at both ends with poisoned guards, borders smaller and larger than the
padding -- and the Python surface against the INT8 witness."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import pc_pipeline as pcp
from requant_ref import s_out_for
import support
from test_gpu_w4 import ptr, weights
from test_gpu_w4pw import image

pytestmark = pytest.mark.gpu
ctx = support.ctx_fixture()
S_IN, ZP_OUT, POISON = np.float32(0.02), 61, 0xEE


def out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


class Conv:
    """a handle of i8ie_conv2d_create_w4_geom, the expected bytes of its input, and its forwards in every layout"""

    def __init__(self, ctx, q, n, geom, zp_in, seed):
        rng = np.random.default_rng(seed)
        (k, stride, pad, dil), c = geom, q.shape[1]
        self.ctx, self.q, self.n, self.geom, self.zp_in = ctx, q, n, geom, zp_in
        self.qw, self.packed, self.qb, s_w = weights(n, c * k * k, rng)
        s_out = s_out_for(S_IN, s_w, c * k * k) / np.float32(8)  # (nibbles: sums a sixteenth of what s_out_for assumes)
        e = dil * (k - 1) + 1  # the oracle has no dilation: the kernel inflated by zeros has the same sums and the same oc
        wide = np.zeros((n, c, e, e), np.int8)
        wide[:, :, ::dil, ::dil] = self.qw.reshape(n, c, k, k)
        self.want, self.acc = pcp.conv2d_pc(q, wide, self.qb, stride, pad, S_IN, zp_in, s_w, s_out, ZP_OUT)
        self.s_w, self.s_out, self.L = s_w, s_out, C.c_void_p()
        abi.ck(abi.lib().i8ie_conv2d_create_w4_geom(ctx.h, ptr(self.packed), ptr(self.qb), ptr(s_w), n, c, k, stride, pad, dil, C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(s_out), C.c_uint8(ZP_OUT)))

    def check(self, kernels, ib=0, ob=0, in_s8=False, out_s8=False, relu=False, nchw=False, shift=0):
        """one forward: the kernels that ran, the sums, the interior bytes, the untouched border and guards.  The input's border
        holds zp_in where w4conv_mfma reads it in place, as an NHWC producer writes it for i8ie_layer_padding, and poison where
        nobody may read it (the direct kernel checks bounds, the reborder pass copies the interior)."""
        m, _, h, w = self.q.shape
        oh, ow = self.want.shape[2:]
        phys = self.q if nchw else support.phys_nhwc(self.q, ib, self.zp_in if kernels == ("w4conv_mfma",) else POISON, in_s8)
        buf = self.ctx.put(np.concatenate([np.zeros(shift, np.uint8), phys.ravel()]))
        out = abi.GuardedU8(self.ctx, (m, self.n, oh, ow) if nchw else (m, oh + 2 * ob, ow + 2 * ob, self.n))
        acc = abi.GuardedU8(self.ctx, (m, oh * ow, self.n), np.int32)
        with self.ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_layer_forward_fused(self.L, C.c_void_p(buf.ptr.value + shift), 0 if nchw else 1 + in_s8, ib, m, h, w,
                                                      C.c_float(S_IN), C.c_uint8(self.zp_in), int(relu), out.ptr, 0 if nchw else 1 + out_s8,
                                                      ob, acc.ptr))
        got, sums, what = out.get(), acc.get(), (self.geom, kernels, ib, ob, in_s8, out_s8, relu, nchw, shift)
        assert {k: v for k, v in names.items() if k != "w4_offsets"} == dict.fromkeys(kernels, 1), (names, what)
        assert out.guards_ok() and acc.guards_ok() and np.array_equal(sums, self.acc), what
        want = np.maximum(self.want, np.uint8(ZP_OUT)) if relu else self.want
        if not nchw:
            ring = got.copy()
            ring[:, ob:ob + oh, ob:ob + ow] = 0xC3
            assert (ring == 0xC3).all(), what  # (the border is the caller's: never written)
            got = (got[:, ob:ob + oh, ob:ob + ow] ^ np.uint8(0x80 if out_s8 else 0)).transpose(0, 3, 1, 2)
        assert np.array_equal(got, want), what
        for b in (buf, out, acc):
            b.free()

    def mfma(self, ib):
        """the launches of an NHWC forward whose input has `ib` border pixels"""
        return ("w4conv_mfma",) if ib >= self.geom[2] else ("reborder_u8_nhwc", "w4conv_mfma")

    def close(self):
        abi.lib().i8ie_layer_destroy(self.L)


# (k, stride, pad, dil): the plain 3 x 3; strided; unpadded; dilated; 5 x 5; the strided shortcut; the 7 x 7 stride-2 stem shape
GEOMS = [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 0, 1), (3, 1, 2, 2), (5, 1, 2, 1), (1, 2, 0, 1), (7, 2, 3, 1)]
# one pixel whose taps are all border but the centre; small; an image edge inside a row tile; odd; 272 output pixels at stride 1
# pad 1 -- past the instance switch at 256, with a ragged last tile
MAPS = [(1, 1, 1), (1, 3, 5), (2, 4, 4), (1, 5, 13), (1, 16, 17)]


def fits(shape, geom):
    k, stride, pad, dil = geom
    return min(out_size(shape[1], k, stride, pad, dil), out_size(shape[2], k, stride, pad, dil)) >= 1


def layouts(pad):
    """each side plain / bordered / re-biased at least once per shape, the input's border below, at and above the padding"""
    return [dict(ib=0), dict(ib=pad, ob=1, in_s8=True, out_s8=True, relu=True), dict(ib=pad + 1, out_s8=True), dict(ib=pad, ob=2, in_s8=True, relu=True)]


@pytest.mark.parametrize("geom,shape", [(g, s) for g in GEOMS for s in MAPS if fits(s, g)])
def test_geometries_against_the_oracle(ctx, geom, shape):
    c, n = ((32, 24), (64, 16), (288, 80))[(GEOMS.index(geom) + MAPS.index(shape)) % 3]
    if c * geom[0] ** 2 > 8192:  # (keeps the oracle's loops short; 288 channels meet 3 x 3 and 1 x 1)
        c, n = 64, 80
    conv = Conv(ctx, image(shape, c, 7 * c + n), n, geom, (0, 128, 255)[(c + n + shape[2]) % 3], c + n)
    try:
        for lay in layouts(geom[2]):
            conv.check(conv.mfma(lay["ib"]), **lay)
    finally:
        conv.close()


@pytest.mark.parametrize("shape", [(1, 3, 5), (1, 16, 17)])
@pytest.mark.parametrize("c,n", list(itertools.product((32, 64, 288), (16, 24, 80))))
def test_channels_and_features(ctx, c, n, shape):
    conv = Conv(ctx, image(shape, c, 5 * c + n), n, (3, 1, 1, 1), (0, 128, 255)[(c + n) % 3], c + n)
    try:
        for lay in layouts(1):
            conv.check(conv.mfma(lay["ib"]), **lay)
    finally:
        conv.close()


@pytest.mark.parametrize("shape,c,n", [((1, 3, 5), 64, 24), ((1, 16, 17), 288, 80)])
def test_every_layout(ctx, shape, c, n):
    conv = Conv(ctx, image(shape, c, 3), n, (3, 1, 1, 1), 131, 5)
    try:
        for ib, ob, in_s8, out_s8, relu in itertools.product((1, 2), (0, 1), (False, True), (False, True), (False, True)):
            conv.check(("w4conv_mfma",), ib=ib, ob=ob, in_s8=in_s8, out_s8=out_s8, relu=relu)
    finally:
        conv.close()


@pytest.mark.parametrize("zp_in", [0, 255])
@pytest.mark.parametrize("shape", [(1, 3, 5), (1, 16, 17)])
def test_all_255_inputs_against_the_nibble_minus_8(ctx, shape, zp_in):
    conv = Conv(ctx, image(shape, 288, 0, fill=255), 24, (3, 1, 1, 1), zp_in, 9)   # (weights(): feature 0 is all -8)
    try:
        assert (conv.qw[0] == -8).all() and (conv.qw[1] == 7).all()
        conv.check(("w4conv_mfma",), ib=1, ob=1)
    finally:
        conv.close()


@pytest.mark.parametrize("geom", [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2)])
@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 4, 4)])
def test_the_direct_kernel(ctx, shape, geom):
    """C % 32 != 0, NCHW operands, an unaligned input and the force-fallback option all reach w4conv_direct; the stateless entry"""
    k, stride, pad, dil = geom
    for c in (20, 64):
        conv = Conv(ctx, image(shape, c, c), 24, geom, 201, 11)
        try:
            conv.check(("w4conv_direct",), nchw=True)
            conv.check(("w4conv_direct",) if c == 20 else ("w4conv_mfma",), ib=pad, ob=1, in_s8=True, out_s8=True, relu=True)
            conv.check(("w4conv_direct",), ib=0, shift=1, ob=1)
            ctx.set_force_fallback(True)
            try:
                conv.check(("w4conv_direct",), ib=pad + 1, out_s8=True)
            finally:
                ctx.set_force_fallback(False)
            m, _, h, w = conv.q.shape
            di, out, acc = ctx.put(conv.q), ctx.empty(conv.want.shape, np.uint8), ctx.empty(conv.acc.shape, np.int32)
            abi.ck(abi.lib().i8ie_conv2d_u8s4_geom(ctx.h, di.ptr, m, c, h, w, ptr(conv.packed), ptr(conv.qb), ptr(conv.s_w), 24, k, stride, pad,
                                                   dil, C.c_float(S_IN), C.c_uint8(201), C.c_float(conv.s_out), C.c_uint8(ZP_OUT), out.ptr,
                                                   acc.ptr))
            assert np.array_equal(out.get(), conv.want) and np.array_equal(acc.get(), conv.acc)
            for b in (di, out, acc):
                b.free()
        finally:
            conv.close()


def test_pointwise_identity(ctx):
    """k = 1, stride 1, pad 0 through the new create entry is the handle of i8ie_conv2d_create_w4: w4pw_mfma runs"""
    conv = Conv(ctx, image((1, 3, 5), 64, 1), 24, (1, 1, 0, 1), 77, 2)
    try:
        conv.check(("w4pw_mfma",), ib=1, ob=1)
        bits, pad = C.c_int(), C.c_int(-1)
        abi.ck(abi.lib().i8ie_layer_weight_bits(conv.L, C.byref(bits)))
        abi.ck(abi.lib().i8ie_layer_padding(conv.L, C.byref(pad)))
        assert (bits.value, pad.value) == (4, 0)
    finally:
        conv.close()


def test_layout_queries(ctx):
    conv = Conv(ctx, image((1, 3, 5), 32, 1), 16, (3, 2, 1, 1), 9, 2)
    try:
        lib, a, b = abi.lib(), C.c_int(-1), C.c_int(-1)
        abi.ck(lib.i8ie_layer_weight_bits(conv.L, C.byref(a)))
        abi.ck(lib.i8ie_layer_padding(conv.L, C.byref(b)))
        assert (a.value, b.value) == (4, 1)
        abi.ck(lib.i8ie_layer_rebiased_io(conv.L, 1, 8, 8, 0, 0, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (1, 1)
        abi.ck(lib.i8ie_layer_rebiased_io(conv.L, 1, 8, 8, 2, 2, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (1, 0)
        abi.ck(lib.i8ie_layer_fuses_pool(conv.L, 1, 8, 8, 2, 2, C.byref(a)))
        abi.ck(lib.i8ie_layer_accepts_f32_input(conv.L, 8, 8, C.byref(b)))
        assert (a.value, b.value) == (0, 0)
        abi.ck(lib.i8ie_layer_preferred_layout(conv.L, C.byref(a)))
        geom = (C.c_int * 8)()
        abi.ck(lib.i8ie_layer_geometry(conv.L, geom))
        assert a.value == 1 and list(geom) == [3, 3, 2, 2, 1, 1, 1, 1]
    finally:
        conv.close()


# ---- the Python surface: a basic residual block, 3 x 3 -> relu -> 3 x 3 stride 2, a strided 1 x 1 shortcut, Add ----------------------
def block(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2 = i8ie.Conv2d(64, 64, 3, padding=1), i8ie.Conv2d(64, 96, 3, stride=2, padding=1)
            self.short, self.add = i8ie.Conv2d(64, 96, 1, stride=2), i8ie.Add()

        def forward(self, x):
            return self.add(self.short(x), self.c2(i8ie.relu(self.c1(x))))

    net, rng = Net(), np.random.default_rng(23)
    for layer, shape in ((net.c1, (64, 64, 3, 3)), (net.c2, (96, 64, 3, 3)), (net.short, (96, 64, 1, 1))):
        layer.load_weight((rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))).astype(np.float32))
        layer.load_bias((rng.standard_normal(shape[0]) * 0.05).astype(np.float32))
    return net


def test_module_convert_spatial_against_the_int8_witness(tmp_path):
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    convs = ("c1", "c2", "short")
    x = np.random.default_rng(4).uniform(-2, 2, (5, 64, 8, 8)).astype(np.float32)
    net = block(i8ie)
    net.prepare()
    net(i8ie.tensor(x))
    net.convert(weight_bits=4, spatial=True)
    assert all(getattr(net, a).weight_bits() == 4 and getattr(net, a).is_per_channel() for a in convs)
    assert net.c2.layer.q_weight().shape == (96, 64, 3, 3) and net.c2.layer.q_weight().dtype == np.int8 and np.abs(net.c2.layer.q_weight()).max() == 7
    assert net.c1.weight_scales().shape == (64,)
    with pytest.raises(RuntimeError):
        net.c1.weight_scale()
    want, again, launches = support.counted_forward(lambda: net(i8ie.tensor(x)))
    assert launches.get("w4conv_mfma") == 3 and "w4conv_direct" not in launches and support.same_bits(again, want)
    state = net.quantized_state_dict()
    assert state["c2.q_weight4"].dtype == np.uint8 and state["c2.q_weight4"].shape == (96, 288) and "c2.q_weight" not in state
    assert state["c2.q_weight4_kernel"].dtype == np.int32 and list(state["c2.q_weight4_kernel"]) == [3, 3]
    witness = block(i8ie)   # per-channel INT8 convs loaded with the unpacked integers
    witness.load_quantized({k: v for k, v in state.items() if ".q_weight4" not in k} | {a + ".q_weight": getattr(net, a).layer.q_weight() for a in convs})
    assert witness.c1.weight_bits() == 8 and support.same_bits(witness(i8ie.tensor(x)).numpy(), want)
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(3):
        assert support.same_bits(g().numpy(), want)
    path = str(tmp_path / "w4conv.npz")
    net.save_quantized(path)
    fresh = block(i8ie)
    fresh.load_quantized_file(path)
    assert fresh.c2.weight_bits() == 4 and np.array_equal(fresh.c2.weight_scales(), net.c2.weight_scales())
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), want)
