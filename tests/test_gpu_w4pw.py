"""4-bit weights for pointwise Conv2d on the GPU (csrc/i8ie_w4pw.hip): both instances of w4pw_mfma and w4pw_direct bit for bit
against the oracle's accumulators requantised per column (tests/pc_pipeline.py: conv2d_pc) on the unpacked integers -- K of one
step, two, and past the panel's 256-chunk; feature-tile tails; pixel counts at each row tile's tail and on either side of the
instance switch; every layout at both ends with poisoned borders and guards -- and the Python surface against the INT8 witness."""
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

pytestmark = pytest.mark.gpu
ctx = support.ctx_fixture()
S_IN, ZP_OUT, POISON = np.float32(0.02), 61, 0xEE


class Conv:
    """a handle of i8ie_conv2d_create_w4, the expected bytes of its input, and its forwards in every layout"""

    def __init__(self, ctx, q, n, zp_in, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.q, self.n, self.zp_in, c = ctx, q, n, zp_in, q.shape[1]
        self.qw, self.packed, self.qb, s_w = weights(n, c, rng)
        s_out = s_out_for(S_IN, s_w, c) / np.float32(8)  # (nibbles: sums a sixteenth of what s_out_for assumes)
        self.want, self.acc = pcp.conv2d_pc(q, self.qw.reshape(n, c, 1, 1), self.qb, 1, 0, S_IN, zp_in, s_w, s_out, ZP_OUT)
        self.s_w, self.s_out, self.L = s_w, s_out, C.c_void_p()
        abi.ck(abi.lib().i8ie_conv2d_create_w4(ctx.h, ptr(self.packed), ptr(self.qb), ptr(s_w), n, c, C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(s_out), C.c_uint8(ZP_OUT)))

    def check(self, kernel, ib=0, ob=0, in_s8=False, out_s8=False, relu=False, nchw=False, shift=0):
        """one forward: the kernel that ran, the sums, the interior bytes, the untouched border and guards"""
        m, _, h, w = self.q.shape
        phys = self.q if nchw else support.phys_nhwc(self.q, ib, POISON, in_s8)
        buf = self.ctx.put(np.concatenate([np.zeros(shift, np.uint8), phys.ravel()]))
        out = abi.GuardedU8(self.ctx, (m, self.n, h, w) if nchw else (m, h + 2 * ob, w + 2 * ob, self.n))
        acc = abi.GuardedU8(self.ctx, (m, h * w, self.n), np.int32)
        with self.ctx.launch_map() as names:
            abi.ck(abi.lib().i8ie_layer_forward_fused(self.L, C.c_void_p(buf.ptr.value + shift), 0 if nchw else 1 + in_s8, ib, m, h, w,
                                                      C.c_float(S_IN), C.c_uint8(self.zp_in), int(relu), out.ptr, 0 if nchw else 1 + out_s8,
                                                      ob, acc.ptr))
        got, sums, what = out.get(), acc.get(), (kernel, ib, ob, in_s8, out_s8, relu, nchw, shift)
        assert {k: v for k, v in names.items() if k != "w4_offsets"} == {kernel: 1}, (names, what)
        assert out.guards_ok() and acc.guards_ok() and np.array_equal(sums, self.acc), what
        want = np.maximum(self.want, np.uint8(ZP_OUT)) if relu else self.want
        if not nchw:
            ring = got.copy()
            ring[:, ob:ob + h, ob:ob + w] = 0xC3
            assert (ring == 0xC3).all(), what  # (the border is the caller's: never written)
            got = (got[:, ob:ob + h, ob:ob + w] ^ np.uint8(0x80 if out_s8 else 0)).transpose(0, 3, 1, 2)
        assert np.array_equal(got, want), what
        for b in (buf, out, acc):
            b.free()

    def close(self):
        abi.lib().i8ie_layer_destroy(self.L)


def image(shape, c, seed, fill=None):
    m, h, w = shape
    rng = np.random.default_rng(seed)
    return np.full((m, c, h, w), fill, np.uint8) if fill is not None else rng.integers(0, 256, (m, c, h, w), dtype=np.uint8)


# pixel counts: 1; 15; 17 and 65 (a row tile of the few-row instance plus 1, four plus 1); 256 | 257 (the instance switch; 257 is four
# row tiles of the many-row instance plus 1); maps with h > 1 and m > 1 so that a border row and an image's edge lie inside a tile
MAPS = [(1, 1, 1), (1, 3, 5), (1, 1, 17), (1, 5, 13), (2, 8, 16), (1, 1, 257)]
# each side plain / bordered / re-biased at least once per shape; the full cross: test_every_layout
SOME = [dict(), dict(ib=1, ob=1, in_s8=True, out_s8=True, relu=True), dict(ib=1, out_s8=True), dict(ob=1, in_s8=True, relu=True)]


@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("c,n", list(itertools.product((32, 64, 288), (16, 24, 80))))
def test_parity_with_the_oracle(ctx, c, n, shape):
    conv = Conv(ctx, image(shape, c, 7 * c + n), n, (0, 128, 255)[(c + n + shape[2]) % 3], c + n)
    try:
        for lay in SOME:
            conv.check("w4pw_mfma", **lay)
    finally:
        conv.close()


@pytest.mark.parametrize("shape,c,n", [((1, 3, 5), 64, 24), ((2, 3, 43), 288, 80)])
def test_every_layout(ctx, shape, c, n):
    conv = Conv(ctx, image(shape, c, 3), n, 131, 5)
    try:
        for ib, ob, in_s8, out_s8, relu in itertools.product((0, 1), (0, 1), (False, True), (False, True), (False, True)):
            conv.check("w4pw_mfma", ib=ib, ob=ob, in_s8=in_s8, out_s8=out_s8, relu=relu)
    finally:
        conv.close()


@pytest.mark.parametrize("zp_in", [0, 255])
@pytest.mark.parametrize("shape", [(1, 1, 15), (1, 1, 257)])
def test_all_255_inputs_against_the_nibble_minus_8(ctx, shape, zp_in):
    conv = Conv(ctx, image(shape, 288, 0, fill=255), 24, zp_in, 9)   # (weights(): feature 0 is all -8)
    try:
        assert (conv.qw[0] == -8).all() and (conv.qw[1] == 7).all()
        conv.check("w4pw_mfma", ib=1, ob=1)
    finally:
        conv.close()


@pytest.mark.parametrize("shape", [(1, 3, 5), (1, 1, 257)])
def test_the_direct_kernel(ctx, shape):
    """C % 32 != 0, NCHW operands, an unaligned input and the force-fallback option all reach w4pw_direct; the stateless entry"""
    for c in (20, 64):
        conv = Conv(ctx, image(shape, c, c), 24, 201, 11)
        try:
            conv.check("w4pw_direct", nchw=True)
            conv.check("w4pw_direct" if c == 20 else "w4pw_mfma", ib=1, ob=1, in_s8=True, out_s8=True, relu=True)
            conv.check("w4pw_direct", shift=1, ob=1)
            ctx.set_force_fallback(True)
            try:
                conv.check("w4pw_direct", ib=1, out_s8=True)
            finally:
                ctx.set_force_fallback(False)
            m, _, h, w = conv.q.shape
            di, out, acc = ctx.put(conv.q), ctx.empty((m, 24, h, w), np.uint8), ctx.empty((m, h * w, 24), np.int32)
            abi.ck(abi.lib().i8ie_conv2d_u8s4(ctx.h, di.ptr, m, c, h, w, ptr(conv.packed), ptr(conv.qb), ptr(conv.s_w), 24, C.c_float(S_IN),
                                              C.c_uint8(201), C.c_float(conv.s_out), C.c_uint8(ZP_OUT), out.ptr, acc.ptr))
            assert np.array_equal(out.get(), conv.want) and np.array_equal(acc.get(), conv.acc)
            for b in (di, out, acc):
                b.free()
        finally:
            conv.close()


# ---- the Python surface: LayerNorm -> 1 x 1 (W4) -> hardswish -> 1 x 1 (W4) -> Add on a [n, 64, 1, 9] map -----------------------
def block(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.norm, self.fc1, self.act = i8ie.LayerNorm(64), i8ie.Conv2d(64, 96, 1), i8ie.Activation("hardswish")
            self.fc2, self.add = i8ie.Conv2d(96, 64, (1, 1)), i8ie.Add()

        def forward(self, x):
            return self.add(x, self.fc2(self.act(self.fc1(self.norm(x)))))

    net, rng = Net(), np.random.default_rng(23)
    for layer, shape in ((net.fc1, (96, 64, 1, 1)), (net.fc2, (64, 96, 1, 1))):
        layer.load_weight((rng.standard_normal(shape) * np.sqrt(2.0 / shape[1])).astype(np.float32))
        layer.load_bias((rng.standard_normal(shape[0]) * 0.05).astype(np.float32))
    return net


def test_module_convert_pointwise_against_the_int8_witness(tmp_path):
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    x = np.random.default_rng(4).uniform(-2, 2, (5, 64, 1, 9)).astype(np.float32)
    net = block(i8ie)
    net.prepare()
    net(i8ie.tensor(x))
    net.convert(weight_bits=4, pointwise=True)
    assert net.fc1.weight_bits() == 4 and net.fc2.weight_bits() == 4 and net.fc1.is_per_channel()
    assert net.fc1.layer.q_weight().shape == (96, 64, 1, 1) and np.abs(net.fc1.layer.q_weight()).max() == 7
    with pytest.raises(RuntimeError):
        net.fc1.weight_scale()
    want, again, launches = support.counted_forward(lambda: net(i8ie.tensor(x)))
    assert launches.get("w4pw_mfma") == 2 and "w4pw_direct" not in launches and support.same_bits(again, want)
    state = net.quantized_state_dict()
    assert state["fc1.q_weight4"].dtype == np.uint8 and state["fc1.q_weight4"].shape == (96, 32) and "fc1.q_weight" not in state
    witness = block(i8ie)   # per-channel INT8 convs loaded with the unpacked integers
    witness.load_quantized({k: v for k, v in state.items() if not k.endswith(".q_weight4")} |
                           {a + ".q_weight": getattr(net, a).layer.q_weight() for a in ("fc1", "fc2")})
    assert witness.fc1.weight_bits() == 8 and support.same_bits(witness(i8ie.tensor(x)).numpy(), want)
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(3):
        assert support.same_bits(g().numpy(), want)
    path = str(tmp_path / "w4pw.npz")
    net.save_quantized(path)
    fresh = block(i8ie)
    fresh.load_quantized_file(path)
    assert fresh.fc2.weight_bits() == 4 and np.array_equal(fresh.fc2.weight_scales(), net.fc2.weight_scales())
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), want)
