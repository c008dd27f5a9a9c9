"""2:4 structured-sparse weights for pointwise Conv2d on the GPU (csrc/i8ie_sp24pw.hip): both instances of sp24pw_mfma and
sp24pw_direct bit for bit against the oracle on the pruned dense integers (orc.conv2d per tensor, tests/pc_pipeline.py per
channel) -- K of a partial step, one step, a step and a part, one chunk, a chunk and a part, and twice the deepest ring; feature
tile tails and a value past the widest block; pixel counts at each row tile's tail and on either side of the instance switch;
every layout at both ends with poisoned borders and guards -- and the Python surface against the INT8 witness."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import pc_pipeline as pcp
from requant_ref import row_scales, s_out_for
import support
from test_gpu_sparse24 import extremes, pattern, pruned, ptr
from test_gpu_w4pw import POISON, SOME, block, image

pytestmark = pytest.mark.gpu
ctx = support.ctx_fixture()
S_IN, ZP_OUT = np.float32(0.02), 61
# K: a partial 128-step (32), one step, a step and a part, one 512-chunk, a chunk and a part; DEEP: the few-pixel instance has
# the deepest ring, 4 stages of one chunk, so 8 chunks load every stage twice (and every stage of the many-pixel instance's
# 2 half-chunk stages eight times)
DEEP = 512 * 2 * 4
KS = [32, 128, 160, 512, 544, DEEP]
# n: one feature tile, a tile tail, several tiles (three blocks of the few-pixel instance), one past the widest block (128)
NS = [16, 24, 80, 129]
# pixel counts: 1; 15; 17 (a row tile of the few-pixel instance plus 1); 256 | 257 and 258 (the instance switch; 257 is four row
# tiles of the many-pixel instance plus 1); maps with h > 1 and m > 1 so that a border row and an image's edge lie inside a tile
MAPS = [(1, 1, 1), (1, 3, 5), (1, 1, 17), (2, 8, 16), (1, 1, 257), (2, 3, 43)]


class Conv:
    """a handle of i8ie_conv2d_create_sp24 from dense 2:4 integers [n, c], the expected bytes of its input, and its forwards in
    every layout"""

    def __init__(self, ctx, q, qw, zp_in, per_channel, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.q, self.zp_in, (self.n, c) = ctx, q, zp_in, qw.shape
        self.qb = rng.integers(-127, 128, self.n, dtype=np.int8)
        self.s_w = row_scales(self.n, rng) if per_channel else np.full(1, 2e-3, np.float32)
        self.s_out = s_out_for(S_IN, self.s_w, c)
        ref = pcp.conv2d_pc if per_channel else lambda *a: orc.conv2d(*a, want_acc=True)
        self.want, self.acc = ref(q, qw.reshape(self.n, c, 1, 1), self.qb, 1, 0, S_IN, zp_in, self.s_w if per_channel else self.s_w[0],
                                  self.s_out, ZP_OUT)
        g = -(-c // 4)
        self.values, self.index = np.empty((self.n, 2 * g), np.int8), np.empty((self.n, (g + 1) // 2), np.uint8)
        abi.ck(abi.lib().i8ie_pack_2_4(ptr(qw), self.n, c, ptr(self.values), ptr(self.index)))
        self.pc, self.L = int(per_channel), C.c_void_p()
        abi.ck(abi.lib().i8ie_conv2d_create_sp24(ctx.h, ptr(self.values), ptr(self.index), ptr(self.qb), self.n, c, ptr(self.s_w), self.pc,
                                                 C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(self.s_out), C.c_uint8(ZP_OUT)))

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
        assert {k: v for k, v in names.items() if k != "sp24_offsets"} == {kernel: 1}, (names, what)
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


def random_2_4(n, c, seed):
    return pruned(np.random.default_rng(seed).integers(-128, 128, (n, c), dtype=np.int8))


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("c", KS)
def test_parity_with_the_oracle(ctx, c, shape, per_channel):
    for n in (NS[(KS.index(c) + MAPS.index(shape)) % 4], NS[(KS.index(c) + MAPS.index(shape) + 2) % 4]):
        conv = Conv(ctx, image(shape, c, 7 * c + n), random_2_4(n, c, c + n), (0, 128, 255)[(c // 32 + n + shape[2]) % 3], per_channel, c + n)
        try:
            for lay in SOME:
                conv.check("sp24pw_mfma", **lay)
        finally:
            conv.close()


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("shape,c,n", [((1, 3, 5), 160, 24), ((2, 3, 43), 544, 129)])
def test_every_layout(ctx, shape, c, n, per_channel):
    conv = Conv(ctx, image(shape, c, 3), random_2_4(n, c, 5), 131, per_channel, 5)
    try:
        for ib, ob, in_s8, out_s8, relu in itertools.product((0, 1), (0, 1), (False, True), (False, True), (False, True)):
            conv.check("sp24pw_mfma", ib=ib, ob=ob, in_s8=in_s8, out_s8=out_s8, relu=relu)
    finally:
        conv.close()


@pytest.mark.parametrize("shape", [(1, 1, 17), (1, 1, 257)])
def test_every_position_pair_in_every_group_slot(ctx, shape):
    """pattern: a wrong pairing of value, position and activation byte cannot cancel"""
    conv = Conv(ctx, image(shape, 544, 11), pattern(24, 544), 7, True, 13)
    try:
        conv.check("sp24pw_mfma", ib=1, ob=1)
    finally:
        conv.close()


@pytest.mark.parametrize("zp_in", [0, 255])
@pytest.mark.parametrize("shape", [(1, 1, 15), (1, 1, 257)])
def test_all_255_inputs_against_the_extremes(ctx, shape, zp_in):
    conv = Conv(ctx, image(shape, 544, 0, fill=255), extremes(24, 544), zp_in, False, 9)
    try:
        conv.check("sp24pw_mfma", ib=1, ob=1)
    finally:
        conv.close()


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 5), (1, 1, 257)])
def test_the_direct_kernel(ctx, shape, per_channel):
    """C % 32 != 0, NCHW operands, an unaligned input and the force-fallback option all reach sp24pw_direct; the stateless entry"""
    for c in (20, 64):
        conv = Conv(ctx, image(shape, c, c), random_2_4(24, c, c), 201, per_channel, 11)
        try:
            conv.check("sp24pw_direct", nchw=True)
            conv.check("sp24pw_direct" if c == 20 else "sp24pw_mfma", ib=1, ob=1, in_s8=True, out_s8=True, relu=True)
            conv.check("sp24pw_direct", shift=1, ob=1)
            ctx.set_force_fallback(True)
            try:
                conv.check("sp24pw_direct", ib=1, out_s8=True)
            finally:
                ctx.set_force_fallback(False)
            m, _, h, w = conv.q.shape
            di, out, acc = ctx.put(conv.q), ctx.empty((m, 24, h, w), np.uint8), ctx.empty((m, h * w, 24), np.int32)
            abi.ck(abi.lib().i8ie_conv2d_u8s8_sp24(ctx.h, di.ptr, m, c, h, w, ptr(conv.values), ptr(conv.index), ptr(conv.qb), ptr(conv.s_w),
                                                   conv.pc, 24, C.c_float(S_IN), C.c_uint8(201), C.c_float(conv.s_out), C.c_uint8(ZP_OUT),
                                                   out.ptr, acc.ptr))
            assert np.array_equal(out.get(), conv.want) and np.array_equal(acc.get(), conv.acc)
            for b in (di, out, acc):
                b.free()
        finally:
            conv.close()


# ---- the Python surface: LayerNorm -> 1 x 1 (2:4) -> hardswish -> 1 x 1 (2:4) -> Add on a [n, 64, 1, 9] map ---------------------
@pytest.mark.parametrize("per_channel", [False, True])
def test_module_convert_conv_sparsity_against_the_int8_witness(tmp_path, per_channel):
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    x = np.random.default_rng(4).uniform(-2, 2, (5, 64, 1, 9)).astype(np.float32)
    net, dense = block(i8ie), block(i8ie)
    for m in (net, dense):
        m.prepare()
        m(i8ie.tensor(x))
    dense.convert(per_channel=per_channel)
    net.convert(per_channel=per_channel, conv_sparsity="2:4")
    for a in ("fc1", "fc2"):   # the quantiser's integers pruned by i8ie_prune_2_4's rule, the dense layer's scales
        layer, qw = getattr(net, a), getattr(dense, a).layer.q_weight()
        assert layer.sparsity() == "2:4" and layer.weight_bits() == 8 and layer.is_per_channel() == per_channel
        assert np.array_equal(layer.layer.q_weight(), pruned(qw.reshape(qw.shape[0], -1)).reshape(qw.shape))
        assert np.array_equal(layer.weight_scales(), getattr(dense, a).weight_scales())
    want, again, launches = support.counted_forward(lambda: net(i8ie.tensor(x)))
    assert launches.get("sp24pw_mfma") == 2 and "sp24pw_direct" not in launches and support.same_bits(again, want)
    saved = net.quantized_state_dict()
    assert saved["fc1.q_weight24"].shape == (96, 32) and saved["fc1.q_index24"].shape == (96, 8) and "fc1.q_weight" not in saved
    witness = block(i8ie)   # INT8 convs loaded with the pruned integers
    witness.load_quantized({k: v for k, v in saved.items() if not k.endswith("24")} |
                           {a + ".q_weight": getattr(net, a).layer.q_weight() for a in ("fc1", "fc2")})
    assert witness.fc1.sparsity() is None and support.same_bits(witness(i8ie.tensor(x)).numpy(), want)
    path = str(tmp_path / "sp24pw.npz")
    net.save_quantized(path)
    fresh = block(i8ie)
    fresh.load_quantized_file(path)
    assert fresh.fc2.sparsity() == "2:4" and np.array_equal(fresh.fc2.layer.q_weight(), net.fc2.layer.q_weight())
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), want)
    g = GraphedForward(fresh, i8ie.tensor(x).prefetch())
    for _ in range(3):
        assert support.same_bits(g().numpy(), want)
    fresh.load_quantized(witness.quantized_state_dict())   # a later 8-bit load returns the layers to dense
    assert fresh.fc1.sparsity() is None and fresh.fc2.sparsity() is None and support.same_bits(fresh(i8ie.tensor(x)).numpy(), want)
