"""4-bit weights for Linear on the GPU (csrc/i8ie_w4lin.hip): w4lin_mfma and w4lin_direct bit for bit against the oracle's
accumulators requantised per column (tests/pc_pipeline.py) on the unpacked integers, at the shapes where the kernels change
path -- row-tile and feature-tile tails, a second row block, K short of / just past one and two 256-value chunks -- and the
Python surface: the INT8 witness, the NHWC-flattened input, forward_dequant, graph replay, save / load, Module.convert."""
import ctypes as C

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
import pc_pipeline as pcp
from requant_ref import row_scales, s_out_for
import support

pytestmark = pytest.mark.gpu
ctx = support.ctx_fixture()
S_IN, ZP_OUT = np.float32(0.02), 61


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def weights(n, k, rng):
    """random nibbles; the first rows all -8, all 7, and -8 / 7 alternating from an even and from an odd position (a swapped
    nibble or a lost sign changes their sums)"""
    qw = rng.integers(-8, 8, (n, k), dtype=np.int8)
    alt = np.where(np.arange(k) % 2 == 0, -8, 7).astype(np.int8)
    for j, row in enumerate((np.full(k, -8), np.full(k, 7), alt, -1 - alt)[:n]):
        qw[j] = row
    packed = np.empty((n, (k + 1) // 2), np.uint8)
    abi.ck(abi.lib().i8ie_pack_w4(ptr(qw), n, k, ptr(packed)))
    return qw, packed, rng.integers(-127, 128, n, dtype=np.int8), row_scales(n, rng)


class W4:
    """a handle of i8ie_linear_create_w4 and its forwards on host arrays"""

    def __init__(self, ctx, packed, qb, s_w, k, s_out):
        self.ctx, self.n, self.k, self.L = ctx, packed.shape[0], k, C.c_void_p()
        abi.ck(abi.lib().i8ie_linear_create_w4(ctx.h, ptr(packed), ptr(qb), ptr(s_w), self.n, k, C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(s_out), C.c_uint8(ZP_OUT)))

    def forward(self, q, zp_in, relu=False, shift=0, hw=(0, 0), dequant=False):
        """(out, acc, {kernel: launches}); shift: bytes the input lies past a 16-byte boundary"""
        m = q.shape[0]
        buf = self.ctx.put(np.concatenate([np.zeros(shift, np.uint8), q.ravel()]))
        out, acc, f = self.ctx.empty((m, self.n), np.uint8), self.ctx.empty((m, self.n), np.int32), self.ctx.empty((m, self.n), np.float32)
        src = C.c_void_p(buf.ptr.value + shift)
        with self.ctx.launch_map() as names:
            if dequant:
                abi.ck(abi.lib().i8ie_layer_forward_dequant(self.L, src, 0, m, 0, 0, C.c_float(S_IN), C.c_uint8(zp_in), int(relu), out.ptr, f.ptr))
            else:
                abi.ck(abi.lib().i8ie_layer_forward_fused(self.L, src, 1 if hw[0] else 0, 0, m, hw[0], hw[1], C.c_float(S_IN),
                                                          C.c_uint8(zp_in), int(relu), out.ptr, 0, 0, acc.ptr))
        res = (f.get() if dequant else out.get(), acc.get(), names)
        for b in (buf, out, acc, f):
            b.free()
        return res

    def close(self):
        abi.lib().i8ie_layer_destroy(self.L)


def ran(names):
    """the launch map without the handle's one-off vectors kernel (the first forward per (s_in, zp_in) runs it)"""
    return {k: v for k, v in names.items() if k != "w4_offsets"}


def u8s4(ctx, q, packed, qb, s_w, k, zp_in, s_out):
    """the stateless entry: (out, acc)"""
    m, n = q.shape[0], packed.shape[0]
    di, out, acc = ctx.put(q), ctx.empty((m, n), np.uint8), ctx.empty((m, n), np.int32)
    abi.ck(abi.lib().i8ie_linear_u8s4(ctx.h, di.ptr, m, k, ptr(packed), ptr(qb), ptr(s_w), n, C.c_float(S_IN), C.c_uint8(zp_in),
                                      C.c_float(s_out), C.c_uint8(ZP_OUT), out.ptr, acc.ptr))
    res = out.get(), acc.get()
    for b in (di, out, acc):
        b.free()
    return res


# K: one chunk's tails (32, 64, 96), just past one chunk of 256 (288) and past two (544); 40: not a multiple of 32.  DEEP: the
# LDS ring takes a stage again while later chunks are in flight -- 9 chunks for the 8 stages of the few-row shape, 4 for the 3
# of the many-row shape
DEEP = [(1, 2304), (16, 2304), (17, 1024), (129, 1024)]


@pytest.mark.parametrize("m,k", [(m, k) for m in (1, 16, 17, 129, 300) for k in (32, 64, 96, 288, 544, 40)] + DEEP)
def test_parity_with_the_oracle(ctx, m, k):
    rng = np.random.default_rng(1000 * m + k)
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    kernel = "w4lin_mfma" if k % 32 == 0 else "w4lin_direct"
    for n, zp_in in ((1, 0), (16, 128), (17, 255), (40, 128)):
        qw, packed, qb, s_w = weights(n, k, rng)
        s_out = s_out_for(S_IN, s_w, k) / np.float32(8)  # (nibbles: sums a sixteenth of what s_out_for assumes)
        want, a0, _ = pcp.linear_pc(q, qw, qb, S_IN, zp_in, s_w, s_out, ZP_OUT)
        got, acc = u8s4(ctx, q, packed, qb, s_w, k, zp_in, s_out)
        assert np.array_equal(acc, a0) and np.array_equal(got, want), (m, n, k, "stateless")
        h = W4(ctx, packed, qb, s_w, k, s_out)
        try:
            got, acc, names = h.forward(q, zp_in, relu=True)
            assert ran(names) == {kernel: 1}, names
            assert np.array_equal(acc, a0) and np.array_equal(got, np.maximum(want, np.uint8(ZP_OUT))), (m, n, k, "relu")
            got, _, names = h.forward(q, zp_in, shift=1)   # an unaligned input: the definition kernel
            assert names == {"w4lin_direct": 1} and np.array_equal(got, want), (m, n, k, "unaligned")
            ctx.set_force_fallback(True)
            try:
                got, acc, names = h.forward(q, zp_in)
            finally:
                ctx.set_force_fallback(False)
            assert names == {"w4lin_direct": 1} and np.array_equal(acc, a0) and np.array_equal(got, want), (m, n, k, "fallback")
        finally:
            h.close()


def test_nhwc_flattened_rows_and_dequant(ctx):
    """rows that are a flattened NHWC activation (c = 16, h * w = 4) walk K in (h, w, c) order; forward_dequant"""
    rng = np.random.default_rng(3)
    m, c, hh, ww, n, zp_in = 33, 16, 2, 2, 24, 121
    k = c * hh * ww
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    qw, packed, qb, s_w = weights(n, k, rng)
    s_out = s_out_for(S_IN, s_w, k) / np.float32(8)
    want, a0, _ = pcp.linear_pc(q, qw, qb, S_IN, zp_in, s_w, s_out, ZP_OUT)
    flat = np.ascontiguousarray(q.reshape(m, c, hh, ww).transpose(0, 2, 3, 1)).reshape(m, k)
    h = W4(ctx, packed, qb, s_w, k, s_out)
    try:
        for _ in range(2):  # (the second call finds the re-packed panel)
            got, acc, names = h.forward(flat, zp_in, hw=(hh, ww))
            assert names.get("w4lin_mfma") == 1 and np.array_equal(acc, a0) and np.array_equal(got, want)
        assert names == {"w4lin_mfma": 1}, names
        ctx.set_force_fallback(True)
        try:
            got, _, names = h.forward(flat, zp_in, hw=(hh, ww))
        finally:
            ctx.set_force_fallback(False)
        assert names == {"w4lin_direct": 1} and np.array_equal(got, want)
        got, _, names = h.forward(q, zp_in, dequant=True)
        assert names.get("w4lin_mfma") == 1 and len(names) == 2, names
        assert support.same_bits(got, orc.dequantize(want, s_out, ZP_OUT))
    finally:
        h.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def u8_tensor(q):
    """an i8ie u8 tensor holding q with scale 1, zero point 0 (x / 1 + 0 truncates to x exactly)"""
    import _CXX_i8ie as cx
    import i8ie

    return i8ie.Tensor(cx.quantize(cx.tensor(np.asarray(q, np.float32)), 1.0, 0))


def test_int8_witness_and_surface():
    """convert(weight_bits=4) holds what the quantiser says, gives the oracle's bytes, and so does an ordinary per-channel
    INT8 Linear loaded with the unpacked integers"""
    import i8ie

    rng = np.random.default_rng(5)
    m, k, n = 70, 320, 48
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    lin = i8ie.Linear(k, n)
    lin.load_weight(w)
    lin.load_bias(b)
    lin.set_output_qparams(0.5, 100)
    lin.convert(weight_bits=4)
    qw, qb, s_w = np.empty((n, k), np.int8), np.empty(n, np.int8), np.empty(n, np.float32)
    abi.ck(abi.lib().i8ie_quantize_weight_w4(ptr(w), n, C.c_int64(k), ptr(b), ptr(qw), ptr(qb), ptr(s_w)))
    assert lin.weight_bits() == 4 and lin.is_per_channel() and np.array_equal(lin.weight_scales(), s_w)
    assert np.array_equal(lin.layer.q_weight(), qw) and np.array_equal(lin.layer.q_bias(), qb)
    with pytest.raises(RuntimeError):
        lin.weight_scale()
    want, _, _ = pcp.linear_pc(q, qw, qb, np.float32(1), 0, s_w, np.float32(0.5), 100)
    got, _, launches = support.counted_forward(lambda: lin(u8_tensor(q)))
    assert launches.get("w4lin_mfma") == 1 and np.array_equal(got, want)
    witness = i8ie.Linear(k, n)
    witness.layer.load_quantized(qw, qb, s_w, 0.5, 100)
    assert witness.weight_bits() == 8 and np.array_equal(witness(u8_tensor(q)).numpy(), want)


def mlp(with_conv):
    """conv (optional) -> fc1 -> relu -> fc2 as an i8ie.Module with random FP32 weights"""
    import i8ie

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            if with_conv:
                self.conv = i8ie.Conv2d(16, 16, 3, padding=1)
            self.fc1 = i8ie.Linear(16 * 16, 64)
            self.fc2 = i8ie.Linear(64, 24)

        def forward(self, x):
            if with_conv:
                x = i8ie.relu(self.conv(x))
            return self.fc2(i8ie.relu(self.fc1(x.reshape(-1, 256))))

    net, rng = Net(), np.random.default_rng(17)
    for name, layer in net._layers():
        shape = (16, 16, 3, 3) if name == "conv" else ((64, 256) if name == "fc1" else (24, 64))
        layer.load_weight((rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))).astype(np.float32))
        layer.load_bias((rng.standard_normal(shape[0]) * 0.05).astype(np.float32))
    return net


def mlp_input(with_conv, batch=20, seed=2):
    x = np.random.default_rng(seed).uniform(-2, 2, (batch, 16, 4, 4)).astype(np.float32)
    return x if with_conv else x.reshape(batch, 256)


def converted(with_conv, weight_bits):
    import i8ie

    net = mlp(with_conv)
    net.prepare()
    net(i8ie.tensor(mlp_input(with_conv, seed=1)))
    net.convert(per_channel=True, weight_bits=weight_bits)
    return net


def test_graph_replay_and_save_load(tmp_path):
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    net, x = converted(False, 4), mlp_input(False)
    want = net(i8ie.tensor(x)).numpy()
    g = GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(3):
        assert support.same_bits(g().numpy(), want)
    state = net.quantized_state_dict()
    assert set(state) == {a + s for a in ("fc1", "fc2") for s in (".q_weight4", ".q_bias", ".qparams", ".w_scales")}
    assert state["fc1.q_weight4"].dtype == np.uint8 and state["fc1.q_weight4"].shape == (64, 128)
    path = str(tmp_path / "w4.npz")
    net.save_quantized(path)
    fresh = mlp(False)
    fresh.load_quantized_file(path)
    assert fresh.fc1.weight_bits() == 4 and np.array_equal(fresh.fc1.layer.q_weight(), net.fc1.layer.q_weight())
    assert support.same_bits(fresh(i8ie.tensor(x)).numpy(), want)


def test_a_second_convert_and_a_refused_load_keep_the_four_bit_state():
    """convert() on a converted layer returns early and a load_quantized with a wrong bias size is refused: the layer keeps
    computing with its 4-bit handle, so it must keep saying so"""
    import i8ie

    net, x = converted(False, 4), mlp_input(False)
    want, qw, state = net(i8ie.tensor(x)).numpy(), net.fc1.layer.q_weight(), net.quantized_state_dict()
    net.convert()
    net.fc1.convert(per_channel=True)
    with pytest.raises(RuntimeError):
        net.fc1.layer.load_quantized(np.zeros((64, 256), np.int8), np.zeros(3, np.int8), 0.5, 1.0, 0)
    assert net.fc1.weight_bits() == 4 and net.fc1.is_per_channel() and np.array_equal(net.fc1.layer.q_weight(), qw)
    again = net.quantized_state_dict()
    assert sorted(again) == sorted(state) and all(np.array_equal(again[k], state[k]) for k in state)
    assert support.same_bits(net(i8ie.tensor(x)).numpy(), want)
    net.fc1.layer.load_quantized(qw, net.fc1.layer.q_bias(), net.fc1.weight_scales(), *net.fc1.output_qparams())  # 8-bit weights do replace them
    assert net.fc1.weight_bits() == 8 and np.array_equal(net.fc1.layer.q_weight(), qw)
    assert support.same_bits(net(i8ie.tensor(x)).numpy(), want)


def test_module_convert_leaves_the_conv_alone():
    import i8ie

    x = mlp_input(True)
    maps = []
    for bits in (8, 4):
        net = converted(True, bits)
        assert [net.conv.weight_bits(), net.fc1.weight_bits(), net.fc2.weight_bits()] == [8, bits, bits]
        maps.append(support.counted_forward(lambda: net(i8ie.tensor(x)))[2])
    int8, w4 = maps
    assert w4.get("w4lin_mfma") == 2 and "w4lin_mfma" not in int8 and "w4lin_direct" not in int8
    others = {k: v for k, v in w4.items() if k != "w4lin_mfma"}
    assert others and all(int8.get(k, 0) >= v for k, v in others.items()), (int8, w4)
