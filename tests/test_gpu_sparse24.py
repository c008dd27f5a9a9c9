"""2:4 structured-sparse weights for Linear on the GPU (csrc/i8ie_sp24lin.hip): sp24lin_mfma and sp24lin_direct bit for bit against
the oracle's bytes and INT32 accumulators on the pruned dense integers (orc.linear per tensor, tests/pc_pipeline.py per channel),
at the shapes where the kernels change path, and the Python surface: the INT8 witness, save / load, graph replay."""
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
# the six position pairs (first < second) of a group of four
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
# K: one instruction (128), a zero tail inside a 128-step (160), the chunk edge (512) and a tail past it (544).  DEEP: the
# few-row instance has the deepest LDS ring, 8 stages of one 512-value chunk; 16 chunks make every stage of it (and of the 3-
# and 2-stage instances) load twice
DEEP = 512 * 2 * 8


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def pruned(qw):
    out = np.empty_like(qw)
    abi.ck(abi.lib().i8ie_prune_2_4(ptr(qw), qw.shape[0], qw.shape[1], ptr(out)))
    return out


def pattern(n, k):
    """group g of feature j keeps pair (g + j) % 6; the kept values are distinct within every run of 62 groups"""
    qw = np.zeros((n, -(-k // 4), 4), np.int8)
    for j in range(n):
        for g in range(qw.shape[1]):
            a, b = PAIRS[(g + j) % 6]
            qw[j, g, a], qw[j, g, b] = 1 + 2 * (g % 62), -2 - 2 * (g % 62)
    return qw.reshape(n, -1)[:, :k].copy()


def extremes(n, k):
    """every group keeps -128 and 127 (which two positions varies), so with activations 0 / 255 the sums reach the range's ends"""
    qw = pattern(n, k)
    return np.where(qw > 0, 127, np.where(qw < 0, -128, 0)).astype(np.int8)


def expected(q, qw, qb, zp_in, s_w, s_out):
    """(bytes, accumulators) of the oracle on dense integers; s_w: a scalar (per tensor) or one per feature"""
    if np.ndim(s_w):
        want, a0, _ = pcp.linear_pc(q, qw, qb, S_IN, zp_in, s_w, s_out, ZP_OUT)
    else:
        want, a0, _ = orc.linear(q, qw, qb, S_IN, zp_in, s_w, s_out, ZP_OUT, want_acc=True)
    return want, a0


class Sp24:
    """a handle of i8ie_linear_create_sp24(_per_channel) from dense 2:4 integers, and its forwards on host arrays"""

    def __init__(self, ctx, qw, qb, s_w, s_out):
        self.ctx, (self.n, k), self.L = ctx, qw.shape, C.c_void_p()
        g = -(-k // 4)
        values, index = np.empty((self.n, 2 * g), np.int8), np.empty((self.n, (g + 1) // 2), np.uint8)
        abi.ck(abi.lib().i8ie_pack_2_4(ptr(qw), self.n, k, ptr(values), ptr(index)))
        if np.ndim(s_w):
            abi.ck(abi.lib().i8ie_linear_create_sp24_per_channel(ctx.h, ptr(values), ptr(index), ptr(qb), self.n, k, ptr(s_w), C.byref(self.L)))
        else:
            abi.ck(abi.lib().i8ie_linear_create_sp24(ctx.h, ptr(values), ptr(index), ptr(qb), self.n, k, C.c_float(s_w), C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(s_out), C.c_uint8(ZP_OUT)))

    def forward(self, q, zp_in, relu=False, hw=(0, 0), fallback=False):
        """(out, acc, {kernel: launches}) without the handle's one-off vectors kernel"""
        m = q.shape[0]
        buf, out, acc = self.ctx.put(q), self.ctx.empty((m, self.n), np.uint8), self.ctx.empty((m, self.n), np.int32)
        self.ctx.set_force_fallback(fallback)
        try:
            with self.ctx.launch_map() as names:
                abi.ck(abi.lib().i8ie_layer_forward_fused(self.L, buf.ptr, 1 if hw[0] else 0, 0, m, hw[0], hw[1], C.c_float(S_IN),
                                                          C.c_uint8(zp_in), int(relu), out.ptr, 0, 0, acc.ptr))
        finally:
            self.ctx.set_force_fallback(False)
        res = (out.get(), acc.get(), {k: v for k, v in names.items() if k != "sp24_offsets"})
        for b in (buf, out, acc):
            b.free()
        return res

    def close(self):
        abi.lib().i8ie_layer_destroy(self.L)


def check(ctx, q, qw, qb, s_w, zp_in, kernel, hw=(0, 0), flat=None):
    """one layer against the oracle: the route under test with a fused relu, then the definition kernel under force-fallback"""
    k = qw.shape[1]
    s_out = s_out_for(S_IN, np.atleast_1d(s_w), k)
    want, a0 = expected(q, qw, qb, zp_in, s_w, s_out)
    h = Sp24(ctx, qw, qb, s_w, s_out)
    try:
        got, acc, names = h.forward(q if flat is None else flat, zp_in, relu=True, hw=hw)
        assert names == {kernel: 1}, names
        assert np.array_equal(acc, a0) and np.array_equal(got, np.maximum(want, np.uint8(ZP_OUT))), (q.shape, qw.shape, kernel)
        got, acc, names = h.forward(q if flat is None else flat, zp_in, hw=hw, fallback=True)
        assert names == {"sp24lin_direct": 1} and np.array_equal(acc, a0) and np.array_equal(got, want), (q.shape, qw.shape, "fallback")
    finally:
        h.close()


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("m", [1, 16, 17, 65, 130])
@pytest.mark.parametrize("k", [128, 160, 512, 544, DEEP, 100])
def test_parity_with_the_oracle(ctx, m, k, per_channel):
    rng = np.random.default_rng(1000 * m + k)
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)
    for n, zp_in in ((16, 0), (20, 128), (33, 255)):
        qw = pruned(rng.integers(-128, 128, (n, k), dtype=np.int8))
        s_w = row_scales(n, rng) if per_channel else np.float32(2e-3)
        check(ctx, q, qw, rng.integers(-127, 128, n, dtype=np.int8), s_w, zp_in, "sp24lin_mfma" if k % 32 == 0 else "sp24lin_direct")


@pytest.mark.parametrize("m,n", [(16, 33), (65, 20), (130, 33)])
def test_every_position_pair_in_every_group_slot_and_the_extremes(ctx, m, n):
    """pattern: a wrong pairing of value, position and activation byte cannot cancel; extremes: -128 / 127 against 0 / 255"""
    rng = np.random.default_rng(m)
    qb, s_w = rng.integers(-127, 128, n, dtype=np.int8), row_scales(n, rng)
    check(ctx, rng.integers(0, 256, (m, 544), dtype=np.uint8), pattern(n, 544), qb, s_w, 7, "sp24lin_mfma")
    q = np.where(rng.integers(0, 2, (m, DEEP)) == 1, 255, 0).astype(np.uint8)
    q[0], q[-1] = 255, 0
    check(ctx, q, extremes(n, DEEP), qb, s_w, 128, "sp24lin_mfma")


def test_nhwc_flattened_rows_take_the_definition_kernel(ctx):
    """rows that are a flattened NHWC activation (c = 32, h * w = 4) walk K in (h, w, c) order: sp24lin_direct, although K % 32 == 0"""
    rng = np.random.default_rng(3)
    m, c, hh, ww, n = 33, 32, 2, 2, 24
    q = rng.integers(0, 256, (m, c * hh * ww), dtype=np.uint8)
    flat = np.ascontiguousarray(q.reshape(m, c, hh, ww).transpose(0, 2, 3, 1)).reshape(m, -1)
    check(ctx, q, pruned(rng.integers(-128, 128, (n, c * hh * ww), dtype=np.int8)), rng.integers(-127, 128, n, dtype=np.int8),
          row_scales(n, rng), 121, "sp24lin_direct", hw=(hh, ww), flat=flat)


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def u8_tensor(q):
    """an i8ie u8 tensor holding q with scale 1, zero point 0 (x / 1 + 0 truncates to x exactly)"""
    import _CXX_i8ie as cx
    import i8ie

    return i8ie.Tensor(cx.quantize(cx.tensor(np.asarray(q, np.float32)), 1.0, 0))


@pytest.mark.parametrize("per_channel", [False, True])
def test_int8_witness_save_load_and_graph_replay(per_channel):
    """convert(sparsity="2:4") holds the quantiser's integers pruned, gives the oracle's bytes, and so does an ordinary INT8
    Linear loaded with them; the compressed state restores the same layer; a captured graph replays the same bytes"""
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    rng = np.random.default_rng(5)
    m, k, n = 70, 320, 48
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    q = rng.integers(0, 256, (m, k), dtype=np.uint8)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.fc = i8ie.Linear(k, n)

        def forward(self, x):
            return self.fc(x)

    net, dense = Net(), i8ie.Linear(k, n)
    for lin in (net.fc, dense):
        lin.load_weight(w)
        lin.load_bias(b)
        lin.set_output_qparams(0.5, 100)
    dense.convert(per_channel=per_channel)
    net.convert(per_channel=per_channel, sparsity="2:4")
    qw, qb, s_w = pruned(dense.layer.q_weight()), dense.layer.q_bias(), dense.weight_scales()
    assert net.fc.sparsity() == "2:4" and dense.sparsity() is None and net.fc.is_per_channel() == per_channel
    assert np.array_equal(net.fc.layer.q_weight(), qw) and np.array_equal(net.fc.layer.q_bias(), qb) and np.array_equal(net.fc.weight_scales(), s_w)
    want = expected_at(q, qw, qb, s_w if per_channel else s_w[0])
    got, _, launches = support.counted_forward(lambda: net.fc(u8_tensor(q)))
    assert launches.get("sp24lin_mfma") == 1 and np.array_equal(got, want)
    witness = i8ie.Linear(k, n)
    witness.load_quantized(qw, qb, s_w if per_channel else float(s_w[0]), 0.5, 100)
    assert witness.sparsity() is None and np.array_equal(witness(u8_tensor(q)).numpy(), want)
    witness.load_quantized(qw, qb, s_w if per_channel else float(s_w[0]), 0.5, 100, sparsity="2:4")   # the same layer, dense integers in
    assert witness.sparsity() == "2:4" and np.array_equal(witness(u8_tensor(q)).numpy(), want)
    state = net.quantized_state_dict()
    assert set(state) == {"fc" + s for s in (".q_weight24", ".q_index24", ".q_bias", ".qparams") + ((".w_scales",) if per_channel else ())}
    assert state["fc.q_weight24"].shape == (n, k // 2) and state["fc.q_index24"].shape == (n, k // 8)
    fresh = Net()
    fresh.load_quantized(state)
    assert fresh.fc.sparsity() == "2:4" and np.array_equal(fresh.fc.layer.q_weight(), qw)
    assert np.array_equal(fresh.fc(u8_tensor(q)).numpy(), want)
    g = GraphedForward(fresh.fc, u8_tensor(q).prefetch())
    for _ in range(3):
        assert np.array_equal(g().numpy(), want)
    fresh.fc.layer.load_quantized(qw, qb, s_w if per_channel else float(s_w[0]), 0.5, 100)   # dense weights do replace the panel
    assert fresh.fc.sparsity() is None and np.array_equal(fresh.fc(u8_tensor(q)).numpy(), want)


def expected_at(q, qw, qb, s_w):
    """the oracle's bytes for input (scale 1, zero point 0) and output (0.5, 100)"""
    if np.ndim(s_w):
        return pcp.linear_pc(q, qw, qb, np.float32(1), 0, s_w, np.float32(0.5), 100)[0]
    return orc.linear(q, qw, qb, np.float32(1), 0, s_w, np.float32(0.5), 100, want_acc=True)[0]
