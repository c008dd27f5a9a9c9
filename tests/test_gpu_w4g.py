"""4-bit weights with group-wise scales along K on the GPU (csrc/i8ie_w4glin.hip): w4glin_mfma and w4glin_direct bit for bit --
accumulators and bytes -- against the restatement of tests/w4g_ref.py (the per-channel Linear on W_eff = m * q), at every group
size, at the K where a group is smaller than gs, partial, ends at a chunk edge or one past it, through the LDS ring's wrap, at
the INT32 bound, and through the Python surface."""
import ctypes as C

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import orc
from requant_ref import row_scales, s_out_for
import support
import w4g_ref

pytestmark = pytest.mark.gpu
ctx = support.ctx_fixture()
S_IN, ZP_OUT = np.float32(0.02), 61


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(q):
    packed = np.empty((q.shape[0], (q.shape[1] + 1) // 2), np.uint8)
    abi.ck(abi.lib().i8ie_pack_w4(ptr(q), q.shape[0], q.shape[1], ptr(packed)))
    return packed


def weights(n, k, gs, rng):
    """random nibbles behind rows of all -8, all 7 and -8 / 7 alternating; the multipliers alternate 1 / 32 between neighbouring
    groups and neighbouring features, so a wrong group or lane index changes the sum"""
    q = rng.integers(-8, 8, (n, k), dtype=np.int8)
    alt = np.where(np.arange(k) % 2 == 0, -8, 7).astype(np.int8)
    for j, row in enumerate((np.full(k, -8), np.full(k, 7), alt, -1 - alt)[:n]):
        q[j] = row
    m = np.where((np.arange(n)[:, None] + np.arange(w4g_ref.groups(k, gs))[None, :]) % 2 == 0, 1, 32).astype(np.uint8)
    return q, m, rng.integers(-127, 128, n, dtype=np.int8), row_scales(n, rng)


class W4G:
    """a handle of i8ie_linear_create_w4g and its forwards on host arrays"""

    def __init__(self, ctx, q, m, qb, s_w, gs, s_out):
        self.ctx, (self.n, self.k), self.L = ctx, q.shape, C.c_void_p()
        abi.ck(abi.lib().i8ie_linear_create_w4g(ctx.h, ptr(pack(q)), ptr(m), ptr(qb), ptr(s_w), self.n, self.k, gs, C.byref(self.L)))
        abi.ck(abi.lib().i8ie_layer_set_output_qparams(self.L, C.c_float(s_out), C.c_uint8(ZP_OUT)))
        bits, size = C.c_int(), C.c_int()
        abi.ck(abi.lib().i8ie_layer_weight_bits(self.L, C.byref(bits)))
        abi.ck(abi.lib().i8ie_layer_group_size(self.L, C.byref(size)))
        assert (bits.value, size.value) == (4, gs)

    def forward(self, x, zp_in, relu=False, shift=0, hw=(0, 0), dequant=False):
        """(out, acc, {kernel: launches}) without the one-off w4g_offsets; shift: bytes the input lies past a 16-byte boundary"""
        rows = x.shape[0]
        buf = self.ctx.put(np.concatenate([np.zeros(shift, np.uint8), x.ravel()]))
        out, acc, f = (self.ctx.empty((rows, self.n), t) for t in (np.uint8, np.int32, np.float32))
        src = C.c_void_p(buf.ptr.value + shift)
        with self.ctx.launch_map() as names:
            if dequant:
                abi.ck(abi.lib().i8ie_layer_forward_dequant(self.L, src, 0, rows, 0, 0, C.c_float(S_IN), C.c_uint8(zp_in), int(relu), out.ptr, f.ptr))
            else:
                abi.ck(abi.lib().i8ie_layer_forward_fused(self.L, src, 1 if hw[0] else 0, 0, rows, hw[0], hw[1], C.c_float(S_IN),
                                                          C.c_uint8(zp_in), int(relu), out.ptr, 0, 0, acc.ptr))
        res = (f.get() if dequant else out.get(), acc.get(), {k: v for k, v in names.items() if k != "w4g_offsets"})
        for b in (buf, out, acc, f):
            b.free()
        return res

    def close(self):
        abi.lib().i8ie_layer_destroy(self.L)


def u8s4g(ctx, x, q, m, qb, s_w, gs, zp_in, s_out):
    """the stateless entry: (out, acc)"""
    (rows, k), n = x.shape, q.shape[0]
    di, out, acc = ctx.put(x), ctx.empty((rows, n), np.uint8), ctx.empty((rows, n), np.int32)
    abi.ck(abi.lib().i8ie_linear_u8s4g(ctx.h, di.ptr, rows, k, ptr(pack(q)), ptr(m), ptr(qb), ptr(s_w), n, gs, C.c_float(S_IN),
                                       C.c_uint8(zp_in), C.c_float(s_out), C.c_uint8(ZP_OUT), out.ptr, acc.ptr))
    res = out.get(), acc.get()
    for b in (di, out, acc):
        b.free()
    return res


def check_forms(ctx, x, q, m, qb, s_w, gs, zp_in, forms=True):
    """stateless and handle (relu folded) on the expected kernel; with `forms` also the shifted input and force-fallback (direct)"""
    k = x.shape[1]
    kernel = "w4glin_mfma" if k % 32 == 0 else "w4glin_direct"
    s_out = s_out_for(S_IN, s_w * np.float32(16), k)  # (|W_eff| averages 16 times a nibble)
    want, a0 = w4g_ref.linear_w4g(x, q, m, qb, gs, S_IN, zp_in, s_w, s_out, ZP_OUT)
    tag = (x.shape, q.shape[0], gs)
    got, acc = u8s4g(ctx, x, q, m, qb, s_w, gs, zp_in, s_out)
    assert np.array_equal(acc, a0) and np.array_equal(got, want), (tag, "stateless")
    h = W4G(ctx, q, m, qb, s_w, gs, s_out)
    try:
        got, acc, names = h.forward(x, zp_in, relu=True)
        assert names == {kernel: 1}, names
        assert np.array_equal(acc, a0) and np.array_equal(got, np.maximum(want, np.uint8(ZP_OUT))), (tag, "relu")
        if forms:
            got, _, names = h.forward(x, zp_in, shift=1)
            assert names == {"w4glin_direct": 1} and np.array_equal(got, want), (tag, "unaligned")
            ctx.set_force_fallback(True)
            try:
                got, acc, names = h.forward(x, zp_in)
            finally:
                ctx.set_force_fallback(False)
            assert names == {"w4glin_direct": 1} and np.array_equal(acc, a0) and np.array_equal(got, want), (tag, "fallback")
    finally:
        h.close()


# K: a group smaller than gs (64 at 128 / 256, 96), a partial last group (96, 288, 544), a group that ends at the chunk edge and one
# past it (288, 544), no multiple of 32 (40: the direct kernel).  DEEP: the ring takes a stage again (9 chunks for the 8 stages
# of the few-row shape, 4 for the 3 of the many-row shape)
@pytest.mark.parametrize("gs", [64, 128, 256])
@pytest.mark.parametrize("rows,k", [(r, k) for r in (1, 16, 17, 129) for k in (64, 96, 288, 544, 40)])
def test_parity_with_the_restatement(ctx, gs, rows, k):
    rng = np.random.default_rng(100000 * gs + 1000 * rows + k)
    x = rng.integers(0, 256, (rows, k), dtype=np.uint8)
    for n, zp_in in ((1, 0), (16, 128), (17, 255), (40, 128)):
        check_forms(ctx, x, *weights(n, k, gs, rng), gs, zp_in)


@pytest.mark.parametrize("rows,k", [(1, 2304), (16, 2304), (17, 1024), (129, 1024)])
def test_the_ring_wraps(ctx, rows, k):
    rng = np.random.default_rng(rows + k)
    check_forms(ctx, rng.integers(0, 256, (rows, k), dtype=np.uint8), *weights(40, k, 128, rng), 128, 7, forms=False)


@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("byte,zp_in", [(255, 0), (0, 255)])
def test_the_int32_bound(ctx, rows, byte, zp_in):
    """K = 32768, every W_eff = -256: |C| = 255 * 256 * 32768 = 2^31 - 8388608, exact (no bias: (float)C + b could round to 2^31)"""
    n, k = 16, 32768
    q, m = np.full((n, k), -8, np.int8), np.full((n, k // 128), 32, np.uint8)
    x = np.full((rows, k), byte, np.uint8)
    want, a0 = w4g_ref.linear_w4g(x, q, m, np.zeros(n, np.int8), 128, S_IN, zp_in, np.full(n, 1e-6, np.float32), np.float32(1), ZP_OUT)
    assert np.abs(a0.astype(np.int64)).max() == 255 * 256 * 32768
    got, acc = u8s4g(ctx, x, q, m, np.zeros(n, np.int8), np.full(n, 1e-6, np.float32), 128, zp_in, np.float32(1))
    assert np.array_equal(acc, a0) and np.array_equal(got, want)


def test_nhwc_flattened_rows_and_dequant(ctx):
    """rows that are a flattened NHWC map (c = 16, h * w = 4) run w4glin_direct although K % 32 == 0; forward_dequant"""
    rng = np.random.default_rng(3)
    rows, c, hh, ww, n, zp_in, gs = 33, 16, 2, 2, 24, 121, 64
    k = c * hh * ww
    x = rng.integers(0, 256, (rows, k), dtype=np.uint8)
    q, m, qb, s_w = weights(n, k, gs, rng)
    s_out = s_out_for(S_IN, s_w * np.float32(16), k)
    want, a0 = w4g_ref.linear_w4g(x, q, m, qb, gs, S_IN, zp_in, s_w, s_out, ZP_OUT)
    flat = np.ascontiguousarray(x.reshape(rows, c, hh, ww).transpose(0, 2, 3, 1)).reshape(rows, k)
    h = W4G(ctx, q, m, qb, s_w, gs, s_out)
    try:
        got, acc, names = h.forward(flat, zp_in, hw=(hh, ww))
        assert names == {"w4glin_direct": 1} and np.array_equal(acc, a0) and np.array_equal(got, want)
        got, _, names = h.forward(x, zp_in, dequant=True)
        assert names.get("w4glin_mfma") == 1 and len(names) == 2, names
        assert support.same_bits(got, orc.dequantize(want, s_out, ZP_OUT))
    finally:
        h.close()


def test_module_surface_save_load_and_graph(tmp_path):
    """a two-layer Module under convert(weight_bits=4, group_size=128): the restatement's bytes, what the layers report, the
    state dict and its round trip, and a HIP graph replay"""
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd.graph import GraphedForward

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = i8ie.Linear(288, 64)
            self.fc2 = i8ie.Linear(64, 24)

        def forward(self, x):
            return self.fc2(i8ie.relu(self.fc1(x)))

    rng = np.random.default_rng(17)
    params = {a: ((rng.standard_t(2, s) * 0.02).astype(np.float32), (rng.standard_normal(s[0]) * 0.05).astype(np.float32))
              for a, s in (("fc1", (64, 288)), ("fc2", (24, 64)))}   # (heavy-tailed rows: the groups get different multipliers)
    qp = {"fc1": (np.float32(0.05), 30), "fc2": (np.float32(0.1), 128)}

    def fresh():
        net = Net()
        for a, (w, b) in params.items():
            getattr(net, a).load_weight(w)
            getattr(net, a).load_bias(b)
            getattr(net, a).set_output_qparams(*qp[a])
        return net

    net = fresh()
    net.convert(weight_bits=4, group_size=128)
    x = rng.integers(0, 256, (20, 288), dtype=np.uint8)
    want, s, zp = x, np.float32(1), 0
    for a in ("fc1", "fc2"):
        layer, (q, m, qb, s_w) = getattr(net, a), w4g_ref.quantize_w4g(*params[a], 128)
        assert (layer.group_size(), layer.weight_bits(), layer.is_per_channel()) == (128, 4, True)
        assert np.array_equal(layer.group_scales(), m) and np.array_equal(layer.layer.q_weight(), q)
        assert np.array_equal(layer.layer.q_bias(), qb) and np.array_equal(layer.weight_scales(), s_w)
        want, _ = w4g_ref.linear_w4g(want, q, m, qb, 128, s, zp, s_w, *qp[a])
        s, zp = qp[a]
        if a == "fc1":
            want = np.maximum(want, np.uint8(zp))
    assert len(np.unique(net.fc1.group_scales())) > 4
    tensor = i8ie.Tensor(cx.quantize(cx.tensor(x.astype(np.float32)), 1.0, 0))   # (x / 1 + 0 truncates to x exactly)
    got, _, launches = support.counted_forward(lambda: net.forward(tensor))
    assert launches.get("w4glin_mfma") == 2 and np.array_equal(got, want)

    xf = rng.uniform(-2, 2, (20, 288)).astype(np.float32)
    eager = net(i8ie.tensor(xf)).numpy()
    g = GraphedForward(net, i8ie.tensor(xf).prefetch())
    for _ in range(3):
        assert support.same_bits(g().numpy(), eager)
    state = net.quantized_state_dict()
    assert set(state) == {a + k for a in ("fc1", "fc2") for k in (".q_weight4", ".q_group_scales", ".group_size", ".q_bias", ".qparams", ".w_scales")}
    assert state["fc1.q_group_scales"].shape == (64, 3) and state["fc1.q_group_scales"].dtype == np.uint8
    assert state["fc1.group_size"].dtype == np.int32 and list(state["fc1.group_size"]) == [128]
    path = str(tmp_path / "w4g.npz")
    net.save_quantized(path)
    back = fresh()
    back.load_quantized_file(path)
    assert back.fc1.group_size() == 128 and np.array_equal(back.fc1.group_scales(), net.fc1.group_scales())
    assert support.same_bits(back(i8ie.tensor(xf)).numpy(), eager)
