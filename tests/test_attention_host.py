"""CPU-side checks of the quantized matmul / softmax definitions (tests/attention_ref.py against independent restatements),
of the host-only table entry i8ie_softmax_table, and of the Python surface.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import attention_ref as ar
import support
from support import i8ie  # noqa: F401

SCALES = [1.0 / 256, 0.01, 0.05, 0.3, 1.0, 0.0]


lib = support.lib_fixture(ar)


@pytest.mark.parametrize("s", SCALES)
def test_softmax_table_entry_equals_ref(lib, s):
    t = np.zeros(256, np.uint32)
    assert lib.i8ie_softmax_table(C.c_float(s), t.ctypes.data_as(C.c_void_p)) == 0
    want = ar.softmax_table(s)
    assert np.array_equal(t, want)
    assert t[0] == 65536 and (np.diff(t.astype(np.int64)) <= 0).all()


def test_softmax_table_argument_errors(lib):
    t = np.zeros(256, np.uint32)
    assert lib.i8ie_softmax_table(C.c_float(0.1), None) == -1
    for bad in (float("nan"), float("inf"), -0.5):
        assert lib.i8ie_softmax_table(C.c_float(bad), t.ctypes.data_as(C.c_void_p)) == -1


@pytest.mark.parametrize("L", [1, 2, 17, 64, 257, 1027])
def test_softmax_u8_within_derived_bound_of_float64(L):
    rng = np.random.default_rng(100 + L)
    for s in SCALES[:5]:
        x = rng.integers(0, 256, (6, L), dtype=np.uint8)
        x[1] = 77                      # an all-equal row
        x[2] = 0
        x[2, L // 2] = 255             # one dominant entry
        q = ar.softmax_u8(x, s)
        # (255 is the largest byte: 256 softmax above it is compared at 255, attention_ref.softmax_u8_bound)
        want = np.minimum(256.0 * ar.softmax(np.float64(np.float32(s)) * x.astype(np.float64)), 255.0)
        err = np.abs(q.astype(np.float64) - want).max()
        assert err <= ar.softmax_u8_bound(L), (L, s, err)
    assert (ar.softmax_u8(np.full((1, 1), 9, np.uint8), 0.3) == 255).all()   # L = 1: 256 clamps to 255


def _triple_loop(a, zp_a, b, zp_b):
    bb, m, k = a.shape
    n = b.shape[2]
    out = np.zeros((bb, m, n), np.int64)
    for t in range(bb):
        for i in range(m):
            for j in range(n):
                for kk in range(k):
                    out[t, i, j] += (int(a[t, i, kk]) - zp_a) * (int(b[t, kk, j]) - zp_b)
    return out


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
def test_matmul_u8_all_transpose_forms_against_triple_loop(orc, ta, tb):
    rng = np.random.default_rng(7)
    bb, m, n, k = 2, 3, 4, 5
    A = rng.integers(0, 256, (bb, m, k), dtype=np.uint8)
    B = rng.integers(0, 256, (bb, k, n), dtype=np.uint8)
    a = np.ascontiguousarray(A.transpose(0, 2, 1)) if ta else A
    b = np.ascontiguousarray(B.transpose(0, 2, 1)) if tb else B
    zp_a, zp_b = 13, 200
    acc = ar.matmul_acc(a, zp_a, b, zp_b, ta, tb)
    want = _triple_loop(A, zp_a, B, zp_b)
    assert np.array_equal(acc.astype(np.int64), want)
    for relu in (False, True):
        q = ar.matmul_u8(a, zp_a, 0.02, b, zp_b, 0.03, 0.9, 40, relu, ta, tb)
        w = orc.down_scale(want.astype(np.int32), 0.02, 0.03, 0.9, 40)
        assert np.array_equal(q, np.maximum(w, 40) if relu else w)
    assert ar.result_shape((2, 3, 2, 2), (2, 4, 4), False, False) == (2, 3, 2, 2)
    assert ar.result_shape((2, 3, 2, 2), (2, 4, 5), False, False) == (2, 3, 5)


def test_matmul_acc_extremes_fit_int32():
    a = np.full((1, 16, ar.MAX_K), 255, np.uint8)
    assert ar.matmul_acc(a, 0, a.transpose(0, 2, 1), 0).max() == 255 * 255 * ar.MAX_K < 2 ** 31
    z = np.zeros_like(a)
    assert ar.matmul_acc(z, 255, z.transpose(0, 2, 1), 255).max() == 255 * 255 * ar.MAX_K


def test_bmm_argument_errors_need_no_gpu(lib):
    """every argument error is I8IE_ERR_ARG before any device call (the ctx is never dereferenced)"""
    g = ar.BmmArgs(b=1, m=2, n=2, k=2, a=ar.mat(4096, 2, 2), bm=ar.mat(8192, 2, 2), out=ar.mat(12288, 2, 2),
                   s_a=1.0, s_b=1.0, s_out=1.0)
    assert lib.i8ie_bmm_u8(None, C.byref(g)) == -1
    fake_ctx = C.create_string_buffer(512)  # (never read: each call below fails its argument check first)
    for field, value in (("k", ar.MAX_K + 1), ("k", 0), ("s_out", 0.0), ("s_out", -1.0), ("s_a", float("inf")),
                         ("out_pix_axis", 3)):
        h = ar.BmmArgs.from_buffer_copy(g)
        setattr(h, field, value)
        assert lib.i8ie_bmm_u8(fake_ctx, C.byref(h)) == -1, field
    h = ar.BmmArgs.from_buffer_copy(g)
    h.a.row_stride, h.a.col_stride = 2, 2   # neither stride is 1
    assert lib.i8ie_bmm_u8(fake_ctx, C.byref(h)) == -1
    h = ar.BmmArgs.from_buffer_copy(g)
    h.out_pix_axis, h.out_h, h.out_w, h.out_border = 2, 3, 1, 1   # n != out_h * out_w
    assert lib.i8ie_bmm_u8(fake_ctx, C.byref(h)) == -1
    assert lib.i8ie_softmax_u8(fake_ctx, 4096, 4096, C.c_int64(1), 65536, C.c_float(0.1)) == -1
    assert lib.i8ie_softmax_u8(fake_ctx, 4096, 4096, C.c_int64(1), 0, C.c_float(0.1)) == -1
    assert lib.i8ie_softmax_u8(fake_ctx, 4096, 4096, C.c_int64(1), 8, C.c_float(float("nan"))) == -1


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    for n in ("MatMul", "matmul", "softmax"):
        assert n in i8ie.__all__ and hasattr(i8ie, n) and hasattr(cx, n)
    mm = i8ie.MatMul(transpose_b=True)
    assert isinstance(mm, i8ie.layer.Weightless) and (mm.transpose_a, mm.transpose_b) == (False, True)
    assert mm.output_qparams() == (1.0, 0) and not mm.layer.is_quantized()
    mm.layer.load_quantized(0.5, 3)
    assert mm.output_qparams() == (0.5, 3) and mm.layer.is_quantized()
    with pytest.raises(RuntimeError):
        mm.load_weight(np.zeros(1, np.float32))


def test_python_level_type_errors(i8ie):
    a = i8ie.tensor(np.zeros((1, 2, 3), np.float32))
    b = i8ie.tensor(np.zeros((1, 3, 2), np.float32))
    for kw in ({"scale": 1.0}, {"zero_point": 0}, {"scale": 1.0, "zero_point": 0}):
        with pytest.raises(TypeError):
            i8ie.matmul(a, b, **kw)


def test_module_saves_a_matmul_as_qparams_only(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.mm1 = i8ie.MatMul(transpose_a=True)

    net = Net()
    net.mm1.layer.load_quantized(0.25, 7)
    sd = net.quantized_state_dict()
    assert list(sd) == ["mm1.qparams"] and sd["mm1.qparams"].tolist() == [0.0, 0.25, 7.0]
    other = Net()
    other.load_quantized(sd)
    assert other.mm1.output_qparams() == (0.25, 7) and other.is_quant


# ---- the "tiny" non-local network: the reference composition alone, with the seeds the GPU test uses ------------------------
BLOCKS = ("a_", "b_")   # the prefixes of nonlocal_tiny's two blocks, in spec order


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_nonlocal_tiny_reference_discriminates(orc, batch, per_channel):
    import spec_ref as sr
    from int8inferenceengine_amd import workloads as wl

    name, entry = "nonlocal_tiny", wl.network("nonlocal_tiny")
    sd = wl.synthetic_state_dict(name, sr.WEIGHT_SEED)
    qp, jqp = sr.fp32_qparams(entry, sd, wl.synthetic_input(name, 8, seed=sr.CALIB_SEED))
    assert sorted(qp) == sorted(wl.layer_names(name)) and sorted(jqp) == sorted(wl.join_names(name))
    trace = {}
    x = wl.synthetic_input(name, batch, seed=sr.INPUT_SEED)
    logits = sr.forward(entry, x, sr.quantize_layers(entry, sd, per_channel), qp, jqp, per_channel, ar.tracer(trace))
    assert logits.shape == (batch, 10) and len(np.unique(logits)) > 1
    assert sorted(trace) == sorted(p + t for p in BLOCKS for t in ("scores", "softmax", "block"))
    assert trace["a_scores"].shape == (batch, 64, 64) and trace["b_scores"].shape == (batch, 16, 16)
    assert trace["a_block"].shape == (batch, 16, 8, 8) and trace["b_block"].shape == (batch, 20, 4, 4)
    for p in BLOCKS:
        assert len(np.unique(trace[p + "softmax"])) >= 16, p
        assert ((trace[p + "scores"] == 0) | (trace[p + "scores"] == 255)).mean() < 0.05, p


def test_nonlocal_configs_and_state_dict():
    from int8inferenceengine_amd import workloads as wl

    assert {"matmul", "softmax", "load"} <= wl.OPS and "nonlocal" not in wl.OPS
    L, spec, shape = wl.network("nonlocal_tiny")
    assert shape == (3, 32, 32) and list(L) == ["stem", "a_theta", "a_phi", "a_g", "a_out", "down", "b_theta", "b_phi", "b_g", "b_out", "fc"]
    assert L["b_theta"] == ("conv", 20, 12, 1, 1, 0) and L["down"] == ("conv", 16, 20, 3, 2, 1) and L["fc"] == ("fc", 20, 10)
    assert wl.op_names("nonlocal_tiny", "matmul") == ["a_mm1", "a_mm2", "b_mm1", "b_mm2"] and wl.add_names("nonlocal_tiny") == ["a_add", "b_add"]
    # by hand: stem 16x16 x 16 x 27; block A at 8x8: four 1x1 convs 16 <-> 16; down 4x4 x 20 x 144; block B at 4x4: four 1x1
    # convs 20 <-> 12; fc 200.  The products of the MatMuls are not counted.
    assert wl.macs_per_image("nonlocal_tiny") == 256 * 16 * 27 + 4 * 64 * 16 * 16 + 16 * 20 * 144 + 4 * 16 * 20 * 12 + 200 == 237768
    C, cspec, _ = wl.network("nonlocal_resnet_cifar")
    R, rspec, _ = wl.network("resnet18_cifar")
    assert C["nl_theta"] == ("conv", 256, 128, 1, 1, 0) and C["nl_out"] == ("conv", 128, 256, 1, 1, 0)
    assert set(C) - set(R) == {"nl_theta", "nl_phi", "nl_g", "nl_out"} and {a: C[a] for a in R} == R
    assert list(C)[list(C).index("s4b1c1") - 4:list(C).index("s4b1c1")] == ["nl_theta", "nl_phi", "nl_g", "nl_out"]
    # the block and its relu sit where stage 3 has ended, and nothing else of resnet18_cifar's spec moved
    cut, block = rspec.index(("save", "s4b1")), wl.network("nonlocal_tiny")[1][3:14]
    assert cspec.index(("add", "nl_add", "nl_x")) == cspec.index(("save", "s4b1")) - 2 and cspec[cspec.index(("save", "s4b1")) - 1] == ("relu",)
    assert cspec[:cut] == rspec[:cut] and cspec[cut + len(block) + 1:] == rspec[cut:] and cspec[cut] == ("save", "nl_x")
    assert [op[0] for op in cspec[cut:cut + len(block)]] == [op[0] for op in block]
    # by hand: every weighted layer of resnet18_cifar (its pinned figure leaves the three 1x1 projections out: 3 x 2097152)
    # and the block's four 1x1 convs 256 <-> 128 at 8x8
    assert wl.macs_per_image("nonlocal_resnet_cifar") == 549131264 + 3 * 2097152 + 4 * 64 * 256 * 128 == 563811328
    a, b = wl.synthetic_state_dict("nonlocal_tiny", 3), wl.synthetic_state_dict("nonlocal_tiny", 3)
    assert sorted(a) == sorted(k + s for k in L for s in (".weight", ".bias"))
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["a_theta.weight"].shape == (16, 16, 1, 1)
    assert wl.FOLDS["nonlocal_tiny"] == {"a_theta": 1 / np.sqrt(16), "b_theta": 1 / np.sqrt(12)} and wl.FOLDS["nonlocal_resnet_cifar"] == {"nl_theta": 1 / np.sqrt(128)}
    net = wl.build("nonlocal_tiny")
    assert type(net).__name__ == "SpecNet_nonlocal_tiny"
    assert [k for k, _ in net._layers()] == wl.join_names("nonlocal_tiny") + wl.layer_names("nonlocal_tiny")
    assert wl.join_names("nonlocal_tiny") == ["a_mm1", "a_mm2", "a_add", "b_mm1", "b_mm2", "b_add"] and wl.layer_names("nonlocal_tiny") == list(L)
    assert (net.a_mm1.transpose_a, net.a_mm1.transpose_b, net.b_mm2.transpose_a, net.b_mm2.transpose_b) == (True, False, False, True)
