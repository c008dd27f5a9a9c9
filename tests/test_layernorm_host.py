"""CPU-side checks of the quantized LayerNorm: the surface and the C-ABI's argument rules, the host-only entry
i8ie_layernorm_affine against the numpy restatement (tests/layernorm_ref.py), the restatement against
torch.nn.functional.layer_norm in float64 within the bound derived in include/i8ie_hip.h, the statistics extremes, and the
module state machine.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
import layernorm_ref as lr
import support
from support import i8ie  # noqa: F401

f32 = np.float32
ENTRIES = ["i8ie_layernorm_affine", "i8ie_layernorm_u8", "i8ie_layernorm_u8_nhwc", "i8ie_layernorm_f32"]
# (s_in, zp_in, s_out, zp_out, eps)
QSETS = [(0.025, 127, 0.02, 128, 1e-5), (0.1, 0, 0.05, 100, 1e-6), (0.004, 255, 0.011, 0, 1e-3), (1.7, 13, 0.03, 255, 1e-5)]


lib = support.lib_fixture(lr)


def test_abi_symbols_declared_and_exported(lib):
    declared = abi.declared_symbols()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name), name


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    for n in ("LayerNorm", "layer_norm"):
        assert n in i8ie.__all__ and hasattr(i8ie, n) and hasattr(cx, n)
    ln = i8ie.LayerNorm(20)
    assert isinstance(ln, i8ie.Layer) and not isinstance(ln, i8ie.layer.Weightless)
    assert (ln.channels, ln.eps) == (20, 1e-5) and ln.output_qparams() == (1.0, 0)
    assert not ln.is_per_channel() and not ln.layer.is_quantized()
    assert np.array_equal(ln.layer.weight(), np.ones(20, f32)) and np.array_equal(ln.layer.bias(), np.zeros(20, f32))
    for call in (ln.weight_scale, ln.weight_scales, ln.q_weight, ln.q_bias, lambda: ln.forward_debug(None)):
        with pytest.raises(RuntimeError, match="LayerNorm"):
            call()
    for bad in (0, 16385):
        with pytest.raises(RuntimeError):
            i8ie.LayerNorm(bad)
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            i8ie.LayerNorm(4, eps=bad)
    with pytest.raises(RuntimeError):
        ln.load_weight(np.ones(19, f32))
    with pytest.raises(RuntimeError):
        ln.load_bias(np.ones((20, 1), f32))


def test_python_level_type_errors(i8ie):
    x = i8ie.tensor(np.zeros((2, 8), f32))
    for kw in ({"scale": 1.0}, {"zero_point": 0}, {"scale": 1.0, "zero_point": 0}):
        with pytest.raises(TypeError):
            i8ie.layer_norm(x, **kw)


def test_argument_errors_need_no_gpu(lib):
    """every argument error is I8IE_ERR_ARG with a message before any device call (the ctx is never dereferenced)"""
    fake = C.create_string_buffer(512)
    p = 4096   # (never dereferenced either)

    def flat(ctx=fake, i=p, o=p, rows=4, Cn=16, g=p, b=p, s_in=0.1, eps=1e-5):
        return lib.i8ie_layernorm_u8(ctx, i, o, rows, Cn, g, b, s_in, eps, 0, 0)

    def nhwc(ctx=fake, i=p, ib=0, o=p, ob=0, n=1, Cn=16, h=2, w=2, g=p, b=p, s_in=0.1, eps=1e-5):
        return lib.i8ie_layernorm_u8_nhwc(ctx, i, ib, 0, o, ob, 0, n, Cn, h, w, g, b, s_in, eps, 0, 0)

    def fp(ctx=fake, i=p, o=p, rows=4, Cn=16, g=p, b=p, eps=1e-5, inner=1):
        return lib.i8ie_layernorm_f32(ctx, i, o, rows, Cn, g, b, eps, inner)

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(i=None), dict(o=None), dict(g=None), dict(b=None), dict(Cn=0), dict(Cn=16385), dict(Cn=-3),
           dict(eps=0.0), dict(eps=-1e-5), dict(eps=nan), dict(eps=inf)]
    for kw in bad + [dict(s_in=0.0), dict(s_in=-0.1), dict(s_in=nan), dict(s_in=inf), dict(rows=0), dict(rows=2 ** 31), dict(g=p + 2)]:
        assert flat(**kw) == -1, kw
        msg = abi.lib().i8ie_last_error().decode()
        assert "i8ie_layernorm_u8" in msg, (kw, msg)
    for kw in bad + [dict(s_in=0.0), dict(s_in=nan), dict(ib=-1), dict(ob=-1), dict(n=0), dict(h=0), dict(w=-2)]:
        assert nhwc(**kw) == -1, kw
        assert "i8ie_layernorm_u8_nhwc" in abi.lib().i8ie_last_error().decode(), kw
    for kw in bad + [dict(rows=0), dict(inner=0), dict(inner=3)]:
        assert fp(**kw) == -1, kw
        assert "i8ie_layernorm_f32" in abi.lib().i8ie_last_error().decode(), kw
    assert "16384" in (flat(Cn=16385), abi.lib().i8ie_last_error().decode())[1]
    # eps so small against s_in^2 that E leaves the doubles' range for 1 / sqrt in fp32
    assert flat(s_in=1e30, eps=1e-38) == -1
    # the host-only entry
    ones = np.ones(4, f32)
    assert lr.affine_entry(lib, ones, ones, 0.5, 3)[0] == 0
    for s in (0.0, -1.0, nan, inf):
        assert lr.affine_entry(lib, ones, ones, s, 3)[0] == -1
    assert lib.i8ie_layernorm_affine(None, ones.ctypes.data, 4, 0.5, 3, ones.ctypes.data, ones.ctypes.data) == -1
    assert lib.i8ie_layernorm_affine(ones.ctypes.data, ones.ctypes.data, 0, 0.5, 3, ones.ctypes.data, ones.ctypes.data) == -1
    assert lr.affine_entry(lib, np.array([nan, 1, 1, 1], f32), ones, 0.5, 3)[0] == -1
    assert lr.affine_entry(lib, np.array([3e38, 1, 1, 1], f32), ones, 0.5, 3)[0] == -1   # gamma / s_out overflows


@pytest.mark.parametrize("zp_out", [0, 1, 128, 255])
@pytest.mark.parametrize("s_out", [0.02, 0.3, 1.0, 3.7e-3])
def test_affine_entry_equals_ref_bit_for_bit(lib, s_out, zp_out):
    rng = np.random.default_rng(int(zp_out * 1000 + s_out * 1e4))
    for Cn in (1, 17, 1024):
        gamma = rng.normal(1.0, 0.7, Cn).astype(f32)
        beta = rng.normal(0.0, 0.5, Cn).astype(f32)
        gamma[0] = 0.0
        if Cn > 2:
            gamma[1], beta[2] = -1.25, -0.0
        rc, g, b = lr.affine_entry(lib, gamma, beta, s_out, zp_out)
        wg, wb = lr.affine(gamma, beta, s_out, zp_out)
        assert rc == 0 and np.array_equal(g.view(np.uint32), wg.view(np.uint32)) and np.array_equal(b.view(np.uint32), wb.view(np.uint32))
        assert g[0] == 0.0 and (Cn < 3 or g[1] < 0)


@pytest.mark.parametrize("Cn", [1, 2, 17, 96, 1024, 16384])
def test_ref_against_torch_float64_within_derived_bound(Cn):
    """|v - y*| <= B(y*) everywhere; the byte equals clamp(trunc(y*)) wherever y* is further than B from an integer; fewer than
    1 % of the bytes fall under that exclusion"""
    rng = np.random.default_rng(300 + Cn)
    rows = 64 if Cn <= 1024 else 6
    total = excluded = 0
    spread = set()
    for s_in, zp_in, s_out, zp_out, eps in QSETS:
        a = rng.integers(0, 256, (rows, Cn), dtype=np.uint8)
        a[1] = (rng.integers(0, 12, Cn) + 100).astype(np.uint8)   # a narrow row: small V
        gamma = rng.normal(1.0, 0.6, Cn).astype(f32)
        beta = rng.normal(0.0, 0.6, Cn).astype(f32)
        g, b = lr.affine(gamma, beta, s_out, zp_out)
        v = lr.layer_norm_v(a, s_in, eps, g, b).astype(np.float64)
        y, TG, Bs = lr.real_parts(a, s_in, zp_in, eps, gamma, beta, s_out, zp_out)
        B = lr.bound(y, TG, Bs)
        err = np.abs(v - y)
        assert (err <= B).all(), (Cn, s_in, float((err / B).max()))
        assert B.max() < 1e-3
        q = lr.layer_norm_u8(a, s_in, eps, gamma, beta, s_out, zp_out)
        sure = np.abs(y - np.rint(y)) > B
        assert np.array_equal(q[sure], lr.clamp_trunc(y)[sure])
        total += q.size
        excluded += int((~sure).sum())
        spread |= set(np.unique(q).tolist())
        # the input zero point drops out: the same bytes under another one
        y2 = lr.real_parts(a, s_in, (zp_in + 77) % 256, eps, gamma, beta, s_out, zp_out)[0]
        assert np.abs(y2 - y).max() < 1e-9 * max(1.0, np.abs(y).max())
    assert excluded < 0.01 * total, (Cn, excluded, total)
    assert Cn <= 2 or len(spread) > 50   # the expected bytes discriminate (C = 2 has T = +-1 or 0 only)


@pytest.mark.parametrize("name,a", lr.extreme_rows(), ids=[n for n, _ in lr.extreme_rows()])
def test_statistics_extremes(name, a):
    Cn = a.shape[1]
    rng = np.random.default_rng(Cn)
    gamma = rng.normal(1.0, 0.5, Cn).astype(f32)
    beta = rng.normal(0.0, 0.5, Cn).astype(f32)
    S1, S2, V = lr.stats(a)   # (asserts S2 < 2^31 and 0 <= V < 2^53)
    for s_in, zp_in, s_out, zp_out, eps in QSETS[:2]:
        q = lr.layer_norm_u8(a, s_in, eps, gamma, beta, s_out, zp_out)
        y, TG, Bs = lr.real_parts(a, s_in, zp_in, eps, gamma, beta, s_out, zp_out)
        B = lr.bound(y, TG, Bs)
        g, b = lr.affine(gamma, beta, s_out, zp_out)
        assert (np.abs(lr.layer_norm_v(a, s_in, eps, g, b).astype(np.float64) - y) <= B).all(), name
        sure = np.abs(y - np.rint(y)) > B
        assert np.array_equal(q[sure], lr.clamp_trunc(y)[sure]), name
        if name.startswith("const"):
            assert (V == 0).all() and np.array_equal(q, np.broadcast_to(lr.clamp_trunc(b), q.shape))
    if name == "half_C16384":
        assert int(V[0, 0]) == (Cn * 255) ** 2 // 4 and int(V[1, 0]) == int(V[0, 0])
    if name == "all255_C16384":
        assert int(S2[0, 0]) == 16384 * 65025 and int(S1[0, 0]) ** 2 == Cn * int(S2[0, 0]) and int(V[0, 0]) == 0


@pytest.mark.parametrize("Cn", [1, 17, 96, 1025])
def test_f32_bound_is_meaningful(Cn):
    """the FP32 form's derived bound stays far below the values it guards (it is a bound, not a tolerance knob)"""
    rng = np.random.default_rng(Cn)
    x = rng.normal(0.3, 2.0, (5, Cn)).astype(f32)
    gamma, beta = rng.normal(1, 0.5, Cn).astype(f32), rng.normal(0, 0.5, Cn).astype(f32)
    bnd = lr.layer_norm_f32_bound(x, gamma, beta, 1e-5)
    assert bnd.shape == x.shape and np.isfinite(bnd).all() and bnd.max() < 2e-3


def test_module_state_dict_and_state_machine(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.norm1 = i8ie.LayerNorm(6, eps=1e-4)
            self.add1 = i8ie.Add()

    rng = np.random.default_rng(3)
    w, b = rng.normal(1, 0.3, 6).astype(f32), rng.normal(0, 0.3, 6).astype(f32)
    net = Net()
    net.load({"norm1.weight": w, "norm1.bias": b})
    assert np.array_equal(net.norm1.layer.weight(), w) and np.array_equal(net.norm1.layer.bias(), b)
    with pytest.raises(RuntimeError):
        net.quantized_state_dict()   # not converted
    net.norm1.set_output_qparams(0.03, 131)
    assert net.norm1.output_qparams() == (pytest.approx(0.03), 131) and not net.norm1.layer.is_quantized()
    with pytest.raises(RuntimeError):
        net.norm1.set_output_qparams(0.03, 256)
    assert [k for k, _ in net._layers()] == ["norm1", "add1"]


def test_convnext_configs_and_state_dict():
    from int8inferenceengine_amd import workloads as wl

    assert not ({"ln", "cnblock", "attn"} & set(wl.OPS))   # "ln" is a layer kind, the blocks are plain op sequences
    L, spec, shape = wl.network("convnext_tiny")
    assert shape == (3, 32, 32) and L["stem"] == ("conv", 3, 16, 4, 4, 0) and L["down"] == ("conv", 16, 20, 3, 2, 1)
    assert L["a_dw"] == ("conv", 16, 16, 7, 1, 3, 16) and L["b_pw1"] == ("conv", 20, 80, 1, 1, 0) and L["b_ln"] == ("ln", 20)
    assert L["t_theta"] == ("conv", 20, 12, 1, 1, 0) and L["head_ln"] == ("ln", 20) and L["fc"] == ("fc", 20, 10)
    cnblock = ["save", "layer", "layer", "layer", "act", "layer", "add"]
    attn = ["save", "layer", "save", "save", "layer", "branch", "matmul", "softmax", "save", "branch", "load", "add"]
    assert [op[0] for op in spec] == ["layer", "layer"] + cnblock + ["layer", "layer"] + cnblock + attn + ["gap", "flatten", "layer", "layer"]
    assert spec[2:9] == [("save", "a_x"), ("layer", "a_dw"), ("layer", "a_ln"), ("layer", "a_pw1"), ("act", "a_act", "hardswish"),
                         ("layer", "a_pw2"), ("add", "a_add", "a_x")]
    assert spec[18:20] == [("save", "t_x"), ("layer", "t_ln")] and spec[-6:-4] == [("load", "t_g"), ("add", "t_add", "t_x")]
    assert wl.layer_names("convnext_tiny") == list(L) == [
        "stem", "stem_ln", "a_dw", "a_ln", "a_pw1", "a_pw2", "down_ln", "down", "b_dw", "b_ln", "b_pw1", "b_pw2", "t_ln", "t_theta",
        "t_phi", "t_g", "t_out", "head_ln", "fc"]
    assert wl.join_names("convnext_tiny") == ["a_act", "a_add", "b_act", "b_add", "t_mm1", "t_mm2", "t_add"]
    # by hand: stem 8x8 x 16 x 48; block a at 8x8, c = 16: 49 c + 8 c^2 per pixel; down 4x4 x 20 x 144; block b at 4x4, c = 20;
    # the attention's four 1x1 convs 20 <-> 12 at 4x4; fc 200.  LayerNorms and MatMuls count nothing.
    assert wl.macs_per_image("convnext_tiny") == 64 * 16 * 48 + 64 * (49 * 16 + 8 * 256) + 16 * 20 * 144 + 16 * (49 * 20 + 8 * 400) \
        + 4 * 16 * 20 * 12 + 200 == 358920
    Cf, cspec, _ = wl.network("convnext_cifar")
    assert wl.add_names("convnext_cifar") == ["s%db%d_add" % (s, b) for s in range(4) for b in range(2)]
    assert [op[0] for op in cspec] == ["layer", "layer"] + (2 * cnblock + ["layer", "layer"]) * 3 + 2 * cnblock + ["gap", "flatten", "layer", "layer"]
    assert Cf["s3b1_pw1"] == ("conv", 512, 2048, 1, 1, 0) and Cf["d3"] == ("conv", 256, 512, 2, 2, 0) and Cf["fc"] == ("fc", 512, 10)
    # by hand: stem 16x16 x 64 x 12; two blocks per stage at (pixels, c) = (256, 64), (64, 128), (16, 256), (4, 512); three
    # 2x2 s2 convs of 2097152 each; fc 5120
    assert wl.macs_per_image("convnext_cifar") == 256 * 64 * 12 + 3 * 2097152 + 5120 \
        + 2 * sum(px * (49 * c + 8 * c * c) for px, c in ((256, 64), (64, 128), (16, 256), (4, 512))) == 76612608
    a, b = wl.synthetic_state_dict("convnext_tiny", 3), wl.synthetic_state_dict("convnext_tiny", 3)
    assert sorted(a) == sorted(k + s for k in L for s in (".weight", ".bias"))
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["a_dw.weight"].shape == (16, 1, 7, 7) and a["b_ln.weight"].shape == (20,)
    assert a["b_ln.weight"].dtype == np.float32 and 0.5 <= a["b_ln.weight"].min() and a["b_ln.weight"].max() <= 1.5 and np.abs(a["b_ln.bias"]).max() <= 0.3
    assert wl.FOLDS["convnext_tiny"] == {"a_pw2": wl.LAYER_SCALE, "b_pw2": wl.LAYER_SCALE, "t_theta": 1 / np.sqrt(12)} and wl.LAYER_SCALE == 0.5
    net = wl.build("convnext_tiny")
    assert type(net).__name__ == "SpecNet_convnext_tiny"
    assert [k for k, _ in net._layers()] == wl.join_names("convnext_tiny") + wl.layer_names("convnext_tiny")
