"""CPU-side checks of the inference BatchNorm: the numpy restatement (tests/batchnorm_ref.py) against torch's CPU batch_norm in
float64 within the bound of include/i8ie_hip.h, i8ie_batchnorm_affine through ctypes (bit for bit, and its refusals), the
argument rules of the launch entries, i8ie.fold_batchnorm on every layer class against the restatement and against torch's
float64 conv -> batch_norm, the state rules of the fold, Module.load's routing and the Python forms' argument rules.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
import batchnorm_ref as bn
import support
from support import i8ie  # noqa: F401

f32, f64 = np.float32, np.float64
ENTRIES = ["i8ie_batchnorm_affine", "i8ie_batchnorm_u8_nhwc", "i8ie_batchnorm_u8", "i8ie_batchnorm_f32"]

lib = support.lib_fixture(bn)


def test_abi_symbols_declared_and_exported(lib):
    declared = abi.declared_symbols()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name), name


# ---- the bound against torch ---------------------------------------------------------------------------------------------------
def test_restatement_against_torch_float64_within_the_bound():
    """40 seeded parameter sets x C = 20 x all 256 bytes: |v - y*| <= B everywhere, q == clamp(trunc(y*)) wherever y* is further
    than B from an integer, and at most 1 % of the cases are left out as too close"""
    Cn = 20
    q = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(256, 1), (256, Cn)).copy()
    total = excluded = 0
    worst = 0.0
    spread = set()
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        gamma, beta, mean, var = bn.random_params(rng, Cn)
        s_in, zp_in, s_out, zp_out = bn.random_qparams(rng)
        eps = f32(1e-5)
        g, b = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
        v = bn.batch_norm_v(q, s_in, zp_in, g, b).astype(f64)
        y, T, Bt = bn.real_parts(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out)
        B = bn.bound(y, T, Bt)
        err = np.abs(v - y)
        worst = max(worst, float((err / B).max()))
        assert (err <= B).all(), (seed, float((err / B).max()))
        for relu in (False, True):
            out = bn.batch_norm_u8(q, s_in, zp_in, gamma, beta, mean, var, eps, s_out, zp_out, relu)
            want = bn.clamp_trunc(y)
            want = np.maximum(want, np.uint8(zp_out)) if relu else want
            sure = np.abs(y - np.rint(y)) > B
            assert np.array_equal(out[sure], want[sure]), (seed, relu)
        total += out.size
        excluded += int((~sure).sum())
        spread |= set(np.unique(out).tolist())
    print("largest |v - y*| / B: %.3f; left out as too close: %d of %d" % (worst, excluded, total))
    assert excluded <= 0.01 * total and len(spread) > 200


def test_fp32_sequence_against_float64():
    rng = np.random.default_rng(5)
    for shape in ((3, 20, 4, 5), (7, 20)):
        gamma, beta, mean, var = bn.random_params(rng, 20)
        var[3] = 0.0
        x = rng.normal(0.2, 2.0, shape).astype(f32)
        err = np.abs(bn.batch_norm_f32(x, gamma, beta, mean, var, 1e-5).astype(f64) - bn.batch_norm_f64(x, gamma, beta, mean, var, 1e-5))
        bound = bn.batch_norm_f32_bound(x, gamma, beta, mean, var, 1e-5)
        assert (err <= bound).all() and bound.max() < 1e-2


# ---- i8ie_batchnorm_affine -----------------------------------------------------------------------------------------------------
def test_affine_entry_is_the_restatement_bit_for_bit(lib):
    for seed, Cn in enumerate((1, 3, 20, 64, 1000, bn.MAX_C)):
        rng = np.random.default_rng(seed)
        gamma, beta, mean, var = bn.random_params(rng, Cn)
        var[0] = 0.0
        gamma[Cn // 2] = 0.0
        for s_in, zp_in, s_out, zp_out, eps, _ in bn.PARAM_SETS:
            rc, g, b = bn.affine_entry(lib, gamma, beta, mean, var, eps, s_out, zp_out)
            wg, wb = bn.affine(gamma, beta, mean, var, eps, s_out, zp_out)
            assert rc == 0 and support.same_bits(g, wg) and support.same_bits(b, wb), (Cn, s_out, zp_out)


def test_affine_entry_refuses(lib):
    nan, inf = float("nan"), float("inf")
    ok = [np.ones(4, f32), np.zeros(4, f32), np.zeros(4, f32), np.ones(4, f32)]

    def call(arrs=ok, eps=1e-5, s_out=0.05, Cn=None):
        rc, g, b = bn.affine_entry(lib, *arrs, eps, s_out, 7, Cn=Cn)
        if rc != 0:
            assert rc == -1 and "i8ie_batchnorm_affine" in abi.lib().i8ie_last_error().decode()
            assert np.isnan(g).all() and np.isnan(b).all()   # an argument error writes nothing
        return rc

    assert call() == 0

    def with_value(i, j, v):
        arrs = [a.copy() for a in ok]
        arrs[i][j] = v
        return arrs

    assert call(with_value(3, 1, -1e-3)) == -1 and "var" in abi.lib().i8ie_last_error().decode()   # var < 0
    for i in range(4):
        for v in (nan, inf, -inf):
            assert call(with_value(i, 2, v)) == -1, (i, v)
    for Cn in (0, -1, 16385):
        assert call(Cn=Cn) == -1, Cn
    for eps in (0.0, -1e-5, nan, inf):
        assert call(eps=eps) == -1, eps
    for s_out in (0.0, -0.05, nan, inf):
        assert call(s_out=s_out) == -1, s_out
    a = np.ones(4, f32)
    p = a.ctypes.data
    for hole in range(6):
        args = [p, p, p, p, p, p]
        args[hole] = None
        assert lib.i8ie_batchnorm_affine(*args[:4], 4, 1e-5, 0.05, 7, *args[4:]) == -1 and b"null" in abi.lib().i8ie_last_error()
    # var = 0 with a tiny eps and a tiny s_out: g overflows
    assert call(with_value(3, 0, 0.0), eps=1e-38, s_out=1e-30) == -1 and "finite" in abi.lib().i8ie_last_error().decode()
    big = [a.copy() for a in ok]
    big[1][:] = 3e38   # beta / s_out overflows b
    assert call(big, s_out=1e-3) == -1


def test_launch_entries_refuse_before_any_device_call(lib):
    """every argument error is I8IE_ERR_ARG with a message before any device call (the ctx is never dereferenced)"""
    fake = C.create_string_buffer(512)
    p = 4096   # (never dereferenced)
    nan, inf = float("nan"), float("inf")

    def nhwc(ctx=fake, i=p, ib=0, o=p, ob=0, n=1, Cn=16, h=2, w=2, g=p, b=p, s_in=0.1):
        return lib.i8ie_batchnorm_u8_nhwc(ctx, i, ib, 0, o, ob, 0, n, Cn, h, w, g, b, s_in, 3, 0, 0)

    def flat(ctx=fake, i=p, o=p, rows=4, Cn=16, inner=1, g=p, b=p, s_in=0.1):
        return lib.i8ie_batchnorm_u8(ctx, i, o, rows, Cn, inner, g, b, s_in, 3, 0, 0)

    def fp(ctx=fake, i=p, o=p, rows=4, Cn=16, inner=1, g=p, b=p, m=p, v=p, eps=1e-5):
        return lib.i8ie_batchnorm_f32(ctx, i, o, rows, Cn, inner, g, b, m, v, eps)

    common = [dict(ctx=None), dict(i=None), dict(o=None), dict(g=None), dict(b=None), dict(Cn=0), dict(Cn=16400), dict(Cn=-4)]
    for kw in common + [dict(s_in=nan), dict(s_in=inf), dict(s_in=3e38), dict(ib=-1), dict(ob=-1), dict(n=0), dict(h=0), dict(w=-2),
                        dict(g=p + 2), dict(b=p + 1), dict(h=65536, w=65536)]:
        assert nhwc(**kw) == -1, kw
        assert "i8ie_batchnorm_u8_nhwc" in abi.lib().i8ie_last_error().decode(), kw
    for kw in common + [dict(s_in=nan), dict(s_in=-inf), dict(rows=0), dict(rows=2 ** 31), dict(inner=0), dict(inner=3), dict(g=p + 2)]:
        assert flat(**kw) == -1, kw
        assert "i8ie_batchnorm_u8" in abi.lib().i8ie_last_error().decode(), kw
    for kw in common + [dict(m=None), dict(v=None), dict(rows=0), dict(inner=3), dict(eps=0.0), dict(eps=nan), dict(eps=inf)]:
        assert fp(**kw) == -1, kw
        assert "i8ie_batchnorm_f32" in abi.lib().i8ie_last_error().decode(), kw


# ---- the fold ----------------------------------------------------------------------------------------------------------------
def _bn(i8ie, Cn, seed, eps=1e-5):
    gamma, beta, mean, var = bn.random_params(np.random.default_rng(seed), Cn)
    L = i8ie.BatchNorm2d(Cn, eps)
    L.load_weight(gamma)
    L.load_bias(beta)
    L.load_running_mean(mean)
    L.load_running_var(var)
    return L, (gamma, beta, mean, var)


def _fold_cases(i8ie):
    """(name, layer, weight shape, output-feature axis, torch float64 forward of (x, w, b), input shape)"""
    import torch
    F = torch.nn.functional
    return [
        ("dense", i8ie.Conv2d(6, 8, 3, padding=1), (8, 6, 3, 3), 0, lambda x, w, b: F.conv2d(x, w, b, 1, 1), (2, 6, 5, 5)),
        ("groups2", i8ie.Conv2d(6, 8, 3, stride=2, padding=1, groups=2), (8, 3, 3, 3), 0, lambda x, w, b: F.conv2d(x, w, b, 2, 1, 1, 2), (2, 6, 5, 5)),
        ("depthwise", i8ie.Conv2d(8, 8, 3, padding=2, groups=8, dilation=2), (8, 1, 3, 3), 0, lambda x, w, b: F.conv2d(x, w, b, 1, 2, 2, 8), (2, 8, 6, 6)),
        ("rect1x3", i8ie.Conv2d(6, 8, (1, 3), padding=(0, 1)), (8, 6, 1, 3), 0, lambda x, w, b: F.conv2d(x, w, b, 1, (0, 1)), (2, 6, 4, 5)),
        ("linear", i8ie.Linear(12, 8), (8, 12), 0, lambda x, w, b: F.linear(x, w, b), (5, 12)),
        ("deconv", i8ie.ConvTranspose2d(6, 8, 3, stride=2, padding=1, output_padding=1), (6, 8, 3, 3), 1,
         lambda x, w, b: F.conv_transpose2d(x, w, b, 2, 1, 1), (2, 6, 4, 4)),
    ]


def test_fold_gives_the_restatements_parameters_and_torchs_function(i8ie):
    import torch

    for i, (name, L, wshape, axis, fwd, xshape) in enumerate(_fold_cases(i8ie)):
        rng = np.random.default_rng(40 + i)
        w, b = rng.normal(0, 0.3, wshape).astype(f32), rng.normal(0, 0.3, 8).astype(f32)
        L.load_weight(w)
        L.load_bias(b)
        assert support.same_bits(L.layer._weight(), w) and support.same_bits(L.layer._bias(), b), name   # as loaded
        B, (gamma, beta, mean, var) = _bn(i8ie, 8, 70 + i)
        assert not B.is_folded()
        i8ie.fold_batchnorm(L, B)
        w2, b2 = bn.fold(w, b, gamma, beta, mean, var, 1e-5, axis)
        assert B.is_folded() and not np.array_equal(w2, w)
        assert support.same_bits(L.layer._weight(), w2) and support.same_bits(L.layer._bias(), b2), name
        t = lambda v: torch.from_numpy(np.asarray(v, f32).astype(f64))  # noqa: E731
        x = t(rng.normal(0, 1, xshape).astype(f32))
        want = torch.nn.functional.batch_norm(fwd(x, t(w), t(b)), t(mean), t(var), t(gamma), t(beta), False, 0.0, float(f64(f32(1e-5)))).numpy()
        got = fwd(x, t(w2), t(b2)).numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (name, np.abs(got - want).max())
        # the folded BatchNorm is the identity: the same object back, nothing launched
        marker = object()
        assert B(marker) is marker
        B.prepare()
        B.convert()
        assert not B.layer.is_quantized() and not B.layer._is_preparing()
        for load in (B.load_weight, B.load_bias, B.load_running_mean, B.load_running_var):   # its parameters are inside the layer now
            with pytest.raises(RuntimeError, match="after the fold"):
                load(gamma)


def test_fold_error_and_state_rules(i8ie):
    conv = i8ie.Conv2d(4, 8, 3)
    B, _ = _bn(i8ie, 8, 1)
    with pytest.raises(RuntimeError, match="output features"):
        i8ie.fold_batchnorm(conv, _bn(i8ie, 4, 2)[0])            # wrong width
    with pytest.raises(RuntimeError, match="output features"):
        i8ie.fold_batchnorm(i8ie.ConvTranspose2d(8, 4, 3), B)    # the feature axis of a ConvTranspose2d is axis 1
    for other in (i8ie.LayerNorm(8), i8ie.Add(), B, None):
        with pytest.raises(TypeError):
            i8ie.fold_batchnorm(other, B)                        # wrong class
    with pytest.raises(TypeError):
        i8ie.fold_batchnorm(conv, i8ie.GroupNorm(2, 8))
    assert not B.is_folded()
    prep = i8ie.Conv2d(4, 8, 3)
    prep.prepare()
    with pytest.raises(RuntimeError, match="preparing"):
        i8ie.fold_batchnorm(prep, B)
    Bp, _ = _bn(i8ie, 8, 3)
    Bp.prepare()
    with pytest.raises(RuntimeError, match="preparing"):
        i8ie.fold_batchnorm(conv, Bp)
    assert not B.is_folded() and not Bp.is_folded()
    i8ie.fold_batchnorm(conv, B)
    with pytest.raises(RuntimeError, match="already folded"):
        i8ie.fold_batchnorm(conv, B)                             # double fold
    with pytest.raises(RuntimeError, match="already folded"):
        i8ie.fold_batchnorm(i8ie.Conv2d(4, 8, 3), B)


def test_module_fold_load_and_state_dict(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = i8ie.Conv2d(3, 8, 3, padding=1)
            self.bn1 = i8ie.BatchNorm2d(8)
            self.fc = i8ie.Linear(8, 4)
            self.bn2 = i8ie.BatchNorm2d(4, eps=1e-3)

    rng = np.random.default_rng(9)
    gamma, beta, mean, var = bn.random_params(rng, 8)
    w, b = rng.normal(0, 0.3, (8, 3, 3, 3)).astype(f32), rng.normal(0, 0.3, 8).astype(f32)
    net = Net()
    net.load({"conv1.weight": w, "conv1.bias": b, "bn1.weight": gamma, "bn1.bias": beta, "bn1.running_mean": mean, "bn1.running_var": var,
              "bn1.num_batches_tracked": np.int64(1234), "bn2.num_batches_tracked": np.int64(7), "fc.other": 1})
    L = net.bn1.layer
    for got, want in ((L.weight(), gamma), (L.bias(), beta), (L.running_mean(), mean), (L.running_var(), var),
                      (net.bn1.running_mean(), mean), (net.bn1.running_var(), var)):
        assert support.same_bits(got, want)
    L2 = net.bn2.layer   # the defaults: 1, 0, 0, 1
    assert np.array_equal(L2.weight(), np.ones(4, f32)) and np.array_equal(L2.bias(), np.zeros(4, f32))
    assert np.array_equal(L2.running_mean(), np.zeros(4, f32)) and np.array_equal(L2.running_var(), np.ones(4, f32))
    assert [k for k, _ in net._layers()] == ["conv1", "bn1", "fc", "bn2"]
    with pytest.raises(RuntimeError):
        net.quantized_state_dict()   # not converted
    net.fold_batchnorm([("conv1", "bn1")])
    w2, b2 = bn.fold(w, b, gamma, beta, mean, var, 1e-5)
    assert net.bn1.is_folded() and not net.bn2.is_folded() and support.same_bits(net.conv1.layer._weight(), w2)
    assert support.same_bits(net.conv1.layer._bias(), b2)
    with pytest.raises(RuntimeError):
        net.fold_batchnorm([("conv1", "bn1")])
    with pytest.raises(TypeError):
        net.fold_batchnorm([("bn2", "bn2")])


def test_construction_and_argument_rules(i8ie):
    import _CXX_i8ie as cx

    for n in ("BatchNorm2d", "batch_norm", "fold_batchnorm"):
        assert n in i8ie.__all__ and hasattr(i8ie, n)
    assert hasattr(cx, "_BatchNorm2d") and hasattr(cx, "_batch_norm") and not hasattr(cx, "BatchNorm2d") and not hasattr(cx, "batch_norm")
    for cls in (cx.Linear, cx.Conv2d, cx._Conv2dRect, cx.ConvTranspose2d):
        assert hasattr(cls, "_weight") and hasattr(cls, "_bias")
    B = i8ie.BatchNorm2d(20)
    assert isinstance(B, i8ie.layer.Norm) and not isinstance(B, i8ie.layer.Weightless)
    assert (B.num_features, B.eps) == (20, 1e-5) and B.output_qparams() == (1.0, 0) and not B.is_folded()
    assert (B.layer.num_features(), B.layer.eps()) == (20, pytest.approx(1e-5)) and not B.is_per_channel() and not B.layer.is_quantized()
    for call in (B.weight_scale, B.weight_scales, B.q_weight, B.q_bias, lambda: B.forward_debug(None)):
        with pytest.raises(RuntimeError, match="BatchNorm2d"):
            call()
    for channels in (0, -3, 16385):
        with pytest.raises(RuntimeError):
            i8ie.BatchNorm2d(channels)
    assert i8ie.BatchNorm2d(16384).num_features == 16384
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            i8ie.BatchNorm2d(4, eps=bad)
    for load in (B.load_weight, B.load_bias, B.load_running_mean, B.load_running_var):
        with pytest.raises(RuntimeError):
            load(np.ones(19, f32))
        with pytest.raises(RuntimeError):
            load(np.ones((20, 1), f32))
    # the FP32 parameters of a layer constructed from sizes are zeros of the weight's shape; torch's layout for ConvTranspose2d
    assert i8ie.ConvTranspose2d(6, 8, 3).layer._weight().shape == (6, 8, 3, 3) and i8ie.Linear(12, 8).layer._weight().shape == (8, 12)
    assert i8ie.Conv2d(6, 8, (1, 3), groups=2).layer._weight().shape == (8, 3, 1, 3) and i8ie.Conv2d(6, 8, 3).layer._bias().shape == (8,)


def test_python_forms_refuse_bad_shapes_and_arguments(i8ie):
    t = lambda *shape: i8ie.tensor(np.zeros(shape, f32))  # noqa: E731
    ones = np.ones(8, f32)
    for kw in ({"scale": 1.0}, {"zero_point": 0}, {"scale": 1.0, "zero_point": 0}):
        with pytest.raises(TypeError):
            i8ie.batch_norm(t(2, 8), ones, ones, **kw)
    bad = [lambda: i8ie.batch_norm(t(8), ones, ones),                       # rank 1
           lambda: i8ie.batch_norm(t(2, 8, 3), ones, ones),                 # rank 3
           lambda: i8ie.batch_norm(t(1, 2, 8, 3, 3), ones, ones),           # rank 5
           lambda: i8ie.batch_norm(t(2, 8, 3, 3), np.ones(7, f32), ones),   # wrong statistics length
           lambda: i8ie.batch_norm(t(2, 8, 3, 3), ones, ones, np.ones((8, 1), f32)),
           lambda: i8ie.batch_norm(t(2, 8, 3, 3), ones, ones, eps=0.0),
           lambda: i8ie.batch_norm(t(2, 8, 3, 3), ones, ones, eps=float("nan")),
           lambda: i8ie.BatchNorm2d(8)(t(2, 6, 3, 3)),                      # c != num_features
           lambda: i8ie.BatchNorm2d(8)(t(2, 3, 8)),                         # rank 3
           lambda: i8ie.BatchNorm2d(8)(t(8))]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
