"""CPU-side checks of the quantized GroupNorm: the surface and the argument rules of the C-ABI and of the Python forms,
i8ie_groupnorm_workspace_bytes on both sides of the LDS budget, the numpy restatement (tests/groupnorm_ref.py) against the
LayerNorm restatement on the gathered rows and against torch.nn.functional.group_norm in float64 within the bound of
include/i8ie_hip.h, the statistics extremes at N = 65536, N = 1, and the module's state dict.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi
import groupnorm_ref as gn
import layernorm_ref as lr
import support
from support import i8ie  # noqa: F401

f32 = np.float32
ENTRIES = ["i8ie_groupnorm_u8_nhwc", "i8ie_groupnorm_workspace_bytes", "i8ie_groupnorm_f32"]
# (s_in, zp_in, s_out, zp_out, eps)
QSETS = [(0.025, 127, 0.02, 128, 1e-5), (0.1, 0, 0.05, 100, 1e-6), (0.004, 255, 0.011, 0, 1e-3), (1.7, 13, 0.03, 255, 1e-5)]
# (C, G, h, w): every group shape of the GPU file, N = 1, the longest row
CASES = [(32, 32, 3, 5), (64, 32, 8, 8), (16, 4, 7, 9), (160, 16, 3, 5), (64, 4, 1, 1), (64, 2, 8, 8), (48, 1, 3, 5), (20, 5, 7, 9),
         (35, 7, 3, 5), (320, 32, 2, 3), (8, 8, 1, 1), (16, 16, 64, 64), (16, 1, 64, 64)]


lib = support.lib_fixture(gn)


def _params(Cn, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(1.0, 0.6, Cn).astype(f32), rng.normal(0.0, 0.6, Cn).astype(f32)


def test_abi_symbols_declared_and_exported(lib):
    declared = abi.declared_symbols()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name), name


def test_surface_names(i8ie):
    import _CXX_i8ie as cx

    for n in ("GroupNorm", "group_norm"):
        # (the extension's entries are private: its public names are recorded whole in tests/golden/binding_surface.json)
        assert n in i8ie.__all__ and hasattr(i8ie, n) and hasattr(cx, "_" + n)
    g = i8ie.GroupNorm(4, 20)   # torch's argument order: num_groups, num_channels
    assert isinstance(g, i8ie.Layer) and not isinstance(g, i8ie.layer.Weightless)
    assert (g.num_groups, g.num_channels, g.eps) == (4, 20, 1e-5) and g.output_qparams() == (1.0, 0)
    assert (g.layer.num_groups(), g.layer.channels()) == (4, 20) and g.groups() == 1   # (Layer.groups() is a conv's)
    assert not g.is_per_channel() and not g.layer.is_quantized()
    assert np.array_equal(g.layer.weight(), np.ones(20, f32)) and np.array_equal(g.layer.bias(), np.zeros(20, f32))
    for call in (g.weight_scale, g.weight_scales, g.q_weight, g.q_bias, lambda: g.forward_debug(None)):
        with pytest.raises(RuntimeError, match="GroupNorm"):
            call()
    for groups, channels in ((3, 20), (0, 20), (4, 0), (1, 16385), (40, 20)):   # C % G, empty, too wide
        with pytest.raises(RuntimeError):
            i8ie.GroupNorm(groups, channels)
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            i8ie.GroupNorm(2, 4, eps=bad)
    with pytest.raises(RuntimeError):
        g.load_weight(np.ones(19, f32))
    with pytest.raises(RuntimeError):
        g.load_bias(np.ones((20, 1), f32))
    assert i8ie.GroupNorm(20, 20).num_groups == 20 and i8ie.GroupNorm(1, 20).num_groups == 1   # InstanceNorm, LayerNorm over (c, h, w)
    assert not isinstance(g, i8ie.LayerNorm) and isinstance(g, i8ie.layer.Norm)


def test_python_forms_refuse_before_any_device_call(i8ie):
    """(an FP32 tensor made from numpy is not on the device yet: every refusal below comes before the upload)"""
    t = lambda *shape: i8ie.tensor(np.zeros(shape, f32))  # noqa: E731
    for kw in ({"scale": 1.0}, {"zero_point": 0}, {"scale": 1.0, "zero_point": 0}):
        with pytest.raises(TypeError):
            i8ie.group_norm(t(2, 8), 2, **kw)
    bad = [lambda: i8ie.group_norm(t(8), 2),                        # rank 1
           lambda: i8ie.group_norm(t(2, 8, 3), 2),                  # rank 3
           lambda: i8ie.group_norm(t(1, 2, 8, 3, 3), 2),            # rank 5
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 3),               # C % G
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 0),
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 2, np.ones(7, f32)),          # wrong weight length
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 2, None, np.ones((8, 1), f32)),
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 2, eps=0.0),
           lambda: i8ie.group_norm(t(2, 8, 3, 3), 2, eps=float("nan")),
           lambda: i8ie.group_norm(t(1, 16, 64, 65), 1),            # N = 66560
           lambda: i8ie.GroupNorm(2, 8)(t(2, 6, 3, 3)),             # c != num_channels
           lambda: i8ie.GroupNorm(2, 8)(t(2, 3, 8)),                # rank 3
           lambda: i8ie.GroupNorm(1, 16)(t(1, 16, 4097))]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()


def test_argument_errors_need_no_gpu(lib):
    """every argument error is I8IE_ERR_ARG with a message before any device call (of the ctx only its options are read)"""
    fake = C.create_string_buffer(512)
    p = 4096   # (never dereferenced)

    def u8(ctx=fake, i=p, ib=0, o=p, ob=0, n=1, Cn=16, G=4, h=2, w=2, g=p, b=p, s_in=0.1, eps=1e-5, ws=p):
        return lib.i8ie_groupnorm_u8_nhwc(ctx, i, ib, 0, o, ob, 0, n, Cn, G, h, w, g, b, s_in, eps, 0, 0, ws)

    def fp(ctx=fake, i=p, o=p, n=1, Cn=16, G=4, hw=4, g=p, b=p, eps=1e-5):
        return lib.i8ie_groupnorm_f32(ctx, i, o, n, Cn, G, hw, g, b, eps)

    nan, inf = float("nan"), float("inf")
    both = [dict(ctx=None), dict(i=None), dict(o=None), dict(g=None), dict(b=None), dict(Cn=0), dict(Cn=16400, G=4), dict(Cn=-4),
            dict(G=0), dict(G=3), dict(G=32), dict(n=0), dict(eps=0.0), dict(eps=-1e-5), dict(eps=nan), dict(eps=inf)]
    for kw in both + [dict(s_in=0.0), dict(s_in=-0.1), dict(s_in=nan), dict(s_in=inf), dict(ib=-1), dict(ob=-1), dict(h=0), dict(w=-2),
                      dict(g=p + 2), dict(Cn=16, G=1, h=64, w=65),            # N = 66560
                      dict(Cn=64, G=32, h=56, w=56, ws=None),                 # the split form needs ws
                      dict(s_in=1e30, eps=1e-38)]:                            # E leaves the range of 1 / sqrt in fp32
        assert u8(**kw) == -1, kw
        assert "i8ie_groupnorm_u8_nhwc" in abi.lib().i8ie_last_error().decode(), kw
    for kw in both + [dict(hw=0), dict(Cn=16, G=1, hw=4097)]:
        assert fp(**kw) == -1, kw
        assert "i8ie_groupnorm_f32" in abi.lib().i8ie_last_error().decode(), kw
    assert "65536" in (u8(Cn=16, G=1, h=64, w=65), abi.lib().i8ie_last_error().decode())[1]
    assert "multiple" in (u8(G=3), abi.lib().i8ie_last_error().decode())[1]


def test_row_length_limit_is_65536(lib):
    """N = 65536 passes the size rules and 65537 does not (the host-only entry applies the same rules as the launch entry)"""
    assert lib.i8ie_groupnorm_workspace_bytes(1, 16, 1, 64, 64) == 0            # N = 65536
    assert lib.i8ie_groupnorm_workspace_bytes(1, 1, 1, 1, 65536) == 0
    assert lib.i8ie_groupnorm_workspace_bytes(1, 1, 1, 1, 65537) == -1
    assert "65536" in abi.lib().i8ie_last_error().decode()
    assert lib.i8ie_groupnorm_workspace_bytes(1, 16, 1, 64, 65) == -1
    assert lib.i8ie_groupnorm_workspace_bytes(1, 17, 17, 65536, 1) == 0        # cg = 1: N = h w
    for bad in ((0, 16, 4, 2, 2), (1, 16, 3, 2, 2), (1, 0, 1, 2, 2), (1, 16, 4, 0, 2), (1, 16400, 4, 1, 1)):
        assert lib.i8ie_groupnorm_workspace_bytes(*bad) == -1, bad
        assert "i8ie_groupnorm_workspace_bytes" in abi.lib().i8ie_last_error().decode()
    # the restatement refuses the same row
    with pytest.raises(AssertionError):
        gn.rows_of(np.zeros((1, 16, 64, 65), np.uint8), 1)


def test_workspace_bytes_on_both_sides_of_the_lds_budget(lib):
    assert gn.IMAGE_BYTES == 98304 and gn.CHUNK_BYTES == 32768
    # C = 64: 1536 pixels fill the budget exactly; one pixel row more takes the split form
    assert gn.form(64, 48, 32) == "image" and gn.form(64, 49, 32) == "split"
    for n, Cn, G, h, w in ((3, 64, 32, 48, 32), (3, 64, 32, 49, 32), (2, 64, 32, 56, 56), (1, 512, 32, 4, 4), (5, 512, 32, 14, 14),
                           (2, 4096, 4096, 5, 5), (2, 4112, 4112, 5, 5), (2, 20, 5, 99, 99), (1, 32, 2, 64, 64), (7, 16, 1, 64, 64)):
        want = gn.workspace_bytes(n, Cn, G, h, w)
        assert lib.i8ie_groupnorm_workspace_bytes(n, Cn, G, h, w) == want, (n, Cn, G, h, w)
    assert gn.workspace_bytes(3, 64, 32, 48, 32) == 0
    assert gn.workspace_bytes(3, 64, 32, 49, 32) == 3 * 4 * 2 * 32 * 4          # 1568 pixels in chunks of 512
    assert gn.workspace_bytes(2, 64, 32, 56, 56) == 2 * 7 * 2 * 32 * 4          # 3136 pixels: six chunks and 64 pixels
    assert gn.workspace_bytes(2, 20, 5, 99, 99) == 0 and gn.workspace_bytes(2, 4112, 4112, 5, 5) == 0   # direct


@pytest.mark.parametrize("case", [c for c in CASES if (c[0] // c[1]) * c[2] * c[3] <= lr.MAX_C], ids=str)
def test_restatement_is_the_layernorm_definition_on_gathered_rows(case):
    """byte for byte: a group of one image is a row of layernorm_ref.layer_norm_u8, gamma / beta repeated per pixel"""
    Cn, G, h, w = case
    rng = np.random.default_rng(sum(case))
    gamma, beta = _params(Cn, Cn)
    for s_in, zp_in, s_out, zp_out, eps in QSETS:
        q = rng.integers(0, 256, (3, Cn, h, w), dtype=np.uint8)
        q[1] = (rng.integers(0, 12, (Cn, h, w)) + 100).astype(np.uint8)   # a narrow image: small V
        for relu in (False, True):
            got = gn.group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out, relu)
            rows = gn.rows_of(q, G)
            want = lr.layer_norm_u8(rows, s_in, eps, gn.per_element(gamma, G, h * w), gn.per_element(beta, G, h * w), s_out, zp_out, relu)
            assert np.array_equal(got, want.reshape(q.shape)), (case, s_in, relu)
    if h == w == 1:   # the flat form of the surface: [n, C] is [n, C, 1, 1]
        assert np.array_equal(gn.group_norm_u8(q[:, :, 0, 0], G, s_in, eps, gamma, beta, s_out, zp_out, relu), got[:, :, 0, 0])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_ref_against_torch_float64_within_derived_bound(case):
    """|v - y*| <= B(y*) everywhere; the byte equals clamp(trunc(y*)) wherever y* is further than B from an integer; fewer than
    1 % of the bytes fall under that exclusion"""
    Cn, G, h, w = case
    N = (Cn // G) * h * w
    rng = np.random.default_rng(300 + sum(case))
    n = 3 if N < 65536 else 1
    total = excluded = 0
    spread = set()
    gamma, beta = _params(Cn, 7 + Cn)
    for s_in, zp_in, s_out, zp_out, eps in QSETS:
        q = rng.integers(0, 256, (n, Cn, h, w), dtype=np.uint8)
        if n > 1:
            q[1] = (rng.integers(0, 12, (Cn, h, w)) + 100).astype(np.uint8)
        g, b = lr.affine(gamma, beta, s_out, zp_out)
        v = gn.group_norm_v(q, G, s_in, eps, g, b).astype(np.float64)
        y, TG, Bs = gn.real_parts(q, G, s_in, zp_in, eps, gamma, beta, s_out, zp_out)
        B = gn.bound(y, TG, Bs)
        err = np.abs(v - y)
        assert (err <= B).all(), (case, s_in, float((err / B).max()))
        assert B.max() < 2e-3
        out = gn.group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out)
        sure = np.abs(y - np.rint(y)) > B
        assert np.array_equal(out[sure], lr.clamp_trunc(y)[sure])
        total += out.size
        excluded += int((~sure).sum())
        spread |= set(np.unique(out).tolist())
        # the input zero point drops out
        y2 = gn.real_parts(q, G, s_in, (zp_in + 77) % 256, eps, gamma, beta, s_out, zp_out)[0]
        assert np.abs(y2 - y).max() < 1e-9 * max(1.0, np.abs(y).max())
    assert excluded < 0.01 * total, (case, excluded, total)
    assert N <= 2 or len(spread) > 50   # the expected bytes discriminate


@pytest.mark.parametrize("name,q", gn.extreme_images(), ids=[n for n, _ in gn.extreme_images()])
def test_statistics_extremes_at_the_longest_row(name, q):
    """C = 16, G = 1, 64 x 64: N = 65536"""
    Cn, G = 16, 1
    gamma, beta = _params(Cn, 5)
    S1, S2, V = gn.stats(gn.rows_of(q, G))   # (asserts S2 < 2^32 and 0 <= V < 2^47)
    for s_in, zp_in, s_out, zp_out, eps in QSETS[:2]:
        out = gn.group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out)
        y, TG, Bs = gn.real_parts(q, G, s_in, zp_in, eps, gamma, beta, s_out, zp_out)
        B = gn.bound(y, TG, Bs)
        g, b = lr.affine(gamma, beta, s_out, zp_out)
        assert (np.abs(gn.group_norm_v(q, G, s_in, eps, g, b).astype(np.float64) - y) <= B).all(), name
        sure = np.abs(y - np.rint(y)) > B
        assert np.array_equal(out[sure], lr.clamp_trunc(y)[sure]), name
        if name in ("const", "all255"):
            assert (V == 0).all() and np.array_equal(out, np.broadcast_to(lr.clamp_trunc(b).reshape(1, Cn, 1, 1), out.shape))
    if name == "half":
        assert (V == (65536 * 255) ** 2 // 4).all() and int(V.max()) < 2 ** 47
    if name == "all255":
        assert int(S2[0, 0, 0]) == 65536 * 65025 >= 2 ** 31 and int(S1[0, 0, 0]) == 65536 * 255   # S2 needs the unsigned 32
    if name == "one_differs":
        assert (V > 0).all() and len(np.unique(out)) > 1


def test_rows_of_one_value():
    """N = 1: V = 0, d = 0, q = clamp(trunc(b[c])) whatever the byte is"""
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    gamma, beta = _params(8, 2)
    out = gn.group_norm_u8(q, 8, 0.025, 1e-5, gamma, beta, 0.02, 128)
    b = lr.affine(gamma, beta, 0.02, 128)[1]
    assert np.array_equal(out, np.broadcast_to(lr.clamp_trunc(b), (4, 8))) and len(np.unique(out)) > 3
    y = gn.real_parts(q, 8, 0.025, 127, 1e-5, gamma, beta, 0.02, 128)[0]
    assert np.abs(y[:, :, 0, 0] - (beta.astype(np.float64) / np.float64(f32(0.02)) + 128)).max() < 1e-9


@pytest.mark.parametrize("case", [(16, 4, 3, 5), (64, 32, 8, 8), (16, 1, 64, 64)], ids=str)
def test_f32_bound_is_meaningful(case):
    Cn, G, h, w = case
    rng = np.random.default_rng(Cn)
    x = rng.normal(0.3, 2.0, (2, Cn, h, w)).astype(f32)
    gamma, beta = _params(Cn, 3)
    bnd = gn.group_norm_f32_bound(x, G, gamma, beta, 1e-5)
    assert bnd.shape == x.shape and np.isfinite(bnd).all() and bnd.max() < (2e-3 if h * w < 4096 else 0.2)
    import torch

    want = torch.nn.functional.group_norm(torch.from_numpy(x.astype(np.float64)), G, torch.from_numpy(gamma.astype(np.float64)),
                                          torch.from_numpy(beta.astype(np.float64)), float(np.float64(f32(1e-5)))).numpy()
    assert np.abs(gn.group_norm_f64(x, G, gamma, beta, 1e-5) - want).max() < 1e-12


def test_module_state_dict_and_state_machine(i8ie):
    """an unconverted module (converting uploads g and b, so the converted round trip is in tests/test_gpu_groupnorm.py)"""
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.gn1 = i8ie.GroupNorm(3, 6, eps=1e-4)
            self.add1 = i8ie.Add()

    rng = np.random.default_rng(3)
    w, b = rng.normal(1, 0.3, 6).astype(f32), rng.normal(0, 0.3, 6).astype(f32)
    net = Net()
    net.load({"gn1.weight": w, "gn1.bias": b})
    assert np.array_equal(net.gn1.layer.weight(), w) and np.array_equal(net.gn1.layer.bias(), b)
    with pytest.raises(RuntimeError):
        net.quantized_state_dict()   # not converted
    net.gn1.set_output_qparams(0.03, 131)
    assert net.gn1.output_qparams() == (pytest.approx(0.03), 131) and not net.gn1.layer.is_quantized()
    with pytest.raises(RuntimeError):
        net.gn1.set_output_qparams(0.03, 256)
    assert [k for k, _ in net._layers()] == ["gn1", "add1"]


def test_private_binding_entries_are_the_recorded_ones():
    """tests/golden/binding_surface.json records the public names of _CXX_i8ie and stays as it is; the signatures and the
    overload order of the two private entries behind i8ie.GroupNorm / i8ie.group_norm are recorded here instead, the same way
    (every callable's __doc__, which pybind11 writes in registration order)"""
    import json
    import os

    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_surface_groupnorm.json")) as f:
        want = json.load(f)
    c = cx._GroupNorm
    names = sorted(n for n in dir(c) if not n.startswith("_") or n in ("__init__", "__call__"))
    assert names == sorted(want["_GroupNorm"]) and {n: getattr(c, n).__doc__ for n in names} == want["_GroupNorm"]
    assert cx._group_norm.__doc__ == want["_group_norm"]


NAME = "groupnorm_tiny"
GROUPNORMS = ("a_gn1", "a_gn2", "d_gn", "b_gn1", "b_gn2", "s_gn")
TRACED = ("pool",) + GROUPNORMS + ("a_add", "b_add", "s_sig", "s_mul", "s_c", "s_attn", "s_add", "gap")


def test_network_walk_discriminates_and_agrees_with_float64():
    """spec_ref's walk of groupnorm_tiny (the network of tests/test_gpu_groupnorm.py), on quantisation parameters from a float64
    forward: every GroupNorm output and the attention's scores, probabilities and result are spread, and the per-channel walk
    differs from the per-tensor one (the expected bytes tell the two modes apart)"""
    import mha_ref as mr
    import spec_ref as sr
    from int8inferenceengine_amd import workloads as wl

    entry = wl.network(NAME)
    sd = wl.synthetic_state_dict(NAME, sr.WEIGHT_SEED)
    x = wl.synthetic_input(NAME, 4, seed=sr.CALIB_SEED)
    qp, jqp = sr.fp32_qparams(entry, sd, x)
    assert sorted(qp) == sorted(entry[0]) == sorted(wl.layer_names(NAME))
    assert sorted(jqp) == sorted(["a_add", "b_add", "s_sig", "s_mul", "s_attn", "s_add", "s_attn" + mr.SCORES])
    outs = {}
    for pc in (False, True):
        trace = {}
        outs[pc] = sr.forward(entry, x, sr.quantize_layers(entry, sd, pc), qp, jqp, pc, sr.traces(mr.tracer(trace, jqp), sr.keeps(TRACED, trace)))
        assert outs[pc].shape == (4, 10) and sorted(trace) == sorted(TRACED + ("s_attn.S", "s_attn.P"))
        for k in GROUPNORMS:
            assert len(np.unique(trace[k])) >= 32 and ((trace[k] == 0) | (trace[k] == 255)).mean() < 0.05, k
        S, P = trace["s_attn.S"], trace["s_attn.P"]
        assert len(np.unique(S)) > 30 and ((S == 0) | (S == 255)).mean() < 0.05 and len(np.unique(P)) >= 16 and len(np.unique(trace["s_attn"])) >= 16
        assert trace["a_gn2"].shape == (4, 16, 8, 8) and trace["s_attn"].shape == (4, 20, 4, 4)
    assert not np.array_equal(outs[False], outs[True])
    assert (outs[False].argmax(1) == outs[True].argmax(1)).all()


def test_registry_networks_and_their_macs():
    from int8inferenceengine_amd import workloads as wl

    L, spec, shape = wl.network(NAME)
    assert shape == (3, 32, 32) and list(L) == ["c1", "a_c1", "a_gn1", "a_c2", "a_gn2", "down", "d_gn", "b_c1", "b_gn1", "b_c2", "b_gn2",
                                                "s_gn", "s_c", "s_qkv", "s_proj", "fc"]
    assert {a: v[1:] for a, v in L.items() if v[0] == "gn"} == {"a_gn1": (4, 16), "a_gn2": (16, 16), "d_gn": (5, 20), "b_gn1": (1, 20),
                                                                 "b_gn2": (10, 20), "s_gn": (4, 20)}
    assert wl.join_names(NAME) == ["a_add", "b_add", "s_sig", "s_mul", "s_attn", "s_add"] and wl.attention_names(NAME) == ["s_attn"]
    # SiLU: the GroupNorm's result is the Mul's first operand, its sigmoid the second
    i = spec.index(("layer", "s_gn"))
    assert spec[i + 1:i + 6] == [("save", "s_g"), ("act", "s_sig", "sigmoid"), ("save", "s_sig"), ("load", "s_g"), ("mul", "s_mul", "s_sig")]
    sd = wl.synthetic_state_dict(NAME, 3)
    assert sorted(sd) == sorted(k + s for k in L for s in (".weight", ".bias"))
    assert sd["b_gn2.weight"].shape == (20,) and 0.5 <= sd["b_gn2.weight"].min() and np.abs(sd["b_gn2.bias"]).max() <= 0.3
    # by hand: c1 16x16 x 16 x 27; two 3x3 convs 16 -> 16 at 8x8; down 4x4 x 20 x 144; at 4x4 three 3x3 convs 20 -> 20, the packed
    # 1x1 20 -> 60 and the 1x1 20 -> 20; fc 200.  GroupNorms, the SiLU and the products inside the Attention count nothing.
    assert wl.macs_per_image(NAME) == 256 * 16 * 27 + 2 * 64 * 16 * 144 + 16 * 20 * 144 + 16 * 20 * (3 * 180 + 60 + 20) + 200 == 650184
    R, rspec, _ = wl.network("groupnorm_resnet_cifar")
    B = wl.network("resnet18_cifar")[0]
    assert all(v[:2] == ("gn", 32) for v in R.values() if v[0] == "gn") and sum(v[0] == "gn" for v in R.values()) == 22
    assert [v for a, v in R.items() if v[0] == "conv" and not a.startswith("m_")] == [v for v in B.values() if v[0] == "conv"]
    assert R["m_qkv"] == ("conv", 256, 768, 1, 1, 0) and ("attention", "m_attn", 4) in rspec and R["fc"] == ("fc", 512, 10)
    # by hand: every weighted layer of resnet18_cifar (its pinned figure leaves the three 1x1 projections out: 3 x 2097152) and
    # the middle block at 8x8: 3x3 256 -> 256, 1x1 256 -> 768, 1x1 256 -> 256
    assert wl.macs_per_image("groupnorm_resnet_cifar") == 549131264 + 3 * 2097152 + 64 * 256 * (2304 + 768 + 256) == 609948672
