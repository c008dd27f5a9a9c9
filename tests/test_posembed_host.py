"""Position embedding and the class token without a GPU: the numpy restatement of the embedding against a
float64 cat + add within the header's bound, i8ie_posembed_table through ctypes, the argument rules of the C entries (refused
before any device call) and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import abi
import posembed_ref as pr
from support import i8ie  # noqa: F401

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return pr.bind(abi.lib())


def _first_diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else (tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


# ---- the embedding's restatement against the real numbers -----------------------------------------------------------------------
@pytest.mark.parametrize("class_token", [False, True])
@pytest.mark.parametrize("name", sorted(pr.SETS))
def test_restatement_against_float64_within_the_headers_bound(name, class_token):
    s_in, zp_in, s_out, zp_out = pr.SETS[name][:4]
    c, h, w = 20, 4, 5
    P, cls = pr.make_table(name, h * w + class_token, c, class_token)
    q = np.random.default_rng(3).integers(0, 256, (3, c, h, w), dtype=np.uint8)
    # two elements whose real value is an integer, or within a rounding of one: a byte at the zero point under a table entry of
    # 0, and under one of fl(3 * s_out)
    q[0, 0, 0, 0] = q[0, 1, 0, 1] = zp_in
    P[class_token + 0, 0], P[class_token + 1, 1] = 0.0, f32(3) * s_out
    got = pr.posembed_u8(q, pr.table(P, cls), class_token, s_in, zp_in, s_out, zp_out).astype(np.int64)
    y, B = pr.real_and_bound(q, P, cls, s_in, zp_in, s_out, zp_out)
    want = np.clip(np.trunc(np.clip(y, -1.0, 256.0)), 0, 255).astype(np.int64)
    near = np.abs(y - np.rint(y)) <= B  # y* within the bound of an integer: the byte may be either neighbour
    differ = got != want
    print(name, class_token, "elements near an integer: %d of %d, differing: %d" % (near.sum(), near.size, differ.sum()))
    assert not (differ & ~near).any(), (name, _first_diff(np.where(near, want, got), want))
    assert np.abs(got - want).max() <= 1
    assert near.any() and near.mean() < 0.5, (name, near.mean())  # such elements exist, and they are a minority


def test_table_entry_adds_the_class_token_into_row_0_only(lib):
    rng = np.random.default_rng(1)
    P, cls = rng.normal(0, 1, (7, 20)).astype(f32), rng.normal(0, 1, 20).astype(f32)
    rc, E = pr.c_table(lib, P, cls)
    assert rc == 0 and _first_diff(E.view(np.uint32), pr.table(P, cls).view(np.uint32)) is None
    assert np.array_equal(E[1:], P[1:]) and np.array_equal(E[0], (cls + P[0]).astype(f32)) and not np.array_equal(E[0], P[0])
    rc, E = pr.c_table(lib, P, None)
    assert rc == 0 and np.array_equal(E.view(np.uint32), P.view(np.uint32))


def test_c_entries_refuse_bad_arguments_before_any_device_call(lib):
    P, E = np.zeros((3, 4), f32), np.full((3, 4), 9, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = lib.i8ie_posembed_table
    assert t(None, None, 3, 4, p(E)) == -1 and b"null" in lib.i8ie_last_error()
    assert t(p(P), None, 3, 4, None) == -1 and b"null" in lib.i8ie_last_error()
    for tokens, c in ((0, 4), (3, 0), (3, 16385), (-1, 4)):
        assert t(p(P), None, tokens, c, p(E)) == -1 and b"dimension" in lib.i8ie_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        Pb = P.copy()
        Pb[2, 3] = bad
        assert t(p(Pb), None, 3, 4, p(E)) == -1 and b"finite" in lib.i8ie_last_error()
        cb = np.zeros(4, f32)
        cb[1] = bad
        assert t(p(P), p(cb), 3, 4, p(E)) == -1 and b"finite" in lib.i8ie_last_error()
    big = np.full((3, 4), 3e38, f32)  # finite entries whose sum is not
    assert t(p(big), p(big[0].copy()), 3, 4, p(E)) == -1 and b"finite" in lib.i8ie_last_error()
    assert (E == 9).all()  # an error is reported before anything is written
    assert t(p(P), None, 3, 4, p(E)) == 0 and (E == 0).all()

    one, ctx = C.c_void_p(64), C.c_void_p(64)  # (never dereferenced: every call below fails its argument check first)

    def u8(ctx=ctx, i=one, o=one, e=one, ib=0, ob=0, n=1, c=4, h=2, w=2, s_in=0.05, s_out=0.05):
        return lib.i8ie_posembed_u8_nhwc(ctx, i, ib, 0, o, ob, 0, n, c, h, w, 1, e, s_in, 128, s_out, 128, 0)

    for kw in ({"ctx": None}, {"i": None}, {"o": None}, {"e": None}):
        assert u8(**kw) == -1 and b"null" in lib.i8ie_last_error(), kw
    for kw in ({"ib": -1}, {"ob": -1}, {"n": 0}, {"c": 0}, {"c": 16385}, {"h": 0}, {"w": -2}, {"h": 1 << 15, "w": 1 << 15}):
        assert u8(**kw) == -1 and b"dimension" in lib.i8ie_last_error(), kw
    for kw in ({"s_in": np.nan}, {"s_in": np.inf}, {"s_in": 3e36}, {"s_out": np.nan}, {"s_out": np.inf}, {"s_out": 0.0}, {"s_out": -0.5}):
        assert u8(**kw) == -1 and b"scale" in lib.i8ie_last_error(), kw
    assert u8(e=C.c_void_p(66)) == -1 and b"aligned" in lib.i8ie_last_error()

    def f(ctx=ctx, i=one, o=one, e=one, n=1, c=4, h=2, w=2):
        return lib.i8ie_posembed_f32(ctx, i, o, n, c, h, w, 0, e)

    for kw in ({"ctx": None}, {"i": None}, {"o": None}, {"e": None}):
        assert f(**kw) == -1 and b"null" in lib.i8ie_last_error(), kw
    for kw in ({"n": 0}, {"c": 0}, {"c": 16385}, {"h": 0}, {"w": 0}):
        assert f(**kw) == -1 and b"dimension" in lib.i8ie_last_error(), kw
    assert f(i=C.c_void_p(66)) == -1 and b"aligned" in lib.i8ie_last_error()


def test_new_symbols_are_declared_and_exported(lib):
    names = abi.declared_symbols()
    for n in ["i8ie_posembed_table", "i8ie_posembed_u8_nhwc", "i8ie_posembed_f32"]:
        assert n in names and hasattr(lib, n), n
    header = open(abi.HEADER).read()
    assert "#define I8IE_POSEMBED_WALK %d\n" % pr.WALK in header


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_surface_names_and_constructor_rules(i8ie):
    import _CXX_i8ie as cx

    for n in ("PositionEmbedding", "position_embedding"):
        assert n in i8ie.__all__ and hasattr(i8ie, n)
    # (the extension's entries are private: its public names are recorded whole in tests/golden/binding_surface.json)
    assert hasattr(cx, "_PositionEmbedding") and hasattr(cx, "_position_embedding")
    assert not hasattr(cx._PositionEmbedding, "set_output_qparams")  # (tests/golden/binding_surface_calibration.json stays as it is)
    assert not hasattr(cx, "PositionEmbedding") and not hasattr(cx, "position_embedding")
    pe = i8ie.PositionEmbedding(16, 2, 3)
    assert isinstance(pe, i8ie.layer.Norm) and (pe.channels, pe.height, pe.width, pe.class_token) == (16, 2, 3, False)
    assert pe.layer.weight().shape == (6, 16) and pe.layer.bias() is None and pe.output_qparams() == (1.0, 0)
    assert i8ie.PositionEmbedding(16, 2, 3, class_token=True).layer.weight().shape == (7, 16)
    for bad in ((0, 2, 3), (16385, 2, 3), (16, 0, 3), (16, 2, -1)):
        with pytest.raises(RuntimeError, match="position_embedding"):
            i8ie.PositionEmbedding(*bad)
    for fn in (pe.weight_scale, pe.weight_scales, pe.q_weight, pe.q_bias):
        with pytest.raises(RuntimeError, match="no INT8 weights"):
            fn()


def test_parameter_loading_rules(i8ie):
    pe, pc = i8ie.PositionEmbedding(4, 2, 3), i8ie.PositionEmbedding(4, 2, 3, class_token=True)
    w6, w7 = np.arange(24, dtype=f32).reshape(6, 4), np.arange(28, dtype=f32).reshape(7, 4)
    pe.load_weight(w6)
    pc.load_weight(w7)
    assert np.array_equal(pe.layer.weight(), w6) and np.array_equal(pc.layer.weight(), w7)
    for layer, bad in ((pe, w7), (pc, w6), (pe, w6.T), (pe, w6.ravel()), (pc, w7[None])):
        with pytest.raises(RuntimeError, match="weight must be float32"):
            layer.load_weight(bad)
    pc.load_bias(np.array([1, 2, 3, 4], f32))
    assert pc.layer.bias().tolist() == [1, 2, 3, 4]
    for bad in (np.zeros(3, f32), np.zeros((4, 1), f32)):
        with pytest.raises(RuntimeError, match="bias must be float32"):
            pc.load_bias(bad)
    with pytest.raises(RuntimeError, match="class_token"):
        pe.load_bias(np.zeros(4, f32))


def test_module_load_and_layers_see_the_layer(i8ie):
    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.pos = i8ie.PositionEmbedding(4, 1, 2, class_token=True)
            self.plain = i8ie.PositionEmbedding(4, 1, 2)
            self.act = i8ie.Activation("hardswish")

    net = Net()
    w3, w2, b = np.full((3, 4), 2, f32), np.full((2, 4), 3, f32), np.full(4, 5, f32)
    net.load({"pos.weight": w3, "pos.bias": b, "plain.weight": w2, "act.other": 1})
    assert [k for k, _ in net._layers()] == ["pos", "plain", "act"]
    assert np.array_equal(net.pos.layer.weight(), w3) and np.array_equal(net.pos.layer.bias(), b) and np.array_equal(net.plain.layer.weight(), w2)
    with pytest.raises(RuntimeError, match="class_token"):
        net.load({"plain.bias": b})
    with pytest.raises(RuntimeError, match="not converted"):
        net.quantized_state_dict()


def test_functional_form_argument_rules(i8ie):
    x = i8ie.tensor(np.zeros((1, 4, 1, 2), f32))
    with pytest.raises(TypeError, match="takes no scale"):
        i8ie.position_embedding(x, np.zeros((2, 4), f32), scale=0.1, zero_point=3)
    with pytest.raises(TypeError, match="takes no scale"):
        i8ie.position_embedding(x, np.zeros((2, 4), f32), zero_point=3)
