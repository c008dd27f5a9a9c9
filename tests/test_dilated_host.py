"""Dilated Conv2d without a GPU: inflate() against torch's dilation= in float64 on the CPU (exact on
integer-valued data), inflation against both weight quantisers of the library, the argument rules of the C entries (made
before any device call), the Python surface, the two networks' MAC counts and registry, and the GPU case lists of
tests/dilated_ref.py class by class, so that a class cannot silently leave them."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import dilated_ref as dl
from support import i8ie  # noqa: F401


def _torch_cases():
    out = []
    for d, k, s, g in itertools.product((1, 2, 3, 4), (2, 3, 5), (1, 2), ("1", "2", "dw")):
        for p in sorted({0, 1, d, d * (k - 1) // 2, d * (k - 1)}):
            out.append((d, k, s, p, g))
    return out


def test_inflate_equals_torch_dilation():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    seen = 0
    for d, k, s, p, g in _torch_cases():
        c = 4
        groups = {"1": 1, "2": 2, "dw": c}[g]
        kc = 2 * c if g == "dw" else 6 if g == "1" else 4
        h, w = d * (k - 1) + 4, d * (k - 1) + 7  # h != w, both at least the inflated kernel without padding
        x = rng.integers(-9, 10, (2, c, h, w)).astype(np.float64)
        wt = rng.integers(-9, 10, (kc, c // groups, k, k)).astype(np.float64)
        b = rng.integers(-9, 10, kc).astype(np.float64)
        F = torch.nn.functional
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=s, padding=p, dilation=d, groups=groups)
        got = F.conv2d(torch.from_numpy(x), torch.from_numpy(dl.inflate(wt, d)), torch.from_numpy(b), stride=s, padding=p, groups=groups)
        assert tuple(got.shape[2:]) == dl.out_hw(h, w, k, s, p, d), (d, k, s, p, g)
        assert torch.equal(got, want), (d, k, s, p, g)
        # ... and the helper module's own float64 composition on the inflated weights
        ref = dl.gr.conv2d_f64(x, dl.inflate(wt, d), b, groups, s, p)
        assert np.array_equal(ref, want.numpy()), (d, k, s, p, g)
        seen += 1
    assert seen >= 4 * 3 * 2 * 3 * 3
    w = np.arange(8).reshape(2, 2, 2) + 1
    assert dl.inflate(w, 1) is not w and np.array_equal(dl.inflate(w, 1), w)
    assert dl.inflate(w, 3).shape == (2, 4, 4) and dl.inflate(w, 3).sum() == w.sum() and dl.inflate(w, 3)[1, 3, 3] == 8


@pytest.mark.parametrize("d", [2, 3, 4])
def test_inflation_commutes_with_both_quantisers(d):
    lib = abi.lib()
    rng = np.random.default_rng(d)
    w = rng.normal(0, 0.2, (6, 4, 3, 3)).astype(np.float32)
    b = rng.normal(0, 0.2, 6).astype(np.float32)
    wi = np.ascontiguousarray(dl.inflate(w, d))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def per_tensor(wt):
        qw, qb, s = np.zeros(wt.shape, np.int8), np.zeros(6, np.int8), C.c_float(0)
        assert lib.i8ie_quantize_weight(P(wt), C.c_int64(wt.size), P(b), C.c_int64(6), P(qw), P(qb), C.byref(s)) == 0
        return qw, qb, np.float32(s.value)

    def per_channel(wt):
        qw, qb, s = np.zeros(wt.shape, np.int8), np.zeros(6, np.int8), np.zeros(6, np.float32)
        assert lib.i8ie_quantize_weight_per_channel(P(wt), 6, C.c_int64(wt.size // 6), P(b), P(qw), P(qb), P(s)) == 0
        return qw, qb, s

    for f in (per_tensor, per_channel):
        (qw, qb, s), (qwi, qbi, si) = f(w), f(wi)
        assert np.array_equal(dl.inflate(qw, d), qwi) and np.array_equal(qb, qbi)
        assert np.array_equal(np.asarray(s).view(np.uint32), np.asarray(si).view(np.uint32))
        # (the weight sums and with them the offset vector are those of the compact kernel)
        assert np.array_equal(qw.reshape(6, -1).astype(np.int64).sum(1), qwi.reshape(6, -1).astype(np.int64).sum(1))


def test_new_symbols_are_declared_and_exported():
    names = abi.declared_symbols()
    lib = abi.lib()
    for n in dl.SYMBOLS:
        assert n in names and hasattr(lib, n), n
    assert lib.i8ie_version() == 1


def test_argument_rules_before_any_device_call():
    lib = dl.bind(abi.lib())
    qw, qb, sw = np.zeros((4, 4 * 9), np.int8), np.zeros(4, np.int8), np.ones(4, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L = C.c_void_p()
    one = C.c_float(1)
    for bad in (0, -3):  # dilation is one integer >= 1 (a null ctx: the check must come first and leave a message)
        assert lib.i8ie_conv2d_create_dilated(None, P(qw), P(qb), 4, 4, 3, 3, 1, 1, 1, bad, C.c_float(0.5), C.byref(L)) == -1
        assert b"dilation" in lib.i8ie_last_error()
        assert lib.i8ie_conv2d_create_dilated_per_channel(None, P(qw), P(qb), 4, 4, 3, 3, 1, 1, 1, bad, P(sw), C.byref(L)) == -1
        assert b"dilation" in lib.i8ie_last_error()
        assert lib.i8ie_conv2d_u8s8_dilated(None, None, 1, 4, 8, 8, None, 4, 3, 3, 1, 1, 1, bad, 0, None, one, one, one, 0, None, None) == -1
        assert b"dilation" in lib.i8ie_last_error()
        assert lib.i8ie_conv2d_f32_dilated(None, None, 1, 4, 8, 8, None, None, 4, 3, 3, 1, 1, 1, bad, None) == -1
        assert b"dilation" in lib.i8ie_last_error()
    # the groups rules hold as on the grouped entries
    assert lib.i8ie_conv2d_create_dilated(None, P(qw), P(qb), 4, 4, 3, 3, 1, 1, 3, 2, C.c_float(0.5), C.byref(L)) == -1
    assert b"groups" in lib.i8ie_last_error()
    # k~ = d (k - 1) + 1 <= H + 2 p and <= W + 2 p: 3x3 at rate 4 spans 9; 6 + 2 = 8 rows do not hold it, 7 + 2 = 9 do
    for h, w in ((6, 9), (9, 6)):
        assert lib.i8ie_conv2d_u8s8_dilated(None, None, 1, 4, h, w, None, 4, 3, 3, 1, 1, 1, 4, 0, None, one, one, one, 0, None, None) == -1
        assert b"kernel larger than padded input" in lib.i8ie_last_error()
        assert lib.i8ie_conv2d_f32_dilated(None, None, 1, 4, h, w, None, None, 4, 3, 3, 1, 1, 1, 4, None) == -1
        assert b"kernel larger than padded input" in lib.i8ie_last_error()
    # (7 x 7 with padding 1 passes the geometry and stops at the null pointers)
    assert lib.i8ie_conv2d_u8s8_dilated(None, None, 1, 4, 7, 7, None, 4, 3, 3, 1, 1, 1, 4, 0, None, one, one, one, 0, None, None) == -1
    assert b"null" in lib.i8ie_last_error()
    assert lib.i8ie_conv2d_f32_dilated(None, None, 1, 4, 7, 7, None, None, 4, 3, 3, 1, 1, 1, 4, None) == -1
    assert b"null" in lib.i8ie_last_error()
    assert lib.i8ie_layer_dilation(None, None) == -1 and b"null" in lib.i8ie_last_error()


def test_conv2d_dilation_surface(i8ie):
    assert i8ie.Conv2d(4, 4, 3, dilation=2).dilation() == 2
    assert i8ie.Conv2d(4, 4, 3, padding=2, groups=4, dilation=3).dilation() == 3
    assert i8ie.Conv2d(4, 4, 3).dilation() == 1 and i8ie.Conv2d(4, 4, 1, dilation=5).dilation() == 5
    assert i8ie.Linear(4, 4).dilation() == 1 and i8ie.ConvTranspose2d(4, 4, 2, 2).dilation() == 1
    for bad in (0, -1):
        with pytest.raises(RuntimeError):
            i8ie.Conv2d(4, 4, 3, dilation=bad)
    L = i8ie.Conv2d(4, 6, 3, groups=2, dilation=2)
    L.load_weight(np.zeros((6, 2, 3, 3), np.float32))  # (the weight keeps its compact shape)
    with pytest.raises(RuntimeError):
        L.load_weight(np.zeros((6, 2, 5, 5), np.float32))


def test_networks_registry_and_macs():
    from int8inferenceengine_amd import workloads as wl

    assert wl.conv_dilation(("conv", 3, 4, 3, 1, 1)) == 1 and wl.conv_dilation(("conv", 3, 4, 3, 1, 1, 1)) == 1
    assert wl.conv_dilation(("conv", 3, 4, 3, 1, 2, 1, 2)) == 2
    assert wl.macs_per_image("alexnet") == wl.ALEXNET_MACS_PER_IMAGE  # (the pinned figures stay)
    # aspp_tiny by hand, true taps (9 per 3x3 whatever the rate), every branch counted
    stem, down, atr = 16 * 16 * 16 * 3 * 9, 8 * 8 * 32 * 16 * 9, 64 * 32 * 32 * 9
    a1, a2, a3, a4 = 64 * 16 * 32, 64 * 16 * 32 * 9, 64 * 20 * 32 * 9, 64 * 32 * 9 + 64 * 16 * 32
    a5, proj, head = 16 * 32, 64 * 32 * 84, 64 * 10 * 32
    assert wl.macs_per_image("aspp_tiny") == stem + down + atr + a1 + a2 + a3 + a4 + a5 + proj + head
    # deeplabv3_cifar: resnet18_cifar's stem and stages 1-3 with their projections, stage 4 at 8 x 8, the pyramid, the head
    s = 1024 * 64 * 3 * 9 + 4 * 1024 * 64 * 64 * 9
    s += 256 * 128 * 64 * 9 + 3 * 256 * 128 * 128 * 9 + 256 * 128 * 64
    s += 64 * 256 * 128 * 9 + 3 * 64 * 256 * 256 * 9 + 64 * 256 * 128
    s += 64 * 512 * 256 * 9 + 3 * 64 * 512 * 512 * 9 + 64 * 512 * 256
    s += 64 * 128 * 512 + 3 * 64 * 128 * 512 * 9 + 128 * 512 + 64 * 128 * 640 + 64 * 10 * 128
    assert wl.macs_per_image("deeplabv3_cifar") == s
    layers = wl.network("deeplabv3_cifar")[0]
    assert [wl.conv_dilation(layers[a]) for a in ("s3b2c2", "s4b1c1", "s4b2c2", "s4b1proj", "aspp_r2", "aspp_r4", "aspp_r6")] == \
        [1, 2, 2, 1, 2, 4, 6]
    assert all(L[5] == wl.conv_dilation(L) for L in layers.values() if wl.conv_dilation(L) > 1)  # padding = rate
    sd = wl.synthetic_state_dict("aspp_tiny")
    assert sd["a4d.weight"].shape == (32, 1, 3, 3) and sd["a3.weight"].shape == (20, 32, 3, 3)
    assert wl.synthetic_input("deeplabv3_cifar", 2).shape == (2, 3, 32, 32)
    assert wl.layer_names("aspp_tiny")[:4] == ["stem", "down", "atr", "a1"] and wl.add_names("aspp_tiny") == ["res"]
    assert wl.concat_names("deeplabv3_cifar") == ["aspp_cat"]
    net = wl.build("aspp_tiny")
    assert [getattr(net, a).dilation() for a in ("stem", "atr", "a1", "a2", "a3", "a4d")] == [1, 2, 1, 2, 3, 2]
    assert net.a4d.groups() == 32
    net.load(sd)


# ---- the GPU case lists --------------------------------------------------------------------------------------------------
def _plain(pred):
    return [c for c in dl.CASES if not c.force and not c.extreme and c.zp_in == dl.ZP_IN and pred(c)]


def test_case_lists_cover_every_class():
    names = [c.name for c in dl.CASES]
    assert len(set(names)) == len(names)
    for c in dl.CASES:
        Cg, Ng, Kg, oh, ow = dl.geom(c)
        assert c.d >= 2 and c.k >= 2 and oh > 0 and ow > 0 and c.c % c.g == 0 and c.kc % c.g == 0, c.name
        assert c.m * c.c * c.h * c.w <= 1 << 17, c.name  # (a fraction of a second each)
    dense = _plain(dl.dconv_takes)
    assert {c.name.rsplit("-", 1)[0] for c in dense} == {n for n, _ in dl.DENSE_S1}
    for pc in (False, True):  # every class per tensor and per channel
        D = [c for c in dense if c.pc == pc]
        assert len(D) == 12 and all(dl.dispatch(c).kernel == "dconv_mfma" for c in D)
        assert any(c.c > 64 and dl.dconv_chunk(c.c) == 64 for c in D) and any(dl.dconv_chunk(c.c) == 32 for c in D)  # chunked K
        assert any(c.c < 64 and c.c % 32 for c in D)                       # a chunk that is no power of two (48)
        assert any(-(-dl.geom(c)[3] // c.d) > 4 and -(-dl.geom(c)[4] // c.d) > 8 for c in D)  # several tiles per plane, both ways
        assert any(c.m * c.d * c.d % dl.DCONV_SLOTS for c in D)            # a last block with empty slots
        assert any(c.h % c.d or c.w % c.d for c in D)                      # phases of unequal size
        assert any(c.kc % 16 for c in D) and any(c.kc > 64 for c in D)     # ragged features; a second feature tile
        assert any(c.h <= c.d and c.w <= c.d for c in D)                   # only the centre tap inside
        assert any(c.p == 0 for c in D) and any(c.p % c.d for c in D) and any(2 * c.p > c.d * (c.k - 1) for c in D)
        assert any(c.k == 5 for c in D) and any(c.k % 2 == 0 for c in D)
        assert any(dl.geom(c)[2] % 64 for c in D)                          # a K tail
        assert any(c.d == 6 and c.m % 2 and c.m * dl.geom(c)[3] * dl.geom(c)[4] > 128 for c in D)  # many images, several tiles
        G = [c for c in _plain(lambda c: not dl.dconv_takes(c)) if c.pc == pc]
        assert any(c.g == 1 and c.s == 1 and c.c % 16 == 0 and c.k > 8 for c in G)   # declined: the LDS plan does not fit
        # (K < 32 cannot be reached by a layer with C % 16 == 0 and k >= 2: the rule only guards the kernel's K step)
        kinds = {(dl.dispatch(c).kernel, dl.dispatch(c).G, dl.dispatch(c).dot4) for c in G}
        assert kinds >= {("gconv_mfma", 16, None), ("gconv_mfma", 4, None), ("gconv_mfma", 1, None), ("gconv_direct", None, False)}
        assert any(c.s == 2 and c.g == 1 for c in G) and any(c.g == 2 for c in G)
        assert {c.s for c in G if c.g == c.c} == {1, 2}                    # atrous depthwise at both strides
        F = [c for c in dl.CASES if c.force and c.pc == pc]
        assert len(F) == 12 and all(dl.dispatch(c) == dl.Dispatch("gconv_direct", None, True) for c in F)
    assert {c.zp_in for c in dl.CASES if c.p > 0} >= {0, 255, dl.ZP_IN}
    assert {dl.dispatch(c).kernel for c in dl.CASES if c.extreme} == {"dconv_mfma", "gconv_direct"}
    assert {(dl.dispatch(c).kernel, c.zp_in) for c in dl.CASES if c.p > 0 and c.zp_in in (0, 255)} == {
        ("dconv_mfma", 0), ("dconv_mfma", 255), ("gconv_direct", 0), ("gconv_direct", 255)}
    for n in dl.LAYOUT_CASES:
        c = dl.BY_NAME[n]
        assert c.kc % 16 == 0 and c.p >= 2  # (re-biased output; an in_border narrower than the padding exists)
    assert dl.BY_NAME[dl.LAYOUT_CASES[0]].g == 1 and dl.BY_NAME[dl.LAYOUT_CASES[1]].g > 1


def test_reference_is_the_oracle_on_inflated_weights(orc):
    c = dl.BY_NAME["byte_gather-pt"]
    d = dl.reference(c)
    assert d["qwi"].shape == (9, 6, 5, 5) and np.array_equal(d["qwi"][:, :, ::2, ::2], d["qw"])
    want, acc = orc.conv2d(d["q"], d["qwi"], d["qb"], c.s, c.p, dl.S_IN, c.zp_in, d["s_w"], d["s_out"], dl.ZP_OUT, want_acc=True)
    assert np.array_equal(want, d["want"]) and np.array_equal(acc, d["acc"])
    assert len(np.unique(d["want"])) > 30  # (not sitting on a clamp)
    assert dl.reference(dl.BY_NAME["phases_unequal-pt-forced"]) is dl.reference(dl.BY_NAME["phases_unequal-pt"])
