"""Resize to any size and adaptive average pooling without a GPU: the integer restatement of
tests/resize_ref.py against torch's CPU interpolate / adaptive_avg_pool2d in float64 over every (L, O) in 1..32, the integer
nearest rule against Fraction and against torch over 1..64, equality with the restatements of the ops the new ones generalise
(upsample at all 64 factor pairs, avg_pool2d at uniform windows, the global pool), i8ie_resize_axis bit for bit, every
I8IE_ERR_ARG rule of the C entries, and the Python surface (argument errors, routing, __all__)."""
import ctypes as C
from fractions import Fraction
import itertools

import numpy as np
import pytest

import abi
import avgpool_ref as ar
import resize_ref as rr
import support
from support import i8ie  # noqa: F401
import upsample_ref as ur

f32 = np.float32
PAIRS32 = list(itertools.product(range(1, 33), repeat=2))  # (L, O)


def _two_axes():
    """every (L, O) in 1..32 once as (h, oh) and once as (w, ow), the two of a case distinct"""
    n = len(PAIRS32)
    for k in range(n):
        (h, oh), (w, ow) = PAIRS32[k], PAIRS32[(k * 37 + 11) % n]  # (37 is a unit mod 1024: a permutation)
        yield h, oh, w, ow


def test_two_axes_covers_every_pair_on_both_axes():
    cases = list(_two_axes())
    assert sorted((h, oh) for h, oh, _, _ in cases) == PAIRS32 and sorted((w, ow) for _, _, w, ow in cases) == PAIRS32
    assert sum((h, oh) != (w, ow) for h, oh, w, ow in cases) >= len(cases) - 1


# ---- the restatement against torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,align", [(rr.BILINEAR, False), (rr.ALIGNED, True)], ids=["not_aligned", "aligned"])
def test_bilinear_against_torch_float64(mode, align):
    """S / D is torch's bilinear value to 1e-9 (float64 has 53 bits and a blend is a handful of operations on values <= 255:
    three orders above anything float64 produces, six below one step of 1 / D), and the byte is within half a code of it"""
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(5)
    worst = 0.0
    for h, oh, w, ow in _two_axes():
        q = rng.integers(0, 256, (1, 2, h, w), dtype=np.uint8)
        want = F.interpolate(torch.from_numpy(q.astype(np.float64)), size=(oh, ow), mode="bilinear", align_corners=align).numpy()
        S, D = rr.bilinear_sd(q, oh, ow, mode)
        err = float(np.abs(S / float(D) - want).max())
        worst = max(worst, err)
        assert err <= 1e-9, (h, oh, w, ow, err)
        out = rr.resize_u8(q, oh, ow, mode)
        assert out.shape == (1, 2, oh, ow) and out.dtype == np.uint8
        assert np.abs(out.astype(np.float64) - want).max() <= 0.5 + 1e-9
        assert np.array_equal(rr.bilinear_f64(q, oh, ow, mode), S / float(D))
    print("worst |S/D - torch| = %.3g" % worst)


def test_nearest_rule_against_fraction_and_torch():
    """the integer rule is floor(o L / O) everywhere; torch's float rule differs only where o L is a multiple of O, and there
    by exactly one index down"""
    import torch
    import torch.nn.functional as F

    differ = []
    for L, O in itertools.product(range(1, 65), repeat=2):
        i0, i1, w0, w1, den = rr.axis(L, O, rr.NEAREST)
        assert den == 1 and np.array_equal(i0, i1) and (w0 == 1).all() and (w1 == 0).all()
        assert i0.tolist() == [int(Fraction(o * L, O).__floor__()) for o in range(O)], (L, O)
        t = F.interpolate(torch.arange(L, dtype=torch.float64).reshape(1, 1, 1, L), size=(1, O), mode="nearest").numpy().ravel().astype(np.int64)
        for o in np.flatnonzero(t != i0):
            assert (o * L) % O == 0 and t[o] == i0[o] - 1, (L, O, int(o), int(t[o]), int(i0[o]))
            differ.append((L, O, int(o)))
    print("%d outputs differ from torch's nearest, e.g. %s" % (len(differ), differ[:4]))


def test_adaptive_windows_and_mean_against_torch_float64():
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(6)
    worst = 0.0
    for L, O in PAIRS32:
        s, l = rr.windows(L, O)
        assert s.min() >= 0 and l.min() >= 1 and (s + l).max() <= L and s[0] == 0 and (s + l)[-1] == L
        assert len(set(l.tolist())) <= 2 and l.max() - l.min() <= 1  # at most two window lengths, one apart
        assert s.tolist() == [(i * L) // O for i in range(O)] and (s + l).tolist() == [-((-(i + 1) * L) // O) for i in range(O)]
    for h, oh, w, ow in _two_axes():
        q = rng.integers(0, 256, (1, 2, h, w), dtype=np.uint8)
        want = F.adaptive_avg_pool2d(torch.from_numpy(q.astype(np.float64)), (oh, ow)).numpy()
        S, n = rr.adaptive_sn(q, oh, ow)
        err = float(np.abs(S / n.astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= 1e-9, (h, oh, w, ow, err)
        assert np.abs(rr.adaptive_u8(q, oh, ow).astype(np.float64) - want).max() <= 0.5 + 1e-9
    print("worst |S/n - torch| = %.3g" % worst)


# ---- where the new ops are the existing ones ---------------------------------------------------------------------------------
def test_equals_upsample_at_all_64_factor_pairs():
    rng = np.random.default_rng(7)
    q = rng.integers(0, 256, (2, 3, 3, 5), dtype=np.uint8)
    q.flat[0], q.flat[-1] = 0, 255
    x = (rng.standard_normal(q.shape) * 3).astype(f32)
    for fh, fw in itertools.product(range(1, 9), repeat=2):
        oh, ow = 3 * fh, 5 * fw
        for name, mode in (("nearest", rr.NEAREST), ("bilinear", rr.BILINEAR)):
            assert np.array_equal(rr.resize_u8(q, oh, ow, mode), ur.upsample_u8(q, fh, fw, name)), (fh, fw, name)
            assert np.array_equal(rr.resize_u8(q, oh, ow, mode, True, 99), ur.upsample_u8(q, fh, fw, name, True, 99))
            assert np.array_equal(rr.resize_f32(x, oh, ow, mode).view(np.uint32), ur.upsample_f32(x, fh, fw, name).view(np.uint32)), (fh, fw, name)


def test_equals_avg_pool_at_uniform_windows_and_the_global_pool():
    rng = np.random.default_rng(8)
    q = rng.integers(0, 256, (2, 3, 12, 8), dtype=np.uint8)
    x = rng.standard_normal(q.shape).astype(f32)
    for oh, ow in [(12, 8), (6, 4), (3, 2), (4, 8), (2, 1), (12, 2), (1, 1)]:
        kh, kw = 12 // oh, 8 // ow
        # (torch's avg_pool2d takes a rectangular window and stride; the restatement's single stride covers kh == kw and one-row outputs)
        if kh == kw:
            assert np.array_equal(rr.adaptive_u8(q, oh, ow), ar.avg_pool2d_u8(q, kh, kw, kh))
            assert np.array_equal(rr.adaptive_f32(x, oh, ow).view(np.uint32), ar.avg_pool2d_f32(x, kh, kw, kh).view(np.uint32))
        S, n = rr.adaptive_sn(q, oh, ow)
        assert (n == kh * kw).all()
        assert np.array_equal(S, q.astype(np.int64).reshape(2, 3, oh, kh, ow, kw).sum(axis=(3, 5)))
    assert np.array_equal(rr.adaptive_u8(q, 1, 1), ar.global_avg_pool2d_u8(q))
    assert np.array_equal(rr.adaptive_u8(q, 1, 1, True, 200), ar.global_avg_pool2d_u8(q, True, 200))


def test_rounding_is_to_nearest_ties_up():
    q = np.array([0, 1], np.uint8).reshape(1, 1, 1, 2)
    assert rr.resize_u8(q, 1, 3, rr.ALIGNED).ravel().tolist() == [0, 1, 1]  # the middle is 1/2: up
    assert rr.resize_u8(q + 254, 1, 3, rr.ALIGNED).ravel().tolist() == [254, 255, 255]
    assert rr.adaptive_u8(q, 1, 1).ravel().tolist() == [1]
    for mode in (rr.BILINEAR, rr.ALIGNED):
        for (L, O) in [(3, 8), (7, 3), (5, 5), (1, 4)]:
            i0, i1, w0, w1, den = rr.axis(L, O, mode)
            assert (w0 + w1 == den).all() and w0.min() >= 1 and w1.min() >= 0 and i0.min() >= 0 and i1.max() <= L - 1
        full = np.full((1, 1, 3, 5), 255, np.uint8)
        S, D = rr.bilinear_sd(full, 7, 11, mode)
        assert (S == 255 * D).all() and (rr.resize_u8(full, 7, 11, mode) == 255).all()
    assert 255 * rr.MAX_D + rr.MAX_D // 2 < 2 ** 31


# ---- the C entries --------------------------------------------------------------------------------------------------------
lib = support.lib_fixture(rr)


def test_resize_axis_bit_for_bit(lib):
    for mode in (rr.NEAREST, rr.BILINEAR, rr.ALIGNED):
        for L, O in PAIRS32 + [(5, 100000), (1 << 30, 3), (7, 1 << 20)]:
            i0, i1, w0, w1, den = rr.axis(L, O, mode)
            for o in (range(O) if O <= 32 else (0, 1, O // 2, O - 2, O - 1)):
                assert rr.c_axis(lib, L, O, mode, o) == (int(i0[o]), int(i1[o]), int(w0[o]), int(w1[o]), int(den)), (mode, L, O, o)


def test_new_symbols_are_declared_and_exported(lib):
    names = ["i8ie_resize_axis", "i8ie_resize2d_u8", "i8ie_resize2d_u8_nhwc", "i8ie_resize2d_f32", "i8ie_adaptive_avgpool2d_u8",
             "i8ie_adaptive_avgpool2d_u8_nhwc", "i8ie_adaptive_avgpool2d_f32"]
    for name in names:
        assert name in abi.declared_symbols() and hasattr(lib, name), name
    header = open(abi.HEADER).read()
    for line in ("#define I8IE_RESIZE_NEAREST 0", "#define I8IE_RESIZE_BILINEAR 1", "#define I8IE_RESIZE_BILINEAR_ALIGNED 2"):
        assert line in header


def test_every_argument_error_comes_before_any_device_call(lib):
    """no GPU is needed: the context is a zeroed host buffer, which only a call that got past its argument checks would use
    (and then fail differently: no rc of -1)"""
    fake = np.zeros(4096, np.uint8)
    h = p = fake.ctypes.data_as(C.c_void_p)
    v = [C.c_int(0) for _ in range(5)]
    r = [C.byref(x) for x in v]
    bad = {
        "axis null": lib.i8ie_resize_axis(3, 4, 1, 0, None, r[1], r[2], r[3], r[4]),
        "axis L": lib.i8ie_resize_axis(0, 4, 1, 0, *r), "axis O": lib.i8ie_resize_axis(3, 0, 1, 0, *r),
        "axis O big": lib.i8ie_resize_axis(3, (1 << 30) + 1, 1, 0, *r),
        "axis mode": lib.i8ie_resize_axis(3, 4, 3, 0, *r), "axis o": lib.i8ie_resize_axis(3, 4, 1, 4, *r), "axis o<0": lib.i8ie_resize_axis(3, 4, 1, -1, *r),
    }
    for name, fn in (("u8", lib.i8ie_resize2d_u8), ("f32", lib.i8ie_resize2d_f32)):
        bad.update({
            name + " ctx": fn(None, p, p, 1, 4, 2, 2, 3, 3, 1), name + " in": fn(h, None, p, 1, 4, 2, 2, 3, 3, 1), name + " out": fn(h, p, None, 1, 4, 2, 2, 3, 3, 1),
            name + " n": fn(h, p, p, 0, 4, 2, 2, 3, 3, 1), name + " c": fn(h, p, p, 1, -1, 2, 2, 3, 3, 1), name + " h": fn(h, p, p, 1, 4, 0, 2, 3, 3, 1),
            name + " w": fn(h, p, p, 1, 4, 2, 0, 3, 3, 1), name + " oh": fn(h, p, p, 1, 4, 2, 2, 0, 3, 1), name + " ow": fn(h, p, p, 1, 4, 2, 2, 3, -2, 1),
            name + " mode": fn(h, p, p, 1, 4, 2, 2, 3, 3, 3), name + " mode<0": fn(h, p, p, 1, 4, 2, 2, 3, 3, -1),
            name + " D": fn(h, p, p, 1, 1, 2, 2, 1024, 1025, 1), name + " D aligned": fn(h, p, p, 1, 1, 2, 2, 2049, 2050, 2),
        })
    nh = lib.i8ie_resize2d_u8_nhwc
    bad.update({
        "nhwc ctx": nh(None, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 3, 3, 1, 0, 0), "nhwc in": nh(h, None, 0, 0, p, 0, 0, 1, 4, 2, 2, 3, 3, 1, 0, 0),
        "nhwc out": nh(h, p, 0, 0, None, 0, 0, 1, 4, 2, 2, 3, 3, 1, 0, 0), "nhwc in_border": nh(h, p, -1, 0, p, 0, 0, 1, 4, 2, 2, 3, 3, 1, 0, 0),
        "nhwc out_border": nh(h, p, 0, 0, p, -1, 0, 1, 4, 2, 2, 3, 3, 1, 0, 0), "nhwc n": nh(h, p, 0, 0, p, 0, 0, 0, 4, 2, 2, 3, 3, 1, 0, 0),
        "nhwc oh": nh(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 0, 3, 1, 0, 0), "nhwc mode": nh(h, p, 0, 0, p, 0, 0, 1, 4, 2, 2, 3, 3, 7, 0, 0),
        "nhwc D": nh(h, p, 0, 0, p, 0, 0, 1, 1, 2, 2, 1024, 1025, 1, 0, 0),
    })
    for name, fn in (("pool u8", lib.i8ie_adaptive_avgpool2d_u8), ("pool f32", lib.i8ie_adaptive_avgpool2d_f32)):
        bad.update({
            name + " ctx": fn(None, p, p, 1, 4, 5, 5, 3, 3), name + " in": fn(h, None, p, 1, 4, 5, 5, 3, 3), name + " out": fn(h, p, None, 1, 4, 5, 5, 3, 3),
            name + " n": fn(h, p, p, 0, 4, 5, 5, 3, 3), name + " w": fn(h, p, p, 1, 4, 5, 0, 3, 3), name + " oh": fn(h, p, p, 1, 4, 5, 5, 0, 3),
            name + " ow": fn(h, p, p, 1, 4, 5, 5, 3, -1), name + " window": fn(h, p, p, 1, 1, 300, 300, 1, 1),
        })
    pn = lib.i8ie_adaptive_avgpool2d_u8_nhwc
    bad.update({
        "pool nhwc ctx": pn(None, p, 0, 0, p, 0, 0, 1, 4, 5, 5, 3, 3, 0, 0), "pool nhwc out": pn(h, p, 0, 0, None, 0, 0, 1, 4, 5, 5, 3, 3, 0, 0),
        "pool nhwc in_border": pn(h, p, -1, 0, p, 0, 0, 1, 4, 5, 5, 3, 3, 0, 0), "pool nhwc out_border": pn(h, p, 0, 0, p, -2, 0, 1, 4, 5, 5, 3, 3, 0, 0),
        "pool nhwc c": pn(h, p, 0, 0, p, 0, 0, 1, 0, 5, 5, 3, 3, 0, 0), "pool nhwc ow": pn(h, p, 0, 0, p, 0, 0, 1, 4, 5, 5, 3, 0, 0, 0),
        "pool nhwc window": pn(h, p, 0, 0, p, 0, 0, 1, 1, 300, 300, 1, 1, 0, 0),
    })
    assert {k: rc for k, rc in bad.items() if rc != -1} == {}
    assert (fake == 0).all() and all(x.value == 0 for x in v)
    # the D limit itself is accepted as far as the argument checks go: the zeroed context then has no device to offer
    assert lib.i8ie_resize_axis(2, 1024, 1, 1023, *r) == 0 and v[4].value == 2048


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_surface_exports(i8ie):
    import _CXX_i8ie as cx

    for name in ("interpolate", "adaptive_avg_pool2d"):
        assert name in i8ie.__all__ and callable(getattr(i8ie, name))
        assert not hasattr(cx, name) and hasattr(cx, "_" + name)  # private to the package: the recorded surface is unchanged
    assert len(i8ie.__all__) == len(set(i8ie.__all__)) and all(hasattr(i8ie, n) for n in i8ie.__all__)


def test_surface_argument_errors_come_before_any_device_call(i8ie):
    """(there is no GPU here: anything that reached the device would fail with another message)"""
    import _CXX_i8ie as cx

    t = i8ie.tensor(np.zeros((2, 3, 4, 5), f32))
    for bad in (lambda: i8ie.interpolate(t, size=2.0), lambda: i8ie.interpolate(t, size=(2, 2.5)), lambda: i8ie.interpolate(t, size=(2, 2, 2)),
                lambda: i8ie.interpolate(t, size="8"), lambda: i8ie.interpolate(t, size=True), lambda: i8ie.interpolate(t, size=(3, None)),
                lambda: i8ie.interpolate(t, scale_factor=(2, 0.5)), lambda: i8ie.interpolate(t, size=(8, 8), mode="bilinear", align_corners=1),
                lambda: i8ie.adaptive_avg_pool2d(t, 2.0), lambda: i8ie.adaptive_avg_pool2d(t, (1, 2, 3)), lambda: i8ie.adaptive_avg_pool2d(t, "3"),
                lambda: i8ie.adaptive_avg_pool2d(t, (True, 2))):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(TypeError, match="size"):
        i8ie.interpolate(t, scale_factor=1.5)
    for bad in (lambda: i8ie.interpolate(t), lambda: i8ie.interpolate(t, size=8, scale_factor=2),
                lambda: i8ie.interpolate(t, size=8, mode="nearest", align_corners=False), lambda: i8ie.interpolate(t, size=8, align_corners=True)):
        with pytest.raises(ValueError):
            bad()
    big = i8ie.tensor(np.zeros((1, 1, 300, 601), f32))
    for bad in (lambda: i8ie.interpolate(t, size=0), lambda: i8ie.interpolate(t, size=(3, -1), mode="bilinear"), lambda: i8ie.interpolate(t, scale_factor=0),
                lambda: i8ie.interpolate(t, size=3, mode="bicubic"), lambda: i8ie.interpolate(t.reshape(6, 20), size=3),
                lambda: i8ie.interpolate(t.reshape(2, 3, 20), scale_factor=2, mode="bilinear"),
                lambda: i8ie.interpolate(t, size=(1024, 1025), mode="bilinear"),
                lambda: i8ie.interpolate(t, size=(2049, 2050), mode="bilinear", align_corners=True),
                lambda: i8ie.adaptive_avg_pool2d(t, 0), lambda: i8ie.adaptive_avg_pool2d(t, (2, -1)), lambda: i8ie.adaptive_avg_pool2d(t.reshape(6, 20), 2),
                lambda: i8ie.adaptive_avg_pool2d(big, (1, 2)),
                lambda: cx._interpolate(t.data, 3, 3, 3), lambda: cx._interpolate(t.data, 3, 3, -1),
                lambda: cx._adaptive_avg_pool2d(t.data, 0, 3)):
        with pytest.raises(RuntimeError, match="interpolate|adaptive_avg_pool2d"):
            bad()


class _Recorder:
    """stands in for the extension inside the i8ie package: records which entry a call reached, with its arguments"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        def entry(x, *args):
            self.calls.append((name,) + args)
            return x
        return entry


def test_routing(i8ie, monkeypatch):
    """a geometry an existing op expresses goes to that op's entry, everything else to the new private ones"""
    t = i8ie.tensor(np.zeros((2, 3, 4, 6), f32))
    rec = _Recorder(i8ie._C)
    monkeypatch.setattr(i8ie, "_C", rec)
    monkeypatch.setattr(i8ie, "Tensor", lambda d: d)

    def reached(fn):
        del rec.calls[:]
        fn()
        assert len(rec.calls) == 1
        return rec.calls[0]

    assert reached(lambda: i8ie.interpolate(t, size=(8, 12))) == ("upsample", 2, 2, 0)
    assert reached(lambda: i8ie.interpolate(t, size=(4, 48), mode="bilinear")) == ("upsample", 1, 8, 1)
    assert reached(lambda: i8ie.interpolate(t, scale_factor=(3, 2), mode="bilinear", align_corners=False)) == ("upsample", 3, 2, 1)
    assert reached(lambda: i8ie.interpolate(t, scale_factor=8)) == ("upsample", 8, 8, 0)
    assert reached(lambda: i8ie.interpolate(t, scale_factor=9)) == ("_interpolate", 36, 54, 0)
    assert reached(lambda: i8ie.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)) == ("_interpolate", 8, 12, 2)
    assert reached(lambda: i8ie.interpolate(t, size=(8, 13), mode="bilinear")) == ("_interpolate", 8, 13, 1)
    assert reached(lambda: i8ie.interpolate(t, size=7)) == ("_interpolate", 7, 7, 0)
    assert reached(lambda: i8ie.interpolate(t, size=(2, 3), mode="bilinear")) == ("_interpolate", 2, 3, 1)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, 1)) == ("global_avg_pool2d",)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, (2, 3))) == ("avg_pool2d", 2, 2)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, (None, None))) == ("avg_pool2d", 1, 1)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, (2, None))) == ("_adaptive_avg_pool2d", 2, 6)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, (2, 2))) == ("_adaptive_avg_pool2d", 2, 2)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, 3)) == ("_adaptive_avg_pool2d", 3, 3)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, (1, 6))) == ("_adaptive_avg_pool2d", 1, 6)
    assert reached(lambda: i8ie.adaptive_avg_pool2d(t, 7)) == ("_adaptive_avg_pool2d", 7, 7)
