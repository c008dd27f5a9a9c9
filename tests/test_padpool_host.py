"""Pooling with padding and ceil_mode without a GPU: the numpy restatement (tests/padpool_ref.py) against torch's CPU
max_pool2d / avg_pool2d in float64 over a grid of 656 geometries, i8ie_pool_output_size against the same grid, the argument
checks (raised before any device call), the C and binding surface, and the new keywords of i8ie.max_pool2d / avg_pool2d."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi
import padpool_ref as ppr
import support
from support import i8ie  # noqa: F401

HEIGHTS, WIDTHS = (3, 4, 7, 10), (5, 8)


def _grid():
    """(k, s, p, ceil_mode, h, w): k 1..5, s 1..4, every legal p, both modes, four heights, two widths"""
    for k in range(1, 6):
        for s in range(1, 5):
            for p in range(k // 2 + 1):
                for ceil_mode in (False, True):
                    for h in HEIGHTS:
                        for w in WIDTHS:
                            if ppr.legal(h, k, s, p) and ppr.legal(w, k, s, p):
                                yield k, s, p, ceil_mode, h, w


GRID = list(_grid())
lib = support.lib_fixture(ppr)


def test_grid_has_the_dropped_window_cases():
    assert len(GRID) == 656
    # (k, s, p, in) = (2, 2, 1, 3): the plain ceil formula gives 3, the window that would start in the trailing padding is dropped
    assert ppr.out_size(3, 2, 2, 1, True) == 2 and ppr.out_size(3, 2, 2, 1, False) == 2
    dropped = [(k, s, p, size) for k, s, p, c, h, w in GRID if c for size in (h, w)
               if ((size + 2 * p - k + s - 1) // s) * s >= size + p]
    assert (2, 2, 1, 3) in dropped and len(set(dropped)) >= 10, len(set(dropped))


def test_reference_against_torch_float64():
    """max: torch's max_pool2d on the bytes as float64 (its padding is -inf, never part of a maximum).  avg: torch's
    avg_pool2d on q - zp (a padded tap is the value zero), zp added back and rounded floor(. + 0.5): ties up.  The mean
    S' / D - zp is a ratio of integers below 2^24 and D <= 25, so the float64 quotient is within 2^-44 of it and the rounding
    decides as the integers do (a non-tie is at least 1 / (2 D) from one)."""
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(7)
    for i, (k, s, p, ceil_mode, h, w) in enumerate(GRID):
        q = rng.integers(0, 256, (2, 2, h, w), dtype=np.uint8)
        q[0, 0], q[0, 1] = 0, 255
        zp = (0, 3, 128, 255)[i % 4]
        t = torch.from_numpy(q.astype(np.float64))
        want = F.max_pool2d(t, k, s, padding=p, ceil_mode=ceil_mode).numpy()
        got = ppr.max_pool2d_u8(q, k, s, p, ceil_mode)
        assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (k, s, p, ceil_mode, h, w)
        assert np.array_equal(ppr.max_pool2d_f64(q, k, s, p, ceil_mode), want)
        assert np.array_equal(ppr.max_pool2d_u8(q, k, s, p, ceil_mode, True, zp), np.maximum(got, zp))
        for include in (True, False):
            a = F.avg_pool2d(t - zp, k, s, padding=p, ceil_mode=ceil_mode, count_include_pad=include).numpy()
            want = np.floor(a + zp + 0.5)
            got = ppr.avg_pool2d_u8(q, k, s, p, ceil_mode, include, False, zp)
            assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (k, s, p, ceil_mode, include, h, w, zp)
            mean, mag, taps = ppr.avg_pool2d_f64(q.astype(np.float64) - zp, k, s, p, ceil_mode, include)
            assert np.allclose(mean, a, rtol=0, atol=1e-9) and taps.min() >= 1 and np.all(mag >= np.abs(mean) - 1e-9)
            assert ppr.divisors(h, w, k, s, p, ceil_mode, include).shape == got.shape[2:]


def test_output_size_entry_against_the_grid(lib):
    for k, s, p, ceil_mode, h, w in GRID:
        for size in (h, w):
            assert lib.i8ie_pool_output_size(size, k, s, p, 1 if ceil_mode else 0) == ppr.out_size(size, k, s, p, ceil_mode)
    assert lib.i8ie_pool_output_size(112, 3, 2, 1, 0) == 56 and lib.i8ie_pool_output_size(224, 7, 2, 3, 0) == 112
    for bad in ((0, 1, 1, 0, 0), (8, 0, 1, 0, 0), (8, 2, 0, 0, 0), (8, 2, 1, -1, 0), (8, 2, 1, 2, 0), (8, 3, 1, 2, 1), (2, 5, 1, 1, 0),
                (-4, 2, 2, 1, 1)):
        assert lib.i8ie_pool_output_size(*bad) == -1 and lib.i8ie_last_error(), bad


def test_new_symbols_are_declared_and_exported(lib):
    names = abi.declared_symbols()
    for n in ppr.SYMBOLS:
        assert n in names and hasattr(lib, n), n


def test_entry_points_check_arguments_before_any_device_call(lib):
    one = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)

    def nchw(f, tail):
        return lambda c=one, i=one, o=one, n=1, ch=4, h=8, w=8, k=3, s=2, p=1, ceil=0: f(c, i, o, n, ch, h, w, k, s, p, ceil, *tail)

    def nhwc(f, tail):
        return lambda c=one, i=one, ib=0, o=one, ob=0, n=1, ch=4, h=8, w=8, k=3, s=2, p=1, ceil=0: f(c, i, ib, 0, o, ob, 0, n, ch, h, w,
                                                                                                 k, s, p, ceil, *tail)

    calls = [nchw(lib.i8ie_maxpool2d_u8_pad, ()), nchw(lib.i8ie_maxpool2d_f32_pad, ()), nchw(lib.i8ie_avgpool2d_u8_pad, (1, 0)),
             nchw(lib.i8ie_avgpool2d_f32_pad, (1,)), nhwc(lib.i8ie_maxpool2d_u8_nhwc_pad, (0, 0)),
             nhwc(lib.i8ie_avgpool2d_u8_nhwc_pad, (1, 0, 0))]
    for call in calls:
        for bad in (dict(c=None), dict(i=None), dict(o=None)):
            assert call(**bad) == -1 and b"null" in lib.i8ie_last_error(), bad
        for bad in (dict(n=0), dict(ch=0), dict(h=-1), dict(w=0), dict(k=0), dict(k=-3), dict(s=0), dict(s=-1), dict(p=-1)):
            assert call(**bad) == -1 and b"dimension" in lib.i8ie_last_error(), bad
        for bad in (dict(p=2), dict(k=2, p=2), dict(k=1, p=1)):  # p > k / 2
            assert call(**bad) == -1 and b"padding" in lib.i8ie_last_error(), bad
        for bad in (dict(h=2, k=5, p=1), dict(w=2, k=5, p=1), dict(h=1, w=1, k=3, p=0)):  # k > in + 2 p
            assert call(**bad) == -1 and b"larger" in lib.i8ie_last_error(), bad
        assert call(h=300, w=300, k=257, p=0) == -1 and b"65536" in lib.i8ie_last_error()
    for call in calls[4:]:
        for bad in (dict(ib=-1), dict(ob=-1)):
            assert call(**bad) == -1 and b"dimension" in lib.i8ie_last_error(), bad


def test_private_binding_entries_are_the_recorded_ones():
    """tests/golden/binding_surface.json records the public names of _CXX_i8ie and stays as it is; the signatures and the
    overload order of the two private entries behind the new keywords are recorded in binding_surface_pool.json"""
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx

    want = support.golden_json("binding_surface_pool.json")
    assert sorted(want) == ["_avg_pool2d_pad", "_max_pool2d_pad"]
    assert {n: getattr(cx, n).__doc__ for n in want} == want
    assert "6TensorIaE" not in want["_max_pool2d_pad"]  # s8 tensors keep the unpadded pool only


def test_python_pools_accept_the_new_keywords(i8ie):
    """The signatures are torch's, and the keywords reach the extension: on a default-constructed tensor (no device needed)
    the unpadded floor geometry raises from the existing entry and everything else from the new one, both before any
    device call."""
    import _CXX_i8ie as cx

    mp, ap = inspect.signature(i8ie.max_pool2d).parameters, inspect.signature(i8ie.avg_pool2d).parameters
    assert list(mp) == ["x", "kernel_size", "stride", "padding", "ceil_mode"]
    assert (mp["padding"].default, mp["ceil_mode"].default) == (0, False)
    assert list(ap) == ["x", "kernel_size", "stride", "padding", "ceil_mode", "count_include_pad"]
    assert (ap["stride"].default, ap["padding"].default, ap["ceil_mode"].default, ap["count_include_pad"].default) == (None, 0, False, True)
    for word in ("padding", "ceil_mode"):
        assert word in i8ie.max_pool2d.__doc__ and word in i8ie.avg_pool2d.__doc__
    assert "count_include_pad" in i8ie.avg_pool2d.__doc__
    tried = 0
    for cls in ("6TensorIfE", "6TensorIhE"):
        e = i8ie.Tensor(getattr(cx, cls)())
        assert e.shape == ()
        for call in (lambda: i8ie.max_pool2d(e, 3, 2, padding=1), lambda: i8ie.max_pool2d(e, 3, 2, ceil_mode=True),
                     lambda: i8ie.max_pool2d(e, 3, 2, 1, True), lambda: i8ie.max_pool2d(e, 3, 2),
                     lambda: i8ie.avg_pool2d(e, 3, 1, padding=1), lambda: i8ie.avg_pool2d(e, 3, padding=1, count_include_pad=False),
                     lambda: i8ie.avg_pool2d(e, 2, ceil_mode=True), lambda: i8ie.avg_pool2d(e, 2)):
            with pytest.raises(RuntimeError, match="expects an NCHW tensor"):
                call()
            tried += 1
    assert tried == 16
