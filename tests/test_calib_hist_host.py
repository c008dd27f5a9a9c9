"""Histogram calibration on the CPU: the numpy restatement (calib_ref.py) against brute force, the host entry
i8ie_calib_hist_range against the restatement bit for bit, the argument rules of the Python surface and the recorded private
binding entries.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import calib_ref as cr
import support
from support import f32, i8ie  # noqa: F401

lib = support.lib_fixture(cr)
f64 = np.float64


def _edge_values():
    """values on and next to bin edges, at the top of the range, zeros of both signs and denormals"""
    e = -3
    w = f32(2.0 ** e)
    k = np.array([-1023, -1022, -513, -1, 0, 1, 2, 511, 1022, 1023], f32)
    on = k * w
    top = np.nextafter(f32(1024) * w, f32(0))
    return np.concatenate([on, np.nextafter(on, f32(np.inf)), np.nextafter(on, f32(-np.inf)), [top, -top],
                           [f32(0.0), f32(-0.0), f32(1e-40), f32(-1e-40), f32(2.0 ** -126), f32(-(2.0 ** -126)), f32(-(2.0 ** -100))]]).astype(f32), e


# ---- calib_ref.py against brute force -------------------------------------------------------------------------------------
def test_bins_against_brute_force():
    rng = np.random.default_rng(0)
    edge, e_edge = _edge_values()
    for x in (rng.normal(0, 3, 5000).astype(f32), rng.uniform(-1e-30, 1e-30, 300).astype(f32), edge,
              np.array([3.0e38, -1.0e38, 5.0], f32)):
        st = cr.observed(x)
        v = np.where(np.abs(x) < f32(2.0 ** -126), f32(0), x)
        absmax = float(np.abs(v).max())
        e = st["exponent"]
        assert e >= -100 and absmax < 1024 * 2.0 ** e and (e == -100 or absmax >= 1024 * 2.0 ** (e - 1))
        want = np.zeros(2048, np.uint64)
        for xv in v:   # one value at a time, python floats: floor of the exact product
            want[int(np.floor(f64(xv) * 2.0 ** -e)) + 1024] += 1
        assert np.array_equal(st["counts"], want) and st["min"] == v.min() and st["max"] == v.max()
    st = cr.observed(edge)
    assert st["exponent"] == e_edge
    # |x| < 2^-126 is +0, bin 1024; the smallest normals are not
    assert cr.observed(np.array([0.0, -0.0, 1e-40, -1e-40], f32))["counts"][1024] == 4
    tiny = cr.observed(np.array([2.0 ** -126, -(2.0 ** -126)], f32))
    assert tiny["exponent"] == -100 and tiny["counts"][1024] == 1 and tiny["counts"][1023] == 1
    zeros = cr.observed(np.zeros(7, f32))
    assert zeros["exponent"] == -100 and zeros["counts"][1024] == 7 and zeros["min"] == 0 and zeros["max"] == 0


def test_exponent_at_the_boundary():
    for e in (-100, -7, 0, 5, 118):
        at = f32(1024 * 2.0 ** e) if e < 118 else None
        below = np.finfo(f32).max if e == 118 else np.nextafter(at, f32(0))
        assert cr.exponent_for(float(below)) == e
        if at is not None:
            assert cr.exponent_for(float(at)) == e + 1
    assert cr.exponent_for(0.0) == -100 and cr.exponent_for(2.0 ** -120) == -100


def test_nonfinite_values_are_counted_and_ignored():
    x = np.array([1.0, np.nan, -2.0, np.inf, -np.inf, np.nan], f32)
    st = cr.observed(x)
    assert st["nonfinite"] == 4 and int(st["counts"].sum()) == 2 and st["min"] == -2 and st["max"] == 1
    none = cr.observed(np.array([np.nan, np.inf], f32))
    assert none["nonfinite"] == 2 and int(none["counts"].sum()) == 0 and none["exponent"] == -100 and none["min"] == np.inf


def test_fold_identity_and_chunk_order():
    rng = np.random.default_rng(1)
    a = rng.normal(0, 1, 4000).astype(f32)
    both = cr.observed(np.concatenate([a, f32(8) * a]))
    assert cr.same_state(cr.observed(a, f32(8) * a), both) and cr.same_state(cr.observed(f32(8) * a, a), both)
    assert both["exponent"] == cr.observed(a)["exponent"] + 3
    chunks = [a, f32(8) * a[:1000], f32(8192) * a[:10], np.array([np.nan], f32), np.zeros(3, f32)]
    want = cr.observed(np.concatenate(chunks))
    for order in itertools.permutations(range(len(chunks))):
        assert cr.same_state(cr.observed(*[chunks[i] for i in order]), want), order
    # a jump of more than eleven exponents puts everything in bins 1023 and 1024
    far = cr.observed(a, np.array([1e30], f32))
    assert far["counts"][1023] == (a < 0).sum() and far["counts"][1024] == (a >= 0).sum() and int(far["counts"].sum()) == a.size + 1


# ---- i8ie_calib_hist_range against the restatement ----------------------------------------------------------------------------
def _states():
    rng = np.random.default_rng(2)
    g = rng.normal(0.3, 1.7, 200000).astype(f32)
    return {
        "gaussian": cr.observed(g),
        "one_sided": cr.observed(np.maximum(g, 0)),
        "negative": cr.observed(-np.abs(g) - f32(1)),
        "single_bin": cr.observed(np.full(1000, 3.25, f32)),
        "empty": cr.observed(np.array([np.nan], f32)),
        "outlier": cr.observed(rng.normal(0, 1, 100000).astype(f32), np.array([50.0], f32)),
        "short": cr.observed(rng.normal(0, 1, 32).astype(f32)),
    }


STATES = _states()
PERCENTILES = (100.0, 99.999, 99.99, 99.9, 99.0, 90.0, 60.0, 50.001)


def _same(a, b):
    return f32(a).tobytes() == f32(b).tobytes()


@pytest.mark.parametrize("name", sorted(STATES))
def test_range_entry_matches_the_restatement(lib, name):
    st = STATES[name]
    cases = [("minmax", 99.99), ("mse", 99.99)] + [("percentile", p) for p in PERCENTILES]
    for method, p in cases:
        rc, lo, hi = cr.lib_range(lib, st, method, p)
        wlo, whi = cr.range_of(st, method, p)
        assert rc == 0 and _same(lo, wlo) and _same(hi, whi), (method, p, lo, hi, wlo, whi)
        s, z = cr.lib_qparams(lib, lo, hi)
        ws, wz = cr.qparams(wlo, whi)
        assert _same(s, ws) and z == wz, (method, p)
    # p = 100 is minmax exactly; the ranges are nested as p falls
    mm = cr.lib_range(lib, st, "minmax")
    assert cr.lib_range(lib, st, "percentile", 100.0) == mm
    prev = mm
    for p in PERCENTILES:
        cur = cr.lib_range(lib, st, "percentile", p)
        assert cur[1] >= prev[1] and cur[2] <= prev[2] and cur[1] <= cur[2], (p, cur, prev)
        prev = cur
    if name == "empty":
        assert mm == (0, f32(0), f32(0)) and cr.lib_qparams(lib, 0.0, 0.0) == (f32(1), 0)
    if name == "short":   # fewer than 1000 values: the true minimum and maximum, not a zero slot
        assert mm[1] == f32(st["min"]) and mm[2] == f32(st["max"]) and mm[1] < 0 < mm[2]


def test_qparams_tail_matches_the_restatement_and_the_reservoir(lib):
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx

    rng = np.random.default_rng(3)
    pairs = [(0.0, 0.0), (-1.0, 1.0), (0.5, 2.0), (-3.0, -1.0), (-1e-30, 1e-30), (-1e36, 1e36), (0.0, 1e-45)]   # (255 * |min| must not overflow a float: the reference leaves that undefined)
    pairs += [tuple(sorted(rng.normal(0, 10 ** rng.uniform(-3, 3), 2))) for _ in range(500)]
    for lo, hi in pairs:
        lo, hi = f32(lo), f32(hi)
        got, want = cr.lib_qparams(lib, lo, hi), cr.qparams(lo, hi)
        assert _same(got[0], want[0]) and got[1] == want[1], (lo, hi, got, want)
        # the reservoir goes through the same tail: its 1000 slots filled once, quantile 1
        fill = np.linspace(lo, hi, 1000).astype(f32)
        fill[0], fill[-1] = lo, hi
        s, z = cx.calibrator_range([fill], 1.0)
        assert _same(s, want[0]) and z == want[1], (lo, hi)


def test_mse_ties_go_to_the_larger_fraction(lib):
    """every candidate truncates the one occupied bin's centre to q = 0, so all 49 errors are equal: j = 64 must win, which is
    the minmax range (the header's maximum has no count of its own: the entry takes header and counters as given)"""
    e = -4
    st = {"exponent": e, "counts": np.zeros(2048, np.uint64), "min": 0.0, "max": float(f32(1000 * 2.0 ** e)), "nonfinite": 0}
    st["counts"][1024] = 5
    errs = {cr.mse_error(st, *cr.qparams(lo, hi)) for _, lo, hi in cr.mse_candidates(st)}
    assert len(errs) == 1 and errs.pop() > 0
    rc, lo, hi = cr.lib_range(lib, st, "mse")
    assert rc == 0 and _same(lo, 0.0) and _same(hi, st["max"])
    assert cr.mse_range(st, want_j=True)[2] == 64


def test_mse_clips_a_far_outlier(lib):
    st = STATES["outlier"]
    rc, lo, hi = cr.lib_range(lib, st, "mse")
    mlo, mhi = cr.minmax_range(st)
    e_mse, e_minmax = cr.mse_error(st, *cr.qparams(lo, hi)), cr.mse_error(st, *cr.qparams(mlo, mhi))
    assert rc == 0 and e_mse < e_minmax and hi < mhi
    assert cr.mse_range(st, want_j=True)[2] < 64


def test_range_entry_refuses_bad_arguments(lib):
    st = STATES["gaussian"]
    for p in (50.0, 49.0, 100.0001, float("nan")):
        assert cr.lib_range(lib, st, "percentile", p)[0] == -1 and b"percentile" in lib.i8ie_last_error()
    h, lo, hi = cr.header_of(st), C.c_float(), C.c_float()
    counts = np.ascontiguousarray(st["counts"])
    assert lib.i8ie_calib_hist_range(C.byref(h), counts.ctypes.data_as(C.c_void_p), 3, C.c_double(99.0), C.byref(lo), C.byref(hi)) == -1
    assert lib.i8ie_calib_hist_range(None, counts.ctypes.data_as(C.c_void_p), 0, C.c_double(99.0), C.byref(lo), C.byref(hi)) == -1
    assert lib.i8ie_calib_hist_state_bytes() == 32 + 8 * 2048 == C.sizeof(cr.Header) + 8 * cr.BINS
    # the device entries check their arguments before any device call
    assert lib.i8ie_calib_hist_reset(None, None) == -1 and lib.i8ie_calib_hist_observe_f32(None, None, 0, None) == -1
    assert lib.i8ie_calib_hist_read(None, None, None, None) == -1


def test_new_symbols_are_declared_and_exported(lib):
    names = abi.declared_symbols()
    for n in cr.SYMBOLS:
        assert n in names and hasattr(lib, n), n


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_set_calibration_round_trips_and_refuses(i8ie):
    assert "set_calibration" in i8ie.__all__ and "calibration" in i8ie.__all__
    before = i8ie.calibration()
    try:
        assert before == {"method": "reservoir", "percentile": 99.99}
        for method, p in (("minmax", 99.99), ("percentile", 99.9), ("mse", 100), ("reservoir", 75.5)):
            i8ie.set_calibration(method, p)
            assert i8ie.calibration() == {"method": method, "percentile": float(p)}
        i8ie.set_calibration("mse")
        assert i8ie.calibration() == {"method": "mse", "percentile": 99.99}
        i8ie.set_calibration()
        assert i8ie.calibration() == {"method": "reservoir", "percentile": 99.99}
        for bad in (("entropy", 99.0), ("", 99.0), (None, 99.0), ("minmax", 50), ("percentile", 100.5), ("reservoir", 0), ("mse", float("nan"))):
            with pytest.raises(ValueError):
                i8ie.set_calibration(*bad)
            assert i8ie.calibration() == {"method": "reservoir", "percentile": 99.99}
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])


def test_histogram_needs_a_preparing_layer_with_a_histogram_observer(i8ie):
    before = i8ie.calibration()
    try:
        layers = [i8ie.Linear(4, 2), i8ie.Conv2d(2, 2, 3), i8ie.Add(), i8ie.LayerNorm(4), i8ie.Attention(2)]
        for L in layers:   # not preparing
            with pytest.raises(RuntimeError):
                L.calibration_histogram()
            with pytest.raises(RuntimeError):
                L.calibration_range("minmax")
        for L in layers:   # prepared under the reservoir
            L.prepare()
            with pytest.raises(RuntimeError, match="reservoir"):
                L.calibration_histogram()
        with pytest.raises(RuntimeError):
            layers[-1].score_calibration_histogram()
        i8ie.set_calibration("minmax")
        fresh = [i8ie.Linear(4, 2), i8ie.Add(), i8ie.Attention(2)]
        for L in fresh:    # prepared under a histogram method, nothing observed yet: the reset state, no device call
            L.prepare()
            h = L.calibration_histogram()
            assert sorted(h) == ["counts", "exponent", "max", "min", "nonfinite"]
            assert h["exponent"] == -100 and h["counts"].dtype == np.uint64 and h["counts"].shape == (2048,) and not h["counts"].any()
            assert h["min"] == np.inf and h["max"] == -np.inf and h["nonfinite"] == 0
            for method in ("minmax", "percentile", "mse"):
                assert L.calibration_range(method) == (1.0, 0, 0.0, 0.0)
            for bad in (("reservoir", 99.0), ("kl", 99.0), ("percentile", 50), ("minmax", 101)):
                with pytest.raises(ValueError):
                    L.calibration_range(*bad)
        assert fresh[-1].score_calibration_histogram()["exponent"] == -100
        assert fresh[-1].score_calibration_range("mse") == (1.0, 0, 0.0, 0.0)
        # the observer was fixed at prepare(): going back to the reservoir does not take the histogram away
        i8ie.set_calibration("reservoir")
        assert fresh[0].calibration_histogram()["exponent"] == -100
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])


def test_host_range_entry_of_the_binding(i8ie):
    import _CXX_i8ie as cx

    for name in ("gaussian", "outlier", "empty", "short"):
        st = STATES[name]
        for method, p in (("minmax", 99.99), ("percentile", 99.9), ("mse", 99.99)):
            got = cx._calib_hist_range((st["exponent"], st["min"], st["max"]), st["counts"], method, p)
            assert got == cr.result_of(st, method, p), (name, method)
    with pytest.raises(ValueError):
        cx._calib_hist_range((0, 0.0, 1.0), np.zeros(2048, np.uint64), "reservoir", 99.0)
    with pytest.raises(ValueError):
        cx._calib_hist_range((0, 0.0, 1.0), np.zeros(7, np.uint64), "minmax", 99.0)


def test_calibrated_takes_a_calibration_keyword():
    import inspect

    from int8inferenceengine_amd import workloads as wl

    p = inspect.signature(wl.calibrated).parameters
    assert list(p)[-1] == "calibration" and p["calibration"].default is None


def test_private_binding_entries_are_the_recorded_ones():
    """tests/golden/binding_surface.json records the public names of _CXX_i8ie and stays as it is (test_binding_surface.py);
    the private entries of histogram calibration are recorded in binding_surface_calibration.json"""
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx

    want = support.golden_json("binding_surface_calibration.json")
    assert sorted(want) == ["classes", "functions"]
    assert sorted(want["functions"]) == ["_calib_hist_range", "_calibration", "_set_calibration"]
    assert {n: getattr(cx, n).__doc__ for n in want["functions"]} == want["functions"]
    per_class = ["_calib_histogram", "_calib_range"]
    classes = sorted(n for n in dir(cx) if isinstance(getattr(cx, n), type) and hasattr(getattr(cx, n), "set_output_qparams"))
    assert sorted(want["classes"]) == classes and len(classes) >= 12
    for cn, members in want["classes"].items():
        extra = ["_score_calib_histogram", "_score_calib_range"] if cn == "Attention" else []
        assert sorted(members) == sorted(per_class + extra), cn
        assert {n: getattr(getattr(cx, cn), n).__doc__ for n in members} == members, cn
