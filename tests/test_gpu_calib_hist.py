"""Histogram calibration on the device: i8ie_calib_hist_observe_f32 through the C-ABI and the observers of the Python surface,
against the numpy restatement (calib_ref.py).  Everything is exact: counts, exponent, minimum, maximum, the non-finite count,
the ranges and the (scale, zero_point) they give."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import calib_ref as cr
import mha_ref as mr
import support
from support import f32, i8ie  # noqa: F401

pytestmark = pytest.mark.gpu

ctx = support.ctx_fixture(cr, mr)
LAUNCHES_PER_OBSERVE = 2   # calib_hist_stats, calib_hist_count (include/i8ie_hip.h, i8ie_calib_hist_observe_f32)


class Hist:
    """one observer state on the device"""

    def __init__(self, ctx, raw=None):
        self.ctx, self.lib = ctx, abi.lib()
        nbytes = self.lib.i8ie_calib_hist_state_bytes()
        if raw is None:
            self.buf = ctx.empty((nbytes,), np.uint8)
            self.reset()
        else:
            assert raw.nbytes == nbytes
            self.buf = ctx.put(raw)

    def reset(self):
        abi.ck(self.lib.i8ie_calib_hist_reset(self.ctx.h, self.buf.ptr))

    def observe(self, x, offset=0):
        """x as n floats that start `offset` floats behind a 16-byte boundary"""
        x = np.ascontiguousarray(x, f32).reshape(-1)
        host = np.full(x.size + 4, np.nan, f32)   # (a read outside [offset, offset + n) would count a non-finite value)
        host[offset:offset + x.size] = x
        d = self.ctx.put(host)
        assert d.ptr.value % 16 == 0
        abi.ck(self.lib.i8ie_calib_hist_observe_f32(self.ctx.h, C.c_void_p(d.ptr.value + 4 * offset), C.c_int64(x.size), self.buf.ptr))
        self.ctx.sync()
        d.free()
        return self

    def read(self):
        h, counts = cr.Header(), np.zeros(cr.BINS, np.uint64)
        abi.ck(self.lib.i8ie_calib_hist_read(self.ctx.h, self.buf.ptr, C.byref(h), counts.ctypes.data_as(C.c_void_p)))
        assert tuple(h.scratch) == (0, 0, 0)   # at rest
        return {"exponent": h.exponent, "counts": counts, "min": h.min, "max": h.max, "nonfinite": h.nonfinite}

    def free(self):
        self.buf.free()


def _check(ctx, chunks, offsets=None):
    hist = Hist(ctx)
    try:
        for i, c in enumerate(chunks):
            hist.observe(c, 0 if offsets is None else offsets[i])
        got, want = hist.read(), cr.observed(*chunks)
        assert cr.same_state(got, want), (got["exponent"], want["exponent"], got["min"], want["min"], got["max"], want["max"],
                                          got["nonfinite"], want["nonfinite"], np.flatnonzero(got["counts"] != want["counts"])[:8])
        return got
    finally:
        hist.free()


# ---- through the C-ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1025, 65543])
def test_sizes_and_pointer_offsets(ctx, n):
    x = np.random.default_rng(n).normal(0.2, 1.5, n).astype(f32)
    for offset in (0, 1, 2, 3):   # 0, 4, 8 and 12 bytes behind a 16-byte boundary
        got = _check(ctx, [x], [offset])
        assert int(got["counts"].sum()) == n and got["nonfinite"] == 0


def test_bin_edges_zeros_and_denormals(ctx):
    e = -3
    w = f32(2.0 ** e)
    k = np.arange(-1023, 1024).astype(f32)
    on = k * w
    x = np.concatenate([on, np.nextafter(on, f32(np.inf)), np.nextafter(on, f32(-np.inf))]).astype(f32)
    got = _check(ctx, [x])
    assert got["exponent"] == e and got["counts"][1024 + 5] == 3 and got["counts"][1024 - 5] == 3   # k w, the float above it, the float below (k + 1) w
    got = _check(ctx, [np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45], f32)])
    assert got["exponent"] == -100 and got["counts"][1024] == 6 and got["min"] == 0 and got["max"] == 0
    assert not np.signbit(f32(got["min"])) and not np.signbit(f32(got["max"]))   # (-0 counts as +0)
    # negative values far below one bin width fall in bin 1023, not 1024, whatever the flush mode: the product underflows
    got = _check(ctx, [np.array([1e30, -(2.0 ** -126), -1e-30, 2.0 ** -126, -1e-40], f32)])
    assert got["counts"][1023] == 2 and got["counts"][1024] == 2


def test_absmax_at_the_exponent_boundary(ctx):
    for e in (-100, -9, 0, 7, 117):
        at = f32(1024 * 2.0 ** e)
        assert _check(ctx, [np.array([1.0 * 2.0 ** (e - 3), -at], f32)])["exponent"] == e + 1
        below = _check(ctx, [np.array([np.nextafter(at, f32(0)), -(2.0 ** e)], f32)])
        assert below["exponent"] == e and below["counts"][2047] == 1
    assert _check(ctx, [np.array([np.finfo(f32).max, np.finfo(f32).min], f32)])["exponent"] == 118


def test_nonfinite_zeros_and_one_bin(ctx):
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, 5000).astype(f32)
    x[rng.integers(0, x.size, 40)] = np.nan
    x[rng.integers(0, x.size, 20)] = np.inf
    x[rng.integers(0, x.size, 20)] = -np.inf
    x[-1], x[0] = np.nan, np.inf   # the scalar tail and the first vector
    got = _check(ctx, [x])
    assert got["nonfinite"] == (~np.isfinite(x)).sum() > 0
    none = _check(ctx, [np.array([np.nan, np.inf, -np.inf], f32)])
    assert none["exponent"] == -100 and none["min"] == np.inf and none["max"] == -np.inf and not none["counts"].any()
    zeros = _check(ctx, [np.zeros(3001, f32)])
    assert zeros["exponent"] == -100 and zeros["counts"][1024] == 3001
    same = _check(ctx, [np.full(1 << 20, 3.7, f32)])
    assert np.count_nonzero(same["counts"]) == 1 and int(same["counts"].max()) == 1 << 20


def test_grid_stride_loop_wraps_the_capped_grid(ctx):
    """the count pass runs at most 512 blocks of 512 lanes with four 16-byte loads each: 4 Mi values per sweep"""
    n = 4 * 512 * 512 * 4 + 4 * 512 * 700 + 3
    x = np.random.default_rng(6).normal(0, 1, n).astype(f32)
    x[x < 0] = 0   # half of the values in one bin
    got = _check(ctx, [x], [1])
    assert int(got["counts"].sum()) == n


def test_chunk_order_does_not_matter(ctx):
    rng = np.random.default_rng(7)
    a = rng.normal(0, 1, 3000).astype(f32)
    chunks = [a, f32(8) * a[:1500] + f32(0.1), f32(8192) * a[:700]]
    want = cr.observed(np.concatenate(chunks))
    exps = [cr.observed(*chunks[:i + 1])["exponent"] for i in range(3)]
    assert exps[1] == exps[0] + 3 and exps[2] == exps[1] + 10
    for order in itertools.permutations(range(3)):
        got = _check(ctx, [chunks[i] for i in order], [order[0], 0, 3])
        assert cr.same_state(got, want), order


def test_sixty_four_bit_carry_and_reset(ctx):
    """a state uploaded with one counter at 2^32 - 1: the next adds carry into the upper word"""
    o = cr.Observer()
    o.min, o.max, o.exponent = f32(-5), f32(1000), 0
    o.counts[1024 + 3] = 2 ** 32 - 1
    o.counts[1024 - 5], o.counts[1024 + 1000] = 1, 1
    raw = np.concatenate([np.frombuffer(bytes(cr.header_of(o.state())), np.uint8), o.counts.view(np.uint8)])
    hist = Hist(ctx, raw)
    try:
        assert cr.same_state(hist.read(), o.state())
        x = np.concatenate([np.full(10, 3.5, f32), np.array([np.nan, -7.25], f32)])
        hist.observe(x)
        want = o.observe(x).state()
        got = hist.read()
        assert cr.same_state(got, want) and int(got["counts"][1027]) == 2 ** 32 + 9 and got["min"] == -7.25
        # a growing exponent folds the large counter too
        big = np.array([5000.0], f32)
        hist.observe(big)
        want = o.observe(big).state()
        got = hist.read()
        assert cr.same_state(got, want) and got["exponent"] == 3 and int(got["counts"].sum()) == 2 ** 32 + 13
        hist.reset()
        assert cr.same_state(hist.read(), cr.Observer().state())
        assert cr.same_state(hist.observe(x).read(), cr.observed(x))
    finally:
        hist.free()


# ---- through Python -----------------------------------------------------------------------------------------------------------
CALIBRATIONS = ("minmax", ("percentile", 99.9), "mse")


def _two_layer(i8ie, seed=3):
    rng = np.random.default_rng(seed)

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = i8ie.Conv2d(3, 8, 3, padding=1)
            self.fc = i8ie.Linear(8 * 6 * 6, 16)

        def forward(self, x):
            return self.fc(i8ie.relu(self.conv1(x)).reshape(x.shape[0], -1))

    net = Net()
    net.load({"conv1.weight": rng.normal(0, 0.3, (8, 3, 3, 3)).astype(f32), "conv1.bias": rng.normal(0, 0.1, 8).astype(f32),
              "fc.weight": rng.normal(0, 0.08, (16, 288)).astype(f32), "fc.bias": rng.normal(0, 0.1, 16).astype(f32)})
    return net


def _args(calibration):
    return calibration if isinstance(calibration, tuple) else (calibration, 99.99)


@pytest.mark.parametrize("calibration", CALIBRATIONS, ids=lambda c: _args(c)[0])
def test_two_layer_module_over_two_batches(i8ie, calibration):
    method, p = _args(calibration)
    before = i8ie.calibration()
    try:
        i8ie.set_calibration(method, p)
        net = _two_layer(i8ie)
        net.prepare()
        rng = np.random.default_rng(11)
        seen = {"conv1": [], "fc": []}
        for scale in (1.0, 9.0):   # (the second batch raises the exponent of both layers)
            x = i8ie.tensor((scale * rng.normal(0, 1, (2, 3, 6, 6))).astype(f32))
            y1 = net.conv1(x)
            y2 = net.fc(i8ie.relu(y1).reshape(2, -1))
            seen["conv1"].append(y1.numpy())
            seen["fc"].append(y2.numpy())
            assert y2.shape == (2, 16)
        want_qp = {}
        for a, ys in seen.items():
            L = getattr(net, a)
            st = cr.observed(*ys)
            assert cr.same_state(L.calibration_histogram(), st), a
            assert int(st["counts"].sum()) == sum(y.size for y in ys)
            for m2, p2 in (_args(c) for c in CALIBRATIONS):   # every method from the one pass
                assert L.calibration_range(m2, p2) == cr.result_of(st, m2, p2), (a, m2)
            want_qp[a] = cr.result_of(st, method, p)[:2]
        # fewer than 1000 values: the Linear's 64 outputs give their true minimum and maximum
        fc = np.concatenate([y.ravel() for y in seen["fc"]])
        assert fc.size < 1000 and net.fc.calibration_range("minmax")[2:] == (float(fc.min()), float(fc.max()))
        net.convert()
        for a, qp in want_qp.items():
            assert getattr(net, a).output_qparams() == qp and qp[0] != 1.0, a
        with pytest.raises(RuntimeError):
            net.fc.calibration_histogram()   # converted: no observer any more
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])


def test_method_is_the_one_in_force_at_convert_and_qparams_override(i8ie):
    before = i8ie.calibration()
    try:
        i8ie.set_calibration("minmax")
        net = _two_layer(i8ie)
        net.prepare()
        rng = np.random.default_rng(12)
        x = rng.normal(0, 1, (4, 3, 6, 6)).astype(f32)
        x[0, 0, 0, 0] = 60.0   # one far outlier
        y1 = net.conv1(i8ie.tensor(x))
        net.fc(i8ie.relu(y1).reshape(4, -1))
        st = cr.observed(y1.numpy())
        net.fc.set_output_qparams(0.125, 31)
        i8ie.set_calibration("percentile", 95.0)
        net.convert()
        assert net.conv1.output_qparams() == cr.result_of(st, "percentile", 95.0)[:2] != cr.result_of(st, "minmax")[:2]
        assert net.fc.output_qparams() == (0.125, 31)
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])


def test_attention_scores_have_an_observer_of_their_own(i8ie, ctx):
    before = i8ie.calibration()
    rng = np.random.default_rng(13)
    b, heads, d, t = 3, 2, 8, 9
    c = 3 * heads * d
    x = rng.normal(0, 1.0, (b, t, c)).astype(f32)
    try:
        i8ie.set_calibration("mse")
        at = i8ie.Attention(heads)
        at.prepare()
        got = at(i8ie.tensor(x)).numpy()
        # the scores the observer saw: the FP32 entry's scores_out_dev on the same input
        dx, dsc, dout = ctx.put(x), ctx.empty((b, heads, t, t), f32), ctx.empty((b, t, heads * d), f32)
        g = mr.AttnArgs(b=b, heads=heads, d=d, tq=t, tk=t, q=mr.AttnMat(dx.ptr.value, t * c, c, 0), k=mr.AttnMat(dx.ptr.value + 4 * heads * d, t * c, c, 0),
                        v=mr.AttnMat(dx.ptr.value + 8 * heads * d, t * c, c, 0), out=mr.mat(dout.ptr.value, t, heads * d), scores_out_dev=dsc.ptr.value)
        abi.ck(abi.lib().i8ie_attention_f32(ctx.h, C.byref(g)))
        scores = dsc.get()
        assert support.same_bits(dout.get(), got)
        for dv in (dx, dsc, dout):
            dv.free()
        st_s, st_o = cr.observed(scores), cr.observed(got)
        assert cr.same_state(at.score_calibration_histogram(), st_s) and cr.same_state(at.calibration_histogram(), st_o)
        for m2, p2 in (_args(cal) for cal in CALIBRATIONS):
            assert at.score_calibration_range(m2, p2) == cr.result_of(st_s, m2, p2), m2
        at.convert()
        assert at.score_qparams() == cr.result_of(st_s, "mse")[:2] and at.output_qparams() == cr.result_of(st_o, "mse")[:2]
        assert at.score_qparams()[0] != 1.0
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])


def _profiled_forward(net, x):
    import _CXX_i8ie as cx

    net(x).numpy()   # the first forward allocates and resets the observers
    cx.synchronize()
    cx.profile_start()
    try:
        net(x).numpy()
    finally:
        prof = cx.profile_stop()
    return support.launch_counts(prof)


def test_launches_per_observe(i8ie):
    import _CXX_i8ie as cx

    before = i8ie.calibration()
    x = i8ie.tensor(np.random.default_rng(14).normal(0, 1, (2, 3, 6, 6)).astype(f32))
    try:
        i8ie.set_calibration("reservoir")
        net = _two_layer(i8ie)
        net.prepare()
        launches = _profiled_forward(net, x)
        assert not [k for k in launches if k.startswith("calib_hist")], launches
        i8ie.set_calibration("minmax")
        cx.set_calibration_mode("host")   # belongs to the reservoir: a histogram observer stays on the device
        net = _two_layer(i8ie)
        net.prepare()
        launches = _profiled_forward(net, x)
        own = {k: v for k, v in launches.items() if k.startswith("calib_hist")}
        assert own == {"calib_hist_stats": 2, "calib_hist_count": 2} and sum(own.values()) == 2 * LAUNCHES_PER_OBSERVE, launches
        assert "calib_sample" not in launches
        assert int(net.conv1.calibration_histogram()["counts"].sum()) == 2 * 2 * 8 * 6 * 6
    finally:
        cx.set_calibration_mode("auto")
        i8ie.set_calibration(before["method"], before["percentile"])


def test_registry_network_under_a_calibration_keyword(i8ie):
    from int8inferenceengine_amd import workloads as wl

    before = i8ie.calibration()
    try:
        i8ie.set_calibration("percentile", 99.5)
        net = wl.calibrated("two_conv", calibration="mse")
        assert i8ie.calibration() == {"method": "percentile", "percentile": 99.5}
        for a in wl.layer_names("two_conv"):
            L = getattr(net, a)
            assert L.layer.is_quantized() and L.output_qparams()[0] != 1.0, a
        y = net(i8ie.tensor(wl.synthetic_input("two_conv", 4, seed=1))).numpy()
        assert np.isfinite(y).all()
        with pytest.raises(ValueError):
            wl.calibrated("two_conv", calibration="entropy")
        assert i8ie.calibration() == {"method": "percentile", "percentile": 99.5}
    finally:
        i8ie.set_calibration(before["method"], before["percentile"])
