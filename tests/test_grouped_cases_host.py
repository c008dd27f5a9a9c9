"""tests/grouped_cases.py without a GPU: the edge list and the default fuzz list reach every kernel instance, tail and
border class they exist for (so a class cannot be dropped from them unnoticed), the per-group reference equals the
dense oracle on block-diagonal weights for every edge case, and the expected bytes are not parked on a clamp."""
import time

import numpy as np
import pytest

import grouped_cases as gc
import grouped_ref as gr

EDGE = gc.EDGE_CASES
FUZZ = gc.fuzz_cases()
WRAP = [c for c in EDGE if gc.dispatch(c).kernel == "gconv_direct" and gc.direct_items(c) > gc.MAX_DIRECT_THREADS]


PRIME_M = {"g1_cg3_k5_ng20_m17", "g4_cg8_kg32_ng1_m31", "g16_cg16_kg64_ng65_m127", "g4_cg8_kg128_ng63_m129"}


def _mfma(cases):
    return [c for c in cases if gc.dispatch(c).kernel == "gconv_mfma"]


def _direct(cases):
    return [c for c in cases if gc.dispatch(c).kernel == "gconv_direct"]


def test_names_are_unique_and_cases_are_small():
    names = [c.name for c in EDGE]
    assert len(set(names)) == len(names)
    for c in EDGE:
        assert gc.header_rejects(c) is None and gc.geom(c)[5] > 0, c.name
        if c in WRAP:
            continue
        assert c.h <= 15 and c.w <= 15 and c.groups <= 4, c.name
        # the batch stays at 1 to 3 except where the pixel count M is prime, or 3 * 43, and is reached with the batch
        assert c.m <= 3 or (gc.geom(c)[5] in (17, 31, 127, 129) and c.name.split("-")[0] in PRIME_M), c.name


def test_dispatch_rule():
    mk = gc._mk
    assert gc.dispatch(mk("a", 1, 32, 8, 2, 3, 1, 1, 5, 5)) == ("gconv_mfma", 16, None, False, 1)
    assert gc.dispatch(mk("b", 1, 8, 6, 2, 3, 1, 1, 5, 5, pc=True)) == ("gconv_mfma", 4, None, True, 0)
    assert gc.dispatch(mk("c", 1, 12, 12, 2, 3, 1, 1, 5, 5)) == ("gconv_mfma", 1, None, False, 0)   # Ng = 6
    assert gc.dispatch(mk("d", 1, 62, 8, 2, 1, 1, 0, 5, 5)) == ("gconv_direct", None, False, False, 1)  # Kg = 31
    assert gc.dispatch(mk("e", 1, 64, 8, 2, 1, 1, 0, 5, 5)).kernel == "gconv_mfma"                      # Kg = 32
    assert gc.dispatch(mk("f", 1, 64, 8, 2, 1, 1, 0, 5, 5, force=True)) == ("gconv_direct", None, True, False, 1)
    assert gc.dispatch(mk("g", 1, 8, 10, 2, 1, 1, 0, 5, 5)) == ("gconv_direct", None, True, False, 0)   # kc % 4 != 0


def test_edge_cases_cover_every_instance():
    seen = {gc.dispatch(c) for c in EDGE}
    for pc in (False, True):
        for vec in (0, 1):
            for G in (16, 4, 1):
                assert ("gconv_mfma", G, None, pc, vec) in seen, (G, pc, vec)
            for dot4 in (False, True):
                assert ("gconv_direct", None, dot4, pc, vec) in seen, (dot4, pc, vec)
    g1 = {(gc.geom(c)[0], c.kh, c.kw) for c in _mfma(EDGE) if gc.dispatch(c).G == 1}
    assert {(6, 3, 3), (7, 3, 3), (65, 1, 1), (3, 5, 5)} <= g1


def test_edge_cases_cover_the_tails():
    ng_mfma = {gc.geom(c)[1] for c in _mfma(EDGE)}
    assert {1, 3, 6, 17, 20, 63, 64, 65, 72} <= ng_mfma
    assert {1, 2, 3, 5, 8} <= {gc.geom(c)[1] for c in _direct(EDGE)}
    assert any(gc.geom(c)[2] == 31 and not gc.dispatch(c).dot4 for c in _direct(EDGE))
    kg = {(gc.geom(c)[2], gc.dispatch(c).G) for c in _mfma(EDGE)}
    assert (32, 4) in kg and (32, 16) in kg
    assert {63, 64, 65, 128} <= {k for k, _ in kg}
    assert any((gc.geom(c)[0], c.kh, c.kw) == (8, 2, 2) for c in _mfma(EDGE))
    assert any((gc.geom(c)[0], c.kh, c.kw) == (32, 1, 1) for c in _mfma(EDGE))
    assert {1, 15, 16, 17, 31, 32, 33, 127, 128, 129} <= {gc.geom(c)[5] for c in _mfma(EDGE)}
    assert len(WRAP) >= 1


def test_edge_cases_cover_the_geometry():
    for sel, what in ((_mfma, "gconv_mfma"), (_direct, "gconv_direct")):
        nhwc_in = [c for c in sel(EDGE) if c.in_nhwc and c.pad > 0]
        rel = {c.ib - c.pad for c in nhwc_in} | {"none" for c in nhwc_in if c.ib == 0}
        assert {"none", -1, 0, 1} <= rel, (what, rel)
        assert any(c.pad >= max(c.kh, c.kw) for c in sel(EDGE)), what
        assert any(c.stride > max(c.kh, c.kw) for c in sel(EDGE)), what
        assert any(c.kh != c.kw for c in sel(EDGE)), what
        assert any(gc.geom(c)[3] == 1 for c in sel(EDGE)) and any(gc.geom(c)[4] == 1 for c in sel(EDGE)), what
    assert any(c.pad > 1 and c.ib == c.pad - 1 for c in EDGE if c.in_nhwc)  # (pad - 1 that is not 0)
    assert any(c.kh < c.kw for c in EDGE) and any(c.kh > c.kw for c in EDGE)
    assert any((c.kh, c.kw) == (c.h, c.w) and c.pad == 0 for c in EDGE)
    assert any(c.h != c.w for c in EDGE)


def test_edge_cases_cover_the_layouts():
    for sel in (_mfma, _direct):
        assert {(a, b) for a in (False, True) for b in (False, True)} <= {(c.in_nhwc, c.out_nhwc) for c in sel(EDGE)}
        assert {0, 1, 2} <= {c.ob for c in sel(EDGE) if c.out_nhwc and c.kc % 16 == 0}
        assert any(c.out_nhwc and c.kc % 16 != 0 and c.ob == 0 for c in sel(EDGE))
    assert any(c.in_nhwc and c.c % 16 != 0 and c.c % 4 == 0 for c in _mfma(EDGE))
    assert any(c.in_nhwc and c.c % 4 != 0 for c in _mfma(EDGE))
    assert any(c.in_nhwc and c.c % 4 != 0 for c in _direct(EDGE))


def test_edge_cases_cover_the_arithmetic():
    for sel in (_mfma, _direct):
        for zp in (0, 255):
            assert any(c.zp_in == zp and c.pad > 0 and not c.extreme for c in sel(EDGE)), zp
    assert any(c.extreme and gc.dispatch(c).G == 1 for c in EDGE)
    assert any(c.extreme and gc.dispatch(c).dot4 is False for c in EDGE)
    for c in EDGE:
        if c.extreme:  # exact by construction: the largest accumulator is far inside INT32
            assert gc.geom(c)[2] * 255 * 128 + 127 * 256 * 256 < 2 ** 31
    zc = [c for c in EDGE if c.zero_col]
    assert any(gc.dispatch(c).kernel == "gconv_mfma" for c in zc)
    for c in zc:
        Ng = gc.geom(c)[1]
        assert c.pc and Ng % 4 != 0 and gc.reference(c)["s_wv"][Ng - 1] == 0.0


def test_fuzz_list_reaches_every_instance():
    assert len(FUZZ) == 48 or "I8IE_GCONV_FUZZ_CASES" in __import__("os").environ
    d = [gc.dispatch(c) for c in FUZZ]
    for pc in (False, True):
        for G in (16, 4, 1):
            assert sum(1 for x in d if x.kernel == "gconv_mfma" and x.G == G and x.pc == pc) >= 3, (G, pc)
        for dot4 in (False, True):
            assert sum(1 for x in d if x.kernel == "gconv_direct" and x.dot4 == dot4 and x.pc == pc) >= 3, (dot4, pc)
    for lay in ((False, False), (False, True), (True, False), (True, True)):
        assert sum(1 for c in FUZZ if (c.in_nhwc, c.out_nhwc) == lay) >= 4, lay
    assert sum(1 for c in FUZZ if c.in_nhwc and c.pad > 0 and c.ib != c.pad) >= 6
    assert gc.fuzz_cases.rejected < len(FUZZ)  # fewer than half of all draws were thrown away
    assert gc.fuzz_cases(8, 5) == gc.fuzz_cases(8, 5) and gc.fuzz_cases(8, 5) != gc.fuzz_cases(8, 6)
    for c in FUZZ:
        assert gc.header_rejects(c) is None and gc.geom(c)[5] > 0


@pytest.mark.parametrize("case", EDGE, ids=[c.name for c in EDGE])
def test_reference_equals_block_diagonal_dense_oracle(orc, case):
    """the per-group composition against one dense oracle convolution; the offsets are compared as
    test_grouped_host.py does (the dense sum walks the zero blocks too).  The grid-stride case is left out: its dense
    weight is 1024 x 1024 and the dense contraction 4.4 GMAC; its kernel is 1 x 1 so that the 1024 per-group oracle calls
    stay short (the time is printed, not asserted)."""
    t0 = time.perf_counter()
    d = gc.reference(case)
    took = time.perf_counter() - t0
    if case in WRAP:
        print("%s: oracle %.2f s" % (case.name, took))
        return
    dense = gr.block_diagonal(d["qw"], case.groups)
    if case.pc:
        import pc_pipeline as pcp

        want, want_acc = pcp.conv2d_pc(d["q"], dense, d["qb"], case.stride, case.pad, gc.S_IN, case.zp_in, d["s_wv"], d["s_out"],
                                       gc.ZP_OUT)
    else:
        want, want_acc = orc.conv2d(d["q"], dense, d["qb"], case.stride, case.pad, gc.S_IN, case.zp_in, d["s_w"], d["s_out"],
                                    gc.ZP_OUT, want_acc=True)
    assert np.array_equal(d["acc"], want_acc)
    assert np.array_equal(d["want"], want)
    assert np.array_equal(orc.conv_offsets(d["qw"].reshape(case.kc, -1), d["qb"], gc.S_IN, case.zp_in),
                          orc.conv_offsets(dense.reshape(case.kc, -1), d["qb"], gc.S_IN, case.zp_in))


@pytest.mark.parametrize("case", EDGE + FUZZ, ids=[c.name for c in EDGE + FUZZ])
def test_expected_bytes_are_not_saturated(orc, case):
    """from the oracle alone: at most a quarter of the expected bytes sit on 0 or 255 (the deliberate extremes aside)"""
    if case.extreme:
        return
    want = gc.reference(case)["want"]
    frac = float(np.mean((want == 0) | (want == 255)))
    assert frac <= 0.25, (case.name, frac)
