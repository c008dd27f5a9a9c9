"""Rectangular Conv2d without a GPU: the restatement of tests/rectconv_ref.py against torch's CPU conv2d
with tuple arguments, exact in float64; the argument rules of the new C entries through a NULL ctx; the Python argument rules,
geometry() and dilation(); and the case lists of the GPU tests."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import rectconv_ref as rr
import support
from support import i8ie  # noqa: F401

lib = support.lib_fixture(rr)


def _torch_acc(q, qw, groups, g, zp_in):
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(q.astype(np.float64) - zp_in)  # (torch pads with 0: shift so that the padding value is zp_in)
    y = F.conv2d(x, torch.from_numpy(qw.astype(np.float64)), None, (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw), groups)
    wsum = qw.astype(np.int64).reshape(qw.shape[0], -1).sum(1)
    return y.numpy().transpose(0, 2, 3, 1) + zp_in * wsum


KS, STRIDES, PADS, DILS, GROUPS = (1, 2, 3, 5, 7), (1, 2), (0, 1, 2, 3), (1, 2), (1, 2, "dw")


def _grid():
    """a sample of the grid for the oracle's embedding route: every (kh, kw) with each group mode, the other numbers drawn"""
    out = []
    rng = np.random.default_rng(7)
    for kh, kw in itertools.product(KS, KS):
        for groups in GROUPS:
            s, p, d = (tuple(int(rng.choice(v)) for _ in range(2)) for v in (STRIDES, PADS, DILS))
            out.append((rr.G(kh, kw, s, p, d), groups))
    return out


def _operands(g, groups, rng):
    c = 4
    grp = c if groups == "dw" else groups
    kc = 4
    eh, ew = rr.extent(g)
    h, w = max(eh - 2 * g.ph, 1) + 2, max(ew - 2 * g.pw, 1) + 3  # non-square maps that hold the kernel
    q = rng.integers(0, 256, (1, c, h, w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (kc, c // grp, g.kh, g.kw), dtype=np.int8)
    return q, qw, grp


@pytest.mark.parametrize("kh", KS)
def test_tap_formula_is_torchs_conv2d_on_the_whole_grid(kh):
    """every point of the grid (5 x 5 kernels, 4 stride pairs, 16 pad pairs, 4 dilation pairs, 3 group modes: 19 200 in all):
    the INT32 sums of the definition against torch's conv2d with tuple arguments, in float64 and exact"""
    rng = np.random.default_rng(kh)
    n = 0
    for kw, sh, sw, ph, pw, dh, dw, groups in itertools.product(KS, STRIDES, STRIDES, PADS, PADS, DILS, DILS, GROUPS):
        g = rr.G(kh, kw, (sh, sw), (ph, pw), (dh, dw))
        q, qw, grp = _operands(g, groups, rng)
        want = _torch_acc(q, qw, grp, g, 121)
        got = rr.conv_acc(q, qw, grp, g, 121)
        assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (g, groups)
        n += 1
    assert n == 19200 // len(KS)


@pytest.mark.parametrize("g,groups", _grid(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_restatement_is_torchs_conv2d(g, groups):
    rng = np.random.default_rng(g.kh * 100 + g.kw)
    c = 4
    grp = c if groups == "dw" else groups
    kc = 8 if groups != "dw" else 4
    eh, ew = rr.extent(g)
    h, w = max(eh - 2 * g.ph, 1) + 5, max(ew - 2 * g.pw, 1) + 8  # non-square maps that hold the kernel
    q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
    qw = rng.integers(-127, 128, (kc, c // grp, g.kh, g.kw), dtype=np.int8)
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    zp = 121
    want = _torch_acc(q, qw, grp, g, zp)
    direct = rr.conv_acc(q, qw, grp, g, zp)
    assert direct.shape == want.shape and np.array_equal(direct.astype(np.float64), want)
    # ... and the embedding route of reference(): pad explicitly, embed, stride 1, subsample
    _, facc = rr.gr.conv2d_grouped(rr.pad_input(q, g, zp), rr.embed(qw, g), qb, grp, 1, 0, rr.S_IN, zp, np.float32(0.002), np.float32(1.0), 37)
    H1, W1 = h + 2 * g.ph - eh + 1, w + 2 * g.pw - ew + 1
    acc = facc.reshape(2, H1, W1, kc)[:, ::g.sh, ::g.sw]
    # (the oracle's accumulators carry the offset vector of src/conv2d.cc:117-124; here zp * wsum < 2^24 is exact in fp32)
    wsum = qw.astype(np.int64).reshape(kc, -1).sum(1)
    oc = (qb.astype(np.float32) / rr.S_IN - (zp * wsum).astype(np.float32)).astype(np.int32)
    assert np.array_equal(acc.astype(np.float64), want + oc)


# ---- argument rules of the C entries: answered before any device call (NULL ctx) ------------------------------------------
BAD = [
    (dict(stride_h=0), b"stride"), (dict(stride_w=0), b"stride"), (dict(stride_w=-1), b"stride"),
    (dict(pad_h=-1), b"padding"), (dict(pad_w=-1), b"padding"),
    (dict(dilation_h=0), b"dilation"), (dict(dilation_w=0), b"dilation"),
    (dict(kh=0), b"dimension"), (dict(kw=0), b"dimension"),
    (dict(groups=0), b"groups"), (dict(groups=3), b"groups"),
]


def _geom(**kw):
    base = dict(kh=1, kw=3, stride_h=1, stride_w=1, pad_h=0, pad_w=1, dilation_h=1, dilation_w=1)
    base.update({k: v for k, v in kw.items() if k != "groups"})
    return rr.CGeom(**base)


@pytest.mark.parametrize("bad,text", BAD, ids=[str(b[0]) for b in BAD])
def test_argument_rules(lib, bad, text):
    g, groups = _geom(**bad), bad.get("groups", 1)
    buf = np.zeros(4096, np.int8)
    p = buf.ctypes.data_as(C.c_void_p)
    L = C.c_void_p()
    sw = np.ones(16, np.float32)
    calls = [
        lambda: lib.i8ie_conv2d_create_rect(None, p, p, 16, 16, groups, C.byref(g), C.c_float(0.01), C.byref(L)),
        lambda: lib.i8ie_conv2d_create_rect_per_channel(None, p, p, 16, 16, groups, C.byref(g), sw.ctypes.data_as(C.c_void_p), C.byref(L)),
        lambda: lib.i8ie_conv2d_u8s8_rect(None, p, 1, 16, 8, 8, p, 16, groups, C.byref(g), 0, p, 0.03, 0.01, 0.05, 0, p, None),
        lambda: lib.i8ie_conv2d_f32_rect(None, p, 1, 16, 8, 8, p, p, 16, groups, C.byref(g), p),
    ]
    for call in calls:
        assert call() == -1 and text in lib.i8ie_last_error().lower(), lib.i8ie_last_error()


def test_null_geometry_and_kernel_larger_than_input(lib):
    buf = np.zeros(4096, np.int8)
    p = buf.ctypes.data_as(C.c_void_p)
    L = C.c_void_p()
    assert lib.i8ie_conv2d_create_rect(None, p, p, 16, 16, 1, None, C.c_float(0.01), C.byref(L)) == -1
    assert lib.i8ie_conv2d_u8s8_rect(None, p, 1, 16, 8, 8, p, 16, 1, None, 0, p, 0.03, 0.01, 0.05, 0, p, None) == -1
    assert lib.i8ie_conv2d_f32_rect(None, p, 1, 16, 8, 8, p, p, 16, 1, None, p) == -1
    assert lib.i8ie_layer_geometry(None, None) == -1
    g = _geom(kw=7, pad_w=0, dilation_w=2)  # spans 13 columns of an 8-wide map
    assert lib.i8ie_conv2d_u8s8_rect(None, p, 1, 16, 8, 8, p, 16, 1, C.byref(g), 0, p, 0.03, 0.01, 0.05, 0, p, None) == -1
    assert b"larger than padded input" in lib.i8ie_last_error()
    assert lib.i8ie_conv2d_f32_rect(None, p, 1, 16, 8, 8, p, p, 16, 1, C.byref(g), p) == -1
    assert b"larger than padded input" in lib.i8ie_last_error()
    # a valid geometry gets as far as the null pointers
    g = _geom()
    assert lib.i8ie_conv2d_create_rect(None, p, p, 16, 16, 1, C.byref(g), C.c_float(0.01), C.byref(L)) == -1
    assert b"null" in lib.i8ie_last_error()


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_python_argument_rules(i8ie):
    import _CXX_i8ie as cx

    for args in [dict(kernel_size=3), dict(kernel_size=(3, 3)), dict(kernel_size=3, stride=(2, 2), padding=[1, 1], dilation=(2, 2))]:
        L = i8ie.Conv2d(4, 8, **args)
        assert type(L.layer) is cx.Conv2d, args
    for args in [dict(kernel_size=(1, 7), padding=(0, 3)), dict(kernel_size=3, stride=(2, 1)), dict(kernel_size=3, padding=(1, 0)),
                 dict(kernel_size=3, dilation=(1, 2), groups=2)]:
        L = i8ie.Conv2d(4, 8, **args)
        assert type(L.layer) is cx._Conv2dRect, args
    for name in ("kernel_size", "stride", "padding", "dilation"):
        for bad in (3.0, (1, 2, 3), (1,), "3", None, (1.0, 2), True):
            args = dict(kernel_size=3)
            args[name] = bad
            with pytest.raises(TypeError):
                i8ie.Conv2d(4, 8, **args)
    for args in [dict(kernel_size=(1, 3), stride=(1, 0)), dict(kernel_size=(1, 3), padding=(0, -1)), dict(kernel_size=(1, 3), dilation=(1, 0)),
                 dict(kernel_size=(0, 3)), dict(kernel_size=(1, 3), groups=3)]:
        with pytest.raises(RuntimeError):
            i8ie.Conv2d(4, 8, **args)
    # the private class has the method set of the extension's Conv2d (and geometry)
    pub = lambda c: {n for n in dir(c) if not n.startswith("_")} | {"__call__", "__init__"}  # noqa: E731
    assert pub(cx._Conv2dRect) - {"geometry"} == pub(cx.Conv2d)


def test_geometry_and_dilation(i8ie):
    L = i8ie.Conv2d(4, 8, (1, 7), padding=(0, 3))
    assert L.geometry() == dict(kernel_size=(1, 7), stride=(1, 1), padding=(0, 3), dilation=(1, 1)) and L.dilation() == 1
    assert L.layer.geometry() == L.geometry() and L.groups() == 1
    L = i8ie.Conv2d(4, 8, 3, stride=2, padding=1, dilation=2, groups=2)
    assert L.geometry() == dict(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1), dilation=(2, 2)) and L.dilation() == 2
    L = i8ie.Conv2d(4, 8, 3, dilation=(2, 1), groups=4)
    assert L.dilation() == (2, 1) and L.groups() == 4 and L.geometry()["dilation"] == (2, 1)
    assert i8ie.Linear(4, 4).geometry() is None
    # the weight is torch's [out, in / groups, kh, kw]; another shape is refused
    L = i8ie.Conv2d(4, 8, (1, 7), groups=2)
    L.load_weight(np.zeros((8, 2, 1, 7), np.float32))
    with pytest.raises(RuntimeError):
        L.load_weight(np.zeros((8, 2, 7, 1), np.float32))


# ---- the case lists ---------------------------------------------------------------------------------------------------------
def test_case_lists_cover_every_kernel_and_class():
    names = {c.name for c in rr.CASES}
    for cls in rr.CLASSES:
        for suffix in ("-pt", "-pc"):
            assert cls + suffix in names, cls + suffix
    kernels = {rr.dispatch(c) for c in rr.CASES}
    assert kernels == {"lconv_mfma", "gconv_mfma", "gconv_direct"}
    assert {n for n, _ in rr.LINES} <= set(rr.LCONV_CLASSES)
    for name in rr.LCONV_CLASSES:  # every case of the line kernel, the zp and extreme ones too, has its forced twin
        for suffix, forced in (("-pt", False), ("-pc", False), ("-pt-forced", True), ("-pc-forced", True)):
            assert name + suffix in names, name + suffix
            c = rr.BY_NAME[name + suffix]
            assert (rr.dispatch(c) == "lconv_mfma") == (not forced), c.name
            assert rr.dispatch(c) in ("lconv_mfma", "gconv_direct")
    for name, _ in rr.GENERAL:
        assert rr.dispatch(rr.BY_NAME[name + "-pt"]) in ("gconv_mfma", "gconv_direct"), name
    assert {rr.dispatch(rr.BY_NAME[n + "-pt"]) for n, _ in rr.GENERAL} == {"gconv_mfma", "gconv_direct"}
    # the budget: one pixel decides
    over, at = rr.BY_NAME["over_lds_budget-pt"], rr.BY_NAME["at_lds_budget-pt"]
    assert rr.lconv_lds(16, 3, over.w) > rr.LCONV_LDS_BUDGET >= rr.lconv_lds(16, 3, at.w) and over.w == at.w + 1
    for n in rr.LAYOUT_CASES:
        assert rr.BY_NAME[n].kc % 16 == 0
    assert rr.dispatch(rr.BY_NAME[rr.LAYOUT_CASES[0]]) == "lconv_mfma" and rr.dispatch(rr.BY_NAME[rr.LAYOUT_CASES[1]]) != "lconv_mfma"
    # a line of 16 + 1 pixels, a line shorter than k - 1, an output longer than the line, rows of one block from several images
    c = rr.BY_NAME["1x7_line17-pt"]
    assert rr.out_hw(c.h, c.w, c.geom)[1] == 17
    c = rr.BY_NAME["1x7_line4-pt"]
    assert c.w < c.geom.kw - 1
    c = rr.BY_NAME["1x3_out_longer-pt"]
    assert rr.out_hw(c.h, c.w, c.geom)[1] > c.w
    c = rr.BY_NAME["7x1_m37-pt"]
    oh, ow = rr.out_hw(c.h, c.w, c.geom)
    assert oh * ow < rr.LCONV_ROWS and (c.m * oh * ow) % rr.LCONV_ROWS != 0
    c = rr.BY_NAME["1x3_c128-pt"]
    assert c.c // rr.lconv_chunk(c.c) == 2
    for n in ("1x3_pad_across-pt", "7x1_pad_across-pt"):  # padding across the line: output lines that lie outside the image
        c = rr.BY_NAME[n]
        assert (c.geom.ph if c.geom.kh == 1 else c.geom.pw) > 0


def test_budget_constant_is_the_kernels():
    import os
    import re

    src = open(os.path.join(abi.ROOT, "int8inferenceengine_amd", "csrc", "i8ie_lconv.h")).read()
    m = re.search(r"I8IE_LCONV_LDS_BUDGET = \(size_t\)(\d+) << (\d+);", src)
    assert m and int(m.group(1)) << int(m.group(2)) == rr.LCONV_LDS_BUDGET
