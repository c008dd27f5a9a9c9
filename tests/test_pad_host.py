"""pad / crop without a GPU: the numpy restatement of tests/pad_ref.py against torch.nn.functional.pad
on the CPU, exactly; fill_byte against quantize's rule; i8ie_pad_output_shape and every argument rule of the entries and the
surface (error type, op name in the message, raised before any device call); the symbols and the surface; and the classes of
case the GPU test's lists must keep."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest

import abi
import pad_ref as pr
import support
from support import i8ie  # noqa: F401

f32 = np.float32
lib = support.lib_fixture(pr)


def _torch_pad(x, mode, l, r, t, b, fill=0):
    import torch
    import torch.nn.functional as F

    tx = torch.from_numpy(np.ascontiguousarray(x))
    if mode == pr.CONSTANT:
        return F.pad(tx, (l, r, t, b), "constant", fill).numpy()
    return F.pad(tx, (l, r, t, b), pr.MODE_NAME[mode]).numpy()


def _amounts(mode, L):
    """every legal amount 0 .. limit of one side (replicate and constant: up to L + 2)"""
    return range(0, (L + 2 if mode in (pr.REPLICATE, pr.CONSTANT) else pr.limit(mode, L)) + 1)


# ---- the restatement against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pr.MODES, ids=[pr.MODE_NAME[m] for m in pr.MODES])
def test_every_axis_length_and_amount_against_torch(mode):
    """one axis at a time (the other one untouched), lengths 1..8, every legal (before, after): float64 index ramps for the
    map, uint8 for the bytes"""
    tried = 0
    for L in range(1, 9):
        ramp = np.arange(2 * 3 * 2 * L, dtype=np.float64).reshape(2, 3, 2, L) + 0.5
        q = np.random.default_rng(L).integers(0, 256, (2, 3, L, 2), dtype=np.uint8)
        for before, after in itertools.product(_amounts(mode, L), repeat=2):
            assert np.array_equal(pr.apply(ramp, mode, before, after, 0, 0, -7.0), _torch_pad(ramp, mode, before, after, 0, 0, -7.0)), (L, before, after)
            assert np.array_equal(pr.apply(q, mode, 0, 0, before, after, 9), _torch_pad(q, mode, 0, 0, before, after, 9)), (L, before, after)
            tried += 1
    assert tried >= (36 if mode == pr.REFLECT else 100)


@pytest.mark.parametrize("mode", pr.MODES, ids=[pr.MODE_NAME[m] for m in pr.MODES])
def test_two_axes_against_torch(mode):
    for h, w in [(1, 1), (1, 5), (4, 3), (3, 4), (5, 7)]:
        ramp = np.arange(2 * 3 * h * w, dtype=np.float64).reshape(2, 3, h, w)
        q = np.random.default_rng(h * 8 + w).integers(0, 256, (2, 3, h, w), dtype=np.uint8)
        ax = lambda L: sorted({a for a in (0, 1, 2, max(_amounts(mode, L))) if a <= max(_amounts(mode, L))})  # noqa: E731
        for l, r, t, b in itertools.product(ax(w), ax(w), ax(h), ax(h)):
            assert pr.apply(q, mode, l, r, t, b).shape == pr.output_shape(mode, l, r, t, b, *q.shape)
            assert np.array_equal(pr.apply(ramp, mode, l, r, t, b, 3.0), _torch_pad(ramp, mode, l, r, t, b, 3.0)), (h, w, l, r, t, b)
            assert np.array_equal(pr.apply(q, mode, l, r, t, b, 200), _torch_pad(q, mode, l, r, t, b, 200)), (h, w, l, r, t, b)
            assert np.array_equal(pr.apply(q, mode, l, r, t, b, 5, True, 127), np.maximum(_torch_pad(q, mode, l, r, t, b, 5), 127))


def test_negative_and_mixed_amounts_against_torch():
    h, w = 4, 5
    ramp = np.arange(2 * 3 * h * w, dtype=np.float64).reshape(2, 3, h, w)
    q = np.random.default_rng(1).integers(0, 256, (2, 3, h, w), dtype=np.uint8)
    tried = 0
    for l, r, t, b in itertools.product(range(-4, 3), range(-4, 3), (-3, -1, 0, 2), (-3, -2, 0, 1)):
        if w + l + r < 1 or h + t + b < 1:
            assert not (pr.legal(pr.CONSTANT, w, l, r) and pr.legal(pr.CONSTANT, h, t, b))
            continue
        assert np.array_equal(pr.apply(ramp, pr.CONSTANT, l, r, t, b, -1.5), _torch_pad(ramp, pr.CONSTANT, l, r, t, b, -1.5)), (l, r, t, b)
        assert np.array_equal(pr.apply(q, pr.CONSTANT, l, r, t, b, 77), _torch_pad(q, pr.CONSTANT, l, r, t, b, 77)), (l, r, t, b)
        tried += 1
    assert tried > 300
    for case in pr.GEOMETRY_CASES:
        hh, ww, (l, r, t, b), modes = case
        x = pr.channel_bytes((2, 3, hh, ww), 3)
        for mode in modes:
            assert np.array_equal(pr.apply(x, mode, l, r, t, b, 9), _torch_pad(x, mode, l, r, t, b, 9)), case


def test_torch_refuses_what_the_limits_refuse():
    x = np.zeros((1, 1, 4, 5), f32)
    with pytest.raises(RuntimeError):
        _torch_pad(x, pr.REFLECT, 5, 0, 0, 0)       # amount == L
    with pytest.raises(RuntimeError):
        _torch_pad(x, pr.CIRCULAR, 6, 0, 0, 0)      # amount > L
    assert not pr.legal(pr.REFLECT, 5, 5, 0) and pr.legal(pr.REFLECT, 5, 4, 4)
    assert not pr.legal(pr.CIRCULAR, 5, 6, 0) and pr.legal(pr.CIRCULAR, 5, 5, 5)
    assert pr.legal(pr.REPLICATE, 1, 65535, 65535) and not pr.legal(pr.REPLICATE, 1, 65536, 0) and not pr.legal(pr.REPLICATE, 5, -1, 0)


def test_crop_against_slicing():
    q = pr.channel_bytes((2, 3, 4, 5), 2)
    for top, left, hh, ww in [(0, 0, 4, 5), (0, 0, 1, 1), (3, 4, 1, 1), (0, 4, 1, 1), (3, 0, 1, 1), (1, 2, 2, 3), (0, 1, 4, 2)]:
        assert np.array_equal(pr.crop(q, top, left, hh, ww), q[:, :, top:top + hh, left:left + ww])


def test_fill_byte_is_quantizes_rule():
    """(u8)(value / scale + zp): fp32 divide, fp32 add, truncation towards zero, the low 8 bits -- no clamp; the conversion
    saturates at the ends of int32 and NaN is 0"""
    for scale, zp in [(0.025, 127), (0.05, 0), (1.0, 255), (0.1, 3)]:
        assert pr.fill_byte(0.0, scale, zp) == zp and pr.fill_byte(-0.0, scale, zp) == zp
        lo, hi = (0 - zp) * scale, (255 - zp) * scale
        for value in np.linspace(lo - 40 * scale, hi + 40 * scale, 173):  # below, inside and above what a byte represents
            t = f32(f32(f32(value) / f32(scale)) + f32(zp))
            assert pr.fill_byte(float(value), scale, zp) == int(np.trunc(t)) % 256, (value, scale, zp)
        assert pr.fill_byte(hi + 10 * scale, scale, zp) == (255 + 10) % 256   # above the range: wraps, as quantize does
    assert pr.fill_byte(1e30, 0.05, 7) == 0xFF and pr.fill_byte(-1e30, 0.05, 7) == 0 and pr.fill_byte(float("nan"), 0.05, 7) == 0
    assert pr.fill_byte(float("inf"), 0.05, 7) == 0xFF


# ---- i8ie_pad_output_shape and the argument rules of the entries ---------------------------------------------------------------
def _shape(lib, mode, amounts, dims):
    out = (C.c_int * 4)(-7, -7, -7, -7)
    rc = lib.i8ie_pad_output_shape(mode, *amounts, *dims, out)
    return rc, tuple(out), lib.i8ie_last_error().decode()


# (mode, (left, right, top, bottom), (n, c, h, w)): every limit at limit and at limit + 1, O = 1 and O = 0
GOOD = [(pr.REFLECT, (4, 4, 3, 3), (2, 3, 4, 5)), (pr.CIRCULAR, (5, 5, 4, 4), (2, 3, 4, 5)), (pr.REPLICATE, (65535, 65535, 65535, 65535), (1, 1, 1, 1)),
        (pr.CONSTANT, (65535, 0, 0, 65535), (1, 1, 1, 1)), (pr.CONSTANT, (-4, 0, -3, 0), (2, 3, 4, 5)), (pr.CONSTANT, (-2, -2, -1, -2), (2, 3, 4, 5)),
        (pr.CONSTANT, (-5, 1, 0, 0), (2, 3, 4, 5)), (pr.CONSTANT, (-1, 2, 1, -2), (2, 3, 5, 7)), (pr.REFLECT, (0, 0, 0, 0), (1, 1, 1, 1)),
        (pr.CIRCULAR, (1, 1, 1, 1), (1, 1, 1, 1))]
BAD = [(pr.REFLECT, (5, 0, 0, 0), (2, 3, 4, 5)), (pr.REFLECT, (0, 5, 0, 0), (2, 3, 4, 5)), (pr.REFLECT, (0, 0, 4, 0), (2, 3, 4, 5)),
       (pr.REFLECT, (0, 0, 0, 4), (2, 3, 4, 5)), (pr.REFLECT, (1, 0, 0, 0), (1, 1, 1, 1)),
       (pr.CIRCULAR, (6, 0, 0, 0), (2, 3, 4, 5)), (pr.CIRCULAR, (0, 6, 0, 0), (2, 3, 4, 5)), (pr.CIRCULAR, (0, 0, 5, 0), (2, 3, 4, 5)),
       (pr.CIRCULAR, (0, 0, 0, 5), (2, 3, 4, 5)),
       (pr.REPLICATE, (65536, 0, 0, 0), (1, 1, 1, 1)), (pr.CONSTANT, (0, 0, 0, 65536), (1, 1, 1, 1)), (pr.CONSTANT, (-65536, 0, 0, 0), (1, 1, 1, 70000)),
       (pr.REFLECT, (-1, 0, 0, 0), (2, 3, 4, 5)), (pr.REPLICATE, (0, 0, 0, -1), (2, 3, 4, 5)), (pr.CIRCULAR, (0, -2, 0, 0), (2, 3, 4, 5)),
       (pr.CONSTANT, (-5, 0, 0, 0), (2, 3, 4, 5)), (pr.CONSTANT, (-3, -2, 0, 0), (2, 3, 4, 5)), (pr.CONSTANT, (0, 0, -2, -2), (2, 3, 4, 5)),
       (pr.CONSTANT, (0, 0, -9, 1), (2, 3, 4, 5)),
       (pr.CONSTANT, (1, 1, 1, 1), (0, 3, 4, 5)), (pr.REFLECT, (1, 1, 1, 1), (2, 0, 4, 5)), (pr.CONSTANT, (1, 1, 1, 1), (2, 3, -4, 5)),
       (pr.CONSTANT, (1, 1, 1, 1), (2, 3, 4, 0))]


def test_output_shape(lib):
    for mode, amounts, dims in GOOD:
        rc, out, msg = _shape(lib, mode, amounts, dims)
        assert rc == 0 and out == pr.output_shape(mode, *amounts, *dims), (mode, amounts, dims, msg)
    for mode, amounts, dims in BAD:
        rc, out, msg = _shape(lib, mode, amounts, dims)
        assert rc == -1 and out == (-7, -7, -7, -7) and msg.startswith("pad:"), (mode, amounts, dims, msg)
        if min(dims) > 0:
            assert not (pr.legal(mode, dims[3], *amounts[:2]) and pr.legal(mode, dims[2], *amounts[2:]))
    for mode in (-1, 4):
        rc, _, msg = _shape(lib, mode, (1, 1, 1, 1), (1, 4, 2, 2))
        assert rc == -1 and "mode" in msg
    assert lib.i8ie_pad_output_shape(0, 1, 1, 1, 1, 1, 4, 2, 2, None) == -1


def test_entries_refuse_before_any_device_call(lib):
    """Every refusal of the three device entries, on a machine without a device: the context is a zeroed block that no refusal
    may read (a call that got past the checks would fail in the HIP runtime with another code), the buffers are host memory
    that is never touched."""
    fake = (C.c_uint8 * 4096)()
    h = C.cast(fake, C.c_void_p)
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    a, b = C.c_void_p(p), C.c_void_p(p + (1 << 15))   # two disjoint halves

    def nhwc(ctx=h, i=a, ib=0, o=b, ob=0, mode=pr.REFLECT, amounts=(1, 1, 1, 1), dims=(1, 4, 2, 2)):
        return lib.i8ie_pad2d_u8_nhwc(ctx, i, ib, 0, o, ob, 0, *dims, mode, *amounts, 0, 0, 0)

    def flat(f, ctx=h, i=a, o=b, mode=pr.REFLECT, amounts=(1, 1, 1, 1), dims=(1, 4, 2, 2)):
        return f(ctx, i, o, *dims, mode, *amounts, 0)

    def refused(rc, word):
        msg = lib.i8ie_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg, word)

    refused(nhwc(ctx=None), "null")
    refused(nhwc(i=None), "null")
    refused(nhwc(o=None), "null")
    refused(nhwc(ib=-1), "bad dimension")
    refused(nhwc(ob=-1), "bad dimension")
    refused(nhwc(o=a), "overlaps")
    refused(nhwc(o=C.c_void_p(p + 15)), "overlaps")                     # the last input byte is the first output byte
    refused(nhwc(i=C.c_void_p(p + 143), o=a, ob=1), "overlaps")         # ... and the bordered result's last byte the first input byte
    for f in (lib.i8ie_pad2d_u8, lib.i8ie_pad2d_f32):
        refused(flat(f, ctx=None), "null")
        refused(flat(f, i=None), "null")
        refused(flat(f, o=None), "null")
        refused(flat(f, o=a), "overlaps")
    refused(flat(lib.i8ie_pad2d_u8, o=C.c_void_p(p + 15)), "overlaps")
    refused(flat(lib.i8ie_pad2d_f32, o=C.c_void_p(p + 60)), "overlaps")
    refused(flat(lib.i8ie_pad2d_f32, i=C.c_void_p(p + 2)), "aligned")
    for mode, amounts, dims in BAD:
        refused(nhwc(mode=mode, amounts=amounts, dims=dims), "pad:")
        refused(flat(lib.i8ie_pad2d_u8, mode=mode, amounts=amounts, dims=dims), "pad:")
        refused(flat(lib.i8ie_pad2d_f32, mode=mode, amounts=amounts, dims=dims), "pad:")
    for mode in (-1, 4):
        refused(nhwc(mode=mode), "mode")
        refused(flat(lib.i8ie_pad2d_u8, mode=mode), "mode")
        refused(flat(lib.i8ie_pad2d_f32, mode=mode), "mode")
    refused(nhwc(amounts=(0, 0, 0, 0), dims=(1, 1 << 20, 1 << 6, 1 << 6)), "2^31")
    assert not buf.any() and not bytes(fake).strip(b"\0")


def test_symbols_declared_and_exported(lib):
    header = open(abi.HEADER).read()
    for name in ("i8ie_pad_output_shape", "i8ie_pad2d_u8_nhwc", "i8ie_pad2d_u8", "i8ie_pad2d_f32"):
        assert name in abi.declared_symbols() and hasattr(lib, name), name
    for macro, k in [("CONSTANT", 0), ("REFLECT", 1), ("REPLICATE", 2), ("CIRCULAR", 3)]:
        assert "#define I8IE_PAD_%s %d" % (macro, k) in header
    assert (pr.CONSTANT, pr.REFLECT, pr.REPLICATE, pr.CIRCULAR) == (0, 1, 2, 3)
    assert "Spatial padding" in header


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_surface_exports_and_private_entry(i8ie):
    import _CXX_i8ie as cx

    for name in ("pad", "crop"):
        assert name in i8ie.__all__ and callable(getattr(i8ie, name)) and not hasattr(cx, name), name
    want = support.golden_json("binding_surface_pad.json")
    assert sorted(want) == ["_pad"]
    assert {n: getattr(cx, n).__doc__ for n in want} == want
    doc = want["_pad"]   # FP32 first, then uint8, then the int8 overload that refuses
    assert doc.index("6TensorIfE") < doc.index("6TensorIhE") < doc.index("6TensorIcE")
    assert list(inspect.signature(i8ie.pad).parameters) == ["x", "pad", "mode", "value"]
    assert inspect.signature(i8ie.pad).parameters["mode"].default == "constant" and inspect.signature(i8ie.pad).parameters["value"].default == 0.0
    assert list(inspect.signature(i8ie.crop).parameters) == ["x", "top", "left", "height", "width"]
    # no Layer class came with them: nothing to prepare or convert
    assert not any(hasattr(i8ie, n) for n in ("Pad", "ReflectionPad2d", "ZeroPad2d", "Crop"))
    assert "_pad" not in support.golden_json("binding_surface.json")


def test_surface_errors_come_before_any_device_call(i8ie):
    """(there is no GPU here: anything that reached the device would fail with another message)"""
    t = i8ie.tensor(np.zeros((2, 3, 4, 5), f32))
    geometry = {
        "pad": [lambda: i8ie.pad(t, (5, 0), "reflect"), lambda: i8ie.pad(t, (0, 0, 0, 4), "reflect"), lambda: i8ie.pad(t, (6, 0), "circular"),
                lambda: i8ie.pad(t, (0, 0, 5, 0), "circular"), lambda: i8ie.pad(t, (-1, 0), "replicate"), lambda: i8ie.pad(t, (0, 0, 0, -1), "reflect"),
                lambda: i8ie.pad(t, (0, -1), "circular"), lambda: i8ie.pad(t, (-5, 0)), lambda: i8ie.pad(t, (0, 0, -2, -2)),
                lambda: i8ie.pad(t, (65536, 0)), lambda: i8ie.pad(t, (0, 0, 0, 65536), "replicate"), lambda: i8ie.pad(t, (1, 1), "zeros"),
                lambda: i8ie.pad(t, (1, 1), "symmetric"), lambda: i8ie.pad(t.reshape(2, 3, 20), (1, 1)), lambda: i8ie.pad(t.reshape(6, 20), (1, 1))],
        "crop": [lambda: i8ie.crop(t, 0, 0, 5, 5), lambda: i8ie.crop(t, 0, 0, 4, 6), lambda: i8ie.crop(t, -1, 0, 2, 2), lambda: i8ie.crop(t, 0, -1, 2, 2),
                 lambda: i8ie.crop(t, 0, 0, 0, 1), lambda: i8ie.crop(t, 0, 0, 1, 0), lambda: i8ie.crop(t, 3, 4, 2, 1), lambda: i8ie.crop(t, 4, 0, 1, 1),
                 lambda: i8ie.crop(t.reshape(2, 3, 20), 0, 0, 1, 1)],
    }
    for name, calls in geometry.items():
        for i, bad in enumerate(calls):
            with pytest.raises(RuntimeError, match=name):
                bad()
    types = {
        "pad": [lambda: i8ie.pad(t, (1.0, 0)), lambda: i8ie.pad(t, (True, 0)), lambda: i8ie.pad(t, (1, 1, "1", 1)), lambda: i8ie.pad(t, 1),
                lambda: i8ie.pad(t, (1, 1, 1)), lambda: i8ie.pad(t, ()), lambda: i8ie.pad(t, (1, 1), "reflect", 1.0),
                lambda: i8ie.pad(t, (1, 1), "replicate", -2), lambda: i8ie.pad(t, (1, 1), "circular", 0.5), lambda: i8ie.pad(t, (1, 1), "constant", "0"),
                lambda: i8ie.pad(t, (1, 1), "constant", None)],
        "crop": [lambda: i8ie.crop(t, 0.0, 0, 1, 1), lambda: i8ie.crop(t, 0, 0, True, 1), lambda: i8ie.crop(t, 0, 0, 1, "1"), lambda: i8ie.crop(t, None, 0, 1, 1)],
    }
    for name, calls in types.items():
        for bad in calls:
            with pytest.raises(TypeError, match=name):
                bad()
    # value = 0 (of either sign) is no value; all-zero amounts are the operand itself, in every mode
    for mode in pr.MODE_NAME.values():
        assert i8ie.pad(t, (0, 0, 0, 0), mode, -0.0) is t and i8ie.pad(t, (0, 0), mode) is t
    assert i8ie.crop(t, 0, 0, 4, 5) is t


def test_s8_tensors_are_refused(i8ie):
    """an int8 tensor is refused with the op's name, whatever it holds (a default-constructed one: no device needed)"""
    import _CXX_i8ie as cx

    s8 = i8ie.Tensor(getattr(cx, "6TensorIcE")())
    for name, call in [("pad", lambda: i8ie.pad(s8, (1, 1))), ("crop", lambda: i8ie.crop(s8, 0, 0, 1, 1))]:
        with pytest.raises(RuntimeError, match=name + ".*int8"):
            call()
    with pytest.raises(RuntimeError, match="pad.*int8"):
        cx._pad(s8.data, 1, 1, 0, 0, 0, 0.0)


# ---- the GPU test's case lists keep every class of case ---------------------------------------------------------------------------
def test_gpu_case_lists_contain_each_class():
    cases = [(h, w, a, m) for h, w, a, modes in pr.GEOMETRY_CASES for m in modes]
    assert {m for _, _, _, m in cases} == set(pr.MODES)                                            # each mode
    for h, w, (l, r, t, b), m in cases:
        assert pr.legal(m, w, l, r) and pr.legal(m, h, t, b), (h, w, l, r, t, b, m)
    assert (5, 7, (2, 1, 3, 0), pr.MODES) in pr.GEOMETRY_CASES
    for mode in (pr.REFLECT, pr.CIRCULAR):                                                        # an amount at its limit, all four sides
        assert any(m == mode and (l, r) == (pr.limit(m, w),) * 2 and (t, b) == (pr.limit(m, h),) * 2 for h, w, (l, r, t, b), m in cases), mode
    assert any(m == pr.REPLICATE and (h, w) == (1, 1) and min(a) > 1 for h, w, a, m in cases)      # one-pixel maps
    assert any(m == pr.REPLICATE and h == 1 and w > 1 for h, w, a, m in cases)
    assert any(a[0] == a[1] == 0 and (a[2] or a[3]) for _, _, a, _ in cases) and any(a[2] == a[3] == 0 and (a[0] or a[1]) for _, _, a, _ in cases)
    corners = {(l == 0, t == 0) for h, w, (l, r, t, b), m in cases if h + t + b == 1 and w + l + r == 1 and min(l, r, t, b) < 0}
    assert corners == {(True, True), (True, False), (False, True), (False, False)}                  # crop to 1 x 1 from each corner
    assert any(min(a) < 0 < max(a) and min(a[:2]) < 0 < max(a[:2]) and min(a[2:]) < 0 < max(a[2:]) for _, _, a, _ in cases)  # mixed signs per axis
    assert {pr.item_width(c) for c in pr.CHANNELS} == {16, 4, 1} and pr.CHANNELS == (3, 20, 16, 48) and pr.BATCH == 2  # each item width
    assert pr.ZPS == (0, 127, 255) and min(pr.FILLS) < 127 < max(pr.FILLS)
    # the seam cases: waves that are all inner, all edge and mixed (and the issue's own two cases are among them)
    assert pr.SEAM_MAP == (40, 40) and {(16, 1), (16, 3)} <= set(pr.SEAM_CASES)
    seen = {"inner": 0, "edge": 0, "mixed": 0}
    for c, p in pr.SEAM_CASES:
        for k, v in pr.wave_classes(pr.BATCH, c, *pr.SEAM_MAP, p, p, p, p).items():
            seen[k] += v
    assert min(seen.values()) > 0, seen
    assert pr.wave_classes(1, 16, 4, 4, 0, 0, 0, 0) == {"inner": 1, "edge": 0, "mixed": 0}
    assert pr.wave_classes(1, 16, 1, 1, 8, 8, 8, 8)["edge"] >= 3
    # the layout matrix: every border and item width; the wrap cases: more items than one grid pass, but not twice as many
    assert pr.IN_BORDERS == (0, 1, 2) and pr.OUT_BORDERS == (0, 1, 2)
    assert [pr.item_width(pr.LAYOUT_CASE[0], s) for s in pr.SKEWS] == [16, 4, 1]
    assert pr.MAX_LANES == 2 ** 19
    for n, c, h, w, (l, r, t, b), mode in pr.WRAP_CASES:
        assert pr.legal(mode, w, l, r) and pr.legal(mode, h, t, b)
        assert pr.MAX_LANES < pr.items(n, c, h + t + b, w + l + r) < 1.05 * pr.MAX_LANES
    assert {pr.item_width(c) for _, c, *_ in pr.WRAP_CASES} == {16, 1}
