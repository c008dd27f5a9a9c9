"""narrow / split / chunk / channel_shuffle / pixel_shuffle / pixel_unshuffle without a GPU: the numpy
restatement of tests/rearrange_ref.py against torch on the CPU, exactly; i8ie_rearrange_output_shape and every argument rule
(error type, op name in the message, raised before any device call); the symbols and the surface; and the classes of case
the GPU test's lists must keep."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi
import rearrange_ref as rr
import support
from support import i8ie  # noqa: F401

f32 = np.float32
lib = support.lib_fixture(rr)


def _bytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the restatement against torch ---------------------------------------------------------------------------------------------
def test_narrow_split_chunk_against_torch():
    import torch

    for shape in [(2, 7, 3, 4), (3, 116, 2, 2), (5, 35)]:
        x = _bytes(shape, shape[1])
        t = torch.from_numpy(x)
        c = shape[1]
        for start, length in [(0, c), (0, 1), (c - 1, 1), (1, c - 1), (c // 2, c - c // 2)]:
            assert np.array_equal(rr.narrow(x, start, length), torch.narrow(t, 1, start, length).numpy())
            assert np.array_equal(rr.narrow(x, start, length, True, 100), np.maximum(torch.narrow(t, 1, start, length).numpy(), 100))
        for sizes in [1, 2, 3, c - 1, c, c + 5, [c], [1, c - 1], [c - 3, 2, 1]]:  # (uneven last parts among them)
            got, want = rr.split(x, sizes), torch.split(t, sizes, 1)
            assert len(got) == len(want) and all(np.array_equal(g, w.numpy()) for g, w in zip(got, want)), sizes
        for chunks in [1, 2, 3, 4, c - 1, c, c + 3]:
            got, want = rr.chunk(x, chunks), torch.chunk(t, chunks, 1)
            assert len(got) == len(want) and all(np.array_equal(g, w.numpy()) for g, w in zip(got, want)), chunks
    assert [p.shape[1] for p in rr.chunk(np.zeros((1, 7, 1, 1), np.uint8), 3)] == [3, 3, 1]
    assert [p.shape[1] for p in rr.chunk(np.zeros((1, 6, 1, 1), np.uint8), 4)] == [2, 2, 2]  # fewer parts than asked for


def test_channel_shuffle_against_torch():
    import torch

    for c in (8, 24, 48):
        x = _bytes((2, c, 3, 2), c)
        for g in (1, 2, 3, 4, 8, c):
            if c % g:
                continue
            want = torch.nn.ChannelShuffle(g)(torch.from_numpy(x.astype(f32))).numpy().astype(np.uint8)
            assert np.array_equal(rr.channel_shuffle(x, g), want), (c, g)
            view = x.reshape(2, g, c // g, 3, 2).transpose(0, 2, 1, 3, 4).reshape(2, c, 3, 2)
            assert np.array_equal(rr.channel_shuffle(x, g), view)
    tried = [g for g in (1, 2, 3, 4, 8) if 24 % g == 0]
    assert tried == [1, 2, 3, 4, 8]


def test_pixel_shuffle_and_unshuffle_against_torch():
    import torch
    import torch.nn.functional as F

    for r in range(1, 9):
        x = _bytes((2, 3 * r * r, 2, 3), r)
        want = F.pixel_shuffle(torch.from_numpy(x.astype(f32)), r).numpy().astype(np.uint8)
        got = rr.pixel_shuffle(x, r)
        assert got.shape == (2, 3, 2 * r, 3 * r) and np.array_equal(got, want), r
        y = _bytes((2, 3, 2 * r, 3 * r), 50 + r)
        want = F.pixel_unshuffle(torch.from_numpy(y.astype(f32)), r).numpy().astype(np.uint8)
        got = rr.pixel_unshuffle(y, r)
        assert got.shape == (2, 3 * r * r, 2, 3) and np.array_equal(got, want), r
        assert np.array_equal(rr.pixel_shuffle(rr.pixel_unshuffle(y, r), r), y)  # shuffle o unshuffle = identity
        assert np.array_equal(rr.pixel_unshuffle(rr.pixel_shuffle(x, r), r), x)
        for zp in rr.ZPS:
            assert np.array_equal(rr.pixel_shuffle(x, r, True, zp), np.maximum(rr.pixel_shuffle(x, r), zp))


def test_channel_bytes_tell_every_channel_apart():
    q = rr.channel_bytes((3, 232, 3, 5), 1)
    assert q.dtype == np.uint8 and q.shape == (3, 232, 3, 5)
    assert len(np.unique(q[0, :, 1, 2])) == 232 and len(np.unique(q[1, 7].ravel())) == 15


# ---- i8ie_rearrange_output_shape and the argument rules -------------------------------------------------------------------------
def _shape(lib, kind, p0, p1, dims):
    out = (C.c_int * 4)(-7, -7, -7, -7)
    rc = lib.i8ie_rearrange_output_shape(kind, p0, p1, *dims, out)
    return rc, tuple(out), lib.i8ie_last_error().decode()


def test_output_shape(lib):
    good = [(rr.NARROW, 3, 5, (2, 35, 3, 4)), (rr.NARROW, 0, 35, (2, 35, 3, 4)), (rr.NARROW, 34, 1, (2, 35, 1, 1)),
            (rr.CHANNEL_SHUFFLE, 1, 0, (2, 35, 3, 4)), (rr.CHANNEL_SHUFFLE, 7, 0, (2, 35, 3, 4)), (rr.CHANNEL_SHUFFLE, 35, 0, (2, 35, 3, 4)),
            (rr.PIXEL_SHUFFLE, 1, 0, (2, 35, 3, 4)), (rr.PIXEL_SHUFFLE, 2, 0, (1, 64, 16, 16)), (rr.PIXEL_SHUFFLE, 8, 0, (1, 64, 2, 3)),
            (rr.PIXEL_UNSHUFFLE, 2, 0, (1, 3, 32, 32)), (rr.PIXEL_UNSHUFFLE, 8, 0, (5, 1, 16, 24)), (rr.PIXEL_UNSHUFFLE, 1, 0, (5, 7, 3, 5))]
    for kind, p0, p1, dims in good:
        rc, out, _ = _shape(lib, kind, p0, p1, dims)
        assert rc == 0 and out == rr.output_shape(kind, p0, p1, *dims), (kind, p0, p1, dims)
    bad = [(rr.NARROW, -1, 5, (2, 35, 3, 4)), (rr.NARROW, 0, 0, (2, 35, 3, 4)), (rr.NARROW, 31, 5, (2, 35, 3, 4)),
           (rr.NARROW, 2 ** 31 - 1, 2 ** 31 - 1, (2, 35, 3, 4)),
           (rr.CHANNEL_SHUFFLE, 0, 0, (2, 35, 3, 4)), (rr.CHANNEL_SHUFFLE, 2, 0, (2, 35, 3, 4)), (rr.CHANNEL_SHUFFLE, -5, 0, (2, 35, 3, 4)),
           (rr.PIXEL_SHUFFLE, 0, 0, (2, 36, 3, 4)), (rr.PIXEL_SHUFFLE, 9, 0, (2, 81, 3, 4)), (rr.PIXEL_SHUFFLE, 2, 0, (2, 35, 3, 4)),
           (rr.PIXEL_UNSHUFFLE, 0, 0, (2, 3, 4, 4)), (rr.PIXEL_UNSHUFFLE, 9, 0, (2, 3, 9, 9)), (rr.PIXEL_UNSHUFFLE, 2, 0, (2, 3, 5, 4)),
           (rr.PIXEL_UNSHUFFLE, 2, 0, (2, 3, 4, 5)), (rr.PIXEL_UNSHUFFLE, 8, 0, (1, 1024, 8, 8)),
           (rr.NARROW, 0, 1, (0, 35, 3, 4)), (rr.CHANNEL_SHUFFLE, 1, 0, (2, 0, 3, 4)), (rr.PIXEL_SHUFFLE, 1, 0, (2, 4, -3, 4))]
    for kind, p0, p1, dims in bad:
        rc, out, msg = _shape(lib, kind, p0, p1, dims)
        assert rc == -1 and out == (-7, -7, -7, -7) and msg.startswith(rr.KIND_NAME[kind] + ":"), (kind, p0, p1, dims, msg)
    rc, _, msg = _shape(lib, 4, 1, 0, (1, 4, 2, 2))
    assert rc == -1 and "kind" in msg
    assert lib.i8ie_rearrange_output_shape(0, 0, 1, 1, 4, 2, 2, None) == -1


def test_symbols_declared_and_exported(lib):
    header = open(abi.HEADER).read()
    for name in ("i8ie_rearrange_output_shape", "i8ie_rearrange_u8_nhwc", "i8ie_rearrange_u8", "i8ie_rearrange_f32"):
        assert name in abi.declared_symbols() and hasattr(lib, name)
    for k, (macro, _) in enumerate([("NARROW", 0), ("CHANNEL_SHUFFLE", 1), ("PIXEL_SHUFFLE", 2), ("PIXEL_UNSHUFFLE", 3)]):
        assert "#define I8IE_REARRANGE_%s %d" % (macro, k) in header
    assert (rr.NARROW, rr.CHANNEL_SHUFFLE, rr.PIXEL_SHUFFLE, rr.PIXEL_UNSHUFFLE) == (0, 1, 2, 3)
    # a null context is an argument error like everywhere else
    assert lib.i8ie_rearrange_u8_nhwc(None, None, 0, 0, None, 0, 0, 1, 4, 2, 2, 1, 2, 0, 0, 0) == -1 and b"null" in lib.i8ie_last_error()
    assert lib.i8ie_rearrange_u8(None, None, None, 1, 4, 2, 2, 1, 2, 0) == -1 and lib.i8ie_rearrange_f32(None, None, None, 1, 4, 2, 2, 1, 2, 0) == -1


# ---- the surface ------------------------------------------------------------------------------------------------------------------
NAMES = ["narrow", "split", "chunk", "channel_shuffle", "pixel_shuffle", "pixel_unshuffle"]


def test_surface_exports_and_private_entries(i8ie):
    import _CXX_i8ie as cx

    for name in NAMES:
        assert name in i8ie.__all__ and callable(getattr(i8ie, name)) and not hasattr(cx, name), name
    want = support.golden_json("binding_surface_rearrange.json")
    assert sorted(want) == ["_channel_shuffle", "_narrow", "_pixel_shuffle", "_pixel_unshuffle"]
    assert {n: getattr(cx, n).__doc__ for n in want} == want
    for doc in want.values():  # FP32 first, then uint8, then the int8 overload that refuses
        assert doc.index("6TensorIfE") < doc.index("6TensorIhE") < doc.index("6TensorIcE")
    assert list(inspect.signature(i8ie.narrow).parameters) == ["x", "start", "length"]
    assert list(inspect.signature(i8ie.channel_shuffle).parameters) == ["x", "groups"]
    # no Layer class came with them: nothing to prepare or convert
    assert not any(hasattr(i8ie, n) for n in ("ChannelShuffle", "PixelShuffle", "PixelUnshuffle", "Narrow"))


def test_surface_errors_come_before_any_device_call(i8ie):
    """(there is no GPU here: anything that reached the device would fail with another message)"""
    t = i8ie.tensor(np.zeros((2, 36, 4, 6), f32))
    rows = t.reshape(8, 216)
    geometry = {
        "narrow": [lambda: i8ie.narrow(t, -1, 4), lambda: i8ie.narrow(t, 0, 0), lambda: i8ie.narrow(t, 30, 7), lambda: i8ie.narrow(t.reshape(2, 36, 24), 0, 1),
                   lambda: i8ie.narrow(rows, 216, 1)],
        "split": [lambda: i8ie.split(t, 0), lambda: i8ie.split(t, [30, 5]), lambda: i8ie.split(t, [36, 0]), lambda: i8ie.split(t, []),
                  lambda: i8ie.split(t.reshape(2, 36, 24), 2)],
        "chunk": [lambda: i8ie.chunk(t, 0), lambda: i8ie.chunk(t, -2), lambda: i8ie.chunk(t.reshape(2, 36, 24), 2)],
        "channel_shuffle": [lambda: i8ie.channel_shuffle(t, 0), lambda: i8ie.channel_shuffle(t, 5), lambda: i8ie.channel_shuffle(t, -1),
                            lambda: i8ie.channel_shuffle(rows, 2)],
        "pixel_shuffle": [lambda: i8ie.pixel_shuffle(t, 0), lambda: i8ie.pixel_shuffle(t, 9), lambda: i8ie.pixel_shuffle(t, 4),
                          lambda: i8ie.pixel_shuffle(rows, 2)],
        "pixel_unshuffle": [lambda: i8ie.pixel_unshuffle(t, 0), lambda: i8ie.pixel_unshuffle(t, 9), lambda: i8ie.pixel_unshuffle(t, 4),
                            lambda: i8ie.pixel_unshuffle(t, 3), lambda: i8ie.pixel_unshuffle(rows, 2)],
    }
    assert sorted(geometry) == sorted(NAMES)
    for name, calls in geometry.items():
        for i, bad in enumerate(calls):
            with pytest.raises(RuntimeError, match=name):
                bad()
    types = {
        "narrow": [lambda: i8ie.narrow(t, 1.0, 4), lambda: i8ie.narrow(t, 0, "4"), lambda: i8ie.narrow(t, True, 4)],
        "split": [lambda: i8ie.split(t, 2.0), lambda: i8ie.split(t, [18, 18.0]), lambda: i8ie.split(t, True)],
        "chunk": [lambda: i8ie.chunk(t, 2.0), lambda: i8ie.chunk(t, "2")],
        "channel_shuffle": [lambda: i8ie.channel_shuffle(t, 2.0), lambda: i8ie.channel_shuffle(t, None), lambda: i8ie.channel_shuffle(t, True)],
        "pixel_shuffle": [lambda: i8ie.pixel_shuffle(t, 2.0), lambda: i8ie.pixel_shuffle(t, (2, 2))],
        "pixel_unshuffle": [lambda: i8ie.pixel_unshuffle(t, 2.0), lambda: i8ie.pixel_unshuffle(t, False)],
    }
    assert sorted(types) == sorted(NAMES)
    for name, calls in types.items():
        for bad in calls:
            with pytest.raises(TypeError, match=name):
                bad()


def test_s8_tensors_are_refused(i8ie):
    """an int8 tensor is refused with the op's name, whatever it holds (a default-constructed one: no device needed)"""
    import _CXX_i8ie as cx

    s8 = i8ie.Tensor(getattr(cx, "6TensorIcE")())
    for name, call in [("narrow", lambda: i8ie.narrow(s8, 0, 2)),
                       ("channel_shuffle", lambda: i8ie.channel_shuffle(s8, 2)), ("pixel_shuffle", lambda: i8ie.pixel_shuffle(s8, 2)),
                       ("pixel_unshuffle", lambda: i8ie.pixel_unshuffle(s8, 2))]:
        with pytest.raises(RuntimeError, match=name + ".*int8"):
            call()


# ---- the GPU test's case lists keep every class of case ---------------------------------------------------------------------------
def test_gpu_case_lists_contain_each_class():
    items = {rr.narrow_item(*case) for case in rr.NARROW_CASES}
    assert items == {16, 8, 4, 2, 1}, items                                  # every item width of narrow_u8_nhwc
    assert any(s == 0 for _, s, _ in rr.NARROW_CASES) and any(s + l == c for c, s, l in rr.NARROW_CASES)
    assert any(s == 0 and l == c for c, s, l in rr.NARROW_CASES) and any(l == 1 for _, _, l in rr.NARROW_CASES)
    assert (116, 58, 58) in rr.NARROW_CASES                                  # the ShuffleNetV2 half
    assert {(h, w) for _, h, w in rr.NARROW_MAPS} == {(3, 5), (1, 1)} and {n for n, _, _ in rr.NARROW_MAPS} == {1, 5}
    assert rr.NARROW_ROWS == (5, 35)

    def perm_mode(A, B):
        return "pair" if A == 2 and B % 4 == 0 else ("quad" if A % 4 == 0 and B % 4 == 0 else "byte")

    fast = [(c, g) for c, g in rr.SHUFFLE_CASES if rr.expected_kernel(rr.CHANNEL_SHUFFLE, c, g) == rr.FAST]
    direct = [(c, g) for c, g in rr.SHUFFLE_CASES if rr.expected_kernel(rr.CHANNEL_SHUFFLE, c, g) == rr.DIRECT]
    assert {perm_mode(g, c // g) for c, g in fast} == {"pair", "quad", "byte"} and len(direct) >= 3
    assert any(g == 1 for _, g in rr.SHUFFLE_CASES) and any(g == c for c, g in rr.SHUFFLE_CASES)
    assert {n for n, _, _ in rr.SHUFFLE_MAPS} == {1, 5}
    kernels = {(r, rr.expected_kernel(rr.PIXEL_SHUFFLE, co * r * r, r)) for co, r in rr.PIXEL_CASES}
    assert {k for _, k in kernels} == {rr.FAST, rr.DIRECT}
    assert {r for _, r in rr.PIXEL_CASES} >= {1, 2, 3, 4, 8}
    assert {perm_mode(co, r * r) for co, r in rr.PIXEL_CASES if co % 16 == 0} >= {"quad", "byte"}
    # the unshuffle of the matching outputs takes the fast path exactly where its input has 16 channels
    assert all((rr.expected_kernel(rr.PIXEL_UNSHUFFLE, co, r) == rr.FAST) == (co % 16 == 0) for co, r in rr.PIXEL_CASES)
    assert rr.ZPS == (0, 127, 255) and rr.IN_BORDERS == (0, 1, 3) and rr.OUT_BORDERS == (0, 1, 2)
    for kind in (rr.NARROW, rr.CHANNEL_SHUFFLE, rr.PIXEL_SHUFFLE, rr.PIXEL_UNSHUFFLE):
        ks = [rr.expected_kernel(k, c, p0, p1) for k, c, p0, p1, _, _ in rr.LAYOUT_CASES if k == kind]
        assert len(ks) == 2 and (kind == rr.NARROW or set(ks) == {rr.FAST, rr.DIRECT}), (kind, ks)
    lay_items = {rr.narrow_item(c, p0, p1) for k, c, p0, p1, _, _ in rr.LAYOUT_CASES if k == rr.NARROW}
    assert lay_items == {16, 1}
