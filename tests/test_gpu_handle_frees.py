"""A layer handle frees what it takes: for one tiny layer per route of csrc/i8ie_layer.hip, per tensor and per channel, the
ctx's live device bytes (i8ie_memory_stats) after create -> one forward (so that lazily made buffers count) -> destroy are
the bytes from before the create."""
import ctypes as C

import numpy as np
import pytest

import abi
import support

pytestmark = pytest.mark.gpu

# route -> (create entry, out features, in channels (Linear: in features), kernel, the entry's further int arguments, input h = w)
LAYERS = {
    "linear": ("i8ie_linear_create", 16, 32, 0, (), 0),
    "A": ("i8ie_conv2d_create", 16, 16, 3, (1, 1), 8),                    # stride, pad
    "B_stem": ("i8ie_conv2d_create", 32, 3, 4, (4, 0), 16),
    "B_no_stem": ("i8ie_conv2d_create", 16, 3, 4, (4, 0), 16),
    "F": ("i8ie_conv2d_create", 8, 5, 3, (1, 0), 8),
    "G_grouped": ("i8ie_conv2d_create_grouped", 8, 8, 3, (1, 0, 2), 8),   # stride, pad, groups
    "G_dilated": ("i8ie_conv2d_create_dilated", 16, 16, 3, (1, 2, 1, 2), 8),  # stride, pad, groups, dilation
    "T": ("i8ie_conv_transpose2d_create", 4, 4, 3, (2, 1, 0), 5),         # stride, pad, output_pad
}
M = 2


ctx = support.ctx_fixture()


def live(ctx):
    n = C.c_size_t(0)
    abi.ck(abi.lib().i8ie_memory_stats(ctx.h, C.byref(n), None, None))
    return n.value


@pytest.mark.parametrize("pc", (False, True), ids=("per_tensor", "per_channel"))
@pytest.mark.parametrize("route", sorted(LAYERS))
def test_destroy_returns_every_byte(ctx, route, pc):
    lib = abi.lib()
    entry, n, c, k, more, hw = LAYERS[route]
    rng = np.random.default_rng(7)
    if route == "linear":
        dims, K, in_shape, out_elems = (n, c), c, (M, c), M * n
    else:
        groups = more[2] if "grouped" in entry or "dilated" in entry else 1
        K = (c // groups) * k * k
        if route == "T":
            o = (hw - 1) * more[0] - 2 * more[1] + k + more[2]
            dims = (n, c, k) + more
        else:
            dil = more[3] if "dilated" in entry else 1
            o = (hw + 2 * more[1] - dil * (k - 1) - 1) // more[0] + 1
            dims = (n, c, k, k) + more
        in_shape, out_elems = (M, c, hw, hw), M * n * o * o
    qw = rng.integers(-127, 128, (n, K)).astype(np.int8)
    qb = rng.integers(-127, 128, n).astype(np.int8)
    sw = np.linspace(0.01, 0.03, n).astype(np.float32)
    x = ctx.put(rng.integers(0, 256, in_shape).astype(np.uint8))
    out = ctx.empty((out_elems,), np.uint8)
    ctx.sync()
    before = live(ctx)
    L = C.c_void_p()
    scale = sw.ctypes.data_as(C.c_void_p) if pc else C.c_float(0.02)
    abi.ck(getattr(lib, entry + ("_per_channel" if pc else ""))(ctx.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p),
                                                                *dims, scale, C.byref(L)))
    held = live(ctx)
    abi.ck(lib.i8ie_layer_set_output_qparams(L, C.c_float(0.5), C.c_uint8(7)))
    abi.ck(lib.i8ie_layer_forward(L, x.ptr, M, hw, hw, C.c_float(0.02), C.c_uint8(3), out.ptr, None))
    ctx.sync()
    abi.ck(lib.i8ie_layer_destroy(L))
    after = live(ctx)
    x.free(); out.free()
    print(route, "per_channel" if pc else "per_tensor", "bytes held by the handle:", held - before)
    assert held > before
    assert after == before
