"""Grouped / depthwise Conv2d without a GPU: the test helper against the oracle (a grouped convolution equals a dense
reference convolution whose weight is zero outside each group's block), the Python surface, the argument checks of the
C entry points (made before any device call) and the paper-AlexNet MAC count."""
import ctypes as C

import numpy as np
import pytest

import abi
import grouped_ref as gr
from support import i8ie  # noqa: F401


@pytest.mark.parametrize("case", [(6, 9, 3, 3, 1, 1, 7, 9), (8, 16, 8, 3, 2, 0, 9, 9), (5, 7, 1, 3, 1, 1, 6, 5)],
                         ids=["c6_kc9_g3", "depthwise_x2_s2", "groups1"])
def test_helper_equals_block_diagonal_dense_oracle(orc, case):
    c, kc, g, k, stride, pad, h, w = case
    rng = np.random.default_rng(c * 100 + kc)
    q = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
    qw = rng.integers(-128, 128, (kc, c // g, k, k), dtype=np.int8)
    qb = rng.integers(-128, 128, kc, dtype=np.int8)
    s_in, zp_in, s_w, s_out, zp_out = np.float32(0.03), 119, np.float32(0.004), np.float32(0.05), 40
    got, acc = gr.conv2d_grouped(q, qw, qb, g, stride, pad, s_in, zp_in, s_w, s_out, zp_out)
    want, want_acc = orc.conv2d(q, gr.block_diagonal(qw, g), qb, stride, pad, s_in, zp_in, s_w, s_out, zp_out, want_acc=True)
    assert np.array_equal(acc, want_acc)
    assert np.array_equal(got, want)
    # the offset vector: the reference's sequential fp32 sums over the [kc, Cg*kh*kw] matrix as it stands
    assert np.array_equal(orc.conv_offsets(qw.reshape(kc, -1), qb, s_in, zp_in),
                          orc.conv_offsets(gr.block_diagonal(qw, g).reshape(kc, -1), qb, s_in, zp_in))


def test_conv2d_groups_surface(i8ie):
    L = i8ie.Conv2d(4, 4, 3, groups=2)
    assert L.groups() == 2
    assert i8ie.Conv2d(4, 4, 3).groups() == 1
    assert i8ie.Linear(4, 4).groups() == 1
    with pytest.raises(RuntimeError):
        i8ie.Conv2d(4, 4, 3, groups=3)
    with pytest.raises(RuntimeError):
        i8ie.Conv2d(4, 6, 3, groups=4)
    with pytest.raises(RuntimeError):
        i8ie.Conv2d(4, 4, 3, groups=0)


def test_load_weight_shape_is_checked(i8ie):
    L = i8ie.Conv2d(4, 4, 3, groups=2)
    L.load_weight(np.zeros((4, 2, 3, 3), np.float32))
    with pytest.raises(RuntimeError):
        L.load_weight(np.zeros((4, 4, 3, 3), np.float32))
    with pytest.raises(RuntimeError):
        L.layer.load_quantized(np.zeros((4, 4, 3, 3), np.int8), np.zeros(4, np.int8), 0.5, 1.0, 0)


@pytest.mark.parametrize("groups,c,kc", [(0, 4, 4), (-2, 4, 4), (3, 4, 6), (3, 6, 4)])
def test_create_rejects_bad_groups_before_any_device_call(groups, c, kc):
    lib = gr.bind(abi.lib())
    qw = np.zeros((kc, max(c // max(groups, 1), 1) * 9), np.int8)
    qb = np.zeros(kc, np.int8)
    sw = np.ones(kc, np.float32)
    L = C.c_void_p()
    # (a null ctx: the argument check must come first and leave a message)
    rc = lib.i8ie_conv2d_create_grouped(None, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), kc, c, 3, 3, 1, 1,
                                        groups, C.c_float(0.5), C.byref(L))
    assert rc == -1 and b"groups" in lib.i8ie_last_error()
    rc = lib.i8ie_conv2d_create_grouped_per_channel(None, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), kc, c,
                                                    3, 3, 1, 1, groups, sw.ctypes.data_as(C.c_void_p), C.byref(L))
    assert rc == -1 and b"groups" in lib.i8ie_last_error()
    rc = lib.i8ie_conv2d_u8s8_grouped(None, None, 1, c, 8, 8, None, kc, 3, 3, 1, 1, groups, 0, None, C.c_float(1), C.c_float(1),
                                      C.c_float(1), 0, None, None)
    assert rc == -1 and b"groups" in lib.i8ie_last_error()
    rc = lib.i8ie_conv2d_f32_grouped(None, None, 1, c, 8, 8, None, None, kc, 3, 3, 1, 1, groups, None)
    assert rc == -1
    assert lib.i8ie_layer_groups(None, None) == -1 and b"null" in lib.i8ie_last_error()


def test_new_symbols_are_declared_and_exported():
    names = abi.declared_symbols()
    lib = abi.lib()
    for n in ["i8ie_conv2d_create_grouped", "i8ie_conv2d_create_grouped_per_channel", "i8ie_layer_groups",
              "i8ie_conv2d_u8s8_grouped", "i8ie_conv2d_f32_grouped"]:
        assert n in names and hasattr(lib, n), n
    assert lib.i8ie_version() == 1


def test_alexnet_paper_workload():
    from int8inferenceengine_amd import workloads as wl

    dense = wl.macs_per_image("alexnet")
    assert dense == wl.ALEXNET_MACS_PER_IMAGE
    conv2, conv4, conv5 = 27 * 27 * 256 * 96 * 25, 13 * 13 * 384 * 384 * 9, 13 * 13 * 256 * 384 * 9
    assert wl.macs_per_image("alexnet_paper") == dense - (conv2 + conv4 + conv5) // 2
    sd = wl.synthetic_state_dict("alexnet_paper")
    assert sd["conv2.weight"].shape == (256, 48, 5, 5) and sd["conv4.weight"].shape == (384, 192, 3, 3)
    assert sd["conv5.weight"].shape == (256, 192, 3, 3) and sd["conv3.weight"].shape == (384, 256, 3, 3)
    assert wl.layer_names("alexnet_paper") == wl.layer_names("alexnet")
    net = wl.build("alexnet_paper")
    assert [getattr(net, a).groups() for a in ("conv1", "conv2", "conv3", "conv4", "conv5")] == [1, 2, 1, 2, 2]
    net.load(sd)  # (the grouped weight shapes are accepted)
