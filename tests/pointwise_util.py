"""Guarded, bordered NHWC buffers for the tests of the two-operand pointwise ops (test_gpu_add.py, test_gpu_mul.py,
test_gpu_pointwise_arms.py).  A helper module, not a conftest."""
import numpy as np

GUARD = 64


def phys(x_nhwc, border, fill, s8, skew=0):
    """[n, h, w, c] u8 -> guarded flat buffer holding [n, h+2b, w+2b, c] with `fill` in the border (re-biased if s8).  The
    buffer proper starts GUARD + skew bytes into the flat array: an allocation is 64-byte aligned and so is GUARD, so `skew`
    is the buffer's misalignment."""
    n, h, w, c = x_nhwc.shape
    p = np.full((n, h + 2 * border, w + 2 * border, c), fill, np.uint8)
    p[:, border:border + h, border:border + w, :] = x_nhwc
    if s8:
        p = p ^ np.uint8(0x80)
    return np.concatenate([np.full(GUARD + skew, 0x5A, np.uint8), p.ravel(), np.full(GUARD, 0x5A, np.uint8)]), p.shape


def interior(go, oshape, border, zp_out, s8, skew=0):
    """the flat result buffer as the call left it -> its interior [n, h, w, c] (the re-bias undone), after checking that the
    guard bytes and every border byte are as phys() made them"""
    assert (go[:GUARD + skew] == 0x5A).all() and (go[-GUARD:] == 0x5A).all(), "guard bytes around the result"
    out = go[GUARD + skew:-GUARD].reshape(oshape)
    if s8:
        out = out ^ np.uint8(0x80)
    n, hp, wp, c = oshape
    h, w = hp - 2 * border, wp - 2 * border
    ring = out.copy()
    ring[:, border:border + h, border:border + w, :] = zp_out
    assert (ring == zp_out).all(), "every border byte of the result holds zp_out"
    return out[:, border:border + h, border:border + w, :]
