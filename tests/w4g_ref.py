"""4-bit weights with integer group scales along K, restated for the tests (include/i8ie_hip.h, "4-bit weights for Linear with
group-wise scales"): the quantiser in float32 and the layer as the per-channel Linear on W_eff = m * q.  numpy only."""
import numpy as np

from pc_pipeline import down_scale_pc

f32 = np.float32


def groups(k, gs):
    return -(-k // gs)


def quantize_w4g(w, b, gs):
    """(q int8 [n, k], m uint8 [n, G], q_b int8 [n], s_w float32 [n]); every operation rounds once to float32"""
    w, b = np.asarray(w, f32), np.asarray(b, f32)
    n, k = w.shape
    a = np.maximum(np.abs(w).max(axis=1), np.abs(b) * f32(7) / f32(127)).astype(f32)
    S = np.where(a == 0, f32(1), a / f32(7)).astype(f32)
    q, m = np.zeros((n, k), np.int8), np.ones((n, groups(k, gs)), np.uint8)
    for g in range(groups(k, gs)):
        cols = slice(g * gs, min(k, (g + 1) * gs))
        top = np.abs(w[:, cols]).max(axis=1).astype(f32)
        mf = np.where(a == 0, f32(1), np.ceil((f32(32) * top) / np.where(a == 0, f32(1), a))).astype(f32)
        mf = np.clip(mf, 1, 32).astype(f32)
        m[:, g] = mf.astype(np.uint8)
        step = ((S * mf).astype(f32) / f32(32)).astype(f32)
        q[:, cols] = np.clip(np.rint(w[:, cols] / step[:, None]), -7, 7).astype(np.int8)
    qb = np.clip(np.rint(b / S), -127, 127).astype(np.int8)
    return q, m, qb, (S / f32(32)).astype(f32)


def w_eff(q, m, gs):
    """int64 [n, k]: m[j, k // gs] * q[j, k]"""
    k = q.shape[1]
    return np.repeat(m.astype(np.int64), gs, axis=1)[:, :k] * q.astype(np.int64)


def linear_w4g(q_in, q, m, qb, gs, s_in, zp_in, s_w, s_out, zp_out):
    """(out u8 [rows, n], acc int32 before the bias step)"""
    w = w_eff(q, m, gs)
    t = np.zeros(w.shape[0], f32)
    for col in (int(zp_in) * w).T:  # the reference's sequential fp32 sum over ascending k
        t = t + col.astype(f32)
    oc = (-t).astype(np.int32)
    acc = q_in.astype(np.int64) @ w.T + oc
    assert np.abs(acc).max() < 2 ** 31
    acc = acc.astype(np.int32)
    biased = (acc.astype(f32) + (f32(32) * qb.astype(f32)) / f32(s_in)).astype(np.int32)
    return down_scale_pc(biased, s_in, s_w, s_out, zp_out), acc
