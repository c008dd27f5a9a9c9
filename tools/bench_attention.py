"""The quantized batched matmul and softmax against the parent's yardsticks.

    python tools/bench_attention.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r15_bench_attention.json]

Matmul: the two products of the "cifar" non-local block per image ([64 x 128] . [128 x 64] and [128 x 64] . [64 x 64]) and a
larger pair at t = 256, d = 64, with the operand and result strides the network presents them with (NHWC projections read as
they lie), at 1000 and 125 images.  The yardstick is the Linear route (a layer handle, i8ie_linear_create / i8ie_layer_forward) timed in the same session on ONE GEMM
of the same m n k total (rows = images x m): its weights are shared by every image, so it moves fewer bytes, and its time is
a lower bound.  Softmax: i8ie_softmax_u8 over the scores against i8ie_relu_u8 over the same byte count.  Timing is the
library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds` rounds of
`iters` profiled calls; a round's figure is its mean per call and the reported one the median over rounds.  The aim is parity
(ratio <= 1); every row records the ratio and MET or MISSED.  The first images of every result are checked against the
definition (numpy) before the timing.  Then nonlocal_resnet_cifar's step through the Python surface with the share its three
attention launches take of the kernel time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [1000, 125]
PAIRS = [("cifar_t64_d128", 64, 128), ("t256_d64", 256, 64)]   # (name, t pixels, d projection width)
f32 = np.float32


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


class Mat(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("batch_stride", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("s8", C.c_int)]


class BmmArgs(C.Structure):
    _fields_ = [("b", C.c_int), ("m", C.c_int), ("n", C.c_int), ("k", C.c_int), ("a", Mat), ("bm", Mat), ("out", Mat),
                ("out_pix_axis", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("out_border", C.c_int),
                ("s_a", C.c_float), ("s_b", C.c_float), ("s_out", C.c_float), ("zp_a", C.c_uint8), ("zp_b", C.c_uint8),
                ("zp_out", C.c_uint8), ("relu", C.c_int), ("acc_dbg_dev", C.c_void_p)]


def down_scale(acc, s_a, s_b, s_out, zp):
    """src/quantize_utils.cc:27-36 in numpy float32, one rounding per operation"""
    v = (acc.astype(f32) * f32(s_a)) * f32(s_b) / f32(s_out) + f32(zp)
    return np.where(v >= 255, 255, np.where(v < 0, 0, np.trunc(v))).astype(np.uint8)


def softmax_u8(x, s):
    E = np.floor(65536.0 * np.exp(-np.float64(f32(s)) * np.arange(256.0)) + 0.5).astype(np.uint64)
    e = E[x.max(axis=-1, keepdims=True).astype(np.int64) - x.astype(np.int64)]
    S = e.sum(axis=-1, keepdims=True)
    return np.minimum((e * np.uint64(256) + S // np.uint64(2)) // S, np.uint64(255)).astype(np.uint8)


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I = C.c_void_p, C.c_int
    lib.i8ie_bmm_u8.argtypes = [P, C.POINTER(BmmArgs)]
    lib.i8ie_softmax_u8.argtypes = [P, P, P, C.c_int64, I, C.c_float]
    lib.i8ie_relu_u8.argtypes = [P, P, P, C.c_int64, C.c_uint8]
    lib.i8ie_linear_create.argtypes = [P, P, P, I, I, C.c_float, P]
    lib.i8ie_layer_set_output_qparams.argtypes = [P, C.c_float, C.c_uint8]
    lib.i8ie_layer_forward.argtypes = [P, P, I, I, I, C.c_float, C.c_uint8, P, P]
    lib.i8ie_layer_destroy.argtypes = [P]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_attention.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def alloc(nbytes):
        d = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(d)))
        return d

    def put(arr):
        d = alloc(arr.nbytes)
        ck(lib.i8ie_memcpy_h2d(ctx, d, arr.ctypes.data_as(P), arr.nbytes))
        return d

    def get(d, shape, dtype=np.uint8):
        host = np.empty(shape, dtype)
        ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), d, host.nbytes))
        return host

    def timed(call):
        for _ in range(args.warmup):
            call()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], {}
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                call()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
            names = {ents[i].name.decode().split("|")[0]: int(ents[i].launches) // args.iters for i in range(cnt.value)}
        return {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_call": names}

    def linear_yardstick(rows, k, n, rng):
        """one GEMM [rows, k] x [n, k]^T through a Linear layer handle (weights packed once, at creation)"""
        x = rng.integers(0, 256, (rows, k), dtype=np.uint8)
        w = rng.integers(-127, 128, (n, k), dtype=np.int8)
        qb = np.zeros(n, np.int8)
        L = P()
        ck(lib.i8ie_linear_create(ctx, w.ctypes.data_as(P), qb.ctypes.data_as(P), n, k, 0.01, C.byref(L)))
        ck(lib.i8ie_layer_set_output_qparams(L, 0.6, 128))
        dx, out = put(x), alloc(rows * n)
        r = timed(lambda: ck(lib.i8ie_layer_forward(L, dx, rows, 0, 0, 0.05, 120, out, None)))
        ck(lib.i8ie_layer_destroy(L))
        for d in (dx, out):
            ck(lib.i8ie_free(ctx, d))
        return r

    results = []
    za, zb, s_a, s_b = 127, 131, f32(0.06), f32(0.06)
    for name, t, d in PAIRS:
        rng = np.random.default_rng(sum(map(ord, name)))
        for m in BATCHES:
            theta, phi, g = (rng.integers(0, 256, (m, t, d), dtype=np.uint8) for _ in range(3))   # NHWC [n, t, d]
            dth, dph, dg = put(theta), put(phi), put(g)
            dsc, dpr, dy = alloc(m * t * t), alloc(m * t * t), alloc(m * t * d)
            s1 = f32(0.06 * 0.06 * 74 * 74 * np.sqrt(d) * 6 / 255)   # +-3 sigma of a random product sum over the byte range
            mm1 = BmmArgs(b=m, m=t, n=t, k=d, a=Mat(dth.value, t * d, d, 1, 0), bm=Mat(dph.value, t * d, 1, d, 0),
                          out=Mat(dsc.value, t * t, t, 1, 0), s_a=s_a, s_b=s_b, s_out=s1, zp_a=za, zp_b=zb, zp_out=128)
            mm2 = BmmArgs(b=m, m=d, n=t, k=t, a=Mat(dg.value, t * d, 1, d, 0), bm=Mat(dpr.value, t * t, 1, t, 0),
                          out=Mat(dy.value, t * d, 1, d, 0), s_a=s_a, s_b=f32(1 / 256), s_out=f32(0.03), zp_a=za, zp_b=0, zp_out=128)
            ck(lib.i8ie_bmm_u8(ctx, C.byref(mm1)))
            ck(lib.i8ie_softmax_u8(ctx, dsc, dpr, m * t, t, s1))
            ck(lib.i8ie_bmm_u8(ctx, C.byref(mm2)))
            k = 2   # the definition on the first images
            sc, pr, y = get(dsc, (m, t, t))[:k], get(dpr, (m, t, t))[:k], get(dy, (m, t, d))[:k]
            acc1 = np.einsum("bik,bjk->bij", theta[:k].astype(np.int64) - za, phi[:k].astype(np.int64) - zb)
            assert np.array_equal(sc, down_scale(acc1, s_a, s_b, s1, 128)), "%s @ %d: scores differ from the definition" % (name, m)
            assert np.array_equal(pr, softmax_u8(sc, s1)), "%s @ %d: softmax differs from the definition" % (name, m)
            acc2 = np.einsum("bjc,bij->bic", g[:k].astype(np.int64) - za, pr.astype(np.int64))
            assert np.array_equal(y, down_scale(acc2, s_a, 1 / 256, 0.03, 128)), "%s @ %d: y differs from the definition" % (name, m)
            row = {"pair": name, "images": m, "t": t, "d": d, "identical_to_definition": True,
                   "scores_saturated_share": float(((sc == 0) | (sc == 255)).mean())}
            for tag, desc, (mm, nn, kk) in (("mm1_scores", mm1, (t, t, d)), ("mm2_apply", mm2, (d, t, t))):
                r = timed(lambda: ck(lib.i8ie_bmm_u8(ctx, C.byref(desc))))
                lin = linear_yardstick(m * mm, kk, nn, rng)
                r.update({"m": mm, "n": nn, "k": kk, "TOPS": 2.0 * m * mm * nn * kk / r["ms"] / 1e9, "linear_same_mnk": lin,
                          "over_linear": r["ms"] / lin["ms"], "aim_parity_with_linear": "MET" if r["ms"] <= lin["ms"] else "MISSED"})
                row[tag] = r
            sm = timed(lambda: ck(lib.i8ie_softmax_u8(ctx, dsc, dpr, m * t, t, s1)))
            relu = timed(lambda: ck(lib.i8ie_relu_u8(ctx, dsc, dpr, m * t * t, 128)))
            sm.update({"bytes": m * t * t, "GBps": 2.0 * m * t * t / sm["ms"] / 1e6, "relu_u8_same_bytes": relu,
                       "over_relu_u8": sm["ms"] / relu["ms"], "aim_parity_with_relu_u8": "MET" if sm["ms"] <= relu["ms"] else "MISSED"})
            row["softmax"] = sm
            for dev in (dth, dph, dg, dsc, dpr, dy):
                ck(lib.i8ie_free(ctx, dev))
            results.append(row)
            print(json.dumps(row), flush=True)
    lib.i8ie_ctx_destroy(ctx)
    return results


def network(args):
    sys.path.insert(0, ROOT)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    name = "nonlocal_resnet_cifar"
    net = wl.calibrated(name, calib_batch=wl.synthetic_input(name, 16, seed=99))
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(wl.synthetic_input(name, m)).prefetch()
        for _ in range(args.warmup):
            net(x).numpy()
        walls = []
        for _ in range(args.rounds):
            cx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.net_steps):
                y = net(x)
            y.numpy()
            walls.append((time.perf_counter() - t0) / args.net_steps * 1e3)
        cx.profile_start()
        for _ in range(args.net_steps):
            net(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        att = sum(v[1] for k, v in prof.items() if k.startswith(("bmm_", "softmax_")))
        by = {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
        wall = statistics.median(walls)
        rows.append({"network": "nonlocal cifar", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                     "attention_ms_per_step": att / args.net_steps, "attention_share_of_kernel_time": att / total,
                     "attention_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith(("bmm_", "softmax_"))) / args.net_steps,
                     "kernel_ms_per_step_by_name": by})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=20)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_attention", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean",
           "aim": "bmm ms <= Linear ms on one GEMM of the same m n k total (a lower bound: shared weights); softmax ms <= relu_u8 ms over the same bytes",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
