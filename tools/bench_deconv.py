"""ConvTranspose2d against the only workaround there was: a dense Conv2d over a zero-inserted input.

    python tools/bench_deconv.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r12_bench_deconv.json]

Per shape and batch size: the same u8 input once as it is (NHWC, no border) through a transposed layer handle, and once
zero-inserted on the host -- stride - 1 positions between neighbouring pixels and k - 1 - pad (+ output_pad) around them, all
holding zp_in -- through the existing dense Conv2d handle (stride 1, padding 0) with the equivalent kernel W~.  The inflated
input is built before the timing, so the workaround is not charged for writing it.  Output bytes are asserted identical.
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop) summed over the kernels of a forward:
`warmup` forwards unprofiled, then `rounds` rounds of `iters` profiled forwards; a round's figure is its mean per forward and
the reported one the median over rounds.  Then unet_cifar's step through the Python surface, with the share its three
up-convs take of the kernel time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, c, kc, k, stride, pad, output_pad, h, w)
SHAPES = [
    ("unet_up3_512_256_4x4", 512, 256, 2, 2, 0, 0, 4, 4),
    ("unet_up2_256_128_8x8", 256, 128, 2, 2, 0, 0, 8, 8),
    ("unet_up1_128_64_16x16", 128, 64, 2, 2, 0, 0, 16, 16),
    ("k4s2p1_64_64_16x16", 64, 64, 4, 2, 1, 0, 16, 16),
    ("k3s2p1op1_128_64_16x16", 128, 64, 3, 2, 1, 1, 16, 16),
]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F = C.c_void_p, C.c_int, C.c_float
    lib.i8ie_conv2d_create.argtypes = [P, P, P, I, I, I, I, I, I, F, P]
    lib.i8ie_conv_transpose2d_create.argtypes = [P, P, P, I, I, I, I, I, I, F, P]
    lib.i8ie_layer_forward_fused.argtypes = [P, P, I, I, I, I, I, F, C.c_uint8, I, P, I, I, P]
    lib.i8ie_layer_set_output_qparams.argtypes = [P, F, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_deconv.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def put(a):
        a = np.ascontiguousarray(a)
        d = P()
        ck(lib.i8ie_malloc(ctx, a.nbytes, C.byref(d)))
        ck(lib.i8ie_memcpy_h2d(ctx, d, a.ctypes.data_as(P), a.nbytes))
        return d

    s_in, zp_in, s_w, zp_out = 0.03, 121, 2e-3, 37
    results = []
    for name, c, kc, k, s, p, op, h, w in SHAPES:
        rng = np.random.default_rng(sum(map(ord, name)))
        wt = rng.integers(-127, 128, (c, kc, k, k), dtype=np.int8)  # torch's layout
        qw = np.ascontiguousarray(wt.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])  # the equivalent kernel W~ [kc, c, k, k]
        qb = rng.integers(-127, 128, kc, dtype=np.int8)
        s_out = float(np.float32(s_in * s_w * np.sqrt(c * k * k / float(s * s)) * 40.0 / 64.0))
        oh, ow = (h - 1) * s - 2 * p + k + op, (w - 1) * s - 2 * p + k + op
        lo = k - 1 - p
        ht, wdt = (h - 1) * s + 1 + 2 * lo + op, (w - 1) * s + 1 + 2 * lo + op
        assert ht - k + 1 == oh and wdt - k + 1 == ow
        layers = {}
        L = P()
        ck(lib.i8ie_conv2d_create(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, 1, 0, s_w, C.byref(L)))
        layers["dense_over_zero_inserted"] = L
        L = P()
        ck(lib.i8ie_conv_transpose2d_create(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, s, p, op, s_w, C.byref(L)))
        layers["transposed"] = L
        for L in layers.values():
            ck(lib.i8ie_layer_set_output_qparams(L, s_out, zp_out))
        for m in BATCHES:
            x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            xt = np.full((m, ht, wdt, c), zp_in, np.uint8)
            xt[:, lo:lo + (h - 1) * s + 1:s, lo:lo + (w - 1) * s + 1:s, :] = x
            feeds = {"transposed": (put(x), h, w), "dense_over_zero_inserted": (put(xt), ht, wdt)}
            row = {"shape": name, "images": m, "c": c, "kc": kc, "kernel": k, "stride": s, "pad": p, "output_pad": op, "h": h, "w": w,
                   "oh": oh, "ow": ow, "macs_transposed": m * h * w * c * kc * k * k, "macs_dense": m * oh * ow * kc * c * k * k,
                   "inflated_input_bytes": int(xt.nbytes), "input_bytes": int(x.nbytes)}
            outs = {}
            nbytes = m * oh * ow * kc
            for tag, L in layers.items():
                dx, hh, ww = feeds[tag]
                do = P()
                ck(lib.i8ie_malloc(ctx, nbytes, C.byref(do)))

                def fwd():
                    ck(lib.i8ie_layer_forward_fused(L, dx, 1, 0, m, hh, ww, s_in, zp_in, 1, do, 1, 0, None))

                for _ in range(args.warmup):
                    fwd()
                ck(lib.i8ie_sync(ctx))
                per_round, names = [], {}
                for _ in range(args.rounds):
                    ck(lib.i8ie_profile_start(ctx, 0))
                    for _ in range(args.iters):
                        fwd()
                    ents, cnt = (Entry * 64)(), C.c_int(0)
                    ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
                    per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
                    names = {ents[i].name.decode(): int(ents[i].launches) // args.iters for i in range(cnt.value)}
                host = np.empty(nbytes, np.uint8)
                ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), do, nbytes))
                outs[tag] = host
                ck(lib.i8ie_free(ctx, do))
                ck(lib.i8ie_free(ctx, dx))
                row[tag] = {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_forward": names}
            assert np.array_equal(outs["transposed"], outs["dense_over_zero_inserted"]), "%s @ %d: output bytes differ" % (name, m)
            row["identical_bytes"] = True
            row["transposed_over_dense"] = row["transposed"]["ms"] / row["dense_over_zero_inserted"]["ms"]
            results.append(row)
            print(json.dumps(row), flush=True)
        for L in layers.values():
            lib.i8ie_layer_destroy(L)
    lib.i8ie_ctx_destroy(ctx)
    return results


def network(args):
    sys.path.insert(0, ROOT)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    name = "unet_cifar"
    net = wl.calibrated(name, calib_batch=wl.synthetic_input(name, 16, seed=99))
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(wl.synthetic_input(name, m)).prefetch()
        for _ in range(args.warmup):
            net(x).numpy()
        cx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.net_steps):
            y = net(x)
        y.numpy()
        wall = (time.perf_counter() - t0) / args.net_steps * 1e3
        cx.profile_start()
        for _ in range(args.net_steps):
            net(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        up = sum(v[1] for k, v in prof.items() if k.startswith("deconv"))
        by = {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
        rows.append({"network": name, "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "images_per_s_wall": m / (wall * 1e-3), "upconv_ms_per_step": up / args.net_steps,
                     "upconv_share_of_kernel_time": up / total,
                     "upconv_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("deconv")) / args.net_steps,
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
    out = {"tool": "bench_deconv", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per forward; median over rounds of the per-round mean",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
