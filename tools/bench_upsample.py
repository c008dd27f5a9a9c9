"""Quantized upsampling against the cheapest pass over the same output: i8ie_relu_u8 on the result's byte count.

    python tools/bench_upsample.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r13_bench_upsample.json]

Per shape (all at x2) and batch size: i8ie_upsample2d_u8_nhwc, nearest and bilinear, once into a flat plain result and once
into a bordered (1) re-biased one, as a 3x3 pad-1 conv asks for it; and i8ie_relu_u8 over as many bytes as the result has, on
the same build.  Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` calls
unprofiled, then `rounds` rounds of `iters` profiled calls; a round's figure is its mean per call and the reported one the
median over rounds.  GB/s counts the input's and the result's bytes once each.  The aim: an upsample takes no longer than
relu_u8 over the result's byte count (it moves 1 + 1 / f^2 bytes per result byte against relu's 2); every row records the
ratio and whether the aim is met.  The flat results' first images are checked against the integer definition before the
timing.  Then unet_bilinear_cifar's step against unet_cifar's through the Python surface, the two alternating, with the
share the upsamples (and the up-convs) take of the kernel time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, c, h, w): unet_cifar's three up-conv inputs as unet_bilinear_cifar upsamples them, and a ResNet-sized map
SHAPES = [("unet_up1_in_64x16x16", 64, 16, 16), ("unet_up2_in_128x8x8", 128, 8, 8), ("unet_up3_in_256x4x4", 256, 4, 4),
          ("64x56x56", 64, 56, 56)]
BATCHES = [1000, 125]
FACTOR = 2
MODES = {"nearest": 0, "bilinear": 1}


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def definition(x, f, mode):
    """the integer definition of include/i8ie_hip.h on an NHWC tensor (numpy, int64)"""
    def taps(L):
        o = np.arange(L * f)
        i, t = o // f, 2 * (o % f) + 1 - f
        i0 = np.where(t >= 0, i, i - 1)
        w1 = np.where(i0 < 0, 0, np.where(t >= 0, t, 2 * f + t))
        i0 = np.maximum(i0, 0)
        return i0, np.minimum(i0 + 1, L - 1), 2 * f - w1, w1

    if mode == "nearest":
        return x[:, np.arange(x.shape[1] * f) // f][:, :, np.arange(x.shape[2] * f) // f]
    q = x.astype(np.int64)
    y0, y1, wy0, wy1 = taps(x.shape[1])
    x0, x1, wx0, wx1 = taps(x.shape[2])
    wy0, wy1, wx0, wx1 = wy0[None, :, None, None], wy1[None, :, None, None], wx0[None, None, :, None], wx1[None, None, :, None]
    r0, r1 = q[:, y0], q[:, y1]
    S = wx0 * (wy0 * r0[:, :, x0] + wy1 * r1[:, :, x0]) + wx1 * (wy0 * r0[:, :, x1] + wy1 * r1[:, :, x1])
    D = 4 * f * f
    return ((S + D // 2) // D).astype(np.uint8)


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I = C.c_void_p, C.c_int
    lib.i8ie_upsample2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [C.c_uint8]
    lib.i8ie_relu_u8.argtypes = [P, P, P, C.c_int64, C.c_uint8]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_upsample.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def alloc(nbytes):
        d = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(d)))
        return d

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
        return statistics.median(per_round), per_round, names

    zp, f = 117, FACTOR
    results = []
    for name, c, h, w in SHAPES:
        rng = np.random.default_rng(sum(map(ord, name)))
        for m in BATCHES:
            x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            in_bytes, out_bytes = x.nbytes, x.nbytes * f * f
            dx = alloc(in_bytes)
            ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), in_bytes))
            d_flat = alloc(out_bytes)
            bordered_bytes = m * (h * f + 2) * (w * f + 2) * c
            d_bord = alloc(bordered_bytes)
            ck(lib.i8ie_fill_border_u8(ctx, d_bord, m, c, h * f, w * f, 1, zp ^ 0x80))
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "factor": f, "input_bytes": in_bytes, "output_bytes": out_bytes}
            ms, rounds, names = timed(lambda: ck(lib.i8ie_relu_u8(ctx, d_flat, d_flat, out_bytes, zp)))
            row["relu_u8_over_output_bytes"] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names, "GBps": 2.0 * out_bytes / ms / 1e6}
            for mode, code in MODES.items():
                ck(lib.i8ie_upsample2d_u8_nhwc(ctx, dx, 0, 0, d_flat, 0, 0, m, c, h, w, f, f, code, 0, zp))
                k = min(m, 8)  # (the first images: the definition in int64 on the host is the slow part)
                host = np.empty((k, h * f, w * f, c), np.uint8)
                ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), d_flat, host.nbytes))
                assert np.array_equal(host, definition(x[:k], f, mode)), "%s @ %d %s: bytes differ from the definition" % (name, m, mode)
                for tag, dst, ob, s8 in (("flat", d_flat, 0, 0), ("bordered_rebiased", d_bord, 1, 1)):
                    ms, rounds, names = timed(lambda: ck(lib.i8ie_upsample2d_u8_nhwc(ctx, dx, 0, 0, dst, ob, s8, m, c, h, w, f, f, code, 1, zp)))
                    ratio = ms / row["relu_u8_over_output_bytes"]["ms"]
                    row[mode + "_" + tag] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names,
                                             "GBps": (in_bytes + out_bytes) / ms / 1e6, "over_relu_u8": ratio,
                                             "aim_no_slower_than_relu_u8": "met" if ratio <= 1.0 else "missed"}
            row["identical_to_definition"] = True
            for d in (dx, d_flat, d_bord):
                ck(lib.i8ie_free(ctx, d))
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

    names = ["unet_bilinear_cifar", "unet_cifar"]
    nets = {n: wl.calibrated(n, calib_batch=wl.synthetic_input(n, 16, seed=99)) for n in names}
    rows = []
    for m in BATCHES:
        xs = {n: i8ie.tensor(wl.synthetic_input(n, m)).prefetch() for n in names}
        for n in names:
            for _ in range(args.warmup):
                nets[n](xs[n]).numpy()
        walls = {n: [] for n in names}
        for _ in range(args.rounds):  # the two networks alternate
            for n in names:
                cx.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.net_steps):
                    y = nets[n](xs[n])
                y.numpy()
                walls[n].append((time.perf_counter() - t0) / args.net_steps * 1e3)
        for n in names:
            cx.profile_start()
            for _ in range(args.net_steps):
                nets[n](xs[n]).numpy()
            prof = cx.profile_stop()
            total = sum(v[1] for v in prof.values())
            up = sum(v[1] for k, v in prof.items() if k.startswith(("upsample", "deconv")))
            by = {}
            for k, v in prof.items():
                by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
            wall = statistics.median(walls[n])
            rows.append({"network": n, "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls[n],
                         "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                         "upsample_or_upconv_ms_per_step": up / args.net_steps, "upsample_or_upconv_share_of_kernel_time": up / total,
                         "upsample_or_upconv_launches_per_step":
                             sum(v[0] for k, v in prof.items() if k.startswith(("upsample", "deconv"))) / args.net_steps,
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
    out = {"tool": "bench_upsample", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean",
           "aim": "upsample ms <= relu_u8 ms over the result's byte count", "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
