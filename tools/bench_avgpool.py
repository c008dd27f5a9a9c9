"""Quantized average pooling against the kernels the library already had, on the same buffers in the same run.

    python tools/bench_avgpool.py [--iters 20] [--rounds 5] [--warmup 5] [--out profiles/r08_bench_avgpool.json]

At 1000 and 125 images, NHWC, border-free:
  windowed   avg_pool2d 2x2/2 and 3x3/2 on [N, 64, 56, 56] and [N, 256, 13, 13], beside i8ie_maxpool2d_u8_nhwc with the same
             window on the same input and output buffers.  Bytes: the whole input once plus the output once.
  global     the global pool on [N, 512, 4, 4] and [N, 512, 7, 7], beside relu_u8 over the same input bytes (1 read + 1 write
             per byte: the streaming yardstick; the pool reads them once and writes 1 / (h w) of them).
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then
`rounds` rounds of `iters` profiled launches; a round's figure is its mean per launch, the reported one the median over
rounds.  GB/s = algorithmic HBM bytes / that time.  The target of each pool is its comparison kernel's byte rate.

Every measured shape runs in a child process of its own under a time limit, and the first failure stops the run: nothing
more is started on a device after a fault or a hang.  Goes through the C-ABI by ctypes only."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WINDOWED = [("c64_56x56", 64, 56, 56), ("c256_13x13", 256, 13, 13)]
GLOBAL = [("c512_4x4", 512, 4, 4), ("c512_7x7", 512, 7, 7)]
BATCHES = [1000, 125]
STEP_TIMEOUT_S = 120


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def run_case(args, kind, name, c, h, w, m):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B, L = C.c_void_p, C.c_int, C.c_uint8, C.c_int64
    lib.i8ie_avgpool2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [B]
    lib.i8ie_maxpool2d_u8_nhwc.argtypes = [P, P, I, P, I] + [I] * 6
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_avgpool.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], set()
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                fn()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            assert sum(int(ents[i].launches) for i in range(cnt.value)) == args.iters
            names |= {ents[i].name.decode().split("|")[0] for i in range(cnt.value)}
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
        return statistics.median(per_round), per_round, sorted(names)

    rng = np.random.default_rng(m + c + h)
    x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
    n_in = x.size
    dx, do = P(), P()
    ck(lib.i8ie_malloc(ctx, n_in, C.byref(dx)))
    ck(lib.i8ie_malloc(ctx, n_in, C.byref(do)))  # (large enough for every leg)
    ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), n_in))
    row = {"kind": kind, "shape": name, "images": m, "c": c, "h": h, "w": w, "input_bytes": n_in}

    def leg(tag, nbytes, fn):
        ms, per_round, names = timed(fn)
        row[tag] = {"ms": ms, "ms_per_round": per_round, "hbm_bytes": nbytes, "gb_per_s": nbytes / (ms * 1e-3) / 1e9, "kernels": names}

    if kind == "windowed":
        for k, s in ((2, 2), (3, 2)):
            n_out = m * ((h - k) // s + 1) * ((w - k) // s + 1) * c
            leg("avgpool_%dx%d_s%d" % (k, k, s), n_in + n_out,
                lambda: ck(lib.i8ie_avgpool2d_u8_nhwc(ctx, dx, 0, 0, do, 0, 0, m, c, h, w, k, k, s, 0, 0)))
            leg("maxpool_%dx%d_s%d" % (k, k, s), n_in + n_out, lambda: ck(lib.i8ie_maxpool2d_u8_nhwc(ctx, dx, 0, do, 0, m, c, h, w, k, s)))
            row["avg_over_max_byte_rate_%dx%d_s%d" % (k, k, s)] = (row["avgpool_%dx%d_s%d" % (k, k, s)]["gb_per_s"]
                                                                   / row["maxpool_%dx%d_s%d" % (k, k, s)]["gb_per_s"])
    else:
        leg("global_avgpool", n_in + m * c, lambda: ck(lib.i8ie_avgpool2d_u8_nhwc(ctx, dx, 0, 0, do, 0, 0, m, c, h, w, h, w, 1, 0, 0)))
        leg("relu_u8", 2 * n_in, lambda: ck(lib.i8ie_relu_u8(ctx, dx, do, n_in, 97)))
        row["gap_over_relu_byte_rate"] = row["global_avgpool"]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
    for d in (dx, do):
        ck(lib.i8ie_free(ctx, d))
    lib.i8ie_ctx_destroy(ctx)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: kind,name,c,h,w,images -- one shape, in this process")
    args = ap.parse_args()

    if args.case:
        kind, name, c, h, w, m = args.case.split(",")
        run_case(args, kind, name, int(c), int(h), int(w), int(m))
        return

    results = []
    for kind, shapes in (("windowed", WINDOWED), ("global", GLOBAL)):
        for name, c, h, w in shapes:
            for m in BATCHES:
                cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--rounds", str(args.rounds), "--warmup",
                       str(args.warmup), "--lib", args.lib, "--case", "%s,%s,%d,%d,%d,%d" % (kind, name, c, h, w, m)]
                try:
                    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
                except subprocess.TimeoutExpired:
                    sys.exit("bench_avgpool.py: %s %s at %d images ran past %d s; stopping" % (kind, name, m, STEP_TIMEOUT_S))
                if done.returncode != 0:
                    sys.exit("bench_avgpool.py: %s %s at %d images ended with status %d; stopping" % (kind, name, m, done.returncode))
                line = done.stdout.strip().splitlines()[-1]
                results.append(json.loads(line))
                print(line, flush=True)

    out = {"tool": "bench_avgpool", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*); median over rounds of the per-round mean per launch",
           "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
