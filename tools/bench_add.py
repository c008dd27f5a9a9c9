"""The quantized residual Add against the streaming kernels the library already had.

    python tools/bench_add.py [--iters 20] [--rounds 5] [--warmup 5] [--out profiles/r07_bench_add.json]

Per activation shape ([N, 256, 13, 13] and [N, 64, 56, 56], NHWC) and batch size (1000, 125):
  add_relu            relu(add(a, b)), all three buffers border-free: the flat form (3 bytes of HBM traffic per element)
  add_relu_block      the same as a basic block runs it: a bordered by 1 and re-biased (the skip tensor as the block's first
                      conv wanted it), b border-free, the result bordered by 1 and re-biased for the next conv
  add_relu_replay     the flat form with s_a = s_b = s_out, where every value sits on a rounding boundary and the kernel
                      replays the exact sequence for all of them (its slowest case)
  relu_u8, rebias_u8  the existing kernels over the same number of elements (1 read + 1 write: 2 bytes per element)
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then
`rounds` rounds of `iters` profiled launches; a round's figure is its mean per launch, the reported one the median over
rounds.  GB/s = algorithmic HBM bytes / that time.  The yardstick of the add is relu_u8's byte rate in the same run.
Goes through the C-ABI by ctypes only."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c256_13x13", 256, 13, 13), ("c64_56x56", 64, 56, 56)]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F, B, L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64
    lib.i8ie_add_u8_nhwc.argtypes = [P, P, I, I, P, I, I, P, I, I, I, I, I, I, F, B, F, B, F, B, I]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_rebias_u8.argtypes = [P, P, P, L]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_add.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def put(a):
        a = np.ascontiguousarray(a)
        d = P()
        ck(lib.i8ie_malloc(ctx, a.nbytes, C.byref(d)))
        ck(lib.i8ie_memcpy_h2d(ctx, d, a.ctypes.data_as(P), a.nbytes))
        return d

    def empty(nbytes):
        d = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(d)))
        return d

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ck(lib.i8ie_sync(ctx))
        per_round = []
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                fn()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            assert sum(int(ents[i].launches) for i in range(cnt.value)) == args.iters
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
        return statistics.median(per_round), per_round

    qp = (0.043, 119, 0.027, 131, 0.061, 97)   # calibrated-looking: three unrelated scales
    eq = (0.05, 128, 0.05, 128, 0.05, 128)
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            a = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            da, db, do = put(a), put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)), empty(n)
            ab = np.full((m, h + 2, w + 2, c), qp[1] ^ 0x80, np.uint8)
            ab[:, 1:-1, 1:-1, :] = a ^ np.uint8(0x80)
            dab, dob = put(ab), empty(ab.size)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, qp[5] ^ 0x80))
            legs = {
                "add_relu": (3, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, da, 0, 0, db, 0, 0, do, 0, 0, m, c, h, w, *qp, 1))),
                "add_relu_block": (3, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, dab, 1, 1, db, 0, 0, dob, 1, 1, m, c, h, w, *qp, 1))),
                "add_relu_replay": (3, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, da, 0, 0, db, 0, 0, do, 0, 0, m, c, h, w, *eq, 1))),
                "relu_u8": (2, lambda: ck(lib.i8ie_relu_u8(ctx, da, do, n, 97))),
                "rebias_u8": (2, lambda: ck(lib.i8ie_rebias_u8(ctx, da, do, n))),
            }
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "elements": n}
            for tag, (bytes_per_el, fn) in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": bytes_per_el,
                            "gb_per_s": bytes_per_el * n / (ms * 1e-3) / 1e9}
            row["add_over_relu_byte_rate"] = row["add_relu"]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
            row["add_block_over_relu_byte_rate"] = row["add_relu_block"]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
            for d in (da, db, do, dab, dob):
                ck(lib.i8ie_free(ctx, d))
            results.append(row)
            print(json.dumps(row), flush=True)
    lib.i8ie_ctx_destroy(ctx)

    out = {"tool": "bench_add", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*); median over rounds of the per-round mean per launch",
           "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
