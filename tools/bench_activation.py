"""The table-driven activation kernel against the streaming kernel the library already had.

    python tools/bench_activation.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r10_bench_activation.json]

out = table[in] per shape ([N, 64, 56, 56] and [N, 96, 16, 16], NHWC) and batch size (1000, 125), on random bytes with a random
permutation as the table (no two equal bytes share a result: the worst case for a lookup):
  lut        flat: both buffers border-free and plain
  lut_block  as an inverted residual block runs it: the input border-free and plain, the result bordered by 1 and re-biased
             for a following 3x3 conv
beside
  relu_u8    the existing kernel over the same bytes
All of them move 2 bytes of HBM traffic per element (1 read + 1 write).  Timing is the library's own per-launch HIP-event
bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then `rounds` rounds of `iters` profiled launches; a
round's figure is its mean per launch, the reported one the median over rounds.  GB/s = algorithmic HBM bytes / that time.
The yardstick is relu_u8's byte rate in the same run.  This part goes through the C-ABI by ctypes only.

Then the step time of mobilenetv2_cifar at the same two batch sizes through the Python surface, with the share of the
profiled kernel time its activation launches take (`--net-steps 0` skips it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c64_56x56", 64, 56, 56), ("c96_16x16", 96, 16, 16)]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B, L = C.c_void_p, C.c_int, C.c_uint8, C.c_int64
    lib.i8ie_lut_u8.argtypes = [P, P, P, L, P]
    lib.i8ie_lut_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, I, I, I, P]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_activation.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    zp_out = 97
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            table = rng.permutation(256).astype(np.uint8)
            tp = table.ctypes.data_as(P)
            di = put(rng.integers(0, 256, n, dtype=np.uint8))
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, zp_out ^ 0x80))
            legs = {
                "relu_u8": lambda: ck(lib.i8ie_relu_u8(ctx, di, do, n, zp_out)),
                "lut": lambda: ck(lib.i8ie_lut_u8(ctx, di, do, n, tp)),
                "lut_block": lambda: ck(lib.i8ie_lut_u8_nhwc(ctx, di, 0, 0, dob, 1, 1, m, c, h, w, tp)),
            }
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "elements": n}
            for tag, fn in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": 2, "gb_per_s": 2 * n / (ms * 1e-3) / 1e9}
            for tag in legs:
                if tag != "relu_u8":
                    row[tag]["over_relu_byte_rate"] = row[tag]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
            for d in (di, do, dob):
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

    name = "mobilenetv2_cifar"
    net = wl.calibrated(name)
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

        def share(prefix):
            return sum(v[1] for k, v in prof.items() if k.startswith(prefix))

        lut = share("lut_u8")
        rows.append({"network": name, "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "activation_ms_per_step": lut / args.net_steps, "activation_share_of_kernel_time": lut / total,
                     "activation_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("lut_u8")) / args.net_steps,
                     "grouped_conv_share_of_kernel_time": share("gconv") / total,
                     "kernel_ms_per_step_by_name": {k.split("|")[0]: 0 for k in prof}})
        by = rows[-1]["kernel_ms_per_step_by_name"]
        for k, v in prof.items():
            by[k.split("|")[0]] += v[1] / args.net_steps
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
    out = {"tool": "bench_activation", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*); median over rounds of the per-round mean per launch",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
