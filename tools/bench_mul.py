"""The quantized broadcast Mul against the Add and the streaming kernels the library already had.

    python tools/bench_mul.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r11_bench_mul.json]

Per activation shape ([N, 96, 8, 8], [N, 576, 4, 4]: squeeze-and-excitation sites of MobileNetV3-small on 32 x 32 input; and
[N, 64, 56, 56]: the Add benchmark's large shape; all NHWC) and batch size (1000, 125):
  mul_gate            a * g, g one byte per image and channel (plain rows), both buffers border-free (2 bytes of HBM traffic per
                      element of a, plus the gate)
  mul_gate_block      the same with the result bordered by 1 and re-biased, as a padded conv behind it wants it
  mul_equal           a * b of equal shapes, border-free: the flat form (3 bytes per element)
  mul_equal_block     ... with the result bordered by 1 and re-biased
  add_relu            i8ie_add_u8_nhwc over the same a (3 bytes per element): the gate form moves two thirds of its bytes
  relu_u8             the existing streaming kernel over the same number of elements (2 bytes per element)
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then
`rounds` rounds of `iters` profiled launches; a round's figure is its mean per launch, the reported one the median over
rounds.  GB/s = algorithmic HBM bytes / that time.  The kernels go through the C-ABI by ctypes only.

Then the step time of mobilenetv3_small_cifar at the same two batch sizes through the Python surface, with the share of the
kernel time its nine multiplies (and its depthwise convolutions) take."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c96_8x8", 96, 8, 8), ("c576_4x4", 576, 4, 4), ("c64_56x56", 64, 56, 56)]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F, B, L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64
    lib.i8ie_mul_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, P, I, I, I, I, I, I, F, B, F, B, F, B, I]
    lib.i8ie_add_u8_nhwc.argtypes = [P, P, I, I, P, I, I, P, I, I, I, I, I, I, F, B, F, B, F, B, I]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_mul.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    gq = (0.043, 119, 1.0 / 255, 0, 0.043, 119)   # a hardsigmoid gate against a's own parameters
    eq = (0.043, 119, 0.027, 131, 0.061, 97)      # calibrated-looking: three unrelated scales (the Add benchmark's)
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            da = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            db = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            dg = put(rng.integers(0, 256, (m, c), dtype=np.uint8))
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, gq[5] ^ 0x80))
            gate_bytes = 2 + 1.0 / (h * w)
            legs = {
                "mul_gate": (gate_bytes, lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, dg, 0, 0, 1, do, 0, 0, m, c, h, w, *gq, 0))),
                "mul_gate_block": (gate_bytes, lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, dg, 0, 0, 1, dob, 1, 1, m, c, h, w, *gq, 0))),
                "mul_equal": (3, lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, db, 0, 0, 0, do, 0, 0, m, c, h, w, *eq, 0))),
                "mul_equal_block": (3, lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, db, 0, 0, 0, dob, 1, 1, m, c, h, w, *eq, 0))),
                "add_relu": (3, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, da, 0, 0, db, 0, 0, do, 0, 0, m, c, h, w, *eq, 1))),
                "relu_u8": (2, lambda: ck(lib.i8ie_relu_u8(ctx, da, do, n, 97))),
            }
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "elements": n}
            for tag, (bytes_per_el, fn) in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": bytes_per_el,
                            "gb_per_s": bytes_per_el * n / (ms * 1e-3) / 1e9}
            row["gate_time_over_add_time"] = row["mul_gate"]["ms"] / row["add_relu"]["ms"]
            row["gate_block_time_over_add_time"] = row["mul_gate_block"]["ms"] / row["add_relu"]["ms"]
            row["equal_time_over_add_time"] = row["mul_equal"]["ms"] / row["add_relu"]["ms"]
            row["gate_time_over_relu_time"] = row["mul_gate"]["ms"] / row["relu_u8"]["ms"]
            for d in (da, db, dg, do, dob):
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

    name = "mobilenetv3_small_cifar"
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

        mul = share("mul_u8")
        rows.append({"network": name, "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "images_per_s_wall": m / (wall * 1e-3),
                     "mul_ms_per_step": mul / args.net_steps, "mul_share_of_kernel_time": mul / total,
                     "mul_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("mul_u8")) / args.net_steps,
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
    out = {"tool": "bench_mul", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
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
