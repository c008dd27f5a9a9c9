"""The quantized BatchNorm kernel against the Mul's gate form and the streaming relu the library already had.

    python tools/bench_batchnorm.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r22_bench_batchnorm.json]

Per activation shape ([N, 64, 32, 32], [N, 128, 16, 16], [N, 256, 8, 8], [N, 512, 4, 4], [N, 64, 56, 56]; all NHWC) and batch
size (1000, 125):
  bn                  relu(bn(a)), both buffers border-free (2 bytes of HBM traffic per element, plus 8 C bytes of g / b)
  bn_block            the same with the result bordered by 1 and re-biased, as a padded conv behind it wants it
  mul_gate            i8ie_mul_u8_nhwc with b_gate != 0 on the same a: the closest existing kernel, it moves the same bytes plus one
                      gate byte per image and channel
  mul_gate_block      ... with the result bordered by 1 and re-biased
  relu_u8             the existing streaming kernel over the same bytes
The aim is bn no slower than the gate form within the project's +-3 % spread: bn / mul_gate <= 1.03 and bn_block / mul_gate_block
<= 1.03, each marked met / MISSED.  Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop), the
method of tools/bench_mul.py: `warmup` launches unprofiled, then `rounds` rounds of `iters` profiled launches; a round's figure is
its mean per launch, the reported one the median over rounds.  The kernels go through the C-ABI by ctypes only.

Then the step time of examples/densenet_cifar10.py's network at the same two batch sizes through the Python surface, with the
share of the kernel time its BatchNorm launches take."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c64_32x32", 64, 32, 32), ("c128_16x16", 128, 16, 16), ("c256_8x8", 256, 8, 8), ("c512_4x4", 512, 4, 4),
          ("c64_56x56", 64, 56, 56)]
BATCHES = [1000, 125]
AIM = 1.03


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F, B, L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64
    lib.i8ie_batchnorm_affine.argtypes = [P, P, P, P, I, F, F, B, P, P]
    lib.i8ie_batchnorm_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, I, I, I, P, P, F, B, I, B]
    lib.i8ie_mul_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, P, I, I, I, I, I, I, F, B, F, B, F, B, I]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_batchnorm.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    s_in, zp_in, s_out, zp_out = 0.043, 119, 0.05, 97
    gq = (s_in, zp_in, 1.0 / 255, 0, s_out, zp_out)   # a hardsigmoid gate into the same output parameters
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            f32 = np.float32
            gamma, beta = rng.normal(1.0, 0.5, c).astype(f32), rng.normal(0.0, 0.5, c).astype(f32)
            mean, var = rng.normal(0.0, 1.0, c).astype(f32), rng.uniform(0.01, 4.0, c).astype(f32)
            g, b = np.zeros(c, f32), np.zeros(c, f32)
            ck(lib.i8ie_batchnorm_affine(gamma.ctypes.data, beta.ctypes.data, mean.ctypes.data, var.ctypes.data, c, 1e-5, s_out, zp_out,
                                         g.ctypes.data, b.ctypes.data))
            da = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            dgate = put(rng.integers(0, 256, (m, c), dtype=np.uint8))
            dg, db = put(g), put(b)
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, zp_out ^ 0x80))
            legs = {
                "bn": (2 + 8.0 / (m * h * w), lambda: ck(lib.i8ie_batchnorm_u8_nhwc(ctx, da, 0, 0, do, 0, 0, m, c, h, w, dg, db, s_in, zp_in, 1, zp_out))),
                "bn_block": (2 + 8.0 / (m * h * w), lambda: ck(lib.i8ie_batchnorm_u8_nhwc(ctx, da, 0, 0, dob, 1, 1, m, c, h, w, dg, db, s_in, zp_in, 1, zp_out))),
                "mul_gate": (2 + 1.0 / (h * w), lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, dgate, 0, 0, 1, do, 0, 0, m, c, h, w, *gq, 1))),
                "mul_gate_block": (2 + 1.0 / (h * w), lambda: ck(lib.i8ie_mul_u8_nhwc(ctx, da, 0, 0, dgate, 0, 0, 1, dob, 1, 1, m, c, h, w, *gq, 1))),
                "relu_u8": (2, lambda: ck(lib.i8ie_relu_u8(ctx, da, do, n, zp_out))),
            }
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "elements": n}
            for tag, (bytes_per_el, fn) in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": bytes_per_el,
                            "gb_per_s": bytes_per_el * n / (ms * 1e-3) / 1e9}
            row["bn_time_over_gate_time"] = row["bn"]["ms"] / row["mul_gate"]["ms"]
            row["bn_block_time_over_gate_block_time"] = row["bn_block"]["ms"] / row["mul_gate_block"]["ms"]
            row["bn_time_over_relu_time"] = row["bn"]["ms"] / row["relu_u8"]["ms"]
            row["aim"] = AIM
            row["flat"] = "met" if row["bn_time_over_gate_time"] <= AIM else "MISSED"
            row["block"] = "met" if row["bn_block_time_over_gate_block_time"] <= AIM else "MISSED"
            for d in (da, dgate, dg, db, do, dob):
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

    spec = importlib.util.spec_from_file_location("densenet_cifar10", os.path.join(ROOT, "examples", "densenet_cifar10.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    net = example.make_model(i8ie)
    net.load(example.synthetic_state_dict(net))
    net.fold_batchnorm(net.folds)
    net.prepare()
    net(i8ie.tensor(np.random.default_rng(1234).standard_normal((64, 3, 32, 32)).astype(np.float32)))
    net.convert()
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(5).standard_normal((m, 3, 32, 32)).astype(np.float32)).prefetch()
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
        by, launches = {}, {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
            launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0] / args.net_steps
        bn_ms = sum(v for k, v in by.items() if k.startswith("batchnorm_u8"))
        rows.append({"network": "examples/densenet_cifar10.py", "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "images_per_s_wall": m / (wall * 1e-3), "batchnorm_ms_per_step": bn_ms,
                     "batchnorm_share_of_kernel_time": bn_ms / (total / args.net_steps),
                     "batchnorm_u8_nhwc_share_of_kernel_time": by.get("batchnorm_u8_nhwc", 0.0) / (total / args.net_steps),
                     "batchnorm_launches_per_step": {k: v for k, v in launches.items() if k.startswith("batchnorm_u8")},
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
    out = {"tool": "bench_batchnorm", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
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
