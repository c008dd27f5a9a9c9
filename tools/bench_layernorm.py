"""The quantized LayerNorm kernels against the streaming kernel the library already had.

    python tools/bench_layernorm.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r16_bench_layernorm.json]

LayerNorm over c per pixel of [N, c, h, w] (NHWC) for the shapes 64x16^2, 128x8^2, 256x4^2, 512x2^2 and 96x56^2 at 1000 and
125 images, on random bytes with random gamma / beta:
  ln        flat: both buffers border-free and plain
  ln_block  the input border-free and plain, the result bordered by 1 and re-biased for a following 3x3 conv
beside
  relu_u8   the existing kernel over the same bytes
All of them move 2 bytes of HBM traffic per element (1 read + 1 write).  Timing is the library's own per-launch HIP-event
bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then `rounds` rounds of `iters` profiled launches; a
round's figure is its mean per launch, the reported one the median over rounds.  The yardstick is relu_u8's byte rate in the
same run; a ratio below 0.97 is written MISSED.  The bytes of the first images are asserted against the definition
(tests/layernorm_ref.py).  This part goes through the C-ABI by ctypes only.

Then the step time of convnext_cifar at the same two batch sizes through the Python surface, with the share of the
profiled kernel time its LayerNorm launches take (`--net-steps 0` skips it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c64_16x16", 64, 16, 16), ("c128_8x8", 128, 8, 8), ("c256_4x4", 256, 4, 4), ("c512_2x2", 512, 2, 2), ("c96_56x56", 96, 56, 56)]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B, L = C.c_void_p, C.c_int, C.c_uint8, C.c_int64
    F = C.c_float
    lib.i8ie_layernorm_u8.argtypes = [P, P, P, L, I, P, P, F, F, I, B]
    lib.i8ie_layernorm_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, I, I, I, P, P, F, F, I, B]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_layernorm.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import layernorm_ref as lr

    zp_out, s_in, s_out, eps = 97, np.float32(0.05), np.float32(0.02), np.float32(1e-5)
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
            g, b = lr.affine(gamma, beta, s_out, zp_out)
            host = rng.integers(0, 256, n, dtype=np.uint8)
            di, dg, db = put(host), put(g), put(b)
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, zp_out ^ 0x80))
            legs = {
                "relu_u8": lambda: ck(lib.i8ie_relu_u8(ctx, di, do, n, zp_out)),
                "ln": lambda: ck(lib.i8ie_layernorm_u8(ctx, di, do, m * h * w, c, dg, db, s_in, eps, 0, zp_out)),
                "ln_block": lambda: ck(lib.i8ie_layernorm_u8_nhwc(ctx, di, 0, 0, dob, 1, 1, m, c, h, w, dg, db, s_in, eps, 0, zp_out)),
            }
            # the bytes of the first two images, both forms, against the definition
            first = 2 * h * w * c
            want = lr.layer_norm_u8(host[:first].reshape(-1, c), s_in, eps, gamma, beta, s_out, zp_out)
            legs["ln"]()
            got = np.empty(first, np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, got.ctypes.data_as(P), do, first))
            assert np.array_equal(got.reshape(-1, c), want), (name, m, "ln")
            legs["ln_block"]()
            got = np.empty(2 * (h + 2) * (w + 2) * c, np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, got.ctypes.data_as(P), dob, got.size))
            got = got.reshape(2, h + 2, w + 2, c)[:, 1:-1, 1:-1, :] ^ np.uint8(0x80)
            assert np.array_equal(got.reshape(-1, c), want), (name, m, "ln_block")
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "elements": n}
            for tag, fn in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": 2, "gb_per_s": 2 * n / (ms * 1e-3) / 1e9}
            for tag in legs:
                if tag != "relu_u8":
                    ratio = row[tag]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
                    row[tag]["over_relu_byte_rate"] = ratio
                    row[tag]["verdict"] = "met" if ratio >= 0.97 else "MISSED"
            for d in (di, do, dob, dg, db):
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

    name = "convnext_cifar"
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

        lut = share("layernorm_u8")
        rows.append({"network": "ConvNeXt(cifar)", "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "layernorm_ms_per_step": lut / args.net_steps, "layernorm_share_of_kernel_time": lut / total,
                     "layernorm_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("layernorm_u8")) / args.net_steps,
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
    out = {"tool": "bench_layernorm", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
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
