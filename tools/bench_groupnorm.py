"""The quantized GroupNorm kernels against two kernels the library already had.

    python tools/bench_groupnorm.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 10] [--out profiles/r18_bench_groupnorm.json]

GroupNorm(32) of [N, c, h, w] (NHWC) at 1000 and 125 images, on random bytes with random gamma / beta:
  gn        flat: both buffers border-free and plain
  gn_block  the input border-free and plain, the result bordered by 1 and re-biased for a following 3x3 conv
for 64x32^2, 128x16^2, 256x8^2, 512x4^2 (the image form) and 64x56^2 (the split form), beside
  ln        i8ie_layernorm_u8_nhwc on the same buffer: the same bytes in and out, the same per-byte arithmetic
  relu_u8   over the same bytes
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds`
rounds of `iters` profiled calls; a round's figure is its kernel time per call (the split form's two launches added), the reported
one the median over rounds.  Aims, from the bytes moved, with the project's spread of 3 %: the image form no slower than the
LayerNorm (gn / ln <= 1.03), the split form at most 1.5 times it (three passes over the bytes against two; <= 1.545).  The bytes of
the first two images are asserted against the definition (tests/groupnorm_ref.py).  This part goes through the C-ABI by ctypes.

Then the step time of workloads' groupnorm_resnet_cifar (the network of examples/groupnorm_resnet_cifar10.py) at the same two
batch sizes through the Python surface, with the share of the profiled kernel time its GroupNorm launches take (`--net-steps 0`
skips it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 32
SHAPES = [("c64_32x32", 64, 32, 32), ("c128_16x16", 128, 16, 16), ("c256_8x8", 256, 8, 8), ("c512_4x4", 512, 4, 4), ("c64_56x56", 64, 56, 56)]
BATCHES = [1000, 125]
SPREAD = 1.03


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import groupnorm_ref as gn
    import layernorm_ref as lr

    lib = gn.bind(C.CDLL(args.lib))
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B, L = C.c_void_p, C.c_int, C.c_uint8, C.c_int64
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_groupnorm.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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
        ck(lib.i8ie_malloc(ctx, max(nbytes, 16), C.byref(d)))
        return d

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], {}
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                fn()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            names = {ents[i].name.decode().split("|")[0]: int(ents[i].launches) // args.iters for i in range(cnt.value)}
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
        return statistics.median(per_round), per_round, names

    zp_out, s_in, s_out, eps = 97, np.float32(0.05), np.float32(0.02), np.float32(1e-5)
    results = []
    for name, c, h, w in SHAPES:
        form = gn.form(c, h, w)
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * c * h * w
            gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
            g, b = lr.affine(gamma, beta, s_out, zp_out)
            host = rng.integers(0, 256, n, dtype=np.uint8)
            di, dg, db = put(host), put(g), put(b)
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * c)
            nws = lib.i8ie_groupnorm_workspace_bytes(m, c, G, h, w)
            ws = put(np.full(max(nws, 16), 0xFF, np.uint8))
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, h, w, 1, zp_out ^ 0x80))
            legs = {
                "relu_u8": lambda: ck(lib.i8ie_relu_u8(ctx, di, do, n, zp_out)),
                "ln": lambda: ck(lib.i8ie_layernorm_u8_nhwc(ctx, di, 0, 0, do, 0, 0, m, c, h, w, dg, db, s_in, eps, 0, zp_out)),
                "ln_block": lambda: ck(lib.i8ie_layernorm_u8_nhwc(ctx, di, 0, 0, dob, 1, 1, m, c, h, w, dg, db, s_in, eps, 0, zp_out)),
                "gn": lambda: ck(lib.i8ie_groupnorm_u8_nhwc(ctx, di, 0, 0, do, 0, 0, m, c, G, h, w, dg, db, s_in, eps, 0, zp_out, ws)),
                "gn_block": lambda: ck(lib.i8ie_groupnorm_u8_nhwc(ctx, di, 0, 0, dob, 1, 1, m, c, G, h, w, dg, db, s_in, eps, 0, zp_out, ws)),
            }
            # the bytes of the first two images, both layouts, against the definition
            first = 2 * h * w * c
            q = np.ascontiguousarray(host[:first].reshape(2, h, w, c).transpose(0, 3, 1, 2))
            want = gn.group_norm_u8(q, G, s_in, eps, gamma, beta, s_out, zp_out).transpose(0, 2, 3, 1)
            legs["gn_block"]()
            got = np.empty(2 * (h + 2) * (w + 2) * c, np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, got.ctypes.data_as(P), dob, got.size))
            assert np.array_equal(got.reshape(2, h + 2, w + 2, c)[:, 1:-1, 1:-1, :] ^ np.uint8(0x80), want), (name, m, "gn_block")
            legs["gn"]()   # (last, so that `do` holds the GroupNorm's bytes and not the LayerNorm's)
            got = np.empty(first, np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, got.ctypes.data_as(P), do, first))
            assert np.array_equal(got.reshape(2, h, w, c), want), (name, m, "gn")
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "groups": G, "form": form, "elements": n}
            for tag, fn in legs.items():
                ms, per_round, names = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "kernels": names, "gb_per_s_at_2_bytes_per_element": 2 * n / (ms * 1e-3) / 1e9}
            aim = SPREAD * (1.0 if form == "image" else 1.5)
            for tag, base in (("gn", "ln"), ("gn_block", "ln_block")):
                ratio = row[tag]["ms"] / row[base]["ms"]
                row[tag]["over_" + base] = ratio
                row[tag]["aim"] = aim
                row[tag]["verdict"] = "met" if ratio <= aim else "MISSED"
                row[tag]["over_relu_u8"] = row[tag]["ms"] / row["relu_u8"]["ms"]
            for d in (di, do, dob, dg, db, ws):
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

    net = wl.calibrated("groupnorm_resnet_cifar", calib_batch=wl.synthetic_input("groupnorm_resnet_cifar", 16, seed=99))
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(wl.synthetic_input("groupnorm_resnet_cifar", m)).prefetch()
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
        mine = sum(v[1] for k, v in prof.items() if k.startswith("groupnorm_u8"))
        by = {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
        launches = {}
        for k, v in prof.items():
            if k.startswith("groupnorm_u8"):
                launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0] / args.net_steps
        rows.append({"network": "GroupNormResNet(cifar)", "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "groupnorm_ms_per_step": mine / args.net_steps, "groupnorm_share_of_kernel_time": mine / total,
                     "groupnorm_launches_per_step": launches, "kernel_ms_per_step_by_name": by})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=10)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_groupnorm", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*); median over rounds of the per-round kernel time per call",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
