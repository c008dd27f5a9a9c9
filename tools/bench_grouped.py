"""Grouped Conv2d against the only workaround there was: a dense layer with block-diagonal weights.

    python tools/bench_grouped.py [--iters 20] [--rounds 5] [--warmup 5] [--out profiles/r06_bench_grouped.json]
    python tools/bench_grouped.py --lib OTHER/libi8ie_hip.so --dense-only --out parent.json     # the dense leg on another build
    python tools/bench_grouped.py --parent parent.json --out profiles/r06_bench_grouped.json    # ... merged into the result

Per shape and batch size: the same u8 input (NHWC with a zero-point border that covers the padding, so the convolution is
the only kernel of a forward), the same weights once as [kc, c/groups, k, k] in a grouped layer handle and once as the
dense [kc, c, k, k] tensor that is zero outside each group's block; output bytes asserted identical.  Timing is the
library's own per-launch HIP-event bracket (i8ie_profile_start / _stop) summed over the kernels of a forward:
`warmup` forwards unprofiled, then `rounds` rounds of `iters` profiled forwards; a round's figure is its mean per forward
and the reported one the median over rounds.  Goes through the C-ABI by ctypes only, so --lib can point at any build."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, c, kc, groups, k, stride, pad, h, w)
SHAPES = [
    ("paper_conv2", 96, 256, 2, 5, 1, 2, 27, 27),
    ("paper_conv4", 384, 384, 2, 3, 1, 1, 13, 13),
    ("paper_conv5", 384, 256, 2, 3, 1, 1, 13, 13),
    ("resnext_g32", 128, 128, 32, 3, 1, 1, 14, 14),
    ("depthwise_256", 256, 256, 256, 3, 1, 1, 14, 14),
]
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
    ap.add_argument("--dense-only", action="store_true", help="time only the block-diagonal dense layer (a build without groups)")
    ap.add_argument("--parent", default=None, help="JSON of a --dense-only run on the parent commit, merged into the result")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F = C.c_void_p, C.c_int, C.c_float
    lib.i8ie_conv2d_create.argtypes = [P, P, P, I, I, I, I, I, I, F, P]
    if not args.dense_only:
        lib.i8ie_conv2d_create_grouped.argtypes = [P, P, P, I, I, I, I, I, I, I, F, P]
    lib.i8ie_layer_forward_fused.argtypes = [P, P, I, I, I, I, I, F, C.c_uint8, I, P, I, I, P]
    lib.i8ie_layer_set_output_qparams.argtypes = [P, F, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_grouped.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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
    for name, c, kc, g, k, stride, pad, h, w in SHAPES:
        rng = np.random.default_rng(sum(map(ord, name)))
        Cg, Ng = c // g, kc // g
        qw = rng.integers(-127, 128, (kc, Cg, k, k), dtype=np.int8)
        qb = rng.integers(-127, 128, kc, dtype=np.int8)
        dense = np.zeros((kc, c, k, k), np.int8)
        for gi in range(g):
            dense[gi * Ng:(gi + 1) * Ng, gi * Cg:(gi + 1) * Cg] = qw[gi * Ng:(gi + 1) * Ng]
        s_out = float(np.float32(s_in * s_w * np.sqrt(Cg * k * k) * 40.0 / 64.0))
        oh, ow = (h - k + 2 * pad) // stride + 1, (w - k + 2 * pad) // stride + 1
        layers = {}
        L = P()
        ck(lib.i8ie_conv2d_create(ctx, dense.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, stride, pad, s_w, C.byref(L)))
        layers["dense_block_diagonal"] = L
        if not args.dense_only:
            L = P()
            ck(lib.i8ie_conv2d_create_grouped(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, stride, pad, g, s_w,
                                              C.byref(L)))
            layers["grouped"] = L
        for L in layers.values():
            ck(lib.i8ie_layer_set_output_qparams(L, s_out, zp_out))
        for m in BATCHES:
            x = np.full((m, h + 2 * pad, w + 2 * pad, c), zp_in, np.uint8)
            x[:, pad:pad + h, pad:pad + w, :] = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            dx = put(x)
            row = {"shape": name, "images": m, "c": c, "kc": kc, "groups": g, "kernel": k, "stride": stride, "pad": pad, "h": h, "w": w,
                   "macs_grouped": m * oh * ow * kc * Cg * k * k, "macs_dense": m * oh * ow * kc * c * k * k}
            outs = {}
            for tag, L in layers.items():
                do = P()
                nbytes = m * oh * ow * kc
                ck(lib.i8ie_malloc(ctx, nbytes, C.byref(do)))

                def fwd():
                    ck(lib.i8ie_layer_forward_fused(L, dx, 1, pad, m, h, w, s_in, zp_in, 1, do, 1, 0, None))

                for _ in range(args.warmup):
                    fwd()
                ck(lib.i8ie_sync(ctx))
                per_round, kernels = [], {}
                for _ in range(args.rounds):
                    ck(lib.i8ie_profile_start(ctx, 0))
                    for _ in range(args.iters):
                        fwd()
                    ents, cnt = (Entry * 64)(), C.c_int(0)
                    ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
                    per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
                    kernels = {ents[i].name.decode(): int(ents[i].launches) // args.iters for i in range(cnt.value)}
                host = np.empty(nbytes, np.uint8)
                ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), do, nbytes))
                outs[tag] = host
                ck(lib.i8ie_free(ctx, do))
                row[tag] = {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_forward": kernels}
            if "grouped" in outs:
                assert np.array_equal(outs["grouped"], outs["dense_block_diagonal"]), "%s @ %d: output bytes differ" % (name, m)
                row["identical_bytes"] = True
                row["grouped_over_dense"] = row["grouped"]["ms"] / row["dense_block_diagonal"]["ms"]
            ck(lib.i8ie_free(ctx, dx))
            results.append(row)
            print(json.dumps(row), flush=True)
        for L in layers.values():
            lib.i8ie_layer_destroy(L)
    lib.i8ie_ctx_destroy(ctx)

    out = {"tool": "bench_grouped", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per forward; median over rounds of the per-round mean",
           "dense_only": bool(args.dense_only), "results": results}
    if args.parent:
        with open(args.parent) as f:
            parent = {(r["shape"], r["images"]): r["dense_block_diagonal"]["ms"] for r in json.load(f)["results"]}
        for r in results:
            r["dense_block_diagonal_parent_commit_ms"] = parent.get((r["shape"], r["images"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
