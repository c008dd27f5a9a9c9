"""Resize to any size and adaptive average pooling against the existing kernels and against the cheapest pass over the same bytes.

    python tools/bench_resize.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 10] [--out profiles/r24_bench_resize.json]

Rows, each at 1000 and at 125 images, through the C-ABI on flat plain NHWC buffers:
  resize_u8_nhwc at x2 on 64x16^2 and 64x56^2 against i8ie_upsample2d_u8_nhwc on the same buffers (identical bytes asserted);
  64x25^2 -> 50^2, 256x13^2 -> 25^2, 64x56^2 -> 28^2 and 10x8^2 -> 32^2 aligned against i8ie_relu_u8 over the result's bytes;
  adaptive_avgpool_u8_nhwc at 256x8^2 -> 4^2 against i8ie_avgpool2d_u8_nhwc(2, 2) (identical bytes asserted), and
  256x8^2 -> 3^2 / 6^2 against i8ie_relu_u8 over the input's bytes.
Before any timing the first images of every result are compared with the integer definition (tests/resize_ref.py).  Timing is
the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds` rounds
of `iters` profiled calls; a round's figure is its mean per call and the reported one the median over rounds.  The aim: ratio
<= 1.03 per row (3 % is the run-to-run spread); every row records the ratio and `met` / `MISSED`.  Then
examples/pspnet_cifar10.py's INT8 step with the share of the new kernels."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_ref as rr  # noqa: E402

BATCHES = [1000, 125]
AIM = 1.03
# (name, c, h, w, oh, ow, mode or "pool", the yardstick)
ROWS = [("x2_64x16x16", 64, 16, 16, 32, 32, rr.BILINEAR, "upsample"), ("x2_64x56x56", 64, 56, 56, 112, 112, rr.BILINEAR, "upsample"),
        ("64x25x25_to_50x50", 64, 25, 25, 50, 50, rr.BILINEAR, "relu_out"), ("256x13x13_to_25x25", 256, 13, 13, 25, 25, rr.BILINEAR, "relu_out"),
        ("64x56x56_to_28x28", 64, 56, 56, 28, 28, rr.BILINEAR, "relu_out"), ("10x8x8_to_32x32_aligned", 10, 8, 8, 32, 32, rr.ALIGNED, "relu_out"),
        ("pool_256x8x8_to_4x4", 256, 8, 8, 4, 4, "pool", "avgpool"), ("pool_256x8x8_to_3x3", 256, 8, 8, 3, 3, "pool", "relu_in"),
        ("pool_256x8x8_to_6x6", 256, 8, 8, 6, 6, "pool", "relu_in")]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = rr.bind(C.CDLL(args.lib))
    lib.i8ie_last_error.restype = C.c_char_p
    P, I = C.c_void_p, C.c_int
    lib.i8ie_upsample2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [C.c_uint8]
    lib.i8ie_avgpool2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [C.c_uint8]
    lib.i8ie_relu_u8.argtypes = [P, P, P, C.c_int64, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_resize.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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
        return {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_call": names}

    zp, results = 117, []
    for name, c, h, w, oh, ow, mode, yard in ROWS:
        rng = np.random.default_rng(sum(map(ord, name)))
        for m in BATCHES:
            x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            in_bytes, out_bytes = x.nbytes, m * oh * ow * c
            dx, dy, dz = alloc(in_bytes), alloc(out_bytes), alloc(out_bytes)
            ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), in_bytes))
            if mode == "pool":
                new = lambda: ck(lib.i8ie_adaptive_avgpool2d_u8_nhwc(ctx, dx, 0, 0, dy, 0, 0, m, c, h, w, oh, ow, 0, zp))
            else:
                new = lambda: ck(lib.i8ie_resize2d_u8_nhwc(ctx, dx, 0, 0, dy, 0, 0, m, c, h, w, oh, ow, mode, 0, zp))
            new()
            k = min(m, 4)  # (the first images: the definition in int64 on the host is the slow part)
            host = np.empty((k, oh, ow, c), np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), dy, host.nbytes))
            q = x[:k].transpose(0, 3, 1, 2)
            want = rr.adaptive_u8(q, oh, ow) if mode == "pool" else rr.resize_u8(q, oh, ow, mode)
            assert np.array_equal(host, want.transpose(0, 2, 3, 1)), "%s @ %d: bytes differ from the definition" % (name, m)
            row = {"row": name, "images": m, "c": c, "in": [h, w], "out": [oh, ow], "input_bytes": in_bytes, "output_bytes": out_bytes,
                   "identical_to_definition": True, "against": yard}
            if yard == "upsample":
                old = lambda: ck(lib.i8ie_upsample2d_u8_nhwc(ctx, dx, 0, 0, dz, 0, 0, m, c, h, w, oh // h, ow // w, 1, 0, zp))
            elif yard == "avgpool":
                old = lambda: ck(lib.i8ie_avgpool2d_u8_nhwc(ctx, dx, 0, 0, dz, 0, 0, m, c, h, w, h // oh, w // ow, h // oh, 0, zp))
            elif yard == "relu_out":
                old = lambda: ck(lib.i8ie_relu_u8(ctx, dz, dz, out_bytes, zp))
            else:
                old = lambda: ck(lib.i8ie_relu_u8(ctx, dx, dx, in_bytes, 0))  # (zp 0: the input keeps its bytes)
            if yard in ("upsample", "avgpool"):
                old()
                a, b = np.empty(out_bytes, np.uint8), np.empty(out_bytes, np.uint8)
                ck(lib.i8ie_memcpy_d2h(ctx, a.ctypes.data_as(P), dy, out_bytes))
                ck(lib.i8ie_memcpy_d2h(ctx, b.ctypes.data_as(P), dz, out_bytes))
                assert np.array_equal(a, b), "%s @ %d: bytes differ from the existing kernel's" % (name, m)
                row["identical_to_existing_kernel"] = True
            row["yardstick"] = timed(old)
            row["new"] = timed(new)
            row["new"]["GBps"] = (in_bytes + out_bytes) / row["new"]["ms"] / 1e6
            row["ratio"] = row["new"]["ms"] / row["yardstick"]["ms"]
            row["aim_ratio_at_most_1.03"] = "met" if row["ratio"] <= AIM else "MISSED"
            for d in (dx, dy, dz):
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

    spec = importlib.util.spec_from_file_location("pspnet_cifar10", os.path.join(ROOT, "examples", "pspnet_cifar10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.make_model(i8ie)
    model.load(mod.synthetic_state_dict(model))
    model.prepare()
    model(i8ie.tensor(np.random.default_rng(99).standard_normal((16, 3, 32, 32)).astype(np.float32)))
    model.convert()
    rows = []
    new = ("resize_u8", "adaptive_avgpool_u8")
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(1234).standard_normal((m, 3, 32, 32)).astype(np.float32)).prefetch()
        for _ in range(args.warmup):
            model(x).numpy()
        walls = []
        for _ in range(args.rounds):
            cx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.net_steps):
                y = model(x)
            y.numpy()
            walls.append((time.perf_counter() - t0) / args.net_steps * 1e3)
        cx.profile_start()
        for _ in range(args.net_steps):
            model(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        own = sum(v[1] for k, v in prof.items() if k.startswith(new))
        by = {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
        wall = statistics.median(walls)
        rows.append({"network": "examples/pspnet_cifar10.py", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                     "new_kernels_ms_per_step": own / args.net_steps, "new_kernels_share_of_kernel_time": own / total,
                     "new_kernel_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith(new)) / args.net_steps,
                     "kernel_ms_per_step_by_name": by})
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
    out = {"tool": "bench_resize", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean",
           "aim": "new ms / yardstick ms <= 1.03 per row", "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
