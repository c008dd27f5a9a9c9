"""The position-embedding kernel against the residual Add and the streaming relu the library already had.

    python tools/bench_posembed.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r26_bench_posembed.json]

Per token map (192 x 8^2, 384 x 8^2 and 768 x 4^2 in the class form, 64 x 32^2 in the plain form; all NHWC) and batch size (1000,
125):
  posembed            relu(pe(a)), both buffers border-free (2 bytes of HBM traffic per element, plus a table that stays in L2)
  posembed_block      the same with the result bordered by 1 and re-biased, as a padded conv behind it wants it
  add                 i8ie_add_u8_nhwc on the same a with an equal-shape u8 b: the yardstick, it moves three bytes per element
  add_block           ... with the result bordered by 1 and re-biased
  relu_u8             the existing streaming kernel over the result's bytes, for scale
The aim is posembed / add <= 1.03 and posembed_block / add_block <= 1.03 (the project's +-3 % spread), each marked met / MISSED.
In the class form the Add runs on the input's h x w map and the embedding writes one more token per image.  Timing is the
library's own per-launch HIP-event bracket (i8ie_profile_start / _stop), the method of tools/bench_mul.py: `warmup` launches
unprofiled, then `rounds` rounds of `iters` profiled launches; a round's figure is its mean per launch, the reported one the median
over rounds.  The kernels go through the C-ABI by ctypes only.

Then the step time of examples/vit_cifar10.py's network at the same two batch sizes through the Python surface, with the share of
the kernel time its posembed launch and its activation lookups take."""
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

SHAPES = [("c192_8x8_class", 192, 8, 8, 1), ("c384_8x8_class", 384, 8, 8, 1), ("c64_32x32_plain", 64, 32, 32, 0), ("c768_4x4_class", 768, 4, 4, 1)]
BATCHES = [1000, 125]
AIM = 1.03


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F, B, L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64
    lib.i8ie_posembed_table.argtypes = [P, P, I, I, P]
    lib.i8ie_posembed_u8_nhwc.argtypes = [P, P, I, I, P, I, I, I, I, I, I, I, P, F, B, F, B, I]
    lib.i8ie_add_u8_nhwc.argtypes = [P, P, I, I, P, I, I, P, I, I, I, I, I, I, F, B, F, B, F, B, I]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_posembed.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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
    aq = (s_in, zp_in, 0.031, 131, s_out, zp_out)   # the Add's second operand into the same output parameters
    results = []
    for name, c, h, w, cls in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            f32 = np.float32
            tokens = h * w + cls
            n_in, n_out = m * c * h * w, m * c * tokens
            oh, ow = (1, tokens) if cls else (h, w)
            table = rng.normal(0, 0.5, (tokens, c)).astype(f32)
            token = rng.normal(0, 0.5, c).astype(f32)
            ck(lib.i8ie_posembed_table(table.ctypes.data, token.ctypes.data if cls else None, tokens, c, table.ctypes.data))
            da = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            dbb = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            de = put(table)
            do, dob = empty(n_out), empty(m * (oh + 2) * (ow + 2) * c)
            dadd, daddb = empty(n_in), empty(m * (h + 2) * (w + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, c, oh, ow, 1, zp_out ^ 0x80))
            ck(lib.i8ie_fill_border_u8(ctx, daddb, m, c, h, w, 1, zp_out ^ 0x80))
            pe_bytes = (n_in + n_out + 4.0 * tokens * c) / n_out
            legs = {
                "posembed": (pe_bytes, n_out, lambda: ck(lib.i8ie_posembed_u8_nhwc(ctx, da, 0, 0, do, 0, 0, m, c, h, w, cls, de, s_in, zp_in, s_out, zp_out, 1))),
                "posembed_block": (pe_bytes, n_out, lambda: ck(lib.i8ie_posembed_u8_nhwc(ctx, da, 0, 0, dob, 1, 1, m, c, h, w, cls, de, s_in, zp_in, s_out, zp_out, 1))),
                "add": (3, n_in, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, da, 0, 0, dbb, 0, 0, dadd, 0, 0, m, c, h, w, *aq, 1))),
                "add_block": (3, n_in, lambda: ck(lib.i8ie_add_u8_nhwc(ctx, da, 0, 0, dbb, 0, 0, daddb, 1, 1, m, c, h, w, *aq, 1))),
                "relu_u8": (2, n_out, lambda: ck(lib.i8ie_relu_u8(ctx, do, do, n_out, zp_out))),
            }
            row = {"shape": name, "images": m, "c": c, "h": h, "w": w, "class_token": cls, "elements_in": n_in, "elements_out": n_out}
            for tag, (bytes_per_el, n, fn) in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": bytes_per_el,
                            "gb_per_s": bytes_per_el * n / (ms * 1e-3) / 1e9}
            row["posembed_time_over_add_time"] = row["posembed"]["ms"] / row["add"]["ms"]
            row["posembed_block_time_over_add_block_time"] = row["posembed_block"]["ms"] / row["add_block"]["ms"]
            row["posembed_time_over_relu_time"] = row["posembed"]["ms"] / row["relu_u8"]["ms"]
            row["aim"] = AIM
            row["flat"] = "met" if row["posembed_time_over_add_time"] <= AIM else "MISSED"
            row["block"] = "met" if row["posembed_block_time_over_add_block_time"] <= AIM else "MISSED"
            for d in (da, dbb, de, do, dob, dadd, daddb):
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

    spec = importlib.util.spec_from_file_location("vit_cifar10", os.path.join(ROOT, "examples", "vit_cifar10.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    net = example.make_model(i8ie)
    net.load(example.synthetic_state_dict())
    net.prepare()
    net(i8ie.tensor(np.random.default_rng(1234).uniform(-1, 1, (64, 3, 32, 32)).astype(np.float32)))
    net.convert()
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(5).uniform(-1, 1, (m, 3, 32, 32)).astype(np.float32)).prefetch()
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
        total = sum(v[1] for v in prof.values()) / args.net_steps
        by, launches = {}, {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
            launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0] / args.net_steps
        pe_ms = sum(v for k, v in by.items() if k.startswith("posembed_"))
        lut_ms = sum(v for k, v in by.items() if k.startswith("lut_u8"))
        rows.append({"network": "examples/vit_cifar10.py", "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total,
                     "images_per_s_wall": m / (wall * 1e-3), "posembed_ms_per_step": pe_ms, "posembed_share_of_kernel_time": pe_ms / total,
                     "activation_lookup_ms_per_step": lut_ms, "activation_lookup_share_of_kernel_time": lut_ms / total,
                     "launches_per_step": launches, "kernel_ms_per_step_by_name": by})
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
    out = {"tool": "bench_posembed", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
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
