"""The quantized channel concatenation against the streaming kernels the library already had.

    python tools/bench_concat.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r09_bench_concat.json]

relu(cat(a, b)) per shape ([N, 64+64, 56, 56] and [N, 128+128, 13, 13], NHWC) and batch size (1000, 125), in four forms:
  copy      both inputs already in the result's quantisation (the copy rule: bytes only)
  one       a copied, b requantised (three unrelated scales)
  both      both requantised
  replay    equal scales, different zero points: every value sits on a rounding boundary and the kernel replays the exact
            sequence for all of them (its slowest case)
  odd       both requantised with c - 1 and c + 1 channels (odd counts: 1-byte items, every byte through the exact
            sequence with its IEEE division; flat only) -- what a concat of channel counts that are no multiple of 4 costs
each of the first four flat (every buffer border-free and plain: the run form) and as a fire module runs it (`_block`: the inputs
border-free and plain, the result bordered by 1 and re-biased for a following 3x3 conv), beside
  relu_u8   the existing kernel over the same number of output bytes
All of them move 2 bytes of HBM traffic per element (1 read + 1 write).  Timing is the library's own per-launch HIP-event
bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then `rounds` rounds of `iters` profiled launches; a
round's figure is its mean per launch, the reported one the median over rounds.  GB/s = algorithmic HBM bytes / that time.
The yardstick is relu_u8's byte rate in the same run.  This part goes through the C-ABI by ctypes only.

Then the step time of squeezenet_cifar at the same two batch sizes through the Python surface, with the share of the
profiled kernel time its concat launches take (`--net-steps 0` skips it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("c64+64_56x56", 64, 56, 56), ("c128+128_13x13", 128, 13, 13)]
BATCHES = [1000, 125]


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F, B, L = C.c_void_p, C.c_int, C.c_float, C.c_uint8, C.c_int64
    lib.i8ie_concat_u8_nhwc.argtypes = [P, I, P, P, P, P, P, P, P, I, I, I, I, I, F, B, I]
    lib.i8ie_relu_u8.argtypes = [P, P, P, L, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_concat.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    s_out, zp_out = 0.061, 97
    forms = {  # (s_a, zp_a), (s_b, zp_b)
        "copy": ((s_out, zp_out), (s_out, zp_out)),
        "one": ((s_out, zp_out), (0.027, 131)),
        "both": ((0.043, 119), (0.027, 131)),
        "replay": ((s_out, 96), (s_out, 99)),
    }
    results = []
    for name, c, h, w in SHAPES:
        for m in BATCHES:
            rng = np.random.default_rng(m + c)
            n = m * 2 * c * h * w  # output elements
            da = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            db = put(rng.integers(0, 256, (m, h, w, c), dtype=np.uint8))
            dr = put(rng.integers(0, 256, n, dtype=np.uint8))
            do, dob = empty(n), empty(m * (h + 2) * (w + 2) * 2 * c)
            ck(lib.i8ie_fill_border_u8(ctx, dob, m, 2 * c, h, w, 1, zp_out ^ 0x80))
            ins, cs, zeros = (P * 2)(da, db), (I * 2)(c, c), (I * 2)(0, 0)

            def cat(form, block):
                (sa, za), (sb, zb) = forms[form]
                s_in, zp_in = (F * 2)(sa, sb), (B * 2)(za, zb)
                out, ob = (dob, 1) if block else (do, 0)
                return lambda: ck(lib.i8ie_concat_u8_nhwc(ctx, 2, ins, cs, zeros, zeros, s_in, zp_in, out, ob, ob, m, h, w, s_out,
                                                          zp_out, 1))

            legs = {"relu_u8": lambda: ck(lib.i8ie_relu_u8(ctx, dr, do, n, zp_out))}
            for form in forms:
                legs["cat_relu_" + form] = cat(form, False)
                legs["cat_relu_" + form + "_block"] = cat(form, True)
            # odd channel counts: byte items and the exact sequence for every byte
            dao = put(rng.integers(0, 256, (m, h, w, c - 1), dtype=np.uint8))
            dbo = put(rng.integers(0, 256, (m, h, w, c + 1), dtype=np.uint8))
            ins_o, cs_o = (P * 2)(dao, dbo), (I * 2)(c - 1, c + 1)
            s_o, zp_o = (F * 2)(0.043, 0.027), (B * 2)(119, 131)
            legs["cat_relu_odd"] = lambda: ck(lib.i8ie_concat_u8_nhwc(ctx, 2, ins_o, cs_o, zeros, zeros, s_o, zp_o, do, 0, 0, m, h, w,
                                                                      s_out, zp_out, 1))
            row = {"shape": name, "images": m, "c": [c, c], "h": h, "w": w, "elements": n}
            for tag, fn in legs.items():
                ms, per_round = timed(fn)
                row[tag] = {"ms": ms, "ms_per_round": per_round, "bytes_per_element": 2, "gb_per_s": 2 * n / (ms * 1e-3) / 1e9}
            for tag in legs:
                if tag != "relu_u8":
                    row[tag]["over_relu_byte_rate"] = row[tag]["gb_per_s"] / row["relu_u8"]["gb_per_s"]
            for d in (da, db, dr, do, dob, dao, dbo):
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

    name = "squeezenet_cifar"
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
        cat = sum(v[1] for k, v in prof.items() if k.startswith("concat_"))
        rows.append({"network": name, "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                     "concat_ms_per_step": cat / args.net_steps, "concat_share_of_kernel_time": cat / total,
                     "concat_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("concat_")) / args.net_steps})
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
    out = {"tool": "bench_concat", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
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
