"""One observe of the histogram calibrator against i8ie_relu_f32 over the same elements, and the calibration forward of AlexNet
under the reservoir and under a histogram observer.

    python tools/bench_calib_hist.py [--iters 20] [--rounds 5] [--warmup 5] [--forward-reps 5] [--out profiles/r23_bench_calib_hist.json]

Per shape (AlexNet's conv1 and conv3 outputs at 100 images, and 1000 x 64 x 16 x 16) and kind of data:
  gaussian      N(0, 1): the bins spread over a few hundred counters
  half_zeros    max(N(0, 1), 0): what a ReLU leaves, half of the values in one bin
  all_equal     one value: every lane of every wave on one counter, the worst contention
i8ie_calib_hist_observe_f32 (two launches: calib_hist_stats, calib_hist_count) and i8ie_relu_f32 both move 8 bytes per element
(two reads against a read and a write), so the aim is observe / relu_f32 <= 1.03, the project's 3 % spread; every row prints met or
MISSED.  Timing is a pair of HIP events on the ctx stream around `iters` back-to-back calls, in one process, the two legs
alternating round by round: a round's figure is its mean per call, the reported one the median over rounds.  The state is reset
once per leg, outside the timed region (the exponent is then the same in every call, and nothing folds).

Then the 100-image AlexNet calibration forward (prepare, one FP32 forward that every layer observes; the method of
tools/calib_time.py), reservoir in device mode against the histogram observer, alternating: wall time of the forward, and the
time and launches of the calibration kernels inside it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("alexnet_conv1_100", (100, 64, 55, 55)), ("alexnet_conv3_100", (100, 384, 13, 13)), ("c64_16x16_1000", (1000, 64, 16, 16))]
AIM = 1.03


def kernels(args):
    lib = C.CDLL(args.lib)
    hip = C.CDLL("libamdhip64.so")
    lib.i8ie_last_error.restype = C.c_char_p
    lib.i8ie_ctx_stream.restype = C.c_void_p
    lib.i8ie_calib_hist_state_bytes.restype = C.c_size_t
    P, L = C.c_void_p, C.c_int64
    lib.i8ie_ctx_stream.argtypes = [P]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_relu_f32.argtypes = [P, P, P, L]
    lib.i8ie_calib_hist_reset.argtypes = [P, P]
    lib.i8ie_calib_hist_observe_f32.argtypes = [P, P, L, P]
    hip.hipEventCreate.argtypes = [C.POINTER(P)]
    hip.hipEventRecord.argtypes = [P, P]
    hip.hipEventSynchronize.argtypes = [P]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), P, P]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_calib_hist.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))
    stream = P(lib.i8ie_ctx_stream(ctx))
    ev0, ev1 = P(), P()
    ck(hip.hipEventCreate(C.byref(ev0)))
    ck(hip.hipEventCreate(C.byref(ev1)))

    def round_ms(fn):
        ck(hip.hipEventRecord(ev0, stream))
        for _ in range(args.iters):
            fn()
        ck(hip.hipEventRecord(ev1, stream))
        ck(hip.hipEventSynchronize(ev1))
        ms = C.c_float()
        ck(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
        return ms.value / args.iters

    state = P()
    ck(lib.i8ie_malloc(ctx, lib.i8ie_calib_hist_state_bytes(), C.byref(state)))
    results = []
    for name, shape in SHAPES:
        n = int(np.prod(shape))
        g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        data = {"gaussian": g, "half_zeros": np.maximum(g, 0), "all_equal": np.full(n, 3.7, np.float32)}
        dx, do = P(), P()
        ck(lib.i8ie_malloc(ctx, 4 * n, C.byref(dx)))
        ck(lib.i8ie_malloc(ctx, 4 * n, C.byref(do)))
        for kind, x in data.items():
            ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), 4 * n))
            ck(lib.i8ie_calib_hist_reset(ctx, state))
            legs = {"observe": lambda: ck(lib.i8ie_calib_hist_observe_f32(ctx, dx, n, state)),
                    "relu_f32": lambda: ck(lib.i8ie_relu_f32(ctx, dx, do, n))}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            ck(lib.i8ie_sync(ctx))
            per_round = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    per_round[k].append(round_ms(fn))
            row = {"shape": name, "dims": list(shape), "elements": n, "data": kind, "aim": AIM}
            for k in legs:
                ms = statistics.median(per_round[k])
                row[k] = {"ms": ms, "ms_per_round": per_round[k], "gb_per_s": 8.0 * n / (ms * 1e-3) / 1e9}
            row["observe_time_over_relu_time"] = row["observe"]["ms"] / row["relu_f32"]["ms"]
            row["verdict"] = "met" if row["observe_time_over_relu_time"] <= AIM else "MISSED"
            results.append(row)
            print(json.dumps(row), flush=True)
        ck(lib.i8ie_free(ctx, dx))
        ck(lib.i8ie_free(ctx, do))
    ck(lib.i8ie_free(ctx, state))
    lib.i8ie_ctx_destroy(ctx)
    return results


def calibration_forward(args):
    sys.path.insert(0, ROOT)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    sd = wl.synthetic_state_dict("alexnet", seed=42)
    xt = i8ie.tensor(wl.synthetic_input("alexnet", 100, seed=7)).prefetch()
    rows = {"reservoir_device": [], "histogram": []}
    before = i8ie.calibration()
    cx.set_calibration_mode("device")
    try:
        for rep in range(args.forward_reps + 1):   # (the first repetition warms both up and is dropped)
            for leg in rows:
                i8ie.set_calibration("reservoir" if leg == "reservoir_device" else "minmax")
                net = wl.build("alexnet")
                net.load(sd)
                net(xt).numpy()
                net.prepare()
                cx.synchronize()
                cx.profile_start(False)
                t0 = time.perf_counter()
                net(xt).numpy()
                cx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                prof = cx.profile_stop()
                t0 = time.perf_counter()
                net.convert()
                cx.synchronize()
                convert = (time.perf_counter() - t0) * 1e3
                calib = {k.split("|")[0]: 0.0 for k in prof if k.startswith("calib_")}
                launches = dict.fromkeys(calib, 0)
                for k, v in prof.items():
                    if k.startswith("calib_"):
                        calib[k.split("|")[0]] += v[1]
                        launches[k.split("|")[0]] += v[0]
                if rep:
                    rows[leg].append({"forward_ms_wall_profiled": wall, "convert_ms_wall": convert, "kernel_ms": sum(v[1] for v in prof.values()),
                                      "calibration_kernel_ms": sum(calib.values()), "calibration_kernel_ms_by_name": calib,
                                      "calibration_launches": launches})
    finally:
        cx.set_calibration_mode("auto")
        i8ie.set_calibration(before["method"], before["percentile"])
    out = {}
    for leg, reps in rows.items():
        out[leg] = {"repetitions": reps}
        for key in ("forward_ms_wall_profiled", "convert_ms_wall", "kernel_ms", "calibration_kernel_ms"):
            out[leg][key + "_median"] = statistics.median(r[key] for r in reps)
        print(json.dumps({"calibration_forward": leg, **{k: v for k, v in out[leg].items() if k != "repetitions"},
                          "launches": reps[-1]["calibration_launches"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forward-reps", type=int, default=5)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_calib_hist", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "HIP events around `iters` back-to-back calls; median over rounds of the per-round mean per call",
           "results": kernels(args)}
    if args.forward_reps > 0:
        out["calibration_forward"] = calibration_forward(args)
    if args.out:
        prior = {}
        if os.path.exists(args.out):   # (tools/calib_accuracy.py writes its section into the same file)
            with open(args.out) as f:
                prior = json.load(f)
        prior["bench_calib_hist"] = out
        with open(args.out, "w") as f:
            json.dump(prior, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
