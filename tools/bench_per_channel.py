"""Per-tensor against per-channel weight scales, in one process (one GPU).

    python tools/bench_per_channel.py [--steps 50] [--warmup 10] [--acc-images 500]

Timing: the AlexNet step at 1000 images (eager, pipelined depth 2: the default run of bench.py) and the 125-image step
replayed as a HIP graph, both modes built from the same synthetic weights; the modes alternate over `--rounds` rounds and
the median step time of each is reported.  Accuracy: AlexNet on synthetic weights whose output rows (and bias) are
scaled log-uniformly over [1/30, 1], each mode against the FP32 model on the same images: top-1 agreement and mean
|logit error|.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--acc-images", type=int, default=500)
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl
    from int8inferenceengine_amd.graph import GraphedForward

    if not torch.cuda.is_available():
        sys.exit("bench_per_channel.py: no GPU visible")
    cx.set_device(0)
    name = "alexnet"
    sd = wl.synthetic_state_dict(name, seed=42)

    def steps(fn, k):  # pipelined depth 2, as bench.py's default run
        pending = None
        for _ in range(k):
            h = fn()
            if pending is not None:
                pending.result()
            pending = h
        if pending is not None:
            pending.result()

    def time_step(fn):
        steps(fn, args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(fn, args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    setups = {}
    for pc in (False, True):
        net = wl.calibrated(name, sd, per_channel=pc)
        x1000 = i8ie.tensor(wl.synthetic_input(name, 1000, seed=1234)).prefetch()
        g125 = GraphedForward(net, i8ie.tensor(wl.synthetic_input(name, 125, seed=1234)).prefetch())
        setups[pc] = (net, x1000, g125)
    cx.synchronize()
    t1000 = {False: [], True: []}
    t125 = {False: [], True: []}
    for _ in range(args.rounds):
        for pc in (False, True):
            net, x1000, g125 = setups[pc]
            t1000[pc].append(time_step(lambda: net(x1000).numpy_async()))
            t125[pc].append(time_step(lambda: g125().numpy_async()))
    del setups
    cx.trim()

    # accuracy on row-scaled weights
    rng = np.random.default_rng(7)
    sd_rows = {}
    for k, v in sd.items():
        sd_rows[k] = v
    for a in wl.layer_names(name):
        f = np.exp(rng.uniform(np.log(1.0 / 30), 0.0, sd[a + ".weight"].shape[0])).astype(np.float32)
        sd_rows[a + ".weight"] = (sd[a + ".weight"] * f.reshape((-1,) + (1,) * (sd[a + ".weight"].ndim - 1))).astype(np.float32)
        sd_rows[a + ".bias"] = (sd[a + ".bias"] * f).astype(np.float32)
    x = wl.synthetic_input(name, args.acc_images, seed=2024)
    fp = wl.build(name)
    fp.load(sd_rows)
    ref = fp(i8ie.tensor(x)).numpy()
    acc = {}
    for pc in (False, True):
        net = wl.calibrated(name, sd_rows, per_channel=pc)
        y = net(i8ie.tensor(x)).numpy()
        acc[pc] = {"top1_agreement_with_fp32": float((y.argmax(1) == ref.argmax(1)).mean()),
                   "mean_abs_logit_error": float(np.abs(y - ref).mean())}

    med = statistics.median
    out = {
        "tool": "bench_per_channel", "network": name, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "step_ms_1000_eager": {"per_tensor": med(t1000[False]), "per_channel": med(t1000[True]),
                               "overhead_pct": 100.0 * (med(t1000[True]) / med(t1000[False]) - 1.0),
                               "per_round": {"per_tensor": t1000[False], "per_channel": t1000[True]}},
        "step_ms_125_graph": {"per_tensor": med(t125[False]), "per_channel": med(t125[True]),
                              "overhead_pct": 100.0 * (med(t125[True]) / med(t125[False]) - 1.0),
                              "per_round": {"per_tensor": t125[False], "per_channel": t125[True]}},
        "accuracy_row_scaled_weights": {"images": args.acc_images, "row_scale_range": [1.0 / 30, 1.0],
                                        "per_tensor": acc[False], "per_channel": acc[True]},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
