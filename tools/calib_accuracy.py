"""What the calibration method does to a converted network's output: AlexNet, the CIFAR ResNet-18 and the CIFAR MobileNetV2 with
the synthetic weights and inputs of workloads, calibrated on one batch and evaluated on another, under the reservoir, minmax,
percentile 99.99, percentile 99.9 and mse.

    python tools/calib_accuracy.py [--eval-images 200] [--out profiles/r23_bench_calib_hist.json]

Per network and method: the mean |logit error| of the INT8 forward against the FP32 forward of the same weights, the same
relative to the mean |FP32 logit|, and the top-1 agreement with the FP32 forward.  Per network: the largest per-op ratio of the
output scales the reservoir and minmax chose (either way round), and the op that has it.  The weights are random, so the numbers
say how the methods differ on these value distributions, not how a trained network behaves."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("alexnet", "resnet18_cifar", "mobilenetv2_cifar")
METHODS = (("reservoir", None), ("minmax", "minmax"), ("percentile_99.99", ("percentile", 99.99)), ("percentile_99.9", ("percentile", 99.9)),
           ("mse", "mse"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-images", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    rows = []
    for name in NETS:
        sd = wl.synthetic_state_dict(name, 42)
        x = wl.synthetic_input(name, args.eval_images, seed=4321)
        fp = wl.build(name)
        fp.load(sd)
        ref = fp(i8ie.tensor(x)).numpy()
        ops = wl.layer_names(name) + wl.join_names(name)
        scales = {}
        for tag, calibration in METHODS:
            try:
                net = wl.calibrated(name, sd, calibration=calibration)
            finally:
                cx.set_calibration_seed(-1)
            got = net(i8ie.tensor(x)).numpy()
            scales[tag] = {a: getattr(net, a).output_qparams()[0] for a in ops}
            err = float(np.abs(got - ref).mean())
            row = {"network": name, "method": tag, "eval_images": args.eval_images, "mean_abs_logit_error": err,
                   "relative_to_mean_abs_logit": err / float(np.abs(ref).mean()),
                   "top1_agreement_with_fp32": float((got.argmax(1) == ref.argmax(1)).mean())}
            rows.append(row)
            print(json.dumps(row), flush=True)
        ratio = {a: max(scales["reservoir"][a] / scales["minmax"][a], scales["minmax"][a] / scales["reservoir"][a]) for a in ops}
        worst = max(ratio, key=ratio.get)
        row = {"network": name, "largest_scale_ratio_reservoir_vs_minmax": ratio[worst], "op": worst,
               "reservoir_scale": scales["reservoir"][worst], "minmax_scale": scales["minmax"][worst], "ops": len(ops)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        prior = {}
        if os.path.exists(args.out):   # (tools/bench_calib_hist.py writes its section into the same file)
            with open(args.out) as f:
                prior = json.load(f)
        prior["calib_accuracy"] = {"tool": "calib_accuracy", "eval_images": args.eval_images, "results": rows}
        with open(args.out, "w") as f:
            json.dump(prior, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
