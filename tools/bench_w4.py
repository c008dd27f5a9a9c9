"""4-bit against 8-bit weights for Linear, in one process (one GPU).

    python tools/bench_w4.py [--steps 200] [--warmup 20] [--rounds 3] [--acc-images 500] [--out profiles/r29_bench_w4.json]

Speed: a per-channel INT8 Linear and a 4-bit Linear of the same shape (fc6, fc7, 768 -> 3072) at 1, 16, 125 and 1000 rows.
The two layers alternate over `--rounds` rounds; a round times `--steps` forwards of each with the library's HIP-event
profiler (every kernel of the forward, quantize excluded: the input is a resident u8 tensor) and the median per-forward
device time is reported, with the bytes per second that is over the packed panel.  Footprint: i8ie memory_stats around
creating an fc6 handle in both forms.  Accuracy: AlexNet on the row-scaled synthetic weights of tools/bench_per_channel.py,
per-tensor, per-channel and 4-bit fc layers with per-channel convs, each against the FP32 model.  Writes one JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("fc6", 9216, 4096), ("fc7", 4096, 4096), ("mlp_768_3072", 768, 3072)]
ROWS = [1, 16, 125, 1000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--acc-images", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_bench_w4.json"))
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    if not torch.cuda.is_available():
        sys.exit("bench_w4.py: no GPU visible")
    cx.set_device(0)
    rng = np.random.default_rng(4)

    def layers(k, n):
        """(INT8 per-channel, 4-bit) from the same FP32 weights; (live bytes each handle added)"""
        w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
        b = (rng.standard_normal(n) * 0.05).astype(np.float32)
        made, grew = [], []
        for bits in (8, 4):
            lin = i8ie.Linear(k, n)
            lin.load_weight(w)
            lin.load_bias(b)
            lin.set_output_qparams(0.5, 128)
            cx.synchronize()
            before = cx.memory_stats()[0]
            lin.convert(per_channel=True, weight_bits=bits)
            cx.synchronize()
            grew.append(int(cx.memory_stats()[0] - before))
            made.append(lin)
        return made, grew

    def device_us(lin, x):
        """median-ready: device time of one forward, every kernel it launches"""
        for _ in range(args.warmup):
            lin(x).data.layout()
        cx.synchronize()
        cx.profile_start()
        for _ in range(args.steps):
            lin(x).data.layout()
        prof = cx.profile_stop()
        return 1e3 * sum(v[1] for v in prof.values()) / args.steps, sorted({k.split("|")[0] for k in prof})

    speed, footprint = [], None
    for name, k, n in SHAPES:
        (l8, l4), grew = layers(k, n)
        if name == "fc6":
            footprint = {"int8_per_channel_bytes": grew[0], "w4_bytes": grew[1], "ratio": grew[1] / grew[0],
                         "w4_panel_bytes": n * k // 2, "w4_vectors_bytes": grew[1] - n * k // 2}
        for m in ROWS:
            q = rng.integers(0, 256, (m, k)).astype(np.float32)
            x = i8ie.Tensor(cx.quantize(cx.tensor(q), 1.0, 0))
            x.data.layout()
            t8, t4, k8, k4 = [], [], None, None
            for _ in range(args.rounds):
                us, k8 = device_us(l8, x)
                t8.append(us)
                us, k4 = device_us(l4, x)
                t4.append(us)
            u8, u4 = statistics.median(t8), statistics.median(t4)
            speed.append({"shape": name, "k": k, "n": n, "rows": m, "int8_us": u8, "w4_us": u4, "w4_over_int8": u4 / u8,
                          "aim_1.03": "met" if u4 <= 1.03 * u8 else "MISSED", "w4_panel_GBps": (n * k / 2) / (u4 * 1e-6) / 1e9,
                          "int8_kernels": k8, "w4_kernels": k4, "per_round_us": {"int8": t8, "w4": t4}})
        del l8, l4
        cx.trim()

    # accuracy on row-scaled weights (tools/bench_per_channel.py's construction)
    name = "alexnet"
    sd = wl.synthetic_state_dict(name, seed=42)
    rs = np.random.default_rng(7)
    sd_rows = dict(sd)
    for a in wl.layer_names(name):
        f = np.exp(rs.uniform(np.log(1.0 / 30), 0.0, sd[a + ".weight"].shape[0])).astype(np.float32)
        sd_rows[a + ".weight"] = (sd[a + ".weight"] * f.reshape((-1,) + (1,) * (sd[a + ".weight"].ndim - 1))).astype(np.float32)
        sd_rows[a + ".bias"] = (sd[a + ".bias"] * f).astype(np.float32)
    x = wl.synthetic_input(name, args.acc_images, seed=2024)
    fp = wl.build(name)
    fp.load(sd_rows)
    ref = fp(i8ie.tensor(x)).numpy()
    acc = {}
    for form, kw in (("per_tensor", {}), ("per_channel", {"per_channel": True}),
                     ("w4_fc_per_channel_convs", {"per_channel": True, "weight_bits": 4})):
        y = wl.calibrated(name, sd_rows, **kw)(i8ie.tensor(x)).numpy()
        acc[form] = {"top1_agreement_with_fp32": float((y.argmax(1) == ref.argmax(1)).mean()),
                     "mean_abs_logit_error": float(np.abs(y - ref).mean())}

    out = {"tool": "bench_w4", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "speed": speed,
           "footprint_fc6": footprint, "accuracy_row_scaled_weights": dict(acc, images=args.acc_images),
           "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "speed": [(s["shape"], s["rows"], round(s["int8_us"], 2), round(s["w4_us"], 2)) for s in speed]}))


if __name__ == "__main__":
    main()
