"""2:4 structured-sparse against dense 8-bit weights for Linear, in one process (one GPU).

    python tools/bench_sparse24.py [--steps 200] [--warmup 20] [--rounds 3] [--out profiles/r30_bench_sparse24.json]

Speed: a per-channel INT8 Linear loaded with the pruned dense integers (the yardstick) and the 2:4 Linear holding the same
integers, for fc6, fc7, 768 -> 3072 and 3072 -> 768 at 1, 16, 125 and 1000 rows.  The two layers alternate over `--rounds`
rounds; a round times `--steps` forwards of each with the library's HIP-event profiler (every kernel of the forward; the input
is a resident u8 tensor) and the median per-forward device time is reported.  The outputs are compared byte for byte at every
timed size.  Footprint: i8ie memory_stats around creating an fc6 handle in both forms.  Writes one JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("fc6", 9216, 4096), ("fc7", 4096, 4096), ("mlp_768_3072", 768, 3072), ("mlp_3072_768", 3072, 768)]
ROWS = [1, 16, 125, 1000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_bench_sparse24.json"))
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie

    if not torch.cuda.is_available():
        sys.exit("bench_sparse24.py: no GPU visible")
    cx.set_device(0)
    rng = np.random.default_rng(4)

    def layers(k, n):
        """(INT8 per-channel on the pruned integers, 2:4) from the same FP32 weights; (live bytes each handle added)"""
        w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
        b = (rng.standard_normal(n) * 0.05).astype(np.float32)
        sparse = i8ie.Linear(k, n)
        sparse.load_weight(w)
        sparse.load_bias(b)
        sparse.set_output_qparams(0.5, 128)
        cx.synchronize()
        before = cx.memory_stats()[0]
        sparse.convert(per_channel=True, sparsity="2:4")
        cx.synchronize()
        grew = [int(cx.memory_stats()[0] - before)]
        dense = i8ie.Linear(k, n)
        before = cx.memory_stats()[0]
        dense.load_quantized(sparse.layer.q_weight(), sparse.layer.q_bias(), sparse.weight_scales(), 0.5, 128)
        cx.synchronize()
        grew.insert(0, int(cx.memory_stats()[0] - before))
        return (dense, sparse), grew

    def device_us(lin, x):
        """device time of one forward, every kernel it launches"""
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
        (l8, ls), grew = layers(k, n)
        if name == "fc6":
            footprint = {"int8_per_channel_bytes": grew[0], "sparse24_bytes": grew[1], "ratio": grew[1] / grew[0],
                         "sparse24_panel_bytes": n * k * 5 // 8, "sparse24_vectors_bytes": grew[1] - n * k * 5 // 8}
        for m in ROWS:
            q = rng.integers(0, 256, (m, k)).astype(np.float32)
            x = i8ie.Tensor(cx.quantize(cx.tensor(q), 1.0, 0))
            x.data.layout()
            same = bool(np.array_equal(l8(x).numpy(), ls(x).numpy()))
            t8, ts, k8, ks = [], [], None, None
            for _ in range(args.rounds):
                us, k8 = device_us(l8, x)
                t8.append(us)
                us, ks = device_us(ls, x)
                ts.append(us)
            u8, us_ = statistics.median(t8), statistics.median(ts)
            hoped = 0.625 if m <= 16 else 0.5  # the byte argument at few rows, the MFMA count at many
            speed.append({"shape": name, "k": k, "n": n, "rows": m, "int8_us": u8, "sparse24_us": us_, "sparse24_over_int8": us_ / u8,
                          "aim_1.03": "met" if us_ <= 1.03 * u8 else "MISSED", "hoped_for_ratio": hoped, "bytes_equal": same,
                          "sparse24_panel_GBps": (n * k * 0.625) / (us_ * 1e-6) / 1e9, "int8_kernels": k8, "sparse24_kernels": ks,
                          "per_round_us": {"int8": t8, "sparse24": ts}})
        del l8, ls
        cx.trim()

    out = {"tool": "bench_sparse24", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "speed": speed,
           "footprint_fc6": footprint, "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "speed": [(s["shape"], s["rows"], round(s["int8_us"], 2), round(s["sparse24_us"], 2), s["bytes_equal"])
                                                   for s in speed]}))


if __name__ == "__main__":
    main()
