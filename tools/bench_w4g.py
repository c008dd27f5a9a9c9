"""Group-wise against per-row scales for 4-bit Linear, in one process (one GPU).

    python tools/bench_w4g.py [--steps 200] [--warmup 20] [--rounds 3] [--acc-images 500] [--out profiles/r31_bench_w4g.json]

Speed: the method of tools/bench_w4.py.  A grouped 4-bit Linear (gs 128; also 64 on fc7) and the ungrouped 4-bit Linear on
the same nibbles (w4lin_mfma, the yardstick) at 1, 16, 125 and 1000 rows; the two alternate over `--rounds` rounds of `--steps`
forwards timed by the library's HIP-event profiler, median per-forward device time.  Before a shape is timed the grouped
layer's bytes at 16 rows are asserted equal to those of the definition kernel (force-fallback).  Footprint: i8ie memory_stats
around creating the fc6 handles.  Accuracy: AlexNet whose fc rows are heavy-tailed (every fc weight of the synthetic state
dict multiplied by |t|, t Student with 2 degrees of freedom, per weight), per-channel INT8, W4 and W4 with gs 128 and 64, each
against the FP32 model.  Random weights say little about a trained network.  Writes one JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("fc6", 9216, 4096, (128,)), ("fc7", 4096, 4096, (128, 64)), ("mlp_768_3072", 768, 3072, (128,)), ("mlp_3072_768", 3072, 768, (128,))]
ROWS = [1, 16, 125, 1000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--acc-images", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_bench_w4g.json"))
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    if not torch.cuda.is_available():
        sys.exit("bench_w4g.py: no GPU visible")
    cx.set_device(0)
    rng = np.random.default_rng(4)

    def handle(k, n, load):
        """(a Linear loaded by `load`, the live bytes its handle added)"""
        lin = i8ie.Linear(k, n)
        cx.synchronize()
        before = cx.memory_stats()[0]
        load(lin.layer)
        cx.synchronize()
        return lin, int(cx.memory_stats()[0] - before)

    def device_us(lin, x):
        for _ in range(args.warmup):
            lin(x).data.layout()
        cx.synchronize()
        cx.profile_start()
        for _ in range(args.steps):
            lin(x).data.layout()
        prof = cx.profile_stop()
        return 1e3 * sum(v[1] for v in prof.values()) / args.steps, sorted({k.split("|")[0] for k in prof})

    def u8(rows, k):
        x = i8ie.Tensor(cx.quantize(cx.tensor(rng.integers(0, 256, (rows, k)).astype(np.float32)), 1.0, 0))
        x.data.layout()
        return x

    speed, footprint = [], {}
    for name, k, n, sizes in SHAPES:
        packed = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
        qb, s_w = rng.integers(-127, 128, n, dtype=np.int8), np.full(n, 2e-4, np.float32)
        flat, grew_flat = handle(k, n, lambda L: L._load_quantized_w4(packed, qb, s_w * 16, 0.5, 128))
        for gs in sizes:
            m = rng.integers(1, 33, (n, -(-k // gs)), dtype=np.uint8)
            grouped, grew = handle(k, n, lambda L: L._load_quantized_w4g(packed, m, gs, qb, s_w, 0.5, 128))
            if name == "fc6":
                footprint = {"w4_bytes": grew_flat, "w4g_bytes": grew, "ratio": grew / grew_flat, "group_size": gs}
            x = u8(16, k)
            fast = grouped(x).numpy()
            cx.force_fallback(True)
            try:
                assert np.array_equal(grouped(x).numpy(), fast), (name, gs, "bytes differ from the definition kernel")
            finally:
                cx.force_fallback(False)
            for rows in ROWS:
                x = u8(rows, k)
                tf, tg, kf, kg = [], [], None, None
                for _ in range(args.rounds):
                    us, kf = device_us(flat, x)
                    tf.append(us)
                    us, kg = device_us(grouped, x)
                    tg.append(us)
                uf, ug = statistics.median(tf), statistics.median(tg)
                speed.append({"shape": name, "k": k, "n": n, "group_size": gs, "rows": rows, "w4_us": uf, "w4g_us": ug, "w4g_over_w4": ug / uf,
                              "aim_1.03": "met" if ug <= 1.03 * uf else "MISSED", "w4_kernels": kf, "w4g_kernels": kg,
                              "per_round_us": {"w4": tf, "w4g": tg}})
            del grouped
        del flat
        cx.trim()

    name = "alexnet"
    sd = dict(wl.synthetic_state_dict(name, seed=42))
    rs = np.random.default_rng(7)
    for a in wl.layer_names(name):
        if sd[a + ".weight"].ndim == 2:
            sd[a + ".weight"] = (sd[a + ".weight"] * np.abs(rs.standard_t(2, sd[a + ".weight"].shape))).astype(np.float32)
    x = wl.synthetic_input(name, args.acc_images, seed=2024)
    fp = wl.build(name)
    fp.load(sd)
    ref = fp(i8ie.tensor(x)).numpy()
    acc = {}
    for form, kw in (("per_channel_int8", {}), ("w4", {"weight_bits": 4}), ("w4_gs128", {"weight_bits": 4, "group_size": 128}),
                     ("w4_gs64", {"weight_bits": 4, "group_size": 64})):
        y = wl.calibrated(name, sd, per_channel=True, **kw)(i8ie.tensor(x)).numpy()
        acc[form] = {"top1_agreement_with_fp32": float((y.argmax(1) == ref.argmax(1)).mean()),
                     "mean_abs_logit_error": float(np.abs(y - ref).mean())}

    out = {"tool": "bench_w4g", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "speed": speed,
           "footprint_fc6": footprint, "accuracy_heavy_tailed_fc_rows": dict(acc, images=args.acc_images),
           "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "speed": [(s["shape"], s["group_size"], s["rows"], round(s["w4_us"], 2), round(s["w4g_us"], 2)) for s in speed],
                      "footprint": footprint, "accuracy": acc}))


if __name__ == "__main__":
    main()
