"""2:4 structured-sparse against dense 8-bit weights for pointwise Conv2d on NHWC token maps, in one process (one GPU).

    python tools/bench_sp24pw.py [--steps 200] [--warmup 20] [--rounds 3] [--out profiles/r34_bench_sp24pw.json]

The method and the shapes of tools/bench_w4pw.py.  Per shape a 2:4 1 x 1 Conv2d and a per-channel INT8 1 x 1 Conv2d loaded with
the same pruned integers read one resident NHWC u8 map [images, in, 1, tokens] (the output of a 1 x 1 conv ahead of them, launched
once); their bytes are asserted equal first.  The two layers alternate over `--rounds` rounds; a round times `--steps` forwards of
each with the library's HIP-event profiler and the median per-forward device time is reported against the aim sparse <= 1.03 x
INT8, beside the hoped-for ratios 0.625 (bytes, few pixels) and 0.5 (MFMA count, many pixels).  Footprint: i8ie memory_stats around
creating the 768 -> 3072 handle in both forms.  Writes one JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, in, out, tokens, images)
SHAPES = [(n, k, o, 65, imgs) for n, k, o in (("qkv_192_576", 192, 576), ("fc1_192_768", 192, 768), ("fc2_768_192", 768, 192))
          for imgs in (1, 16, 125, 1000)]
SHAPES += [(n, k, o, 197, imgs) for n, k, o in (("fc1_768_3072", 768, 3072), ("fc2_3072_768", 3072, 768)) for imgs in (1, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_bench_sp24pw.json"))
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie

    if not torch.cuda.is_available():
        sys.exit("bench_sp24pw.py: no GPU visible")
    cx.set_device(0)
    rng = np.random.default_rng(4)

    def conv(k, n, sparse, like=None):
        """(a converted 1 x 1 Conv2d, the live bytes its handle added); like: load that 2:4 layer's integers as dense INT8"""
        layer = i8ie.Conv2d(k, n, 1)
        cx.synchronize()
        before = cx.memory_stats()[0]
        if like is not None:
            layer.layer.load_quantized(like.layer.q_weight(), like.layer.q_bias(), like.weight_scales(), *like.output_qparams())
        else:
            layer.load_weight((rng.standard_normal((n, k, 1, 1)) * 0.05).astype(np.float32))
            layer.load_bias((rng.standard_normal(n) * 0.05).astype(np.float32))
            layer.set_output_qparams(0.5, 128)
            layer.convert(per_channel=True, conv_sparsity="2:4" if sparse else None)
        cx.synchronize()
        return layer, int(cx.memory_stats()[0] - before)

    def device_us(layer, x):
        for _ in range(args.warmup):
            layer(x).data.layout()
        cx.synchronize()
        cx.profile_start()
        for _ in range(args.steps):
            layer(x).data.layout()
        prof = cx.profile_stop()
        return 1e3 * sum(v[1] for v in prof.values()) / args.steps, sorted({k.split("|")[0] for k in prof})

    speed, footprint, made = [], None, {}
    for name, k, n, tokens, images in SHAPES:
        if name not in made:
            l4, b4 = conv(k, n, True)
            l8, b8 = conv(k, n, False, like=l4)
            made = {name: (l4, l8, conv(k, k, False)[0])}
            if name == "fc1_768_3072":
                footprint = {"int8_per_channel_bytes": b8, "sp24_bytes": b4, "ratio": b4 / b8, "sp24_panel_bytes": n * k * 5 // 8}
        l4, l8, ahead = made[name]
        q = rng.integers(0, 256, (images, k, 1, tokens)).astype(np.float32)
        x = ahead(i8ie.Tensor(cx.quantize(cx.tensor(q), 1.0, 0)))
        assert x.data.layout() == 1, "the map is not resident NHWC"
        assert np.array_equal(l8(x).numpy(), l4(x).numpy()), (name, images)
        t8, t4, k8, k4 = [], [], None, None
        for _ in range(args.rounds):
            us, k8 = device_us(l8, x)
            t8.append(us)
            us, k4 = device_us(l4, x)
            t4.append(us)
        u8, u4 = statistics.median(t8), statistics.median(t4)
        speed.append({"shape": name, "in": k, "out": n, "images": images, "rows": images * tokens, "int8_us": u8, "sp24_us": u4,
                      "sp24_over_int8": u4 / u8, "aim_1.03": "met" if u4 <= 1.03 * u8 else "MISSED",
                      "hoped_for": 0.625 if images * tokens <= 256 else 0.5, "int8_kernels": k8, "sp24_kernels": k4,
                      "per_round_us": {"int8": t8, "sp24": t4}})
        print(json.dumps({k_: speed[-1][k_] for k_ in ("shape", "rows", "int8_us", "sp24_us", "sp24_over_int8", "aim_1.03", "hoped_for", "int8_kernels", "sp24_kernels")}), flush=True)

    out = {"tool": "bench_sp24pw", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "speed": speed,
           "footprint_fc1_768_3072": footprint, "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
