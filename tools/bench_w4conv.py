"""4-bit against 8-bit weights for k x k Conv2d on NHWC maps, in one process (one GPU).

    python tools/bench_w4conv.py [--steps 200] [--warmup 20] [--rounds 3] [--out profiles/r33_bench_w4conv.json]

The method of tools/bench_w4pw.py.  Per shape a 4-bit Conv2d (Layer.convert(weight_bits=4, spatial=True)) and a per-channel INT8
Conv2d loaded with the same integers read one resident NHWC u8 map (the output of a 3 x 3 conv ahead of them, launched once,
with the border both ask for); their bytes are asserted equal first.  The two layers alternate over `--rounds` rounds; a round
times `--steps` forwards of each with the library's HIP-event profiler and the median per-forward device time is reported
against the aim W4 <= 1.03 x INT8.  Footprint: i8ie memory_stats around creating the 512 -> 512 3 x 3 handle in both forms.
resnet18_cifar: device time per forward of 100 images and the live bytes its conversion adds, INT8 against spatial=True, and the
top-1 agreement of both with the FP32 model over 500 synthetic images (random weights: says little).  Writes one JSON file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, in, out, k, stride, pad, map, images)
SHAPES = [("c%d_3x3_%d" % (c, hw), c, c, 3, 1, 1, hw, imgs) for c, hw in ((64, 32), (128, 16), (256, 8), (512, 4)) for imgs in (1000, 125)]
SHAPES += [("down_128_256_3x3s2", 128, 256, 3, 2, 1, 16, imgs) for imgs in (1000, 125)]
SHAPES += [("short_128_256_1x1s2", 128, 256, 1, 2, 0, 16, imgs) for imgs in (1000, 125)]
SHAPES += [("c64_3x3_56", 64, 64, 3, 1, 1, 56, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_bench_w4conv.json"))
    args = ap.parse_args()

    import numpy as np

    import torch  # first: libi8ie_hip.so binds to the HIP runtime torch loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    if not torch.cuda.is_available():
        sys.exit("bench_w4conv.py: no GPU visible")
    cx.set_device(0)
    rng = np.random.default_rng(4)

    def conv(c, n, k, stride, pad, bits, like=None):
        """(a converted Conv2d, the live bytes its handle added); like: load that 4-bit layer's integers as INT8"""
        layer = i8ie.Conv2d(c, n, k, stride, pad)
        cx.synchronize()
        before = cx.memory_stats()[0]
        if like is not None:
            layer.layer.load_quantized(like.layer.q_weight(), like.layer.q_bias(), like.weight_scales(), *like.output_qparams())
        else:
            layer.load_weight((rng.standard_normal((n, c, k, k)) * 0.05).astype(np.float32))
            layer.load_bias((rng.standard_normal(n) * 0.05).astype(np.float32))
            layer.set_output_qparams(0.5, 128)
            layer.convert(per_channel=True, weight_bits=bits, spatial=bits == 4)
        cx.synchronize()
        return layer, int(cx.memory_stats()[0] - before)

    def device_us(forward):
        for _ in range(args.warmup):
            forward()
        cx.synchronize()
        cx.profile_start()
        for _ in range(args.steps):
            forward()
        prof = cx.profile_stop()
        return 1e3 * sum(v[1] for v in prof.values()) / args.steps, sorted({k.split("|")[0] for k in prof})

    def alternate(f8, f4):
        t8, t4, k8, k4 = [], [], None, None
        for _ in range(args.rounds):
            us, k8 = device_us(f8)
            t8.append(us)
            us, k4 = device_us(f4)
            t4.append(us)
        return statistics.median(t8), statistics.median(t4), k8, k4, {"int8": t8, "w4": t4}

    speed, footprint, made = [], None, {}
    for name, c, n, k, stride, pad, hw, images in SHAPES:
        if name not in made:
            l4, b4 = conv(c, n, k, stride, pad, 4)
            l8, b8 = conv(c, n, k, stride, pad, 8, like=l4)
            made = {name: (l4, l8, conv(c, c, 3, 1, 1, 8)[0])}
            if name == "c512_3x3_4":
                footprint = {"int8_per_channel_bytes": b8, "w4_bytes": b4, "ratio": b4 / b8, "w4_nibble_bytes": n * c * k * k // 2}
        l4, l8, ahead = made[name]
        q = rng.integers(0, 256, (images, c, hw, hw)).astype(np.float32)
        x = ahead(i8ie.Tensor(cx.quantize(cx.tensor(q), 1.0, 0)))
        assert np.array_equal(l8(x).numpy(), l4(x).numpy()), (name, images)
        assert x.data.layout() == 1, "the map is not resident NHWC"
        u8, u4, k8, k4, rounds = alternate(lambda: l8(x).data.layout(), lambda: l4(x).data.layout())
        speed.append({"shape": name, "in": c, "out": n, "k": k, "stride": stride, "map": hw, "images": images, "int8_us": u8, "w4_us": u4,
                      "w4_over_int8": u4 / u8, "aim_1.03": "met" if u4 <= 1.03 * u8 else "MISSED", "int8_kernels": k8, "w4_kernels": k4,
                      "per_round_us": rounds})
        print(json.dumps({k_: speed[-1][k_] for k_ in ("shape", "images", "int8_us", "w4_us", "w4_over_int8", "aim_1.03", "int8_kernels", "w4_kernels")}), flush=True)
    made.clear()

    def resnet(**convert):
        cx.trim()
        before = cx.memory_stats()[0]
        net = wl.calibrated("resnet18_cifar", **convert)
        cx.trim()
        return net, int(cx.memory_stats()[0] - before)

    n8, h8 = resnet()
    n4, h4 = resnet(weight_bits=4, spatial=True)
    xs = wl.synthetic_input("resnet18_cifar", 500, seed=1234)
    x = i8ie.tensor(xs[:100]).prefetch()
    u8, u4, _, k4, rounds = alternate(lambda: n8(x).numpy(), lambda: n4(x).numpy())
    fp32 = wl.build("resnet18_cifar")
    fp32.load(wl.synthetic_state_dict("resnet18_cifar"))
    top = {tag: np.concatenate([net(i8ie.tensor(xs[i:i + 100])).numpy().argmax(1) for i in range(0, 500, 100)])
           for tag, net in (("fp32", fp32), ("int8", n8), ("w4", n4))}
    model = {"int8_step_us": u8, "w4_step_us": u4, "w4_over_int8": u4 / u8, "per_round_us": rounds, "w4_kernels": k4,
             "int8_handle_bytes": h8, "w4_handle_bytes": h4, "handle_ratio": h4 / h8,
             "top1_agreement_with_fp32": {"int8": float((top["int8"] == top["fp32"]).mean()), "w4": float((top["w4"] == top["fp32"]).mean()),
                                          "note": "500 synthetic images, random weights, INT8 here per-tensor as Module.convert() makes it: says little"}}
    print(json.dumps(model), flush=True)

    out = {"tool": "bench_w4conv", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "speed": speed,
           "footprint_c512_3x3": footprint, "resnet18_cifar_100_images": model, "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
