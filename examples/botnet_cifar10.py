#!/usr/bin/env python3
"""A ResNet-style network for 32x32 CIFAR-10 whose last stage replaces the 3x3 convs of its bottleneck blocks with 4-head self-attention (BoTNet, Srinivas et al. 2021, without the relative-position term) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Each attention block is one packed 1x1 conv c -> 3c and one fused launch (i8ie.Attention); the 1 / sqrt(d) factor is folded into the query filters.  The network is an i8ie.Module subclass defined here, outside the network registry.  Runs on seeded synthetic weights and inputs."""
import argparse
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)

HEADS = 4
INPUT = (3, 32, 32)
# attr -> ("conv", in, out, k, stride, pad) | ("fc", in, out), in creation order
LAYERS = {
    "stem": ("conv", 3, 32, 3, 1, 1),
    # stage 1, 32x32: one basic block
    "s1a": ("conv", 32, 32, 3, 1, 1), "s1b": ("conv", 32, 32, 3, 1, 1),
    # stage 2, 16x16: one basic block with a projection shortcut
    "s2a": ("conv", 32, 64, 3, 2, 1), "s2b": ("conv", 64, 64, 3, 1, 1), "s2s": ("conv", 32, 64, 1, 2, 0),
    # stage 3, 8x8 (t = 64): two bottleneck blocks, the 3x3 conv of each replaced by self-attention at width 128 (d = 32)
    "s3in": ("conv", 64, 256, 3, 2, 1),
    "b1r": ("conv", 256, 128, 1, 1, 0), "b1qkv": ("conv", 128, 384, 1, 1, 0), "b1e": ("conv", 128, 256, 1, 1, 0),
    "b2r": ("conv", 256, 128, 1, 1, 0), "b2qkv": ("conv", 128, 384, 1, 1, 0), "b2e": ("conv", 128, 256, 1, 1, 0),
    "fc": ("fc", 256, 10)}
QUERY_FILTERS = {"b1qkv": 128, "b2qkv": 128}   # the first filters of a packed projection are the queries


def synthetic_state_dict(seed=42):
    """He-uniform weights, U(-1, 1) / sqrt(fan_in) biases; the query filters carry 1 / sqrt(d)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for attr, L in LAYERS.items():
        shape = (L[2], L[1], L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
        fan_in = int(np.prod(shape[1:]))
        fold = np.ones(shape[0])
        if attr in QUERY_FILTERS:
            fold[:QUERY_FILTERS[attr]] = 1.0 / np.sqrt(QUERY_FILTERS[attr] // HEADS)
        w = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)
        sd[attr + ".weight"] = (w * fold.reshape((-1,) + (1,) * (len(shape) - 1))).astype(np.float32)
        sd[attr + ".bias"] = (rng.uniform(-1, 1, shape[0]) / np.sqrt(fan_in) * fold).astype(np.float32)
    return sd


def synthetic_input(batch, seed=1234):
    """normalised-image-like input, inside quantize()'s no-wrap window for scale 0.025 / zero point 127"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (batch,) + INPUT).astype(np.float32)
    a = rng.uniform(0.2, 1.0, (batch, INPUT[0], 1, 1)).astype(np.float32)
    return ((u * a - np.float32(0.45)) / np.float32(0.226)).astype(np.float32)


def build():
    import int8inferenceengine_amd  # noqa: F401
    import i8ie

    class BoTNet(i8ie.Module):
        def __init__(self):
            super().__init__()
            for attr, L in LAYERS.items():
                if L[0] == "conv":
                    setattr(self, attr, i8ie.Conv2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5]))
                else:
                    setattr(self, attr, i8ie.Linear(L[1], L[2]))
            self.add1, self.add2, self.add_b1, self.add_b2 = i8ie.Add(), i8ie.Add(), i8ie.Add(), i8ie.Add()
            self.b1attn, self.b2attn = i8ie.Attention(HEADS), i8ie.Attention(HEADS)

        def bot(self, x, reduce, qkv, attn, expand, add):
            y = i8ie.relu(reduce(x))
            y = i8ie.relu(attn(qkv(y)))          # the place of the bottleneck's 3x3 conv
            return i8ie.relu(add(expand(y), x))

        def forward(self, x):
            x = i8ie.relu(self.stem(x))
            x = i8ie.relu(self.add1(self.s1b(i8ie.relu(self.s1a(x))), x))
            x = i8ie.relu(self.add2(self.s2b(i8ie.relu(self.s2a(x))), self.s2s(x)))
            x = i8ie.relu(self.s3in(x))
            x = self.bot(x, self.b1r, self.b1qkv, self.b1attn, self.b1e, self.add_b1)
            x = self.bot(x, self.b2r, self.b2qkv, self.b2attn, self.b2e, self.add_b2)
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 256))

    return BoTNet()


def calibrated(calib_images=16, seed=42):
    """the reference workflow: prepare -> one FP32 batch -> convert"""
    import i8ie

    net = build()
    net.load(synthetic_state_dict(seed))
    net.prepare()
    net(i8ie.tensor(synthetic_input(calib_images, seed=99)))
    net.convert()
    return net


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--save-quantized", help="write the converted model to this .npz")
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import i8ie

    model = build()
    model.load(synthetic_state_dict())
    xs = synthetic_input(args.batch * args.batches)
    tens = [i8ie.tensor(xs[i:i + args.batch]).prefetch() for i in range(0, len(xs), args.batch)]

    def evaluate(tag):
        i8ie.synchronize()
        t0 = time.perf_counter()
        preds = [i8ie.argmax(model(x), axis=1).numpy() for x in tens]
        dt = time.perf_counter() - t0
        preds = np.concatenate(preds).astype(np.int64)
        print("%-18s %8.1f ms  %10.0f img/s" % (tag, dt * 1e3, len(preds) / dt))
        return preds

    evaluate("FP32 (warm-up)")
    p_fp32 = evaluate("FP32")
    t0 = time.perf_counter()
    model.prepare()
    model(tens[0])
    model.convert()
    print("%-18s %8.1f ms" % ("prepare+convert", (time.perf_counter() - t0) * 1e3))
    evaluate("INT8 (warm-up)")
    p_int8 = evaluate("INT8")
    print("no labels: INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images"
          % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))
    for a in ("b1attn", "b2attn"):
        print("%s: score qparams %s, output qparams %s" % (a, getattr(model, a).score_qparams(), getattr(model, a).output_qparams()))
    if args.save_quantized:
        model.save_quantized(args.save_quantized)
        again = build()
        again.load_quantized_file(args.save_quantized)
        same = np.array_equal(again(tens[0]).numpy(), model(tens[0]).numpy())
        print("saved %s; reloaded model reproduces the logits: %s" % (args.save_quantized, same))


if __name__ == "__main__":
    main()
