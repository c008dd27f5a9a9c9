#!/usr/bin/env python3
"""A GroupNorm ResNet-18 for 32x32 CIFAR-10 (Wu & He 2018: resnet18_cifar's topology with GroupNorm(32, c) behind every conv) with one diffusion-style residual block at 8x8 (GroupNorm, SiLU written as x * sigmoid(x), 3x3 conv, 4-head self-attention, skips) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  The network is an i8ie.Module subclass defined here, outside the network registry.  Runs on seeded synthetic weights and inputs."""
import argparse
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)

HEADS = 4
GROUPS = 32
INPUT = (3, 32, 32)
STAGES = [(64, 1), (128, 2), (256, 2), (512, 2)]   # (channels, stride of the first block); two basic blocks each
MID = 256                                          # the diffusion-style block sits behind the 8x8 stage


def _layers():
    """attr -> ("conv", in, out, k, stride, pad) | ("gn", channels) | ("fc", in, out), in creation order"""
    L = {"stem": ("conv", 3, 64, 3, 1, 1), "stem_gn": ("gn", 64)}
    cin = 64
    for s, (c, stride) in enumerate(STAGES):
        for b in range(2):
            p, st = "s%db%d_" % (s, b), stride if b == 0 else 1
            L[p + "c1"], L[p + "gn1"] = ("conv", cin, c, 3, st, 1), ("gn", c)
            L[p + "c2"], L[p + "gn2"] = ("conv", c, c, 3, 1, 1), ("gn", c)
            if st != 1 or cin != c:
                L[p + "sc"], L[p + "scgn"] = ("conv", cin, c, 1, st, 0), ("gn", c)
            cin = c
        if c == MID:
            L["m_gn"], L["m_c"], L["m_gn2"] = ("gn", c), ("conv", c, c, 3, 1, 1), ("gn", c)
            L["m_qkv"], L["m_proj"] = ("conv", c, 3 * c, 1, 1, 0), ("conv", c, c, 1, 1, 0)
    L["fc"] = ("fc", 512, 10)
    return L


LAYERS = _layers()


def synthetic_state_dict(seed=42):
    """He-uniform weights, U(-1, 1) / sqrt(fan_in) biases, gamma from U(0.5, 1.5), beta from U(-0.3, 0.3); the query filters of
    the packed projection carry 1 / sqrt(d)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for attr, L in LAYERS.items():
        if L[0] == "gn":
            sd[attr + ".weight"] = rng.uniform(0.5, 1.5, L[1]).astype(np.float32)
            sd[attr + ".bias"] = rng.uniform(-0.3, 0.3, L[1]).astype(np.float32)
            continue
        shape = (L[2], L[1], L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
        fan_in = int(np.prod(shape[1:]))
        fold = np.ones(shape[0])
        if attr == "m_qkv":
            fold[:MID] = 1.0 / np.sqrt(MID // HEADS)
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

    class GroupNormResNet(i8ie.Module):
        def __init__(self):
            super().__init__()
            for attr, L in LAYERS.items():
                if L[0] == "conv":
                    setattr(self, attr, i8ie.Conv2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5]))
                elif L[0] == "gn":
                    setattr(self, attr, i8ie.GroupNorm(GROUPS, L[1]))
                else:
                    setattr(self, attr, i8ie.Linear(L[1], L[2]))
            for s in range(len(STAGES)):
                for b in range(2):
                    setattr(self, "s%db%d_add" % (s, b), i8ie.Add())
            self.m_sig, self.m_mul, self.m_attn = i8ie.Activation("sigmoid"), i8ie.Mul(), i8ie.Attention(HEADS)
            self.m_add1, self.m_add2 = i8ie.Add(), i8ie.Add()

        def block(self, x, p):
            g = lambda a: getattr(self, p + a)  # noqa: E731
            y = i8ie.relu(g("gn1")(g("c1")(x)))
            y = g("gn2")(g("c2")(y))
            skip = g("scgn")(g("sc")(x)) if hasattr(self, p + "sc") else x
            return i8ie.relu(g("add")(y, skip))

        def middle(self, x):
            """GroupNorm, SiLU, conv, skip; then GroupNorm, self-attention, skip"""
            g = self.m_gn(x)
            y = self.m_c(self.m_mul(g, self.m_sig(g)))   # SiLU = x * sigmoid(x)
            x = self.m_add1(y, x)
            y = self.m_proj(self.m_attn(self.m_qkv(self.m_gn2(x))))
            return i8ie.relu(self.m_add2(y, x))

        def forward(self, x):
            x = i8ie.relu(self.stem_gn(self.stem(x)))
            for s, (c, _) in enumerate(STAGES):
                x = self.block(self.block(x, "s%db0_" % s), "s%db1_" % s)
                if c == MID:
                    x = self.middle(x)
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 512))

    return GroupNormResNet()


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
    if args.save_quantized:
        model.save_quantized(args.save_quantized)
        again = build()
        again.load_quantized_file(args.save_quantized)
        same = np.array_equal(again(tens[0]).numpy(), model(tens[0]).numpy())
        print("saved %s; reloaded model reproduces the logits: %s" % (args.save_quantized, same))


if __name__ == "__main__":
    main()
