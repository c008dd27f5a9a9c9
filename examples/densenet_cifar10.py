#!/usr/bin/env python3
"""A DenseNet-BC for 32x32 input (Huang et al. 2017: growth rate 12, three dense blocks of `--layers` layers, each layer
BN -> ReLU -> 1x1 (4 x growth) -> BN -> ReLU -> 3x3 (growth) joined to its input by a Concat; transitions BN -> ReLU -> 1x1 (half
the channels) -> avg_pool2d(2); BN -> ReLU -> global average pool -> fc 10) on the MI355X engine: FP32 run, prepare / convert,
INT8 run, agreement of the two argmaxes and the step time.  Self-contained: the network is written out below as an i8ie.Module.
Seeded synthetic weights and running statistics (no checkpoint is shipped), loaded through Module.load() with torch's keys
(`<attr>.running_mean`, `<attr>.running_var`, `<attr>.num_batches_tracked`).  The BatchNorm behind each bottleneck 1x1 conv is
folded into it (Module.fold_batchnorm: no launch); the ones behind a Concat cannot be folded and run the quantized BatchNorm
kernel with the ReLU folded in.  Not in the reference: it has no normalisation, no concat and no average pool."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROWTH = 12


def make_model(i8ie, layers=6):
    class DenseNet(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes, self.bn_widths, self.folds, self.blocks = {}, {}, [], []
            c = 2 * GROWTH
            self.conv("stem", 3, c, 3, 1)
            for b in range(3):
                names = []
                for i in range(layers):
                    n = "b%d_l%d" % (b, i)
                    self.bn(n + "_bn1", c)                       # behind a Concat (or the stem, which the Concat reads too): the kernel
                    self.conv(n + "_c1", c, 4 * GROWTH, 1, 0)
                    self.bn(n + "_bn2", 4 * GROWTH)              # behind the bottleneck conv: folded into it
                    self.folds.append((n + "_c1", n + "_bn2"))
                    self.conv(n + "_c2", 4 * GROWTH, GROWTH, 3, 1)
                    setattr(self, n + "_cat", i8ie.Concat())
                    names.append(n)
                    c += GROWTH
                self.blocks.append(names)
                if b < 2:
                    self.bn("t%d_bn" % b, c)
                    self.conv("t%d_c" % b, c, c // 2, 1, 0)
                    c //= 2
            self.bn("final_bn", c)
            self.fc = i8ie.Linear(c, 10)
            self.weight_shapes["fc"] = (10, c)
            self.width = c

        def conv(self, name, cin, cout, k, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, padding=padding))
            self.weight_shapes[name] = (cout, cin, k, k)

        def bn(self, name, c):
            setattr(self, name, i8ie.BatchNorm2d(c))
            self.bn_widths[name] = c

        def at(self, name):
            return getattr(self, name)

        def forward(self, x):
            x = self.stem(x)
            for b, names in enumerate(self.blocks):
                for n in names:
                    y = i8ie.relu(self.at(n + "_bn1")(x))
                    y = i8ie.relu(self.at(n + "_bn2")(self.at(n + "_c1")(y)))
                    x = self.at(n + "_cat")([x, self.at(n + "_c2")(y)])
                if b < 2:
                    x = i8ie.avg_pool2d(self.at("t%d_c" % b)(i8ie.relu(self.at("t%d_bn" % b)(x))), 2)
            x = i8ie.relu(self.final_bn(x))
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, self.width))

    return DenseNet()


def synthetic_state_dict(model, seed=0):
    """He-uniform weights and small biases for every Conv2d / Linear, and for every BatchNorm2d a gamma near 1, a small beta and
    running statistics of the size a trained network's have, under torch's key names; seeded"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in model.weight_shapes.items():
        fan_in = int(np.prod(shape[1:]))
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.05, 0.05, shape[0]).astype(np.float32)
    for name, c in model.bn_widths.items():
        sd[name + ".weight"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.2, 0.2, c).astype(np.float32)
        sd[name + ".running_mean"] = rng.normal(0.0, 0.3, c).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[name + ".num_batches_tracked"] = np.int64(1000)
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=125)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=6, help="dense layers per block (6: DenseNet-BC-40)")
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import i8ie

    model = make_model(i8ie, args.layers)
    model.load(synthetic_state_dict(model))
    model.fold_batchnorm(model.folds)
    x = i8ie.tensor(np.random.default_rng(1234).standard_normal((args.batch, 3, 32, 32)).astype(np.float32)).prefetch()

    def evaluate(tag):
        pred = i8ie.argmax(model(x), axis=1).numpy()  # warm-up
        i8ie.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pred = i8ie.argmax(model(x), axis=1).numpy()
        dt = (time.perf_counter() - t0) / args.steps
        print("%-6s step %8.2f ms  %9.0f img/s" % (tag, dt * 1e3, args.batch / dt))
        return pred.astype(np.int64)

    p_fp32 = evaluate("FP32")
    model.prepare()
    model(x)
    model.convert()
    p_int8 = evaluate("INT8")
    folded = sum(model.at(n).is_folded() for n in model.bn_widths)
    print("%d BatchNorm2d layers: %d folded into their 1x1 conv, %d on the quantized kernel" % (len(model.bn_widths), folded,
                                                                                              len(model.bn_widths) - folded))
    print("INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images" % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))


if __name__ == "__main__":
    main()
