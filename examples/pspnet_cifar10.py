#!/usr/bin/env python3
"""A PSPNet-style segmentation network for 32x32 input (Zhao et al. 2017, scaled down) on the MI355X engine: resnet18_cifar's
stem and first three stages (256 channels of 8x8), a pyramid pooling module -- adaptive_avg_pool2d to 1, 2, 3 and 6 bins, a
1x1 conv to 64 channels each, interpolate(size=(8, 8), mode="bilinear") back to the feature size, Concat with the feature map
at 512 -- a 3x3 conv, a 1x1 conv to 10 classes and interpolate(size=(32, 32), mode="bilinear", align_corners=True).  Bins 1
and 2 reach 8x8 by the integer factors 8 and 4 (the upsample kernel); bins 3 and 6 and the final aligned resize take the
resize kernel, bins 3 and 6 the adaptive pool kernel.  FP32 run, prepare / convert, INT8 run, per-pixel agreement of the two
argmaxes and the step time.  Self-contained: the network is written out below as an i8ie.Module.  Seeded synthetic weights and
input (no checkpoint is shipped).  Not in the reference: it has no resize, no adaptive pool, no add and no concat."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BINS = (1, 2, 3, 6)


def make_model(i8ie):
    class PSPNet(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.conv("stem", 3, 64, 3, 1, 1)
            self.blocks = []  # (prefix, has a projection shortcut)
            in_c = 64
            for stage, out_c in enumerate((64, 128, 256), start=1):
                for block in (1, 2):
                    p = "s%db%d" % (stage, block)
                    stride = 2 if (stage > 1 and block == 1) else 1
                    self.conv(p + "c1", in_c, out_c, 3, stride, 1)
                    self.conv(p + "c2", out_c, out_c, 3, 1, 1)
                    proj = stride != 1 or in_c != out_c
                    if proj:
                        self.conv(p + "proj", in_c, out_c, 1, stride, 0)
                    setattr(self, p + "add", i8ie.Add())
                    self.blocks.append((p, proj))
                    in_c = out_c
            for b in BINS:
                self.conv("ppm%d" % b, 256, 64, 1, 1, 0)
            self.cat = i8ie.Concat()
            self.fuse = self.conv("fuse", 256 + 64 * len(BINS), 128, 3, 1, 1)
            self.conv("head", 128, 10, 1, 1, 0)

        def conv(self, name, cin, cout, k, stride, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding))
            self.weight_shapes[name] = (cout, cin, k, k)
            return getattr(self, name)

        def cr(self, name, x):
            return i8ie.relu(getattr(self, name)(x))

        def forward(self, x):
            x = self.cr("stem", x)
            for p, proj in self.blocks:
                y = getattr(self, p + "c2")(self.cr(p + "c1", x))
                skip = getattr(self, p + "proj")(x) if proj else x
                x = i8ie.relu(getattr(self, p + "add")(y, skip))
            pyramid = [i8ie.interpolate(self.cr("ppm%d" % b, i8ie.adaptive_avg_pool2d(x, b)), size=(8, 8), mode="bilinear") for b in BINS]
            x = self.cr("fuse", self.cat([x] + pyramid))
            return i8ie.interpolate(self.head(x), size=(32, 32), mode="bilinear", align_corners=True)

    return PSPNet()


def synthetic_state_dict(model, seed=0):
    """He-uniform weights and small biases for every Conv2d of the model, seeded"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in model.weight_shapes.items():
        fan_in = int(np.prod(shape[1:]))
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.05, 0.05, shape[0]).astype(np.float32)
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=125)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import i8ie

    model = make_model(i8ie)
    model.load(synthetic_state_dict(model))
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
    assert p_int8.shape == (args.batch, 32, 32)
    print("INT8 per-pixel argmax agrees with FP32 on %.2f %% of %d pixels of %d synthetic images"
          % (100.0 * (p_fp32 == p_int8).mean(), p_int8.size, len(p_int8)))


if __name__ == "__main__":
    main()
