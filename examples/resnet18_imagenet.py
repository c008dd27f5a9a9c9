#!/usr/bin/env python3
"""ResNet-18 at 224x224 (He et al. 2015, the ImageNet form: 7x7 stride-2 stem, max_pool2d(3, 2, padding=1), four stages of
two basic blocks, global average pool, fc 512 -> 1000) on the MI355X engine: FP32 run, prepare / convert, INT8 run, agreement
of the two argmaxes and the step time.  Self-contained: the network is written out below as an i8ie.Module.  Seeded synthetic
weights and input (no checkpoint is shipped).  Not in the reference: it has no add, no average pool and no padded pool."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))  # (channels, stride of the stage's first block)


def make_model(i8ie):
    class ResNet18(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.conv("stem", 3, 64, 7, 2, 3)
            cin = 64
            for si, (c, stride) in enumerate(STAGES, 1):
                for b in (1, 2):
                    s = stride if b == 1 else 1
                    self.conv("s%db%dc1" % (si, b), cin, c, 3, s, 1)
                    self.conv("s%db%dc2" % (si, b), c, c, 3, 1, 1)
                    if s != 1 or cin != c:
                        self.conv("s%db%dproj" % (si, b), cin, c, 1, s, 0)
                    setattr(self, "s%db%dadd" % (si, b), i8ie.Add())
                    cin = c
            self.fc = i8ie.Linear(512, 1000)
            self.weight_shapes["fc"] = (1000, 512)

        def conv(self, name, cin, cout, k, stride, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding))
            self.weight_shapes[name] = (cout, cin, k, k)

        def forward(self, x):
            x = i8ie.max_pool2d(i8ie.relu(self.stem(x)), 3, 2, padding=1)
            for si in range(1, len(STAGES) + 1):
                for b in (1, 2):
                    name = "s%db%d" % (si, b)
                    y = getattr(self, name + "c2")(i8ie.relu(getattr(self, name + "c1")(x)))
                    skip = getattr(self, name + "proj")(x) if hasattr(self, name + "proj") else x
                    x = i8ie.relu(getattr(self, name + "add")(y, skip))
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 512))

    return ResNet18()


def synthetic_state_dict(model, seed=0):
    """He-uniform weights and small biases for every Conv2d / Linear of the model, seeded"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in model.weight_shapes.items():
        fan_in = int(np.prod(shape[1:]))
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.05, 0.05, shape[0]).astype(np.float32)
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import i8ie

    model = make_model(i8ie)
    model.load(synthetic_state_dict(model))
    x = i8ie.tensor(np.random.default_rng(1234).standard_normal((args.batch, 3, 224, 224)).astype(np.float32)).prefetch()

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
    print("INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images" % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))


if __name__ == "__main__":
    main()
