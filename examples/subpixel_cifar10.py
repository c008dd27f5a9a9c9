#!/usr/bin/env python3
"""A small sub-pixel network for 32x32 input (the ESPCN idea, Shi et al. 2016, as a segmentation-style head: a
`pixel_unshuffle(2)` space-to-depth stem 3x32x32 -> 12x16x16, three 3x3 convs at 16x16, a 1x1 conv to 10 * 4 channels and
`pixel_shuffle(2)` back to a 10-class map at 32x32) on the MI355X engine: FP32 run, prepare / convert, INT8 run, agreement of
the per-pixel argmaxes and the step time.  Self-contained: the network is written out below as an i8ie.Module.  Seeded
synthetic weights and input (no checkpoint is shipped).  Not in the reference: it has neither op."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = 10


def make_model(i8ie):
    class SubPixel(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.conv("c1", 12, 64, 3, 1, 1)
            self.conv("c2", 64, 64, 3, 1, 1)
            self.conv("c3", 64, 32, 3, 1, 1)
            self.conv("head", 32, CLASSES * 4, 1, 1, 0)

        def conv(self, name, cin, cout, k, stride, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding))
            self.weight_shapes[name] = (cout, cin, k, k)

        def forward(self, x):
            x = i8ie.pixel_unshuffle(x, 2)
            for name in ("c1", "c2", "c3"):
                x = i8ie.relu(getattr(self, name)(x))
            return i8ie.pixel_shuffle(self.head(x), 2)

    return SubPixel()


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
    assert p_fp32.shape == (args.batch, 32, 32)
    model.prepare()
    model(x)
    model.convert()
    p_int8 = evaluate("INT8")
    print("INT8 per-pixel argmax agrees with FP32 on %.2f %% of %d pixels of %d synthetic images" % (
        100.0 * (p_fp32 == p_int8).mean(), p_int8.size, len(p_int8)))


if __name__ == "__main__":
    main()
