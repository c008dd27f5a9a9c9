#!/usr/bin/env python3
"""An Inception-v3-style network for 32x32 input (Szegedy et al. 2015, scaled down: a stem, an A block with an
avg_pool2d(3, 1, padding=1) branch, a reduction block, two C blocks with 1x7 / 7x1 chains at 16x16, a reduction, an E block with
1x3 / 3x1 pairs at 8x8, Concat joins, global average pool, fc 10) on the MI355X engine: FP32 run, prepare / convert, INT8 run,
agreement of the two argmaxes and the step time.  Self-contained: the network is written out below as an i8ie.Module.  Seeded
synthetic weights and input (no checkpoint is shipped).  Not in the reference: it has no rectangular kernel, no concat and no
average pool."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_model(i8ie):
    class Inception(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.rect_layers = []
            # stem: 32x32
            self.conv("stem1", 3, 32, 3, 1, 1)
            self.conv("stem2", 32, 64, 3, 1, 1)
            # A block at 32x32: 1x1 | 1x1 -> 5x5 | 1x1 -> 3x3 -> 3x3 | avg_pool(3, 1, 1) -> 1x1   -> 32 + 32 + 48 + 16 = 128
            self.conv("a_1", 64, 32, 1, 1, 0)
            self.conv("a_5a", 64, 32, 1, 1, 0)
            self.conv("a_5b", 32, 32, 5, 1, 2)
            self.conv("a_3a", 64, 32, 1, 1, 0)
            self.conv("a_3b", 32, 48, 3, 1, 1)
            self.conv("a_3c", 48, 48, 3, 1, 1)
            self.conv("a_p", 64, 16, 1, 1, 0)
            self.a_cat = i8ie.Concat()
            # reduction to 16x16: 3x3 / 2 | 1x1 -> 3x3 -> 3x3 / 2 | max_pool(3, 2, 1)               -> 32 + 32 + 128 = 192
            self.conv("r1_3", 128, 32, 3, 2, 1)
            self.conv("r1_da", 128, 32, 1, 1, 0)
            self.conv("r1_db", 32, 32, 3, 1, 1)
            self.conv("r1_dc", 32, 32, 3, 2, 1)
            self.r1_cat = i8ie.Concat()
            # two C blocks at 16x16, 192 -> 192: 1x1 | 1x1 -> 1x7 -> 7x1 | 1x1 -> 7x1 -> 1x7 -> 7x1 -> 1x7 | avg_pool -> 1x1
            for b, mid in (("c1", 64), ("c2", 96)):
                self.conv(b + "_1", 192, 48, 1, 1, 0)
                self.conv(b + "_7a", 192, mid, 1, 1, 0)
                self.conv(b + "_7b", mid, mid, (1, 7), 1, (0, 3))
                self.conv(b + "_7c", mid, 48, (7, 1), 1, (3, 0))
                self.conv(b + "_da", 192, mid, 1, 1, 0)
                self.conv(b + "_db", mid, mid, (7, 1), 1, (3, 0))
                self.conv(b + "_dc", mid, mid, (1, 7), 1, (0, 3))
                self.conv(b + "_dd", mid, mid, (7, 1), 1, (3, 0))
                self.conv(b + "_de", mid, 48, (1, 7), 1, (0, 3))
                self.conv(b + "_p", 192, 48, 1, 1, 0)
                setattr(self, b + "_cat", i8ie.Concat())
            # reduction to 8x8: 1x1 -> 3x3 / 2 | 1x1 -> 1x7 -> 7x1 -> 3x3 / 2 | max_pool(3, 2, 1)     -> 64 + 64 + 192 = 320
            self.conv("r2_3a", 192, 64, 1, 1, 0)
            self.conv("r2_3b", 64, 64, 3, 2, 1)
            self.conv("r2_7a", 192, 64, 1, 1, 0)
            self.conv("r2_7b", 64, 64, (1, 7), 1, (0, 3))
            self.conv("r2_7c", 64, 64, (7, 1), 1, (3, 0))
            self.conv("r2_7d", 64, 64, 3, 2, 1)
            self.r2_cat = i8ie.Concat()
            # E block at 8x8: 1x1 | 1x1 -> (1x3, 3x1) | 1x1 -> 3x3 -> (1x3, 3x1) | avg_pool -> 1x1   -> 64 + 2*64 + 2*64 + 64 = 384
            self.conv("e_1", 320, 64, 1, 1, 0)
            self.conv("e_3a", 320, 96, 1, 1, 0)
            self.conv("e_3b1", 96, 64, (1, 3), 1, (0, 1))
            self.conv("e_3b2", 96, 64, (3, 1), 1, (1, 0))
            self.conv("e_da", 320, 96, 1, 1, 0)
            self.conv("e_db", 96, 96, 3, 1, 1)
            self.conv("e_dc1", 96, 64, (1, 3), 1, (0, 1))
            self.conv("e_dc2", 96, 64, (3, 1), 1, (1, 0))
            self.conv("e_p", 320, 64, 1, 1, 0)
            self.e_cat = i8ie.Concat()
            self.fc = i8ie.Linear(384, 10)
            self.weight_shapes["fc"] = (10, 384)

        def conv(self, name, cin, cout, k, stride, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding))
            kh, kw = (k, k) if isinstance(k, int) else k
            self.weight_shapes[name] = (cout, cin, kh, kw)
            if kh != kw:
                self.rect_layers.append(name)

        def cr(self, name, x):
            return i8ie.relu(getattr(self, name)(x))

        def chain(self, names, x):
            for n in names:
                x = self.cr(n, x)
            return x

        def forward(self, x):
            x = self.chain(["stem1", "stem2"], x)
            x = self.a_cat([self.cr("a_1", x), self.chain(["a_5a", "a_5b"], x), self.chain(["a_3a", "a_3b", "a_3c"], x),
                            self.cr("a_p", i8ie.avg_pool2d(x, 3, 1, padding=1))])
            x = self.r1_cat([self.cr("r1_3", x), self.chain(["r1_da", "r1_db", "r1_dc"], x), i8ie.max_pool2d(x, 3, 2, padding=1)])
            for b in ("c1", "c2"):
                x = getattr(self, b + "_cat")([self.cr(b + "_1", x), self.chain([b + "_7a", b + "_7b", b + "_7c"], x),
                                               self.chain([b + "_da", b + "_db", b + "_dc", b + "_dd", b + "_de"], x),
                                               self.cr(b + "_p", i8ie.avg_pool2d(x, 3, 1, padding=1))])
            x = self.r2_cat([self.chain(["r2_3a", "r2_3b"], x), self.chain(["r2_7a", "r2_7b", "r2_7c", "r2_7d"], x),
                             i8ie.max_pool2d(x, 3, 2, padding=1)])
            t3 = self.cr("e_3a", x)
            td = self.chain(["e_da", "e_db"], x)
            x = self.e_cat([self.cr("e_1", x), self.cr("e_3b1", t3), self.cr("e_3b2", t3), self.cr("e_dc1", td), self.cr("e_dc2", td),
                            self.cr("e_p", i8ie.avg_pool2d(x, 3, 1, padding=1))])
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 384))

    return Inception()


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
    print("%d rectangular layers: %s" % (len(model.rect_layers), ", ".join(
        "%s %dx%d" % ((n,) + getattr(model, n).geometry()["kernel_size"]) for n in model.rect_layers)))
    print("INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images" % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))


if __name__ == "__main__":
    main()
