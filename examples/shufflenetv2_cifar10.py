#!/usr/bin/env python3
"""ShuffleNetV2 x1.0 for 32x32 input (Ma et al. 2018: a 3x3 stem at stride 1 and no stem pool, stages of 116 / 232 / 464 channels
with 4 / 8 / 4 units, a 1x1 conv to 1024, global average pool, fc 10) on the MI355X engine: FP32 run, prepare / convert, INT8
run, agreement of the two argmaxes and the step time.  A basic unit is `x1, x2 = chunk(x, 2)`, a 1x1 -> depthwise 3x3 -> 1x1
branch on x2, `cat` and `channel_shuffle(2)`; a down-sampling unit runs two branches on the whole input at stride 2.  The
58- and 116-channel halves exercise the narrow item widths.  Self-contained: the network is written out below as an
i8ie.Module.  Seeded synthetic weights and input (no checkpoint is shipped).  Not in the reference: it has no grouped conv, no
concat, no split and no shuffle."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = [(116, 4), (232, 8), (464, 4)]  # (width, units: one down-sampling unit and units - 1 basic ones)


def make_model(i8ie):
    class ShuffleNetV2(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.units = []  # (name, "down" / "basic")
            self.conv("stem", 3, 24, 3, 1, 1)
            cin = 24
            for s, (width, units) in enumerate(STAGES, start=2):
                half = width // 2
                for u in range(units):
                    name = "s%du%d" % (s, u)
                    if u == 0:  # both branches see the whole input and halve the map
                        self.conv(name + "_l_dw", cin, cin, 3, 2, 1, groups=cin)
                        self.conv(name + "_l_pw", cin, half, 1, 1, 0)
                        self.conv(name + "_r_pw1", cin, half, 1, 1, 0)
                        self.conv(name + "_r_dw", half, half, 3, 2, 1, groups=half)
                    else:
                        self.conv(name + "_r_pw1", half, half, 1, 1, 0)
                        self.conv(name + "_r_dw", half, half, 3, 1, 1, groups=half)
                    self.conv(name + "_r_pw2", half, half, 1, 1, 0)
                    setattr(self, name + "_cat", i8ie.Concat())
                    self.units.append((name, "down" if u == 0 else "basic"))
                cin = width
            self.conv("conv5", 464, 1024, 1, 1, 0)
            self.fc = i8ie.Linear(1024, 10)
            self.weight_shapes["fc"] = (10, 1024)

        def conv(self, name, cin, cout, k, stride, padding, groups=1):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding, groups=groups))
            self.weight_shapes[name] = (cout, cin // groups, k, k)

        def cr(self, name, x):
            return i8ie.relu(getattr(self, name)(x))

        def right(self, name, x):  # 1x1 + relu, depthwise 3x3 (no relu), 1x1 + relu
            return self.cr(name + "_r_pw2", getattr(self, name + "_r_dw")(self.cr(name + "_r_pw1", x)))

        def forward(self, x):
            x = self.cr("stem", x)
            for name, kind in self.units:
                if kind == "down":
                    left = self.cr(name + "_l_pw", getattr(self, name + "_l_dw")(x))
                    parts = [left, self.right(name, x)]
                else:
                    x1, x2 = i8ie.chunk(x, 2)
                    parts = [x1, self.right(name, x2)]
                x = i8ie.channel_shuffle(getattr(self, name + "_cat")(parts), 2)
            x = self.cr("conv5", x)
            return self.fc(i8ie.global_avg_pool2d(x).reshape(-1, 1024))

    return ShuffleNetV2()


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
    print("%d units: %d with chunk + cat + channel_shuffle(2), %d down-sampling" % (
        len(model.units), sum(k == "basic" for _, k in model.units), sum(k == "down" for _, k in model.units)))
    print("INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images" % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))


if __name__ == "__main__":
    main()
