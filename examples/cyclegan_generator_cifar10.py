#!/usr/bin/env python3
"""A Johnson / CycleGAN ResNet generator for 32x32 input (Johnson et al. 2016, Zhu et al. 2017, scaled down): pad(reflect 3) ->
7x7 conv (3 -> 32) -> InstanceNorm -> relu; two stride-2 3x3 convs (64, 128), each with InstanceNorm + relu; three residual
blocks of pad(reflect 1) -> 3x3 conv, padding 0 -> InstanceNorm -> relu -> pad(reflect 1) -> conv -> InstanceNorm -> Add; two
ConvTranspose2d(3, stride 2, padding 1, output_padding 1) with InstanceNorm + relu; pad(reflect 3) -> 7x7 conv to 3 channels
-> tanh.  InstanceNorm is GroupNorm(c, c).  On the MI355X engine: FP32 run, prepare / convert, INT8 run, the step time at
1000 and 125 images, the share of the pad kernels in the INT8 step's kernel time, and the mean absolute difference of the FP32
and the INT8 output images (no threshold: the weights are random).  Self-contained: the network is written out below as an
i8ie.Module.  Seeded synthetic weights and input (no checkpoint is shipped).  Not in the reference: it has no padding op."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PAD_KERNELS = ("pad_u8_nhwc", "pad_u8_direct", "pad_f32")
BLOCKS = 3


def make_model(i8ie):
    class Generator(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.weight_shapes = {}
            self.conv("c1", 3, 32, 7, 1, 0)
            self.conv("d1", 32, 64, 3, 2, 1)
            self.conv("d2", 64, 128, 3, 2, 1)
            for b in range(BLOCKS):
                self.conv("r%da" % b, 128, 128, 3, 1, 0)
                self.conv("r%db" % b, 128, 128, 3, 1, 0)
                setattr(self, "r%d_add" % b, i8ie.Add())
            self.deconv("u1", 128, 64)
            self.deconv("u2", 64, 32)
            self.out = i8ie.Conv2d(32, 3, 7, stride=1, padding=0)
            self.weight_shapes["out"] = (3, 32, 7, 7)
            self.tanh = i8ie.Activation("tanh")

        def conv(self, name, cin, cout, k, stride, padding):
            setattr(self, name, i8ie.Conv2d(cin, cout, k, stride=stride, padding=padding))
            setattr(self, name + "_in", i8ie.GroupNorm(cout, cout))
            self.weight_shapes[name] = (cout, cin, k, k)

        def deconv(self, name, cin, cout):
            setattr(self, name, i8ie.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1))
            setattr(self, name + "_in", i8ie.GroupNorm(cout, cout))
            self.weight_shapes[name] = (cin, cout, 3, 3)

        def cn(self, name, x):
            return getattr(self, name + "_in")(getattr(self, name)(x))

        def forward(self, x):
            x = i8ie.relu(self.cn("c1", i8ie.pad(x, (3, 3, 3, 3), "reflect")))
            x = i8ie.relu(self.cn("d1", x))
            x = i8ie.relu(self.cn("d2", x))
            for b in range(BLOCKS):
                y = i8ie.relu(self.cn("r%da" % b, i8ie.pad(x, (1, 1, 1, 1), "reflect")))
                y = self.cn("r%db" % b, i8ie.pad(y, (1, 1, 1, 1), "reflect"))
                x = getattr(self, "r%d_add" % b)(x, y)
            x = i8ie.relu(self.cn("u1", x))
            x = i8ie.relu(self.cn("u2", x))
            return self.tanh(self.out(i8ie.pad(x, (3, 3, 3, 3), "reflect")))

    return Generator()


def synthetic_state_dict(model, seed=0):
    """He-uniform weights and small biases for every conv of the model, seeded (the norms keep gamma = 1, beta = 0)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in model.weight_shapes.items():
        fan_in = int(np.prod(shape[1:]))
        sd[name + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.05, 0.05, shape[0] if name[0] != "u" else shape[1]).astype(np.float32)
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1000, 125])
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie

    model = make_model(i8ie)
    model.load(synthetic_state_dict(model))
    xs = {m: i8ie.tensor(np.random.default_rng(1234).uniform(-1, 1, (m, 3, 32, 32)).astype(np.float32)).prefetch() for m in args.batches}

    def evaluate(tag):
        images = {}
        for m, x in xs.items():
            images[m] = model(x).numpy()  # warm-up
            i8ie.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                y = model(x)
            images[m] = y.numpy()
            dt = (time.perf_counter() - t0) / args.steps
            print("%-6s %5d images  step %8.2f ms  %9.0f img/s" % (tag, m, dt * 1e3, m / dt))
        return images

    fp32 = evaluate("FP32")
    model.prepare()
    model(xs[min(xs)])
    model.convert()
    int8 = evaluate("INT8")
    for m, x in xs.items():
        cx.profile_start()
        for _ in range(args.steps):
            model(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        pads = sum(v[1] for k, v in prof.items() if k.split("|")[0] in PAD_KERNELS)
        launches = sum(v[0] for k, v in prof.items() if k.split("|")[0] in PAD_KERNELS) // args.steps
        print("%5d images: %d pad launches per step, %.3f of %.3f ms of kernel time (%.1f %%)"
              % (m, launches, pads / args.steps, total / args.steps, 100.0 * pads / total))
    for m in xs:
        assert fp32[m].shape == int8[m].shape == (m, 3, 32, 32)
        print("%5d images: mean |FP32 - INT8| of the output images %.4f (range [-1, 1])" % (m, float(np.abs(fp32[m] - int8[m]).mean())))


if __name__ == "__main__":
    main()
