#!/usr/bin/env python3
"""A two-stage Swin Transformer for 32x32 input (Liu et al. 2021, scaled down): a 4x4 patch embedding to 64 channels at 8x8
(2 heads of d = 32), two blocks, patch merging -- pixel_unshuffle(2) + LayerNorm + 1x1 conv -- to 128 channels at 4x4 (4 heads of
d = 32), two more blocks.  The blocks of a stage alternate shift = 0 and shift = window // 2 over 4x4 windows, each with its own
relative position bias table: Attention(heads, window=4, shift=, relative_position_bias=True) is one launch, with no roll, no
mask tensor and no gather of the table at run time.  Blocks are pre-LN with hardswish MLPs (where the paper has GELU, which the
engine does not have); the 1/sqrt(d) of every attention is folded into its q projection.  Then LayerNorm, global average pool
and Linear(128, 10).  On the MI355X engine: FP32 run, prepare / convert, INT8 run, the step time at 1000 and 125 images, the
share of the shifted-window attention launches in the INT8 step's kernel time, and the agreement of the FP32 and INT8 argmaxes.
Self-contained: the network is written out below as an i8ie.Module.  Seeded synthetic weights and input (no checkpoint is
shipped).  Not in the reference: it has no attention or normalisation op."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = [(64, 2), (128, 4)]   # channels, heads
WINDOW, DEPTH, MLP_RATIO, PATCH = 4, 2, 2, 4
SWIN_KERNELS = ("attn_mfma_swin", "attn_direct_swin")


def make_model(i8ie):
    class Swin(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.patch = i8ie.Conv2d(3, STAGES[0][0], PATCH, stride=PATCH)
            self.patch_ln = i8ie.LayerNorm(STAGES[0][0])
            for s, (c, heads) in enumerate(STAGES):
                if s > 0:
                    setattr(self, "s%d_merge_ln" % s, i8ie.LayerNorm(4 * STAGES[s - 1][0]))
                    setattr(self, "s%d_merge" % s, i8ie.Conv2d(4 * STAGES[s - 1][0], c, 1))
                for b in range(DEPTH):
                    q = "s%d_b%d_" % (s, b)
                    setattr(self, q + "ln1", i8ie.LayerNorm(c))
                    setattr(self, q + "qkv", i8ie.Conv2d(c, 3 * c, 1))
                    setattr(self, q + "attn", i8ie.Attention(heads, window=WINDOW, shift=(b % 2) * (WINDOW // 2), relative_position_bias=True))
                    setattr(self, q + "proj", i8ie.Conv2d(c, c, 1))
                    setattr(self, q + "add1", i8ie.Add())
                    setattr(self, q + "ln2", i8ie.LayerNorm(c))
                    setattr(self, q + "fc1", i8ie.Conv2d(c, MLP_RATIO * c, 1))
                    setattr(self, q + "act", i8ie.Activation("hardswish"))
                    setattr(self, q + "fc2", i8ie.Conv2d(MLP_RATIO * c, c, 1))
                    setattr(self, q + "add2", i8ie.Add())
            self.ln = i8ie.LayerNorm(STAGES[-1][0])
            self.head = i8ie.Linear(STAGES[-1][0], 10)

        def forward(self, x):
            x = self.patch_ln(self.patch(x))
            for s in range(len(STAGES)):
                if s > 0:
                    x = getattr(self, "s%d_merge" % s)(getattr(self, "s%d_merge_ln" % s)(i8ie.pixel_unshuffle(x, 2)))
                for b in range(DEPTH):
                    L = lambda name: getattr(self, "s%d_b%d_%s" % (s, b, name))  # noqa: E731
                    x = L("add1")(x, L("proj")(L("attn")(L("qkv")(L("ln1")(x)))))
                    x = L("add2")(x, L("fc2")(L("act")(L("fc1")(L("ln2")(x)))))
            x = i8ie.adaptive_avg_pool2d(self.ln(x), 1)
            return self.head(x.reshape(-1, STAGES[-1][0]))

    return Swin()


def synthetic_state_dict(seed=0):
    """seeded weights: Xavier-uniform projections (every q projection scaled by 1/sqrt(d)), LayerNorms near the identity,
    relative position bias tables of standard deviation 0.5 (a trained Swin's are of that order)"""
    rng = np.random.default_rng(seed)
    sd = {}

    def dense(name, cout, cin, k=1, conv=True):
        lim = np.sqrt(6.0 / (cin * k * k + cout))
        sd[name + ".weight"] = rng.uniform(-lim, lim, (cout, cin, k, k) if conv else (cout, cin)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.02, 0.02, cout).astype(np.float32)

    def norm(name, c):
        sd[name + ".weight"] = rng.normal(1.0, 0.05, c).astype(np.float32)
        sd[name + ".bias"] = rng.normal(0.0, 0.05, c).astype(np.float32)

    dense("patch", STAGES[0][0], 3, PATCH)
    norm("patch_ln", STAGES[0][0])
    for s, (c, heads) in enumerate(STAGES):
        if s > 0:
            norm("s%d_merge_ln" % s, 4 * STAGES[s - 1][0])
            dense("s%d_merge" % s, c, 4 * STAGES[s - 1][0])
        scale = np.float32(1.0 / np.sqrt(c // heads))
        for b in range(DEPTH):
            q = "s%d_b%d_" % (s, b)
            norm(q + "ln1", c)
            dense(q + "qkv", 3 * c, c)
            sd[q + "qkv.weight"][:c] *= scale
            sd[q + "qkv.bias"][:c] *= scale
            sd[q + "attn.relative_position_bias_table"] = rng.normal(0.0, 0.5, ((2 * WINDOW - 1) ** 2, heads)).astype(np.float32)
            dense(q + "proj", c, c)
            norm(q + "ln2", c)
            dense(q + "fc1", MLP_RATIO * c, c)
            dense(q + "fc2", c, MLP_RATIO * c)
    norm("ln", STAGES[-1][0])
    dense("head", 10, STAGES[-1][0], conv=False)
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
    model.load(synthetic_state_dict())
    xs = {m: i8ie.tensor(np.random.default_rng(1234).uniform(-1, 1, (m, 3, 32, 32)).astype(np.float32)).prefetch() for m in args.batches}

    def evaluate(tag):
        preds = {}
        for m, x in xs.items():
            model(x).numpy()  # warm-up
            i8ie.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                y = model(x)
            preds[m] = y.numpy().argmax(1)
            dt = (time.perf_counter() - t0) / args.steps
            print("%-6s %5d images  step %8.2f ms  %9.0f img/s" % (tag, m, dt * 1e3, m / dt))
        return preds

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
        ms = sum(v[1] for k, v in prof.items() if k.split("|")[0] in SWIN_KERNELS)
        launches = sum(v[0] for k, v in prof.items() if k.split("|")[0] in SWIN_KERNELS) // args.steps
        print("%5d images: %.3f ms of kernel time per step; shifted-window attention: %d launches, %.3f ms (%.1f %%)"
              % (m, total / args.steps, launches, ms / args.steps, 100.0 * ms / total))
    for m in xs:
        print("%5d images: INT8 argmax agrees with FP32 argmax on %.2f %% of the synthetic images" % (m, 100.0 * (fp32[m] == int8[m]).mean()))


if __name__ == "__main__":
    main()
