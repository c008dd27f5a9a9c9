#!/usr/bin/env python3
"""A Vision Transformer for 32x32 input (Dosovitskiy et al. 2021, scaled down to ViT-Tiny's width): patch conv 4x4 stride 4 to
192 channels (64 tokens) -> PositionEmbedding(192, 8, 8, class_token=True) -> six pre-LN encoder blocks (LayerNorm, qkv 1x1 conv,
Attention with 3 heads of d = 64, proj 1x1, Add; LayerNorm, 1x1 to 768, hardswish, 1x1 to 192, Add) -> LayerNorm -> the class column
(crop) -> Linear(192, 10).  The token map is [n, 192, 1, 65]; the 1/sqrt(d) of the attention is folded into the q third of the
qkv projection; hardswish stands where the paper has GELU, which the engine does not have.  On the MI355X engine: FP32 run,
prepare / convert, INT8 run, the step time at 1000 and 125 images, the share of the posembed launch and of the activation lookups
in the INT8 step's kernel time, and the agreement of the FP32 and INT8 argmaxes.
Self-contained: the network is written out below as an i8ie.Module.  Seeded synthetic weights and input (no checkpoint is
shipped).  Not in the reference: it has no attention, normalisation or embedding op."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTH, HEADS, MLP, DEPTH, GRID = 192, 3, 768, 6, 8


def make_model(i8ie):
    class ViT(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.patch = i8ie.Conv2d(3, WIDTH, 4, stride=4)
            self.pos = i8ie.PositionEmbedding(WIDTH, GRID, GRID, class_token=True)
            for b in range(DEPTH):
                p = "b%d_" % b
                setattr(self, p + "ln1", i8ie.LayerNorm(WIDTH))
                setattr(self, p + "qkv", i8ie.Conv2d(WIDTH, 3 * WIDTH, 1))
                setattr(self, p + "attn", i8ie.Attention(HEADS))
                setattr(self, p + "proj", i8ie.Conv2d(WIDTH, WIDTH, 1))
                setattr(self, p + "add1", i8ie.Add())
                setattr(self, p + "ln2", i8ie.LayerNorm(WIDTH))
                setattr(self, p + "fc1", i8ie.Conv2d(WIDTH, MLP, 1))
                setattr(self, p + "act", i8ie.Activation("hardswish"))
                setattr(self, p + "fc2", i8ie.Conv2d(MLP, WIDTH, 1))
                setattr(self, p + "add2", i8ie.Add())
            self.ln = i8ie.LayerNorm(WIDTH)
            self.head = i8ie.Linear(WIDTH, 10)

        def forward(self, x):
            x = self.pos(self.patch(x))  # [n, 192, 1, 65]
            for b in range(DEPTH):
                L = lambda name: getattr(self, "b%d_%s" % (b, name))  # noqa: E731
                x = L("add1")(x, L("proj")(L("attn")(L("qkv")(L("ln1")(x)))))
                x = L("add2")(x, L("fc2")(L("act")(L("fc1")(L("ln2")(x)))))
            x = self.ln(x)
            return self.head(i8ie.crop(x, 0, 0, 1, 1).reshape(-1, WIDTH))

    return ViT()


def synthetic_state_dict(seed=0):
    """seeded weights: Xavier-uniform projections (the q third of every qkv scaled by 1/sqrt(d)), a N(0, 0.02) position table
    and class token, LayerNorms near the identity"""
    rng = np.random.default_rng(seed)
    sd = {}

    def dense(name, cout, cin, k=1, conv=True):
        lim = np.sqrt(6.0 / (cin * k * k + cout))
        sd[name + ".weight"] = rng.uniform(-lim, lim, (cout, cin, k, k) if conv else (cout, cin)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.02, 0.02, cout).astype(np.float32)

    def norm(name):
        sd[name + ".weight"] = rng.normal(1.0, 0.05, WIDTH).astype(np.float32)
        sd[name + ".bias"] = rng.normal(0.0, 0.05, WIDTH).astype(np.float32)

    dense("patch", WIDTH, 3, 4)
    sd["pos.weight"] = rng.normal(0, 0.02, (GRID * GRID + 1, WIDTH)).astype(np.float32)
    sd["pos.bias"] = rng.normal(0, 0.02, WIDTH).astype(np.float32)
    for b in range(DEPTH):
        p = "b%d_" % b
        norm(p + "ln1")
        dense(p + "qkv", 3 * WIDTH, WIDTH)
        scale = np.float32(1.0 / np.sqrt(WIDTH // HEADS))  # the attention's 1/sqrt(d), folded into the q projection
        sd[p + "qkv.weight"][:WIDTH] *= scale
        sd[p + "qkv.bias"][:WIDTH] *= scale
        dense(p + "proj", WIDTH, WIDTH)
        norm(p + "ln2")
        dense(p + "fc1", MLP, WIDTH)
        dense(p + "fc2", WIDTH, MLP)
    norm("ln")
    dense("head", 10, WIDTH, conv=False)
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
        line = "%5d images: %.3f ms of kernel time per step" % (m, total / args.steps)
        for label, prefix in (("posembed", "posembed_"), ("activation lookups", "lut_u8")):
            ms = sum(v[1] for k, v in prof.items() if k.startswith(prefix))
            launches = sum(v[0] for k, v in prof.items() if k.startswith(prefix)) // args.steps
            line += "; %s: %d launches, %.3f ms (%.1f %%)" % (label, launches, ms / args.steps, 100.0 * ms / total)
        print(line)
    for m in xs:
        print("%5d images: INT8 argmax agrees with FP32 argmax on %.2f %% of the synthetic images" % (m, 100.0 * (fp32[m] == int8[m]).mean()))


if __name__ == "__main__":
    main()
