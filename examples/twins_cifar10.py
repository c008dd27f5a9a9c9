#!/usr/bin/env python3
"""A Twins-SVT for 32x32 input (Chu et al. 2021, scaled down): two stages, 64 channels at 16x16 (patch conv 2x2 stride 2, 2 heads
of d = 32) and 128 channels at 8x8 (patch conv 2x2 stride 2, 4 heads of d = 32).  Each stage is a locally grouped block --
Attention(heads, window=4) over the non-overlapping 4x4 windows of the map -- the conditional position encoding (a depthwise 3x3
conv plus Add), and a globally sub-sampled block, whose keys and values come from a stride-2 conv of the map (Tq = 4 Tk).  Blocks
are pre-LN with hardswish MLPs (where the paper has GELU); the 1/sqrt(d) of every attention is folded into its q projection.  Then
LayerNorm, global average pool and Linear(128, 10).  On the MI355X engine: FP32 run, prepare / convert, INT8 run, the step time
at 1000 and 125 images, the share of the windowed attention launches in the INT8 step's kernel time, and the agreement of the
FP32 and INT8 argmaxes.
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

STAGES = [(64, 2, 16), (128, 4, 8)]   # channels, heads, map side
WINDOW, MLP_RATIO = 4, 2


def make_model(i8ie):
    class Twins(i8ie.Module):
        def __init__(self):
            super().__init__()
            cin = 3
            for s, (c, heads, _) in enumerate(STAGES):
                p = "s%d_" % s
                setattr(self, p + "patch", i8ie.Conv2d(cin, c, 2, stride=2))
                for kind in ("l", "g"):   # the locally grouped block, then the globally sub-sampled one
                    q = p + kind + "_"
                    setattr(self, q + "ln1", i8ie.LayerNorm(c))
                    setattr(self, q + "attn", i8ie.Attention(heads, window=WINDOW if kind == "l" else None))
                    setattr(self, q + "proj", i8ie.Conv2d(c, c, 1))
                    setattr(self, q + "add1", i8ie.Add())
                    setattr(self, q + "ln2", i8ie.LayerNorm(c))
                    setattr(self, q + "fc1", i8ie.Conv2d(c, MLP_RATIO * c, 1))
                    setattr(self, q + "act", i8ie.Activation("hardswish"))
                    setattr(self, q + "fc2", i8ie.Conv2d(MLP_RATIO * c, c, 1))
                    setattr(self, q + "add2", i8ie.Add())
                setattr(self, p + "l_qkv", i8ie.Conv2d(c, 3 * c, 1))
                setattr(self, p + "pos", i8ie.Conv2d(c, c, 3, padding=1, groups=c))
                setattr(self, p + "pos_add", i8ie.Add())
                setattr(self, p + "g_q", i8ie.Conv2d(c, c, 1))
                setattr(self, p + "g_sr", i8ie.Conv2d(c, c, 2, stride=2))
                setattr(self, p + "g_k", i8ie.Conv2d(c, c, 1))
                setattr(self, p + "g_v", i8ie.Conv2d(c, c, 1))
                cin = c
            self.ln = i8ie.LayerNorm(cin)
            self.head = i8ie.Linear(cin, 10)

        def forward(self, x):
            for s in range(len(STAGES)):
                L = lambda name: getattr(self, "s%d_%s" % (s, name))  # noqa: E731
                x = L("patch")(x)
                x = L("l_add1")(x, L("l_proj")(L("l_attn")(L("l_qkv")(L("l_ln1")(x)))))
                x = L("l_add2")(x, L("l_fc2")(L("l_act")(L("l_fc1")(L("l_ln2")(x)))))
                x = L("pos_add")(x, L("pos")(x))
                y = L("g_ln1")(x)
                r = L("g_sr")(y)
                x = L("g_add1")(x, L("g_proj")(L("g_attn")(L("g_q")(y), L("g_k")(r), L("g_v")(r))))
                x = L("g_add2")(x, L("g_fc2")(L("g_act")(L("g_fc1")(L("g_ln2")(x)))))
            x = i8ie.adaptive_avg_pool2d(self.ln(x), 1)
            return self.head(x.reshape(-1, STAGES[-1][0]))

    return Twins()


def synthetic_state_dict(seed=0):
    """seeded weights: Xavier-uniform projections (every q projection scaled by 1/sqrt(d)), LayerNorms near the identity"""
    rng = np.random.default_rng(seed)
    sd = {}

    def dense(name, cout, cin, k=1, conv=True, groups=1):
        lim = np.sqrt(6.0 / (cin // groups * k * k + cout // groups))
        sd[name + ".weight"] = rng.uniform(-lim, lim, (cout, cin // groups, k, k) if conv else (cout, cin)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-0.02, 0.02, cout).astype(np.float32)

    def norm(name, c):
        sd[name + ".weight"] = rng.normal(1.0, 0.05, c).astype(np.float32)
        sd[name + ".bias"] = rng.normal(0.0, 0.05, c).astype(np.float32)

    cin = 3
    for s, (c, heads, _) in enumerate(STAGES):
        p = "s%d_" % s
        scale = np.float32(1.0 / np.sqrt(c // heads))
        dense(p + "patch", c, cin, 2)
        for kind in ("l", "g"):
            q = p + kind + "_"
            norm(q + "ln1", c)
            dense(q + "proj", c, c)
            norm(q + "ln2", c)
            dense(q + "fc1", MLP_RATIO * c, c)
            dense(q + "fc2", c, MLP_RATIO * c)
        dense(p + "l_qkv", 3 * c, c)
        sd[p + "l_qkv.weight"][:c] *= scale
        sd[p + "l_qkv.bias"][:c] *= scale
        dense(p + "pos", c, c, 3, groups=c)
        dense(p + "g_q", c, c)
        sd[p + "g_q.weight"] *= scale
        sd[p + "g_q.bias"] *= scale
        dense(p + "g_sr", c, c, 2)
        dense(p + "g_k", c, c)
        dense(p + "g_v", c, c)
        cin = c
    norm("ln", cin)
    dense("head", 10, cin, conv=False)
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
        for label, names in (("windowed attention", ("attn_mfma_win", "attn_direct_win")), ("global attention", ("attn_mfma", "attn_direct"))):
            ms = sum(v[1] for k, v in prof.items() if k.split("|")[0] in names)
            launches = sum(v[0] for k, v in prof.items() if k.split("|")[0] in names) // args.steps
            line += "; %s: %d launches, %.3f ms (%.1f %%)" % (label, launches, ms / args.steps, 100.0 * ms / total)
        print(line)
    for m in xs:
        print("%5d images: INT8 argmax agrees with FP32 argmax on %.2f %% of the synthetic images" % (m, 100.0 * (fp32[m] == int8[m]).mean()))


if __name__ == "__main__":
    main()
