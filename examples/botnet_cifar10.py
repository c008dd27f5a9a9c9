#!/usr/bin/env python3
"""A ResNet-style network for 32x32 CIFAR-10 whose last stage replaces the 3x3 convs of its bottleneck blocks with 4-head self-attention (BoTNet, Srinivas et al. 2021, without the relative-position term) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Each attention block is one packed 1x1 conv c -> 3c and one fused launch (i8ie.Attention); the 1 / sqrt(d) factor is folded into the query filters.  Runs on seeded synthetic weights and inputs."""
from _common import run


def report(model):
    for a in ("b1attn", "b2attn"):
        print("%s: score qparams %s, output qparams %s" % (a, getattr(model, a).score_qparams(), getattr(model, a).output_qparams()))


if __name__ == "__main__":
    run("botnet_cifar", __doc__, report)
