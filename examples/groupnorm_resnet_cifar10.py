#!/usr/bin/env python3
"""A GroupNorm ResNet-18 for 32x32 CIFAR-10 (Wu & He 2018: resnet18_cifar's topology with GroupNorm(32, c) behind every conv) with one diffusion-style residual block at 8x8 (GroupNorm, SiLU written as x * sigmoid(x), 3x3 conv, 4-head self-attention, skips) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Runs on seeded synthetic weights and inputs."""
from _common import run

if __name__ == "__main__":
    run("groupnorm_resnet_cifar", __doc__)
