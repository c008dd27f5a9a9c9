#!/usr/bin/env python3
"""A ConvNeXt for 32x32 CIFAR-10 (patchify stem 2x2 s2, stages of (2, 2, 2, 2) blocks at 64 / 128 / 256 / 512 channels, each block depthwise 7x7 -> LayerNorm -> 1x1 to 4c -> hardswish -> 1x1 back -> residual add; Liu et al. 2022) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Not in the reference: it has no normalisation that is computed at run time.  Runs on seeded synthetic weights and inputs."""
from _common import run

if __name__ == "__main__":
    run("convnext_cifar", __doc__)
