#!/usr/bin/env python3
"""ResNet-18 for 32x32 CIFAR-10 (He et al. 2015: 3x3 stem, no stem max-pool, four stages of two basic blocks, global average pool, fc) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and top-1.  Not in the reference: it has neither an add nor an average pool."""
from _common import run

if __name__ == "__main__":
    run("resnet18_cifar", __doc__)
