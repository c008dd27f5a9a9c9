#!/usr/bin/env python3
"""SqueezeNet 1.1 for 32x32 CIFAR-10 (Iandola et al. 2016: 3x3 stem, eight fire modules, floor-mode max-pools, 1x1 classifier conv, global average pool) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and top-1.  Not in the reference: it has no channel concatenation."""
from _common import run

if __name__ == "__main__":
    run("squeezenet_cifar", __doc__)
