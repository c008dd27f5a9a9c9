#!/usr/bin/env python3
"""MobileNetV3-small for 32x32 CIFAR-10 (Howard et al. 2019, table 2: inverted residual blocks with 3x3 and 5x5 depthwise convolutions, hardswish, and squeeze-and-excitation -- a global average pool, two Linears, a hardsigmoid and a broadcast multiply -- behind nine of the eleven depthwise convolutions; the stem and the first block at stride 1) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and top-1.  Not in the reference: it has no hardswish, no depthwise convolution, no residual add and no multiply."""
from _common import run

if __name__ == "__main__":
    run("mobilenetv3_small_cifar", __doc__)
