#!/usr/bin/env python3
"""MobileNetV2 at width 1.0 for 32x32 CIFAR-10 (Sandler et al. 2018, table 2: inverted residual blocks of 1x1 expansion, depthwise 3x3 and linear 1x1 projection, relu6 throughout; the stem and the second stage at stride 1) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and top-1.  Not in the reference: it has no relu6, no depthwise convolution and no residual add."""
from _common import run

if __name__ == "__main__":
    run("mobilenetv2_cifar", __doc__)
