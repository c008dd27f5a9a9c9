#!/usr/bin/env python3
"""DeepLabV3 for 32x32 CIFAR-10 images (resnet18_cifar10.py's stem and stages 1-3, stage 4 kept at stride 1 with its 3x3 convolutions dilated at rate 2, an atrous spatial pyramid with a 1x1 branch, three 3x3 branches at rates 2 / 4 / 6 and the image-pool branch, a 1x1 head to 10 maps and a bilinear x4 upsample) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and the agreement of the per-pixel argmax over the 10 maps (run it without --data labels: the output is a map per class, not a label per image).  Random weights.  Not in the reference: its Conv2d has no dilation, and it has no resize op and no concatenation."""
from _common import run

if __name__ == "__main__":
    run("deeplabv3_cifar", __doc__)
