#!/usr/bin/env python3
"""The "bilinear" U-Net for 32x32 CIFAR-10 images (unet_cifar10.py's network with each 2x2 stride-2 transposed convolution replaced by a bilinear x2 upsample and a 1x1 convolution to the skip's width, the usual replacement for up-convs) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and the agreement of the per-pixel argmax over the 10 maps (run it without --data labels: the output is a map per class, not a label per image).  Not in the reference: it has no resize op and no concatenation."""
from _common import run

if __name__ == "__main__":
    run("unet_bilinear_cifar", __doc__)
