#!/usr/bin/env python3
"""U-Net for 32x32 CIFAR-10 images (Ronneberger et al. 2015 at widths 64 / 128 / 256 / 512: two padded 3x3 convolutions per level, 2x2 max-pools down, 2x2 stride-2 transposed convolutions up, the skips joined by channel concatenation, a 1x1 head to 10 maps) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and the agreement of the per-pixel argmax over the 10 maps (run it without --data labels: the output is a map per class, not a label per image).  Not in the reference: it has no transposed convolution and no concatenation."""
from _common import run

if __name__ == "__main__":
    run("unet_cifar", __doc__)
