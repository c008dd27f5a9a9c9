#!/usr/bin/env python3
"""ResNet-18 for 32x32 CIFAR-10 with one non-local (self-attention) block after stage 3 (256 channels at 8x8, projection width 128; Wang et al. 2018) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Not in the reference: it has no op that contracts two activation tensors, and no softmax.  Runs on seeded synthetic weights and inputs."""
from _common import run

if __name__ == "__main__":
    run("nonlocal_resnet_cifar", __doc__)
