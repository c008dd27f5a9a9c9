#!/usr/bin/env python3
"""AlexNet on 224x224 CIFAR-10 with 4-bit fc layers: convert(per_channel=True, weight_bits=4) keeps the convs INT8 with per-channel
scales and stores fc6, fc7 and fc8 (58 of the 61 million parameters) as packed nibbles; FP32 run, prepare/convert, INT8 run, timing and top-1.
--group-size 64 | 128 | 256 (default: off) gives the fc layers group-wise scales along in_features (convert(group_size=))."""
import argparse
import sys

from _common import run


def report(model):
    bits = {a: getattr(model, a).weight_bits() for a, v in model.__dict__.items() if hasattr(v, "weight_bits")}
    saved = {k: v.nbytes for k, v in model.quantized_state_dict().items()}
    print("weight bits per layer: %s" % bits)
    print("group size per layer: %s" % {a: getattr(model, a).group_size() for a in bits})
    print("saved model: %.1f MB, of which %.1f MB packed 4-bit weights" % (sum(saved.values()) / 1e6, sum(v for k, v in saved.items() if k.endswith(".q_weight4")) / 1e6))


if __name__ == "__main__":
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--group-size", type=int, choices=(64, 128, 256), default=None)
    args, sys.argv[1:] = own.parse_known_args()
    run("alexnet", __doc__, report=report, convert={"per_channel": True, "weight_bits": 4, "group_size": args.group_size})
