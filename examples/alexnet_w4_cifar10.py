#!/usr/bin/env python3
"""AlexNet on 224x224 CIFAR-10 with 4-bit fc layers: convert(per_channel=True, weight_bits=4) keeps the convs INT8 with per-channel
scales and stores fc6, fc7 and fc8 (58 of the 61 million parameters) as packed nibbles; FP32 run, prepare/convert, INT8 run, timing and top-1."""
from _common import run


def report(model):
    bits = {a: getattr(model, a).weight_bits() for a, v in model.__dict__.items() if hasattr(v, "weight_bits")}
    saved = {k: v.nbytes for k, v in model.quantized_state_dict().items()}
    print("weight bits per layer: %s" % bits)
    print("saved model: %.1f MB, of which %.1f MB packed 4-bit weights" % (sum(saved.values()) / 1e6, sum(v for k, v in saved.items() if k.endswith(".q_weight4")) / 1e6))


if __name__ == "__main__":
    run("alexnet", __doc__, report=report, convert={"per_channel": True, "weight_bits": 4})
