#!/usr/bin/env python3
"""single Linear(784,10) on MNIST with 2:4 structured-sparse weights: convert(sparsity="2:4") quantises as usual, then keeps the two
largest of every four weights along in_features and stores them compressed (0.625 of the dense bytes); FP32 run, prepare/convert,
INT8 run, timing and top-1.  784 is no multiple of 32, so this layer runs on sp24lin_direct; a Linear with in_features % 32 == 0
runs on the sparse MFMA kernel."""
from _common import run


def report(model):
    kept = {a: v.sparsity() for a, v in model.__dict__.items() if hasattr(v, "sparsity")}
    saved = {k: v.nbytes for k, v in model.quantized_state_dict().items()}
    print("sparsity per layer: %s" % kept)
    print("saved model: %d bytes, of which %d compressed values and %d positions" % (
        sum(saved.values()), sum(v for k, v in saved.items() if k.endswith(".q_weight24")), sum(v for k, v in saved.items() if k.endswith(".q_index24"))))


if __name__ == "__main__":
    run("mnist_fc", __doc__, report=report, convert={"sparsity": "2:4"})
