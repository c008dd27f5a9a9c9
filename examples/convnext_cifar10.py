#!/usr/bin/env python3
"""A ConvNeXt for 32x32 CIFAR-10 (patchify stem 2x2 s2, stages of (2, 2, 2, 2) blocks at 64 / 128 / 256 / 512 channels, each block depthwise 7x7 -> LayerNorm -> 1x1 to 4c -> hardswish -> 1x1 back -> residual add; Liu et al. 2022) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and agreement of the two.  Not in the reference: it has no normalisation that is computed at run time.  Runs on seeded synthetic weights and inputs."""
import argparse
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on the path)

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--save-quantized", help="write the converted model to this .npz")
    args = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch first)
    import int8inferenceengine_amd  # noqa: F401
    import i8ie
    from int8inferenceengine_amd import convnext_net as nl

    model = nl.build("cifar")
    model.load(nl.synthetic_state_dict("cifar"))
    xs = nl.synthetic_input("cifar", args.batch * args.batches, seed=1234)
    tens = [i8ie.tensor(xs[i:i + args.batch]).prefetch() for i in range(0, len(xs), args.batch)]

    def evaluate(tag):
        i8ie.synchronize()
        t0 = time.perf_counter()
        preds = [i8ie.argmax(model(x), axis=1).numpy() for x in tens]
        dt = time.perf_counter() - t0
        preds = np.concatenate(preds).astype(np.int64)
        print("%-18s %8.1f ms  %10.0f img/s" % (tag, dt * 1e3, len(preds) / dt))
        return preds

    evaluate("FP32 (warm-up)")
    p_fp32 = evaluate("FP32")
    t0 = time.perf_counter()
    model.prepare()
    model(tens[0])
    model.convert()
    print("%-18s %8.1f ms" % ("prepare+convert", (time.perf_counter() - t0) * 1e3))
    evaluate("INT8 (warm-up)")
    p_int8 = evaluate("INT8")
    print("no labels: INT8 argmax agrees with FP32 argmax on %.2f %% of %d synthetic images" % (100.0 * (p_fp32 == p_int8).mean(), len(p_int8)))
    if args.save_quantized:
        model.save_quantized(args.save_quantized)
        again = nl.build("cifar")
        again.load_quantized_file(args.save_quantized)
        print("saved %s; reloaded model reproduces the logits: %s" % (args.save_quantized, np.array_equal(again(tens[0]).numpy(), model(tens[0]).numpy())))
