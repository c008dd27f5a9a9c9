#!/usr/bin/env python3
"""ResNet-18 for 32x32 CIFAR-10 (He et al. 2015: 3x3 stem, no stem max-pool, four stages of two basic blocks, global average pool, fc) on the MI355X engine: FP32 run, prepare/convert, INT8 run, timing and top-1.  Not in the reference: it has neither an add nor an average pool.  --weight-bits 4: every 3x3 conv and strided shortcut with in_channels % 32 == 0 and the fc as packed 4-bit weights (Module.convert(weight_bits=4, spatial=True)); prints the live device bytes of the layer handles against an INT8 conversion of the same model."""
import sys

from _common import run


def handle_bytes(convert):
    """live device bytes that converting a calibrated resnet18_cifar adds: its layer handles"""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd import workloads as wl
    cx.trim()
    before = cx.memory_stats()[0]
    net = wl.calibrated("resnet18_cifar", **convert)
    cx.trim()
    grown = cx.memory_stats()[0] - before
    del net
    return grown


if __name__ == "__main__":
    four = "--weight-bits" in sys.argv and sys.argv[sys.argv.index("--weight-bits") + 1] == "4"
    if "--weight-bits" in sys.argv:
        at = sys.argv.index("--weight-bits")
        del sys.argv[at:at + 2]

    def report(model):
        w4, i8 = handle_bytes(dict(weight_bits=4, spatial=True)), handle_bytes({})
        print("layer handles: W4 %.2f MB, INT8 %.2f MB (%.3f of INT8)" % (w4 / 1e6, i8 / 1e6, w4 / max(i8, 1)))

    run("resnet18_cifar", __doc__, report if four else None, dict(weight_bits=4, spatial=True) if four else None)
