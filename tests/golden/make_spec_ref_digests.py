"""Records tests/golden/spec_ref_digests.json: sha256 digests of what the numpy spec interpreter (tests/spec_ref.py) gives for
every case of tests/spec_ref_cases.py -- the logits and traced tensors of every registry network at two images, per tensor and
per channel, and the parameters of the float64 calibration stand-in.

The committed table was recorded before spec_ref existed, from the interpreters it replaced, each network through the one its
tests called: pipeline.forward / pc_pipeline.forward_pc (alexnet, simple_conv, two_conv, mnist_fc), grouped_ref.forward
(alexnet_paper), add_ref.forward (resnet_tiny), avgpool_ref.forward (resnet_tiny_gap, resnet18_cifar), concat_ref.forward (the
fire networks), act_ref.forward and fp32_qparams (the MobileNetV2s, act_tiny), mul_ref.forward and fp32_qparams (se_tiny,
mobilenetv3_small_cifar), deconv_ref.forward and fp32_qparams (the U-Nets), upsample_ref.forward (upsample_tiny,
unet_bilinear_cifar) and dilated_ref.forward (aspp_tiny, deeplabv3_cifar); later, the same way, attention_ref.nonlocal_forward
and nonlocal_fp32_qparams (the non-local networks) and the ConvNeXt walk of tests/test_gpu_layernorm.py with a float64 stand-in
written beside it (the ConvNeXts), and mha_ref.net_forward and the GroupNorm walk of tests/test_gpu_groupnorm.py (mha_tiny,
groupnorm_tiny; botnet_cifar and groupnorm_resnet_cifar had no walk before spec_ref's, so their entries pin the interpreter
and prove nothing more).  Those are gone, so this script now records what spec_ref gives.  Run it on a tree whose expected bytes are the ones to keep, never to make a failing replay pass:

    python tests/golden/make_spec_ref_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import spec_ref_cases as sc  # noqa: E402


def main():
    table = {"%s-%s" % (name, "pc" if pc else "pt"): sc.case(name, pc) for name in sc.FAMILY for pc in (False, True)}
    with open(os.path.join(HERE, "spec_ref_digests.json"), "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d traced tensors" % (len(table), sum(len(c["trace"]) for c in table.values())))


if __name__ == "__main__":
    main()
