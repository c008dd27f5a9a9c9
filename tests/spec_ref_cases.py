"""The cases behind tests/golden/spec_ref_digests.json: every registry network through the numpy spec interpreter at two
images, per tensor and per channel, with fixed seeds and fixed output parameters, reduced to sha256 digests.  A helper module,
not a conftest.  tests/golden/make_spec_ref_digests.py records the table, tests/test_spec_ref_host.py replays it.

  FAMILY          which op family's tests own a network (it decides what is traced, and whether the float64 stand-in for
                  calibration or synthetic parameters give the output (scale, zero_point)s)
  case(...)       the digests of one (network, per_channel): logits, every traced tensor, and the stand-in's parameters"""
import zlib

import numpy as np

import attention_ref as atr
import deconv_ref as dr
import groupnorm_ref as gnr
import layernorm_ref as lnr
import mha_ref as mhr
import mul_ref as mr
import spec_ref as sr
import upsample_ref as ur
from support import sha

BATCH = 2
FAMILY = {
    "alexnet": "plain", "simple_conv": "plain", "two_conv": "plain", "mnist_fc": "plain", "alexnet_paper": "plain",
    "resnet_tiny": "plain", "resnet_tiny_gap": "plain", "resnet18_cifar": "plain",
    "fire_tiny": "concat", "squeezenet_cifar": "concat",
    "mobilenetv2_tiny": "act", "act_tiny": "act", "mobilenetv2_cifar": "act",
    "se_tiny": "mul", "mobilenetv3_small_cifar": "mul",
    "unet_tiny": "deconv", "unet_cifar": "deconv",
    "upsample_tiny": "upsample", "unet_bilinear_cifar": "upsample", "aspp_tiny": "upsample", "deeplabv3_cifar": "upsample",
    "nonlocal_tiny": "attention", "nonlocal_resnet_cifar": "attention",
    "convnext_tiny": "layernorm", "convnext_cifar": "layernorm",
    "mha_tiny": "mha", "botnet_cifar": "mha", "groupnorm_tiny": "groupnorm", "groupnorm_resnet_cifar": "groupnorm",
}
# the families whose host tests take their parameters from fp32_qparams
CALIBRATED = ("act", "mul", "deconv", "attention", "layernorm", "mha", "groupnorm")


def synthetic_qparams(attrs):
    """a fixed (scale in [0.02, 0.06), zero_point in [64, 192)) per attribute name"""
    out = {}
    for a in attrs:
        h = zlib.crc32(a.encode())
        out[a] = (float(np.float32(0.02 + (h % 1000) * 4e-5)), 64 + (h >> 10) % 128)
    return out


def trace_digests(trace):
    """a dict {attr: bytes} or {attr: (gate, bytes, floor)}, or a list [(op, bytes)] -> {key: digest(s)}"""
    if isinstance(trace, list):
        return {"%d:%r" % (i, op): sha(q) for i, (op, q) in enumerate(trace)}
    return {a: [None if v[0] is None else sha(v[0]), sha(v[1]), v[2]] if isinstance(v, tuple) else sha(v) for a, v in trace.items()}


def run(family, entry, x, qlayers, qp, jqp, per_channel):
    """(logits, what the family's tests trace) of one forward"""
    layers, spec, _ = entry
    trace = [] if family == "upsample" else {}
    tracer = {"plain": None, "concat": sr.outputs_of("concat", trace), "act": sr.outputs_of("act", trace),
              "mul": mr.tracer(spec, trace), "deconv": dr.tracer(layers, trace), "upsample": ur.tracer(trace),
              "attention": atr.tracer(trace), "layernorm": sr.traces(lnr.tracer(layers, trace), atr.tracer(trace)),
              "mha": mhr.tracer(trace, jqp), "groupnorm": gnr.tracer(layers, trace)}[family]
    return sr.forward(entry, x, qlayers, qp, jqp, per_channel, tracer), trace


_QPARAMS = {}


def case(name, per_channel, run=run, fp32_qparams=None, quantize_layers=None):
    """the digests of one network; the three functions default to spec_ref's"""
    from int8inferenceengine_amd import workloads as wl

    entry, family = wl.network(name), FAMILY[name]
    sd = wl.synthetic_state_dict(name, sr.WEIGHT_SEED)
    out = {}
    if family in CALIBRATED:
        if name not in _QPARAMS:  # (the same for both values of per_channel)
            _QPARAMS[name] = (fp32_qparams or sr.fp32_qparams)(entry, sd, wl.synthetic_input(name, sr.CALIB_IMAGES, seed=sr.CALIB_SEED))
        qp, jqp = _QPARAMS[name]
        out["qparams"] = {a: [int(np.float32(s).view(np.uint32)), int(zp)] for a, (s, zp) in sorted(dict(qp, **jqp).items())}
    else:
        qp = synthetic_qparams(wl.layer_names(name))
        jqp = synthetic_qparams(wl.join_names(name))
    qlayers = (quantize_layers or sr.quantize_layers)(entry, sd, per_channel)
    logits, trace = run(family, entry, wl.synthetic_input(name, BATCH, seed=sr.INPUT_SEED), qlayers, qp, jqp, per_channel)
    assert logits.dtype == np.float32 and logits.shape[0] == BATCH
    out["logits"], out["distinct"], out["trace"] = sha(logits), int(np.unique(logits).size), trace_digests(trace)
    return out
