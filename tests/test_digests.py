"""Committed SHA-256 digests of full-size AlexNet outputs (tests/golden/alexnet_digests.json, written by
tests/golden/make_digests.py): the oracle's per-layer u8 outputs and logits at fixed seeds and fixed output
qparams.  The CPU test replays the oracle alone, so an edit that changes the oracle's arithmetic is caught even
if the kernels are changed the same way in the same round; the GPU tests hold the product
to the same digests at the batch sizes BASELINE.json names (100 and 1000) and check that the seeded calibration
still produces the fixture's qparams."""
import json
import os
import struct

import numpy as np
import pytest

import support
from conftest import GOLDEN

FIX = json.load(open(os.path.join(GOLDEN, "alexnet_digests.json")))


def _qparams():
    return {a: (np.float32(struct.unpack("<f", bytes.fromhex(v["scale_f32_hex"]))[0]), int(v["zero_point"]))
            for a, v in FIX["qparams"].items()}


@pytest.mark.parametrize("case", [c for c in FIX["cases"] if c["batch"] <= 100], ids=lambda c: "batch%d" % c["batch"])
def test_oracle_reproduces_committed_digests(orc, case):
    import pipeline
    from int8inferenceengine_amd import workloads as wl

    entry = wl.NETWORKS["alexnet"]
    sd = wl.synthetic_state_dict("alexnet", seed=FIX["weights_seed"])
    qlayers = pipeline.quantize_layers(entry, sd)
    x = wl.synthetic_input("alexnet", case["batch"], seed=case["input_seed"])
    cap = {}
    logits = pipeline.forward(entry, x, qlayers, _qparams(), capture=cap)
    got = {k: support.sha(v) for k, v in cap.items() if isinstance(v, np.ndarray)}
    got["_logits_f32"] = support.sha(logits)
    assert got == case["sha256"]


@pytest.fixture(scope="module")
def calibrated_alexnet():
    import int8inferenceengine_amd  # noqa: F401
    from int8inferenceengine_amd import workloads as wl

    return wl.calibrated("alexnet", wl.synthetic_state_dict("alexnet", seed=FIX["weights_seed"]))


@pytest.mark.gpu
def test_seeded_calibration_reproduces_the_fixture_qparams(calibrated_alexnet):
    from int8inferenceengine_amd import workloads as wl

    want = _qparams()
    for a in wl.layer_names("alexnet"):
        s, z = getattr(calibrated_alexnet, a).output_qparams()
        assert np.float32(s) == want[a][0] and int(z) == want[a][1], a


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: "batch%d" % c["batch"])
def test_gpu_alexnet_matches_committed_digests(calibrated_alexnet, case):
    """Whole-network parity at BASELINE batch sizes: logits bit-identical to the oracle's (digest), and, at batch
    100 and 1000, directly against a fresh oracle run as well (sample/notebooks/AlexNet_cifar10_resize224.ipynb:212-218)."""
    import i8ie
    import pipeline
    from int8inferenceengine_amd import workloads as wl

    x = wl.synthetic_input("alexnet", case["batch"], seed=case["input_seed"])
    got = calibrated_alexnet(i8ie.tensor(x)).numpy()
    assert support.sha(got) == case["sha256"]["_logits_f32"]
    entry = wl.NETWORKS["alexnet"]
    qlayers = pipeline.quantize_layers(entry, wl.synthetic_state_dict("alexnet", seed=FIX["weights_seed"]))
    want = pipeline.forward(entry, x, qlayers, _qparams())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
