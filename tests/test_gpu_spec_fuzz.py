"""Seeded random networks over the whole op grammar (tests/spec_fuzz.py) through the `i8ie` surface, bit for bit against the
numpy interpreter (tests/spec_ref.py): the deferred-op machinery of the binding -- pending nodes, bordered NHWC storage,
re-bias and relu folding, two consumers of one pending tensor -- sees producer / consumer pairs nobody wrote down.  Each case
runs eager, under force-fallback, as two replays of one HIP graph and a second time eager (cached borders and layouts).
I8IE_FUZZ_CASES scales the case count as it scales tests/test_gpu_fuzz.py (default 48 there: 32 cases here)."""
import os

import numpy as np
import pytest

import net_cases as nc
import spec_fuzz as sf
import spec_ref as sr
from support import i8ie, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
N_CASES = int(os.environ.get("I8IE_FUZZ_CASES", "48"))
N_PROVEN = 32   # tests/test_spec_fuzz_host.py: N_DEFAULT


def _run(i8ie, case, name, guard=True):
    from int8inferenceengine_amd import workloads as wl

    entry, per_channel, batch = case["entry"], case["per_channel"], case["batch"]
    wl.NETWORKS[name], wl.FOLDS[name] = entry, case["folds"]
    try:
        sd = wl.synthetic_state_dict(name, case["weight_seed"])
        calib = wl.synthetic_input(name, sf.calib_images(entry), seed=case["calib_seed"])
        net = wl.calibrated(name, sd, calib_batch=calib, per_channel=per_channel)
        qp = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
        jqp = {a: nc.qparams_of(net, a) for a in wl.join_names(name) + [a + sr.mhr.SCORES for a in wl.attention_names(name)]}
        x = wl.synthetic_input(name, batch, seed=case["input_seed"])
        traced = []
        want = sr.forward(entry, x, sr.quantize_layers(entry, sd, per_channel), qp, jqp, per_channel, sf.collect(traced))
        text = "%s\nbatch %d per_channel %s" % (sf.describe(entry), batch, per_channel)
        # The guard on the bytes compared here (the product's calibration differs from spec_ref.fp32_qparams): asserted for the
        # cases tests/test_spec_fuzz_host.py proves it for.  Beyond them (a hunt with I8IE_FUZZ_CASES raised) it is a condition on
        # the reference that a few random cases in a thousand miss: printed, since a red case has to mean the product.
        if guard:
            sf.assert_discriminates(traced, want, text)
        else:
            print("discrimination (rich, saturated): %.3f %.3f" % sf.discrimination(traced))
        try:
            nc.check_bit_exact(i8ie, net, name, x, want, fallback=True, graph=True)
            assert same_bits(net(i8ie.tensor(x)).numpy(), want), "second eager forward"
        except AssertionError as e:
            raise AssertionError("%s: first divergence: %s\n%s" % (e, sf.first_divergence(i8ie, net, name, x, traced), text)) from None
    finally:
        del wl.NETWORKS[name], wl.FOLDS[name]


@pytest.mark.parametrize("index", range(max(N_CASES * 2 // 3, 8)))
def test_random_grammar_network_against_spec_ref(i8ie, index):
    _run(i8ie, sf.case(index), "_spec_fuzz_%d" % index, guard=index < N_PROVEN)


def test_padded_pools_in_a_hand_written_network(i8ie):
    """groupnorm_tiny with its max-pool as ("pool", 3, 2, 1) and an ("avgpool", 3, 2, 1, True, False) ahead of the head: the
    padded pools inside a real chain, whatever the generator draws"""
    _run(i8ie, sf.padpool_case(), "_spec_fuzz_padpool")
