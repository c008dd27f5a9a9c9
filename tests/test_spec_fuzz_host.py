"""The random-network generator (tests/spec_fuzz.py) and the reference it feeds (tests/spec_ref.py), checked on the CPU with the
seeds tests/test_gpu_spec_fuzz.py uses: every default spec is well-formed, the numpy interpreter runs it for both weight
quantisations, the sweep as a whole holds every block kind and option at least twice, and the expected bytes discriminate."""
import collections

import numpy as np
import pytest

import spec_fuzz as sf
import spec_ref as sr
from int8inferenceengine_amd import workloads as wl

N_DEFAULT = 32


def _reference(case, per_channel, forward=None, trace=None):
    """(logits, qp, jqp) of a case from the float64 stand-in for calibration: the entry is registered under a private name
    while the synthetic weights and inputs are drawn"""
    name = "_spec_fuzz_host"
    wl.NETWORKS[name], wl.FOLDS[name] = case["entry"], case["folds"]
    try:
        sd = wl.synthetic_state_dict(name, case["weight_seed"])
        calib = wl.synthetic_input(name, sf.calib_images(case["entry"]), seed=case["calib_seed"])
        x = wl.synthetic_input(name, case["batch"], seed=case["input_seed"])
    finally:
        del wl.NETWORKS[name], wl.FOLDS[name]
    qp, jqp = sr.fp32_qparams(case["entry"], sd, calib)
    qlayers = sr.quantize_layers(case["entry"], sd, per_channel)
    return (forward or sr.forward)(case["entry"], x, qlayers, qp, jqp, per_channel, trace), qp, jqp


@pytest.fixture(scope="module")
def cases():
    return [sf.case(i) for i in range(N_DEFAULT)] + [sf.padpool_case()]


def test_every_default_spec_is_well_formed(cases):
    for case in cases:
        layers, spec, shape = case["entry"]
        assert all(op[0] in wl.OPS and op[0] in sr.OPS for op in wl._walk(spec)), sf.describe(case["entry"])
        walked = sf.shapes(case["entry"])    # asserts the legality of every op on what it reads
        named = [op[1] for op, _, _ in walked if op[0] == "layer"]
        assert sorted(named) == sorted(layers), "every layer is used once"
        joins = [op[1] for op in wl._walk(spec) if op[0] in ("add", "mul", "concat", "act", "matmul", "attention")]
        assert len(set(joins + named)) == len(joins) + len(named), "attribute names are unique"
        assert case["batch"] in sf.BATCHES
    inputs = [c["entry"][2] for c in cases[:N_DEFAULT]]
    assert all(c == 3 and 12 <= h <= 32 and 12 <= w <= 32 for c, h, w in inputs)
    assert sum(h != w for _, h, w in inputs) > N_DEFAULT // 2, "non-square inputs"
    assert {c["batch"] for c in cases[:N_DEFAULT]} == set(sf.BATCHES)
    assert all(2 <= sum(op[0] == "save" and op[1].startswith("t") for op in c["entry"][1]) <= 5 for c in cases[:N_DEFAULT])


def test_the_generator_is_deterministic():
    a, b = sf.case(3), sf.case(3)
    assert repr(a) == repr(b)
    assert repr(sf.case(4)["entry"]) != repr(a["entry"])


def test_the_sweep_covers_every_block_kind_and_option(cases):
    """every name of spec_fuzz.REQUIRED occurs in at least two default cases: a fixed seed list silently stops covering an arm
    when the generator is edited, and this is what notices"""
    count = collections.Counter()
    for case in cases[:N_DEFAULT]:
        count.update(sf.features(case["entry"]))
    print(sorted(count.items()))
    assert not [(k, count[k]) for k in sorted(sf.REQUIRED) if count[k] < 2]
    shared = sum(any(op[0] == "branch" and op[1].startswith("t") for op in case["entry"][1]) for case in cases[:N_DEFAULT])
    assert shared >= 2, "a saved tensor read again by a later block"


@pytest.mark.parametrize("index", list(range(N_DEFAULT)) + ["padpool"])
def test_reference_runs_and_its_bytes_discriminate(index):
    """spec_ref.fp32_qparams + spec_ref.forward run the case under both weight quantisations; the logits are finite and not
    constant, at least 90 % of the traced op outputs hold at least 16 distinct byte values, and fewer than half of all traced
    bytes are 0 or 255"""
    case = sf.padpool_case() if index == "padpool" else sf.case(index)
    text = sf.describe(case["entry"]) + "\nbatch %d" % case["batch"]
    for per_channel in (False, True):
        traced = []
        logits, qp, jqp = _reference(case, per_channel, trace=sf.collect(traced))
        assert logits.dtype == np.float32 and np.isfinite(logits).all(), text
        assert logits.shape[0] == case["batch"], text
        assert all(np.isfinite(s) and s > 0 and 0 <= zp <= 255 for s, zp in list(qp.values()) + list(jqp.values())), text
        rich, saturated = sf.assert_discriminates(traced, logits, text)
        print("case %s per_channel %s: %d traced outputs, %.3f rich, %.3f saturated" % (index, per_channel, len(traced), rich,
                                                                                        saturated))


def test_padded_pools_pass_through_the_spec():
    """a pool op with a tail takes padpool_ref's definition in spec_ref.forward and the same output-size rule in the MAC
    walk; without a tail nothing changes"""
    import padpool_ref as ppr

    for size, k, s, p, ceil in ((32, 3, 2, 1, False), (17, 3, 2, 1, True), (13, 2, 2, 0, True), (8, 5, 3, 2, True), (9, 3, 2, 0, False)):
        assert wl.pool_out_size(size, k, s, p, ceil) == ppr.out_size(size, k, s, p, ceil)
    case = sf.padpool_case()
    shapes = {op: shape for op, shape, _ in sf.shapes(case["entry"]) if op[0] in ("pool", "avgpool")}
    assert shapes == {("pool", 3, 2, 1): (16, 8, 8), ("avgpool", 3, 2, 1, True, False): (20, 3, 3)}
    layers, spec, shape = case["entry"]
    assert wl._macs(layers, spec, shape[1:], {}, True) == wl._macs(*wl.network("groupnorm_tiny")[:2], shape[1:], {}, True)


def test_first_divergence_names_the_altered_top_level_op(cases):
    """first_divergence against a stand-in for net_cases.traced that replays the reference's own top-level tensors: None while
    they agree; with one byte of one op altered, that op's position and the op itself -- for every top-level op of every
    default case (a relu inside a branch is the same tuple as one at the top level: entries are picked by position)"""
    for case in cases:
        spec = case["entry"][1]
        traced = []
        _reference(case, case["per_channel"], trace=sf.collect(traced))
        top = [op for op in spec if op[0] not in ("save", "branch", "load")]
        assert [op for op, _ in sf.top_level(spec, traced)] == top
        assert len(traced) == len(sf.shapes(case["entry"])) >= len(top)
        name = "_spec_fuzz_host"
        wl.NETWORKS[name] = case["entry"]
        try:
            for alter in [None] + list(range(len(top))):
                def replay(i8ie, net, name_, x, trace):
                    for i, (op, q) in enumerate(sf.top_level(spec, traced)):
                        if i == alter:
                            q = q.copy()
                            q.flat[q.size // 2] ^= 1
                        trace(op, (q, 1.0, 0), None)

                line = sf.first_divergence(None, None, name, None, traced, traced=replay)
                if alter is None:
                    assert line is None
                else:
                    assert line.startswith("top-level op %d %r: 1 of %d bytes differ" % (alter, top[alter], traced_size(spec, traced, alter))), line
        finally:
            del wl.NETWORKS[name]


def traced_size(spec, traced, i):
    return sf.top_level(spec, traced)[i][1].size
