"""What one INT8 forward of each small network launches, pinned as the full profile_stop() key -> launch count map.  The
binding decides these launches -- deferral, relu folding, border hand-over, pool fusion, the dequantising head -- and none of
them may change when its closures move between files.

Each network is calibrated with workloads.calibrated, runs one forward at batch 2 to warm the caches (packed weights, bordered
buffers), and a second one between profile_start() and profile_stop(); the counted region ends as in
test_gpu_operand_rules.py, by launching what is pending, with the bytes observed outside it.  Counts only, no times.

tests/golden/binding_launches.json was recorded by this file's `__main__` on the MI355X at the commit before the binding was
split into csrc/binding/.  Two processes at that commit gave the same maps, so the keys are compared whole, nothing stripped.

usage:  python tests/test_gpu_binding_launches.py OUT.json
"""
import json
import os

import pytest

import support

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "binding_launches.json")
NETS = ("two_conv", "mnist_fc", "resnet_tiny_gap", "fire_tiny", "mobilenetv2_tiny", "act_tiny", "se_tiny", "unet_tiny",
        "upsample_tiny", "aspp_tiny", "nonlocal_tiny", "convnext_tiny")
BATCH = 2


def launches(name):
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    net = wl.calibrated(name)
    x = wl.synthetic_input(name, BATCH, seed=5)
    net(i8ie.tensor(x)).numpy()
    cx.synchronize()
    cx.profile_start()
    try:
        y = net(i8ie.tensor(x))
        y.data.layout()  # launches what is pending; the bytes are observed outside the counted region
    finally:
        prof = cx.profile_stop()
    y.numpy()
    return {k: int(v[0]) for k, v in sorted(prof.items())}


golden = support.json_fixture(GOLDEN)


@pytest.mark.parametrize("name", NETS)
def test_forward_launches_what_was_recorded(name, golden):
    got = launches(name)
    print(name, got)
    assert got == golden[name]


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(HERE))
    with open(sys.argv[1], "w") as f:
        json.dump({n: launches(n) for n in NETS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1])
