"""The registry of workloads.py without a GPU: one ordered set of networks (tests/pinned_networks.py), their pinned MAC
figures, network(name), and build()'s refusal of a spec op it does not know."""
import pytest

import pinned_networks as pn


def test_registry_macs_and_unknown_ops(monkeypatch):
    from int8inferenceengine_amd import workloads as wl

    assert list(wl.NETWORKS) == pn.NAMES and len(pn.NAMES) == 29
    assert pn.NAMES[21:25] == ["nonlocal_tiny", "nonlocal_resnet_cifar", "convnext_tiny", "convnext_cifar"]
    assert pn.NAMES[25:] == ["mha_tiny", "botnet_cifar", "groupnorm_tiny", "groupnorm_resnet_cifar"]
    assert not hasattr(wl, "EXTRA_NETWORKS")
    assert {n: wl.macs_per_image(n) for n in pn.MACS} == pn.MACS
    assert wl.MAIN_PATH_MACS == set(pn.NAMES[:19])
    assert all(wl.network(n) is wl.NETWORKS[n] for n in pn.NAMES)
    with pytest.raises(KeyError, match="unknown network 'no_such_network'"):
        wl.network("no_such_network")

    layers = {"c": ("conv", 3, 4, 3, 1, 1), "fc": ("fc", 64, 10)}
    for spec in ([("layer", "c"), ("relu",), ("bogus",), ("layer", "fc")],
                 [("layer", "c"), ("save", "t"), ("branch", "t", [("relu",), ("bogus",)]), ("flatten", 64), ("layer", "fc")]):
        monkeypatch.setitem(wl.NETWORKS, "bogus_net", (layers, spec, (3, 4, 4)))
        with pytest.raises(ValueError, match="bogus"):
            wl.build("bogus_net")
    monkeypatch.setitem(wl.NETWORKS, "bogus_net", (layers, [("layer", "c"), ("relu",), ("flatten", 64), ("layer", "fc")], (3, 4, 4)))
    net = wl.build("bogus_net")
    assert wl.layer_names("bogus_net") == ["c", "fc"] and net.c.groups() == 1 and net.c.dilation() == 1
    assert wl.macs_per_image("bogus_net") == 16 * 4 * 27 + 640  # (not of the closed set: every weighted layer)
