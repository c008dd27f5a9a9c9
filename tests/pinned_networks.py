"""The registry of int8inferenceengine_amd/workloads.py as the tests pin it: every name in registry order, and macs_per_image of
the networks whose figure is pinned as a number (the later ones are summed by hand in the host test of their family)."""
MACS = {
    "alexnet": 1131201056, "simple_conv": 25252800, "two_conv": 2293000, "mnist_fc": 7840, "alexnet_paper": 720351776,
    "resnet_tiny": 9572352, "resnet_tiny_gap": 9552192, "resnet18_cifar": 549131264, "fire_tiny": 1344128,
    "squeezenet_cifar": 5224448, "mobilenetv2_tiny": 4375168, "act_tiny": 2092192, "mobilenetv2_cifar": 87976448,
    "se_tiny": 2093608, "mobilenetv3_small_cifar": 17507328, "unet_tiny": 6913024, "unet_cifar": 574947328,
    "nonlocal_tiny": 237768, "nonlocal_resnet_cifar": 563811328, "convnext_tiny": 358920, "convnext_cifar": 76612608,
    "mha_tiny": 315712, "botnet_cifar": 58558976, "groupnorm_tiny": 650184, "groupnorm_resnet_cifar": 609948672,
}
NAMES = list(MACS)[:17] + ["upsample_tiny", "unet_bilinear_cifar", "aspp_tiny", "deeplabv3_cifar"] + list(MACS)[17:]
