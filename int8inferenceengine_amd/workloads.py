"""The networks the reference benchmarks (its notebooks) expressed against the
`i8ie` surface, plus seeded synthetic weights / inputs.

The reference's trained checkpoints (alex_cifar10_224.pt, conv_cifar10_32.pt,
fc_mnist28.pt, conv28.pt) and the datasets are not in its repository, so every
measurement here uses random-init weights of the same architecture and
synthetic inputs of the same shape and value range.

A network is a list of ops ("spec") so that the same definition drives the HIP
product path (SpecNet, through i8ie) and the CPU oracle in tests/bench.
"""
import numpy as np

# name -> (layers, spec, input_shape CHW)
#   layers: {attr: ("conv", in_c, out_c, k, stride, pad[, groups[, dilation]]) | ("fc", in_f, out_f)
#                  | ("deconv", in_c, out_c, k, stride, pad, output_pad)   i8ie.ConvTranspose2d, weight [in_c, out_c, k, k]
#                  | ("ln", channels)     i8ie.LayerNorm: float32 gamma / beta, no INT8 weights, no MACs
#                  | ("gn", groups, channels)   i8ie.GroupNorm: every rule of "ln"}
#   spec  : [("layer", attr) | ("relu",) | ("flatten", features)
#            | ("pool", k, s[, pad[, ceil_mode]])   i8ie.max_pool2d(x, k, s, pad, ceil_mode)
#            | ("save", tag)              remember the current tensor under `tag`
#            | ("add", attr, tag)         x = getattr(net, attr)(x, saved[tag]); attr names an i8ie.Add (not in `layers`)
#            | ("branch", tag, [ops...])  run ops on saved[tag] and store the result back under `tag` (projection shortcut)
#            | ("avgpool", k, s[, pad[, ceil_mode[, count_include_pad]]])   i8ie.avg_pool2d(x, k, s, pad, ceil_mode, count_include_pad)
#            | ("gap",)                   i8ie.global_avg_pool2d(x)
#            | ("concat", attr, [tags])   x = getattr(net, attr)([x] + [saved[t] for t in tags]); attr names an i8ie.Concat
#            | ("act", attr, kind[, param])  x = getattr(net, attr)(x); attr names an i8ie.Activation(kind, param)
#            | ("mul", attr, tag)         x = getattr(net, attr)(x, saved[tag]); attr names an i8ie.Mul; saved[tag] has x's
#                                         shape or is its gate [n, c] (the branch of a squeeze-and-excitation block)
#            | ("upsample", factor, mode) x = i8ie.upsample(x, factor, mode); factor an int or (fh, fw), mode "nearest" / "bilinear"
#            | ("matmul", attr, tag, transpose_a, transpose_b)   x = getattr(net, attr)(x, saved[tag]); attr names an
#                                         i8ie.MatMul(transpose_a, transpose_b)
#            | ("softmax",)               x = i8ie.softmax(x): scale 1/256, zero point 0, nothing to calibrate
#            | ("attention", attr, heads)                x = getattr(net, attr)(x), x packed [n, 3c, h, w]; attr names an
#                                         i8ie.Attention(heads)
#            | ("attention", attr, heads, tag_k, tag_v)  x = getattr(net, attr)(x, saved[tag_k], saved[tag_v])
#            | ("load", tag)              x = saved[tag] (what a branch computed becomes the current tensor)]
NETWORKS = {
    # sample/notebooks/AlexNet_cifar10_resize224.ipynb:47-71
    "alexnet": (
        {
            "conv1": ("conv", 3, 96, 11, 4, 2), "conv2": ("conv", 96, 256, 5, 1, 2),
            "conv3": ("conv", 256, 384, 3, 1, 1), "conv4": ("conv", 384, 384, 3, 1, 1),
            "conv5": ("conv", 384, 256, 3, 1, 1), "fc1": ("fc", 256 * 6 * 6, 4096),
            "fc2": ("fc", 4096, 4096), "fc3": ("fc", 4096, 10),
        },
        [("layer", "conv1"), ("relu",), ("pool", 3, 2), ("layer", "conv2"), ("relu",), ("pool", 3, 2),
         ("layer", "conv3"), ("relu",), ("layer", "conv4"), ("relu",), ("layer", "conv5"), ("relu",),
         ("pool", 3, 2), ("flatten", 9216), ("layer", "fc1"), ("relu",), ("layer", "fc2"), ("relu",),
         ("layer", "fc3")],
        (3, 224, 224),
    ),
    # sample/notebooks/Simple_Convolution_cifar10.ipynb:40-57 (3 convs + fc)
    "simple_conv": (
        {"conv1": ("conv", 3, 20, 5, 1, 0), "conv2": ("conv", 20, 50, 5, 1, 0),
         "conv3": ("conv", 50, 120, 5, 1, 0), "fc": ("fc", 960 * 8, 10)},
        [("layer", "conv1"), ("relu",), ("layer", "conv2"), ("relu",), ("pool", 2, 2), ("layer", "conv3"),
         ("relu",), ("flatten", 7680), ("layer", "fc")],
        (3, 32, 32),
    ),
    # unittest/test_quantized_layer.py:26-42 (2 convs, 1x28x28)
    "two_conv": (
        {"conv1": ("conv", 1, 20, 5, 1, 0), "conv2": ("conv", 20, 50, 5, 1, 0),
         "fc1": ("fc", 800, 500), "fc2": ("fc", 500, 10)},
        [("layer", "conv1"), ("pool", 2, 2), ("layer", "conv2"), ("pool", 2, 2), ("flatten", 800),
         ("layer", "fc1"), ("relu",), ("layer", "fc2")],
        (1, 28, 28),
    ),
    # sample/notebooks/Fully_Connected_mnist.ipynb:28-35
    "mnist_fc": ({"fc": ("fc", 784, 10)}, [("flatten", 784), ("layer", "fc")], (1, 28, 28)),
}

# The AlexNet of the paper (Krizhevsky et al. 2012, figure 2): conv2, conv4 and conv5 have groups = 2.  Not in the reference
# (its Conv2d has no groups); everything else is the "alexnet" entry.
NETWORKS["alexnet_paper"] = (
    dict(NETWORKS["alexnet"][0], conv2=("conv", 96, 256, 5, 1, 2, 2), conv4=("conv", 384, 384, 3, 1, 1, 2),
         conv5=("conv", 384, 256, 3, 1, 1, 2)),
    NETWORKS["alexnet"][1],
    NETWORKS["alexnet"][2],
)


# A small residual network (He et al. 2015 basic blocks, one with a projection shortcut, one with a grouped conv as in
# ResNeXt): what the Add exists for.  Not in the reference (it joins no two tensors).
NETWORKS["resnet_tiny"] = (
    {
        "stem": ("conv", 3, 16, 3, 1, 1),
        "b1c1": ("conv", 16, 16, 3, 1, 1), "b1c2": ("conv", 16, 16, 3, 1, 1),
        "b2c1": ("conv", 16, 32, 3, 2, 1), "b2c2": ("conv", 32, 32, 3, 1, 1), "b2proj": ("conv", 16, 32, 1, 2, 0),
        "b3c1": ("conv", 32, 32, 3, 1, 1, 4), "b3c2": ("conv", 32, 32, 1, 1, 0),
        "fc": ("fc", 32 * 8 * 8, 10),
    },
    [("layer", "stem"), ("relu",),
     ("save", "x1"), ("layer", "b1c1"), ("relu",), ("layer", "b1c2"), ("add", "add1", "x1"), ("relu",),
     ("save", "x2"), ("layer", "b2c1"), ("relu",), ("layer", "b2c2"), ("branch", "x2", [("layer", "b2proj")]),
     ("add", "add2", "x2"), ("relu",),
     ("save", "x3"), ("layer", "b3c1"), ("relu",), ("layer", "b3c2"), ("add", "add3", "x3"), ("relu",),
     ("pool", 2, 2), ("flatten", 2048), ("layer", "fc")],
    (3, 32, 32),
)


# resnet_tiny with the head every residual network has: average pooling down to [n, c, 1, 1] instead of a wide flatten
NETWORKS["resnet_tiny_gap"] = (
    dict({k: v for k, v in NETWORKS["resnet_tiny"][0].items() if k != "fc"}, fc=("fc", 32, 10)),
    NETWORKS["resnet_tiny"][1][:-3] + [("avgpool", 2, 2), ("gap",), ("flatten", 32), ("layer", "fc")],
    (3, 32, 32),
)


def _resnet18_cifar():
    """ResNet-18 for CIFAR-10 (He et al. 2015, section 4.2 style stem: 3x3, no stem max-pool): four stages of two basic
    blocks at 64 / 128 / 256 / 512 channels, stride 2 and a 1x1 projection shortcut at the start of stages 2-4."""
    layers = {"stem": ("conv", 3, 64, 3, 1, 1)}
    spec = [("layer", "stem"), ("relu",)]
    in_c = 64
    for stage, out_c in enumerate((64, 128, 256, 512), start=1):
        for block in (1, 2):
            p = "s%db%d" % (stage, block)
            stride = 2 if (stage > 1 and block == 1) else 1
            layers[p + "c1"] = ("conv", in_c, out_c, 3, stride, 1)
            layers[p + "c2"] = ("conv", out_c, out_c, 3, 1, 1)
            spec += [("save", p), ("layer", p + "c1"), ("relu",), ("layer", p + "c2")]
            if stride != 1 or in_c != out_c:
                layers[p + "proj"] = ("conv", in_c, out_c, 1, stride, 0)
                spec.append(("branch", p, [("layer", p + "proj")]))
            spec += [("add", p + "add", p), ("relu",)]
            in_c = out_c
    layers["fc"] = ("fc", 512, 10)
    spec += [("gap",), ("flatten", 512), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


NETWORKS["resnet18_cifar"] = _resnet18_cifar()


def _fire(layers, spec, p, in_c, squeeze, e1, e3, relu_after=False):
    """A fire module (Iandola et al. 2016): 1x1 squeeze, then a 1x1 and a 3x3 expand side by side, joined along the channels.
    relu_after: one ReLU behind the concat instead of one on each expand branch (the same function; it folds into the concat)."""
    layers[p + "s"] = ("conv", in_c, squeeze, 1, 1, 0)
    layers[p + "e1"] = ("conv", squeeze, e1, 1, 1, 0)
    layers[p + "e3"] = ("conv", squeeze, e3, 3, 1, 1)
    r = [] if relu_after else [("relu",)]
    spec += [("layer", p + "s"), ("relu",), ("save", p), ("layer", p + "e1")] + r
    spec += [("branch", p, [("layer", p + "e3")] + r), ("concat", p + "cat", [p])] + ([("relu",)] if relu_after else [])
    return e1 + e3


def _fire_tiny():
    """Two fire modules (the second with channel counts that are no multiple of 16 and its ReLU behind the concat), then an
    Inception-style reduction: a max-pool, a 4-group 3x3 conv and a 1x1 conv side by side.  What the Concat exists for."""
    layers = {"stem": ("conv", 3, 16, 3, 1, 1)}
    spec = [("layer", "stem"), ("relu",)]
    c = _fire(layers, spec, "fa", 16, 8, 16, 16)
    c = _fire(layers, spec, "fb", c, 12, 20, 12, relu_after=True)
    layers["rg"] = ("conv", c, 16, 3, 2, 1, 4)
    layers["r1"] = ("conv", c, 16, 1, 2, 0)
    spec += [("save", "rg"), ("save", "r1"), ("pool", 2, 2), ("branch", "rg", [("layer", "rg"), ("relu",)]),
             ("branch", "r1", [("layer", "r1"), ("relu",)]), ("concat", "rcat", ["rg", "r1"])]
    layers["fc"] = ("fc", c + 32, 10)
    spec += [("gap",), ("flatten", c + 32), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _squeezenet_cifar():
    """SqueezeNet 1.1 (Iandola et al. 2016; the 1.1 revision's pool placement) for CIFAR-10: a 3x3 stem at stride 1, eight fire
    modules at the original widths, 3x3 stride-2 floor-mode max-pools, a 1x1 classifier conv to 10, global average pool."""
    layers = {"stem": ("conv", 3, 64, 3, 1, 1)}
    spec = [("layer", "stem"), ("relu",), ("pool", 3, 2)]
    c = 64
    for i, (sq, ex) in enumerate(((16, 64), (16, 64), (32, 128), (32, 128), (48, 192), (48, 192), (64, 256), (64, 256)), start=2):
        c = _fire(layers, spec, "fire%d" % i, c, sq, ex, ex)
        if i in (3, 5):
            spec.append(("pool", 3, 2))
    layers["classifier"] = ("conv", c, 10, 1, 1, 0)
    spec += [("layer", "classifier"), ("relu",), ("gap",), ("flatten", 10)]
    return layers, spec, (3, 32, 32)


NETWORKS["fire_tiny"] = _fire_tiny()
NETWORKS["squeezenet_cifar"] = _squeezenet_cifar()


def _inverted_residual(layers, spec, p, in_c, out_c, t, stride):
    """An inverted residual block (Sandler et al. 2018, figure 3b): 1x1 expansion by t + relu6 (left out at t = 1), depthwise
    3x3 + relu6, linear 1x1 projection; a residual Add around it where the stride is 1 and the channel counts agree."""
    mid = in_c * t
    skip = stride == 1 and in_c == out_c
    if skip:
        spec.append(("save", p))
    if t != 1:
        layers[p + "e"] = ("conv", in_c, mid, 1, 1, 0)
        spec += [("layer", p + "e"), ("act", p + "ea", "relu6")]
    layers[p + "d"] = ("conv", mid, mid, 3, stride, 1, mid)
    layers[p + "p"] = ("conv", mid, out_c, 1, 1, 0)
    spec += [("layer", p + "d"), ("act", p + "da", "relu6"), ("layer", p + "p")]
    if skip:
        spec.append(("add", p + "add", p))
    return out_c


def _mobilenetv2_tiny():
    """A MobileNetV2 in small: a 3x3 stem, three inverted residual blocks (two with their Add, one at stride 2), a 1x1 head,
    global average pool, fc.  What the Activation exists for: every non-linearity is a relu6."""
    layers = {"stem": ("conv", 3, 16, 3, 1, 1)}
    spec = [("layer", "stem"), ("act", "stema", "relu6")]
    c = _inverted_residual(layers, spec, "b1", 16, 16, 2, 1)
    c = _inverted_residual(layers, spec, "b2", c, 24, 2, 2)
    c = _inverted_residual(layers, spec, "b3", c, 24, 4, 1)
    layers["head"] = ("conv", c, 64, 1, 1, 0)
    layers["fc"] = ("fc", 64, 10)
    spec += [("layer", "head"), ("act", "heada", "relu6"), ("gap",), ("flatten", 64), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _act_tiny():
    """Every other kind of Activation, and every lane width of its kernel (16, 20 and 35 channels), in one network."""
    layers = {"c1": ("conv", 3, 16, 3, 1, 1), "c2": ("conv", 16, 20, 3, 2, 1), "c3": ("conv", 20, 35, 1, 1, 0),
              "c4": ("conv", 35, 16, 1, 1, 0), "c5": ("conv", 16, 16, 3, 1, 1), "fc": ("fc", 16, 10)}
    spec = [("layer", "c1"), ("act", "a1", "hardswish"), ("layer", "c2"), ("act", "a2", "leaky_relu", 0.1),
            ("layer", "c3"), ("act", "a3", "hardsigmoid"), ("layer", "c4"), ("act", "a4", "sigmoid"),
            ("layer", "c5"), ("act", "a5", "tanh"), ("gap",), ("flatten", 16), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _mobilenetv2_cifar():
    """MobileNetV2 at width 1.0 (Sandler et al. 2018, table 2) for CIFAR-10: the stem and the second stage at stride 1 for
    32x32 input, head 1x1 320 -> 1280, global average pool, fc 1280 -> 10."""
    layers = {"stem": ("conv", 3, 32, 3, 1, 1)}
    spec = [("layer", "stem"), ("act", "stema", "relu6")]
    c = 32
    for stage, (t, out_c, n, s) in enumerate(((1, 16, 1, 1), (6, 24, 2, 1), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
                                              (6, 160, 3, 2), (6, 320, 1, 1)), start=1):
        for block in range(1, n + 1):
            c = _inverted_residual(layers, spec, "s%db%d" % (stage, block), c, out_c, t, s if block == 1 else 1)
    layers["head"] = ("conv", c, 1280, 1, 1, 0)
    layers["fc"] = ("fc", 1280, 10)
    spec += [("layer", "head"), ("act", "heada", "relu6"), ("gap",), ("flatten", 1280), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def make_divisible(v, divisor=8):
    """the channel rounding of the MobileNet family: to the nearest multiple of `divisor`, at least `divisor`, never more
    than 10 % below v"""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _squeeze_excite(layers, spec, p, c, squeeze):
    """A squeeze-and-excitation block (Hu et al. 2018, with MobileNetV3's hardsigmoid): the current [n, c, h, w] tensor times
    a gate of one value per image and channel, made from its global average by two Linears.  What the Mul exists for."""
    layers[p + "fc1"] = ("fc", c, squeeze)
    layers[p + "fc2"] = ("fc", squeeze, c)
    spec += [("save", p), ("branch", p, [("gap",), ("flatten", c), ("layer", p + "fc1"), ("relu",), ("layer", p + "fc2"),
                                         ("act", p + "hs", "hardsigmoid")]), ("mul", p + "mul", p)]


def _se_tiny():
    """Every form of the Mul in one network: squeeze-and-excitation at 16, 20 and 35 channels (16-, 4- and 1-byte items of
    its kernel), the first feeding a 3x3 pad-1 conv, and the product of two conv outputs of one shape, followed by a relu and
    a 3x3 pad-1 conv."""
    layers = {"c1": ("conv", 3, 16, 3, 1, 1), "c2": ("conv", 16, 20, 3, 2, 1), "c3": ("conv", 20, 35, 1, 1, 0),
              "c4a": ("conv", 35, 16, 1, 1, 0), "c4b": ("conv", 35, 16, 3, 1, 1), "c5": ("conv", 16, 16, 3, 1, 1), "fc": ("fc", 16, 10)}
    spec = [("layer", "c1"), ("act", "a1", "hardswish")]
    _squeeze_excite(layers, spec, "s1", 16, 8)
    spec += [("layer", "c2"), ("act", "a2", "hardswish")]
    _squeeze_excite(layers, spec, "s2", 20, 8)
    spec += [("layer", "c3"), ("relu",)]
    _squeeze_excite(layers, spec, "s3", 35, 12)
    spec += [("save", "m"), ("layer", "c4a"), ("branch", "m", [("layer", "c4b")]), ("mul", "mab", "m"),
             ("relu",), ("layer", "c5"), ("relu",), ("gap",), ("flatten", 16), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _mobilenetv3_small_cifar():
    """MobileNetV3-small (Howard et al. 2019, table 2) for CIFAR-10, with torchvision's squeeze-and-excitation: behind the
    depthwise activation, squeeze width make_divisible(exp / 4, 8), none on the last 1x1 conv.  The stem and the first block
    run at stride 1 for 32x32 input (the first block then has a residual Add); head 1x1 -> 576 with hardswish, global
    average pool, fc 576 -> 1024 with hardswish, fc 1024 -> 10."""
    layers = {"stem": ("conv", 3, 16, 3, 1, 1)}
    spec = [("layer", "stem"), ("act", "stema", "hardswish")]
    c = 16
    #        k  exp  out  SE     HS     stride
    table = [(3, 16, 16, True, False, 1), (3, 72, 24, False, False, 2), (3, 88, 24, False, False, 1), (5, 96, 40, True, True, 2),
             (5, 240, 40, True, True, 1), (5, 240, 40, True, True, 1), (5, 120, 48, True, True, 1), (5, 144, 48, True, True, 1),
             (5, 288, 96, True, True, 2), (5, 576, 96, True, True, 1), (5, 576, 96, True, True, 1)]
    for i, (k, exp, out_c, se, hs, stride) in enumerate(table, start=1):
        p = "b%d" % i
        act = (lambda a: ("act", a, "hardswish")) if hs else (lambda a: ("relu",))
        skip = stride == 1 and c == out_c
        if skip:
            spec.append(("save", p))
        if exp != c:
            layers[p + "e"] = ("conv", c, exp, 1, 1, 0)
            spec += [("layer", p + "e"), act(p + "ea")]
        layers[p + "d"] = ("conv", exp, exp, k, stride, k // 2, exp)
        spec += [("layer", p + "d"), act(p + "da")]
        if se:
            _squeeze_excite(layers, spec, p + "se", exp, make_divisible(exp / 4, 8))
        layers[p + "p"] = ("conv", exp, out_c, 1, 1, 0)
        spec.append(("layer", p + "p"))
        if skip:
            spec.append(("add", p + "add", p))
        c = out_c
    layers["head"] = ("conv", c, 576, 1, 1, 0)
    layers["fc1"] = ("fc", 576, 1024)
    layers["fc2"] = ("fc", 1024, 10)
    spec += [("layer", "head"), ("act", "heada", "hardswish"), ("gap",), ("flatten", 576), ("layer", "fc1"),
             ("act", "fc1a", "hardswish"), ("layer", "fc2")]
    return layers, spec, (3, 32, 32)


NETWORKS["mobilenetv2_tiny"] = _mobilenetv2_tiny()
NETWORKS["act_tiny"] = _act_tiny()
NETWORKS["mobilenetv2_cifar"] = _mobilenetv2_cifar()
NETWORKS["se_tiny"] = _se_tiny()
NETWORKS["mobilenetv3_small_cifar"] = _mobilenetv3_small_cifar()


def _unet_tiny():
    """A U-Net in small (two levels down by max-pool): what the ConvTranspose2d exists for.  Three up-convs, 2x2 stride 2 and
    4x4 stride 2 pad 1 side by side out of the bottleneck and 3x3 stride 2 pad 1 output_pad 1 above them; the skips joined by
    Concat at 47 (= 20 + 7 + 20) and 24 channels; a 3x3 pad-1 conv behind each join; a 1x1 head to 10 maps of 32 x 32."""
    layers = {"enc1": ("conv", 3, 12, 3, 1, 1), "enc2": ("conv", 12, 20, 3, 1, 1), "bott": ("conv", 20, 32, 3, 1, 1),
              "up2a": ("deconv", 32, 20, 2, 2, 0, 0), "up2b": ("deconv", 32, 7, 4, 2, 1, 0), "dec2": ("conv", 47, 20, 3, 1, 1),
              "up1": ("deconv", 20, 12, 3, 2, 1, 1), "dec1": ("conv", 24, 12, 3, 1, 1), "head": ("conv", 12, 10, 1, 1, 0)}
    spec = [("layer", "enc1"), ("relu",), ("save", "e1"), ("pool", 2, 2),
            ("layer", "enc2"), ("relu",), ("save", "e2"), ("pool", 2, 2),
            ("layer", "bott"), ("relu",), ("save", "b"),
            ("layer", "up2a"), ("branch", "b", [("layer", "up2b")]), ("concat", "cat2", ["b", "e2"]), ("layer", "dec2"), ("relu",),
            ("layer", "up1"), ("relu",), ("concat", "cat1", ["e1"]), ("layer", "dec1"), ("relu",), ("layer", "head")]
    return layers, spec, (3, 32, 32)


def _unet_cifar(bilinear=False):
    """U-Net (Ronneberger et al. 2015) at widths 64 / 128 / 256 / 512 for 32 x 32 input: two padded 3x3 convs per level, 2x2
    max-pools down, 2x2 stride-2 up-convs, the skips joined by Concat, a 1x1 head to 10 maps.  bilinear: the usual replacement
    for the up-convs, a bilinear x2 upsample and a 1x1 conv to the skip's width."""
    layers, spec = {}, []

    def double(p, in_c, out_c):
        layers[p + "a"] = ("conv", in_c, out_c, 3, 1, 1)
        layers[p + "b"] = ("conv", out_c, out_c, 3, 1, 1)
        spec.extend([("layer", p + "a"), ("relu",), ("layer", p + "b"), ("relu",)])

    widths = (64, 128, 256, 512)
    c = 3
    for i, wd in enumerate(widths[:-1], start=1):
        double("d%d" % i, c, wd)
        spec.extend([("save", "s%d" % i), ("pool", 2, 2)])
        c = wd
    double("mid", c, widths[-1])
    c = widths[-1]
    for i in (3, 2, 1):
        wd = widths[i - 1]
        if bilinear:
            layers["up%d" % i] = ("conv", c, wd, 1, 1, 0)
            spec.append(("upsample", 2, "bilinear"))
        else:
            layers["up%d" % i] = ("deconv", c, wd, 2, 2, 0, 0)
        spec.extend([("layer", "up%d" % i), ("concat", "cat%d" % i, ["s%d" % i])])
        double("u%d" % i, 2 * wd, wd)
        c = wd
    layers["head"] = ("conv", c, 10, 1, 1, 0)
    spec.append(("layer", "head"))
    return layers, spec, (3, 32, 32)


NETWORKS["unet_tiny"] = _unet_tiny()
NETWORKS["unet_cifar"] = _unet_cifar()


def _upsample_tiny():
    """Every form of the upsample in one network.  A feature pyramid (Lin et al. 2017): a bottom-up path to 35 channels of
    4 x 4, then three top-down steps at 35, 20 and 16 channels (1-, 4- and 16-byte items of the kernel), each a nearest x2
    upsample, a lateral 1x1 conv of the bottom-up map, their Add and a 3x3 pad-1 conv.  Behind it a bilinear x2 of a conv
    output with its relu directly behind, joined by Concat with a skip; a bilinear (2, 3) upsample in front of a 3x3 pad-1
    conv; a 1x1 head to 10 maps of 32 x 48."""
    layers = {"c1": ("conv", 3, 16, 3, 1, 1), "c2": ("conv", 16, 20, 3, 2, 1), "c3": ("conv", 20, 35, 3, 2, 1),
              "c4": ("conv", 35, 35, 3, 2, 1)}
    spec = [("layer", "c1"), ("relu",), ("save", "f1"), ("layer", "c2"), ("relu",), ("save", "f2"),
            ("layer", "c3"), ("relu",), ("save", "f3"), ("layer", "c4"), ("relu",)]
    for i, c, out_c in ((3, 35, 20), (2, 20, 16), (1, 16, 16)):
        layers["l%d" % i] = ("conv", c, c, 1, 1, 0)
        layers["p%d" % i] = ("conv", c, out_c, 3, 1, 1)
        spec += [("upsample", 2, "nearest"), ("branch", "f%d" % i, [("layer", "l%d" % i)]), ("add", "a%d" % i, "f%d" % i),
                 ("layer", "p%d" % i), ("relu",)]
    layers.update({"d1": ("conv", 16, 20, 3, 1, 1), "dec": ("conv", 36, 16, 3, 1, 1), "e1": ("conv", 16, 16, 3, 1, 1),
                   "head": ("conv", 16, 10, 1, 1, 0)})
    spec += [("save", "t"), ("pool", 2, 2), ("layer", "d1"), ("upsample", 2, "bilinear"), ("relu",), ("concat", "cat1", ["t"]),
             ("layer", "dec"), ("relu",), ("pool", 2, 2), ("upsample", (2, 3), "bilinear"), ("layer", "e1"), ("relu",),
             ("layer", "head")]
    return layers, spec, (3, 32, 32)


NETWORKS["upsample_tiny"] = _upsample_tiny()
NETWORKS["unet_bilinear_cifar"] = _unet_cifar(bilinear=True)


def _aspp_tiny():
    """An atrous spatial pyramid (Chen et al. 2017) in small: what Conv2d's dilation exists for.  Two stride-2 3x3 convs down
    to 32 channels of 8 x 8, a dilated 3x3 conv (rate 2), then five branches over that map -- 1x1; 3x3 at rate 2; 3x3 at rate
    3 to 20 channels; a depthwise 3x3 at rate 2 with its 1x1; the image pool (gap, 1x1, relu, nearest x8) -- joined by Concat
    at 84 channels, a 1x1 projection, the residual Add with the pyramid's input, a 1x1 head to 10 and a bilinear x4 to 32 x 32."""
    layers = {"stem": ("conv", 3, 16, 3, 2, 1), "down": ("conv", 16, 32, 3, 2, 1), "atr": ("conv", 32, 32, 3, 1, 2, 1, 2),
              "a1": ("conv", 32, 16, 1, 1, 0), "a2": ("conv", 32, 16, 3, 1, 2, 1, 2), "a3": ("conv", 32, 20, 3, 1, 3, 1, 3),
              "a4d": ("conv", 32, 32, 3, 1, 2, 32, 2), "a4p": ("conv", 32, 16, 1, 1, 0), "a5": ("conv", 32, 16, 1, 1, 0),
              "proj": ("conv", 84, 32, 1, 1, 0), "head": ("conv", 32, 10, 1, 1, 0)}
    spec = [("layer", "stem"), ("relu",), ("layer", "down"), ("relu",), ("layer", "atr"), ("relu",),
            ("save", "x"), ("save", "b2"), ("save", "b3"), ("save", "b4"), ("save", "b5"), ("layer", "a1"),
            ("branch", "b2", [("layer", "a2")]), ("branch", "b3", [("layer", "a3")]),
            ("branch", "b4", [("layer", "a4d"), ("layer", "a4p")]),
            ("branch", "b5", [("gap",), ("layer", "a5"), ("relu",), ("upsample", 8, "nearest")]),
            ("concat", "cat", ["b2", "b3", "b4", "b5"]), ("layer", "proj"), ("add", "res", "x"), ("layer", "head"),
            ("upsample", 4, "bilinear")]
    return layers, spec, (3, 32, 32)


def _deeplabv3_cifar():
    """DeepLabV3 (Chen et al. 2017) for 32 x 32 input: resnet18_cifar's stem and stages 1-3 (256 channels of 8 x 8), stage 4
    kept at stride 1 with its 3x3 convs at rate 2 (512 channels, output stride 4), the pyramid -- a 1x1 branch, three 3x3
    branches at rates 2 / 4 / 6 (padding = rate) and the image-pool branch, 128 channels each -- joined by Concat at 640, a 1x1
    to 128, a 1x1 head to 10 and a bilinear x4."""
    rl, rs, shape = _resnet18_cifar()
    layers = {a: L for a, L in rl.items() if not a.startswith("s4") and a != "fc"}
    cut = rs.index(("save", "s4b1"))
    spec = list(rs[:cut])
    in_c = 256
    for block in (1, 2):
        p = "s4b%d" % block
        layers[p + "c1"] = ("conv", in_c, 512, 3, 1, 2, 1, 2)
        layers[p + "c2"] = ("conv", 512, 512, 3, 1, 2, 1, 2)
        spec += [("save", p), ("layer", p + "c1"), ("relu",), ("layer", p + "c2")]
        if in_c != 512:
            layers[p + "proj"] = ("conv", in_c, 512, 1, 1, 0)
            spec.append(("branch", p, [("layer", p + "proj")]))
        spec += [("add", p + "add", p), ("relu",)]
        in_c = 512
    layers["aspp1"] = ("conv", 512, 128, 1, 1, 0)
    tags = []
    for rate in (2, 4, 6):
        layers["aspp_r%d" % rate] = ("conv", 512, 128, 3, 1, rate, 1, rate)
        tags.append("r%d" % rate)
        spec.append(("save", tags[-1]))
    layers["aspp_pool"] = ("conv", 512, 128, 1, 1, 0)
    spec += [("save", "ip"), ("layer", "aspp1"), ("relu",)]
    spec += [("branch", "r%d" % rate, [("layer", "aspp_r%d" % rate), ("relu",)]) for rate in (2, 4, 6)]
    spec += [("branch", "ip", [("gap",), ("layer", "aspp_pool"), ("relu",), ("upsample", 8, "nearest")]),
             ("concat", "aspp_cat", tags + ["ip"])]
    layers["aspp_proj"] = ("conv", 640, 128, 1, 1, 0)
    layers["head"] = ("conv", 128, 10, 1, 1, 0)
    spec += [("layer", "aspp_proj"), ("relu",), ("layer", "head"), ("upsample", 4, "bilinear")]
    return layers, spec, shape


NETWORKS["aspp_tiny"] = _aspp_tiny()
NETWORKS["deeplabv3_cifar"] = _deeplabv3_cifar()


# {network: {attr: factor}}: what synthetic_state_dict folds into a layer's weight and bias (1.0 where nothing is named); one
# factor for the layer, or a float64 vector [out] of one per filter
FOLDS = {}
LAYER_SCALE = 0.5  # the layer-scale factor of a ConvNeXt block, folded into its second 1x1 conv


def _attention(layers, spec, folds, p, c, d):
    """Single-head self-attention over the t = h * w pixels of the current [n, c, h, w] tensor y, into saved[p + "g"]:
    theta, phi, g = 1x1 convs c -> d of y; s = mm1(theta, phi), transpose_a: [n, t, t], s[i, j] = sum_c theta[c, i] phi[c, j];
    pr = softmax(s) over j; z = mm2(g, pr), transpose_b: [n, d, h, w], z[c, i] = sum_j g[c, j] pr[i, j]; out(z), a 1x1 conv
    d -> c.  The 1/sqrt(d) of the scores is folded into theta.  What the MatMul and the softmax exist for."""
    for r in ("theta", "phi", "g"):
        layers[p + r] = ("conv", c, d, 1, 1, 0)
    layers[p + "out"] = ("conv", d, c, 1, 1, 0)
    folds[p + "theta"] = 1.0 / np.sqrt(d)
    spec += [("save", p + "phi"), ("save", p + "g"), ("layer", p + "theta"), ("branch", p + "phi", [("layer", p + "phi")]),
             ("matmul", p + "mm1", p + "phi", True, False), ("softmax",), ("save", p + "pr"),
             ("branch", p + "g", [("layer", p + "g"), ("matmul", p + "mm2", p + "pr", False, True), ("layer", p + "out")])]


def _nonlocal(layers, spec, folds, p, c, d):
    """A non-local block (Wang et al. 2018): x = add(attention(x), x)"""
    spec.append(("save", p + "x"))
    _attention(layers, spec, folds, p, c, d)
    spec += [("load", p + "g"), ("add", p + "add", p + "x")]


def _attn(layers, spec, folds, p, c, d):
    """A pre-LN attention block: x = add(attention(ln(x)), x); one LayerNorm feeds the three projections"""
    layers[p + "ln"] = ("ln", c)
    spec += [("save", p + "x"), ("layer", p + "ln")]
    _attention(layers, spec, folds, p, c, d)
    spec += [("load", p + "g"), ("add", p + "add", p + "x")]


def _cnblock(layers, spec, folds, p, c):
    """A ConvNeXt block (Liu et al. 2022): depthwise 7x7, LayerNorm(c), 1x1 c -> 4c, hardswish, 1x1 4c -> c (LAYER_SCALE
    folded in), the residual Add.  What the LayerNorm exists for."""
    layers[p + "dw"] = ("conv", c, c, 7, 1, 3, c)
    layers[p + "ln"] = ("ln", c)
    layers[p + "pw1"] = ("conv", c, 4 * c, 1, 1, 0)
    layers[p + "pw2"] = ("conv", 4 * c, c, 1, 1, 0)
    folds[p + "pw2"] = LAYER_SCALE
    spec += [("save", p + "x"), ("layer", p + "dw"), ("layer", p + "ln"), ("layer", p + "pw1"), ("act", p + "act", "hardswish"),
             ("layer", p + "pw2"), ("add", p + "add", p + "x")]


def _nonlocal_tiny(folds):
    """3x32x32: conv 3->16 3x3 s2 p1, relu, max-pool 2/2 (8x8, t = 64), block A (c = 16, d = 16), relu, conv 16->20 3x3 s2 p1
    (a bordered consumer), relu (4x4, t = 16), block B (c = 20, d = 12: k = 12 takes bmm_direct), relu, global average
    pool, fc 20->10"""
    layers = {"stem": ("conv", 3, 16, 3, 2, 1)}
    spec = [("layer", "stem"), ("relu",), ("pool", 2, 2)]
    _nonlocal(layers, spec, folds, "a_", 16, 16)
    layers["down"] = ("conv", 16, 20, 3, 2, 1)
    spec += [("relu",), ("layer", "down"), ("relu",)]
    _nonlocal(layers, spec, folds, "b_", 20, 12)
    layers["fc"] = ("fc", 20, 10)
    spec += [("relu",), ("gap",), ("flatten", 20), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _nonlocal_resnet_cifar(folds):
    """resnet18_cifar with one non-local block (c = 256, d = 128) and a relu after stage 3 (8x8)"""
    base_layers, base_spec, shape = _resnet18_cifar()
    block_layers, block = {}, []
    _nonlocal(block_layers, block, folds, "nl_", 256, 128)
    cut = base_spec.index(("save", "s4b1"))
    layers = {}
    for attr, L in base_layers.items():  # (the block's layers where stage 4 begins)
        if attr == "s4b1c1":
            layers.update(block_layers)
        layers[attr] = L
    return layers, base_spec[:cut] + block + [("relu",)] + base_spec[cut:], shape


def _convnext_tiny(folds):
    """3x32x32: stem conv 3->16 4x4 s4 (8x8), LayerNorm(16), a block at c = 16, a downsample LayerNorm(16) -> conv 16->20 3x3
    s2 p1 (an LN result that carries a border; 4x4), a block at c = 20 (rows that are no multiple of 16), an attention block
    at c = 20, d = 12, global average pool, LayerNorm(20) on [n, 20], fc 20->10"""
    layers = {"stem": ("conv", 3, 16, 4, 4, 0), "stem_ln": ("ln", 16)}
    spec = [("layer", "stem"), ("layer", "stem_ln")]
    _cnblock(layers, spec, folds, "a_", 16)
    layers["down_ln"] = ("ln", 16)
    layers["down"] = ("conv", 16, 20, 3, 2, 1)
    spec += [("layer", "down_ln"), ("layer", "down")]
    _cnblock(layers, spec, folds, "b_", 20)
    _attn(layers, spec, folds, "t_", 20, 12)
    layers["head_ln"] = ("ln", 20)
    layers["fc"] = ("fc", 20, 10)
    spec += [("gap",), ("flatten", 20), ("layer", "head_ln"), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _convnext_cifar(folds):
    """ConvNeXt (Liu et al. 2022) for 32x32 input: patchify stem 3->64 2x2 s2 + LN (16x16), stages of (2, 2, 2, 2) blocks at
    64 / 128 / 256 / 512 with LN + 2x2 s2 conv between them, global average pool, LN, fc 512->10"""
    layers = {"stem": ("conv", 3, 64, 2, 2, 0), "stem_ln": ("ln", 64)}
    spec = [("layer", "stem"), ("layer", "stem_ln")]
    c = 64
    for s in range(4):
        if s:
            layers["d%d_ln" % s] = ("ln", c)
            layers["d%d" % s] = ("conv", c, 2 * c, 2, 2, 0)
            spec += [("layer", "d%d_ln" % s), ("layer", "d%d" % s)]
            c *= 2
        for b in range(2):
            _cnblock(layers, spec, folds, "s%db%d_" % (s, b), c)
    layers["head_ln"] = ("ln", c)
    layers["fc"] = ("fc", c, 10)
    spec += [("gap",), ("flatten", c), ("layer", "head_ln"), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _mha(layers, spec, folds, qkv, attn, c, heads):
    """Fused multi-head self-attention of the current [n, c, h, w] tensor: one packed 1x1 conv c -> 3c (query, key and value
    filters in that order, the 1/sqrt(d) of the scores folded into the query filters) and one i8ie.Attention(heads)."""
    layers[qkv] = ("conv", c, 3 * c, 1, 1, 0)
    folds[qkv] = np.where(np.arange(3 * c) < c, 1.0 / np.sqrt(c // heads), 1.0)
    spec += [("layer", qkv), ("attention", attn, heads)]


def _silu(spec, p):
    """x * sigmoid(x) of the current tensor x, with x the first operand of the Mul"""
    spec += [("save", p + "g"), ("act", p + "sig", "sigmoid"), ("save", p + "sig"), ("load", p + "g"), ("mul", p + "mul", p + "sig")]


def _mha_tiny(folds):
    """3x32x32: conv 3->16 3x3 s2 p1, relu, max-pool 2/2 (8x8, t = 64), [LayerNorm, packed 1x1 conv 16 -> 48, Attention(2) at
    d = 8 (attn_direct), 1x1 conv] + skip, relu, conv 16->32 3x3 s2 p1 (a bordered consumer; 4x4, t = 16), [three 1x1 convs,
    Attention(2) of three tensors at d = 16 (attn_mfma), 1x1 conv] + skip, relu, global average pool, fc 32->10.  What the
    Attention exists for."""
    layers = {"c1": ("conv", 3, 16, 3, 2, 1), "ln1": ("ln", 16)}
    spec = [("layer", "c1"), ("relu",), ("pool", 2, 2), ("save", "x1"), ("layer", "ln1")]
    _mha(layers, spec, folds, "qkv1", "attn1", 16, 2)
    layers.update({"proj1": ("conv", 16, 16, 1, 1, 0), "c2": ("conv", 16, 32, 3, 2, 1)})
    for r in ("q2", "k2", "v2", "proj2"):
        layers[r] = ("conv", 32, 32, 1, 1, 0)
    layers["fc"] = ("fc", 32, 10)
    folds["q2"] = 1.0 / np.sqrt(32 // 2)
    spec += [("layer", "proj1"), ("add", "add1", "x1"), ("relu",), ("layer", "c2"),
             ("save", "x2"), ("save", "k2"), ("save", "v2"), ("layer", "q2"), ("branch", "k2", [("layer", "k2")]),
             ("branch", "v2", [("layer", "v2")]), ("attention", "attn2", 2, "k2", "v2"), ("layer", "proj2"), ("add", "add2", "x2"),
             ("relu",), ("gap",), ("flatten", 32), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _botnet_cifar(folds):
    """A ResNet-style network for 32x32 input whose last stage replaces the 3x3 convs of its bottleneck blocks with 4-head
    self-attention (BoTNet, Srinivas et al. 2021, without the relative-position term): stem 3->32, a basic block at 32 (32x32),
    one at 64 with a projection shortcut (16x16), conv 64->256 3x3 s2 (8x8, t = 64), two bottleneck blocks 256 -> 128 ->
    attention at d = 32 -> 256, global average pool, fc 256->10"""
    layers = {"stem": ("conv", 3, 32, 3, 1, 1), "s1a": ("conv", 32, 32, 3, 1, 1), "s1b": ("conv", 32, 32, 3, 1, 1),
              "s2a": ("conv", 32, 64, 3, 2, 1), "s2b": ("conv", 64, 64, 3, 1, 1), "s2s": ("conv", 32, 64, 1, 2, 0),
              "s3in": ("conv", 64, 256, 3, 2, 1)}
    spec = [("layer", "stem"), ("relu",),
            ("save", "x1"), ("layer", "s1a"), ("relu",), ("layer", "s1b"), ("add", "add1", "x1"), ("relu",),
            ("save", "x2"), ("layer", "s2a"), ("relu",), ("layer", "s2b"), ("branch", "x2", [("layer", "s2s")]),
            ("add", "add2", "x2"), ("relu",), ("layer", "s3in"), ("relu",)]
    for p in ("b1", "b2"):
        layers[p + "r"] = ("conv", 256, 128, 1, 1, 0)
        spec += [("save", p), ("layer", p + "r"), ("relu",)]
        _mha(layers, spec, folds, p + "qkv", p + "attn", 128, 4)
        layers[p + "e"] = ("conv", 128, 256, 1, 1, 0)
        spec += [("relu",), ("layer", p + "e"), ("add", "add_" + p, p), ("relu",)]
    layers["fc"] = ("fc", 256, 10)
    spec += [("gap",), ("flatten", 256), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _gn_block(layers, spec, p, in_c, c, groups, stride=1, shortcut="", relu=True):
    """A basic residual block with a GroupNorm behind each conv: x = [relu](add(gn2(c2(relu(gn1(c1(x))))), skip)), skip = x or,
    where `shortcut` names one, its 1x1 conv at the block's stride with `shortcut` + "gn" behind it.  groups: of gn1 and gn2"""
    layers[p + "c1"], layers[p + "gn1"] = ("conv", in_c, c, 3, stride, 1), ("gn", groups[0], c)
    layers[p + "c2"], layers[p + "gn2"] = ("conv", c, c, 3, 1, 1), ("gn", groups[1], c)
    spec += [("save", p + "x"), ("layer", p + "c1"), ("layer", p + "gn1"), ("relu",), ("layer", p + "c2"), ("layer", p + "gn2")]
    if shortcut:
        layers[p + shortcut], layers[p + shortcut + "gn"] = ("conv", in_c, c, 1, stride, 0), ("gn", groups[1], c)
        spec.append(("branch", p + "x", [("layer", p + shortcut), ("layer", p + shortcut + "gn")]))
    spec += [("add", p + "add", p + "x")] + ([("relu",)] if relu else [])


def _groupnorm_tiny(folds):
    """3x32x32: conv 3->16 3x3 s2 p1, relu, max-pool 2/2 (8x8), a residual block at 16 channels with GN(4) and GN(16) (an
    InstanceNorm; its first GN feeds a bordered consumer), conv 16->20 3x3 s2 p1 (4x4), GN(5), relu, a residual block at 20
    channels with GN(1) and GN(10) and no relu behind its Add, the SiLU block [GN(4), x * sigmoid(x) (two consumers of one
    pending GN), conv 3x3 p1, packed 1x1 conv 20 -> 60, Attention(2) at d = 10, 1x1 conv] + skip, relu, global average pool,
    fc 20->10.  20 channels are no multiple of 16: those GroupNorms take the direct form, the 16-channel ones the image form.
    What the GroupNorm exists for."""
    layers = {"c1": ("conv", 3, 16, 3, 2, 1)}
    spec = [("layer", "c1"), ("relu",), ("pool", 2, 2)]
    _gn_block(layers, spec, "a_", 16, 16, (4, 16))
    layers["down"], layers["d_gn"] = ("conv", 16, 20, 3, 2, 1), ("gn", 5, 20)
    spec += [("layer", "down"), ("layer", "d_gn"), ("relu",)]
    _gn_block(layers, spec, "b_", 20, 20, (1, 10), relu=False)
    layers["s_gn"], layers["s_c"] = ("gn", 4, 20), ("conv", 20, 20, 3, 1, 1)
    spec += [("save", "s_x"), ("layer", "s_gn")]
    _silu(spec, "s_")
    spec.append(("layer", "s_c"))
    _mha(layers, spec, folds, "s_qkv", "s_attn", 20, 2)
    layers["s_proj"], layers["fc"] = ("conv", 20, 20, 1, 1, 0), ("fc", 20, 10)
    spec += [("layer", "s_proj"), ("add", "s_add", "s_x"), ("relu",), ("gap",), ("flatten", 20), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _groupnorm_resnet_cifar(folds):
    """A GroupNorm ResNet-18 for 32x32 input (Wu & He 2018: resnet18_cifar's topology with GroupNorm(32, c) behind every conv,
    the shortcuts' included) with one diffusion-style block behind the 8x8 stage: GroupNorm, SiLU written as x * sigmoid(x),
    3x3 conv, skip; then GroupNorm, 4-head self-attention at d = 64, 1x1 conv, skip, relu"""
    layers = {"stem": ("conv", 3, 64, 3, 1, 1), "stem_gn": ("gn", 32, 64)}
    spec = [("layer", "stem"), ("layer", "stem_gn"), ("relu",)]
    in_c = 64
    for s, (c, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2))):
        for b in range(2):
            st = stride if b == 0 else 1
            _gn_block(layers, spec, "s%db%d_" % (s, b), in_c, c, (32, 32), st, "sc" if st != 1 or in_c != c else "")
            in_c = c
        if c == 256:
            layers["m_gn"], layers["m_c"], layers["m_gn2"] = ("gn", 32, c), ("conv", c, c, 3, 1, 1), ("gn", 32, c)
            spec += [("save", "m_x"), ("layer", "m_gn")]
            _silu(spec, "m_")
            spec += [("layer", "m_c"), ("add", "m_add1", "m_x"), ("save", "m_x2"), ("layer", "m_gn2")]
            _mha(layers, spec, folds, "m_qkv", "m_attn", c, 4)
            layers["m_proj"] = ("conv", c, c, 1, 1, 0)
            spec += [("layer", "m_proj"), ("add", "m_add2", "m_x2"), ("relu",)]
    layers["fc"] = ("fc", 512, 10)
    spec += [("gap",), ("flatten", 512), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


for _name, _make in (("nonlocal_tiny", _nonlocal_tiny), ("nonlocal_resnet_cifar", _nonlocal_resnet_cifar),
                     ("convnext_tiny", _convnext_tiny), ("convnext_cifar", _convnext_cifar), ("mha_tiny", _mha_tiny),
                     ("botnet_cifar", _botnet_cifar), ("groupnorm_tiny", _groupnorm_tiny),
                     ("groupnorm_resnet_cifar", _groupnorm_resnet_cifar)):
    NETWORKS[_name] = _make(FOLDS.setdefault(_name, {}))


def network(name):
    """the (layers, spec, input shape) entry of a network"""
    if name not in NETWORKS:
        raise KeyError("unknown network %r" % (name,))
    return NETWORKS[name]


def _walk(spec):
    """every op of a spec in order, the ops inside ("branch", tag, [ops]) included"""
    for op in spec:
        if op[0] == "branch":
            yield from _walk(op[2])
        else:
            yield op


# the op names a spec may hold: build() refuses any other
OPS = frozenset(("layer", "relu", "pool", "avgpool", "gap", "save", "branch", "add", "mul", "concat", "act", "upsample", "flatten",
                 "matmul", "softmax", "load", "attention"))


def conv_groups(L):
    """groups of a ("conv", ...) layer tuple: its optional 7th element"""
    return L[6] if len(L) > 6 else 1


def conv_dilation(L):
    """dilation of a ("conv", ...) layer tuple: its optional 8th element"""
    return L[7] if len(L) > 7 else 1


def pool_out_size(size, k, s, pad=0, ceil_mode=False):
    """output size of one axis of a ("pool", ...) / ("avgpool", ...) op: the rule of i8ie_pool_output_size (a ceil-mode window
    that would start beyond the input and its padding is dropped)"""
    o = (size + 2 * pad - k + (s - 1 if ceil_mode else 0)) // s + 1
    return o - 1 if ceil_mode and (o - 1) * s >= size + pad else o


def upsample_factors(factor):
    """(fh, fw) of an ("upsample", factor, mode) op: factor is an int or a pair"""
    return tuple(factor) if isinstance(factor, (tuple, list)) else (factor, factor)


# MACs per image: the algorithmic work of the INT8 contractions
ALEXNET_MACS_PER_IMAGE = 1131201056


# The networks whose figures were pinned while macs_per_image skipped the convs of a branch (projection shortcuts, fire
# expands, the second up-conv of unet_tiny) and counted only the Linears found inside one.  Their figures are quoted in the
# documents and pinned by tests, so they keep that counting.  This set is closed: a new network counts every weighted layer.
MAIN_PATH_MACS = frozenset((
    "alexnet", "simple_conv", "two_conv", "mnist_fc", "alexnet_paper", "resnet_tiny", "resnet_tiny_gap", "resnet18_cifar",
    "fire_tiny", "squeezenet_cifar", "mobilenetv2_tiny", "act_tiny", "mobilenetv2_cifar", "se_tiny", "mobilenetv3_small_cifar",
    "unet_tiny", "unet_cifar", "upsample_tiny", "unet_bilinear_cifar"))


def _macs(layers, ops, hw, saved, branch_convs, in_branch=False):
    """MACs of the weighted layers of `ops` from an (h, w) map on, those of its branches included, with true taps (a dilated
    kernel's zeros are no work); without branch_convs a branch counts its Linears only.  Weighted layers only: a LayerNorm
    has none, and the products of a ("matmul", ...) or an ("attention", ...) of activations are not counted (no channel count is
    tracked here).
    Returns (macs, (h, w) behind the ops)."""
    total = 0
    convs = branch_convs or not in_branch
    h, w = hw
    for op in ops:
        if op[0] == "layer":
            L = layers[op[1]]
            if L[0] == "conv":
                _, ic, oc, k, s, p = L[:6]
                e = conv_dilation(L) * (k - 1) + 1
                h, w = (h - e + 2 * p) // s + 1, (w - e + 2 * p) // s + 1
                total += convs * h * w * oc * (ic // conv_groups(L)) * k * k
            elif L[0] == "deconv":  # the real MACs: every input pixel meets every tap once
                _, ic, oc, k, s, p, op_ = L
                total += convs * h * w * ic * oc * k * k
                h, w = (h - 1) * s - 2 * p + k + op_, (w - 1) * s - 2 * p + k + op_
            elif L[0] == "fc":
                total += L[1] * L[2]
            # ("ln", c), ("gn", groups, c): no MACs, the same map
        elif op[0] in ("pool", "avgpool"):
            h, w = pool_out_size(h, *op[1:5]), pool_out_size(w, *op[1:5])
        elif op[0] == "gap":
            h, w = 1, 1
        elif op[0] == "upsample":
            fh, fw = upsample_factors(op[1])
            h, w = h * fh, w * fw
        elif op[0] == "save":
            saved[op[1]] = (h, w)
        elif op[0] == "load":
            h, w = saved[op[1]]
        elif op[0] == "branch":
            t, saved[op[1]] = _macs(layers, op[2], saved[op[1]], saved, branch_convs, True)
            total += t
        # ("act", ...), like relu, flatten, add, mul and concat, has no MACs and keeps the shape; matmul and softmax leave
        # (h, w) alone too: the map behind them is read only by 1x1 convs or replaced by a load.  So does attention, whose
        # result has its query's map
    return total, (h, w)


def macs_per_image(name):
    """MACs of one image through network(name): every weighted layer, true taps.  The networks of MAIN_PATH_MACS leave out
    the convs of their branches."""
    layers, spec, (c, h, w) = network(name)
    return _macs(layers, spec, (h, w), {}, name not in MAIN_PATH_MACS)[0]


def synthetic_state_dict(name, seed=42):
    """He-uniform weights, U(-1/sqrt(fan_in), 1/sqrt(fan_in)) biases, both times the layer's factor (or each filter's) in FOLDS;
    a LayerNorm or GroupNorm gets gamma from U(0.5, 1.5) and beta from U(-0.3, 0.3); keys '<attr>.weight'/'<attr>.bias'."""
    rng = np.random.default_rng(seed)
    layers = network(name)[0]
    folds = FOLDS.get(name, {})
    sd = {}
    for attr, L in layers.items():
        if L[0] in ("ln", "gn"):
            sd[attr + ".weight"] = rng.uniform(0.5, 1.5, L[-1]).astype(np.float32)
            sd[attr + ".bias"] = rng.uniform(-0.3, 0.3, L[-1]).astype(np.float32)
            continue
        fold = np.asarray(folds.get(attr, 1.0), np.float64)
        if L[0] == "deconv":  # [in, out, k, k]; an output pixel sums in * ceil(k / stride)^2 products
            shape, n_out = (L[1], L[2], L[3], L[3]), L[2]
            fan_in = L[1] * (-(-L[3] // L[4])) ** 2
        else:
            shape = (L[2], L[1] // conv_groups(L), L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
            fan_in, n_out = int(np.prod(shape[1:])), shape[0]
        filter_axis = 1 if L[0] == "deconv" else 0
        per_filter = fold.reshape([-1 if axis == filter_axis else 1 for axis in range(len(shape))])
        sd[attr + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in) * per_filter).astype(np.float32)
        sd[attr + ".bias"] = (rng.uniform(-1, 1, n_out) / np.sqrt(fan_in) * fold).astype(np.float32)
    return sd


def synthetic_input(name, batch, seed=1234):
    """Normalised-image-like input, inside quantize()'s no-wrap window for scale 0.025 / zp 127."""
    c, h, w = network(name)[2]
    rng = np.random.default_rng(seed)
    if name in ("mnist_fc", "two_conv"):
        return rng.uniform(0, 1, (batch, c, h, w)).astype(np.float32)  # ToTensor() only
    u = rng.uniform(0, 1, (batch, c, h, w)).astype(np.float32)
    a = rng.uniform(0.2, 1.0, (batch, c, 1, 1)).astype(np.float32)
    return ((u * a - np.float32(0.45)) / np.float32(0.226)).astype(np.float32)


def build(name):
    """An i8ie.Module running network(name) on the GPU."""
    import int8inferenceengine_amd  # noqa: F401  (puts i8ie / _CXX_i8ie on sys.path)
    import i8ie

    layers, spec, _ = network(name)
    for op in _walk(spec):
        if op[0] not in OPS:
            raise ValueError("network %r: unknown spec op %r" % (name, op[0]))

    class SpecNet(i8ie.Module):
        def __init__(self):
            super().__init__()
            for op in _walk(spec):
                if op[0] == "add":
                    setattr(self, op[1], i8ie.Add())
                elif op[0] == "mul":
                    setattr(self, op[1], i8ie.Mul())
                elif op[0] == "concat":
                    setattr(self, op[1], i8ie.Concat())
                elif op[0] == "act":
                    setattr(self, op[1], i8ie.Activation(op[2], op[3] if len(op) > 3 else None))
                elif op[0] == "matmul":
                    setattr(self, op[1], i8ie.MatMul(transpose_a=op[3], transpose_b=op[4]))
                elif op[0] == "attention":
                    setattr(self, op[1], i8ie.Attention(op[2]))
            for attr, L in layers.items():
                if L[0] == "deconv":
                    setattr(self, attr, i8ie.ConvTranspose2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5], output_padding=L[6]))
                elif L[0] == "conv":
                    setattr(self, attr, i8ie.Conv2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5], groups=conv_groups(L),
                                                    dilation=conv_dilation(L)))
                elif L[0] == "ln":
                    setattr(self, attr, i8ie.LayerNorm(L[1]))
                elif L[0] == "gn":
                    setattr(self, attr, i8ie.GroupNorm(L[1], L[2]))
                else:
                    setattr(self, attr, i8ie.Linear(L[1], L[2]))

        def run(self, ops, x, saved):
            for op in ops:
                if op[0] == "layer":
                    x = getattr(self, op[1])(x)
                elif op[0] == "relu":
                    x = i8ie.relu(x)
                elif op[0] == "pool":
                    x = i8ie.max_pool2d(x, *op[1:])
                elif op[0] == "avgpool":
                    x = i8ie.avg_pool2d(x, *op[1:])
                elif op[0] == "gap":
                    x = i8ie.global_avg_pool2d(x)
                elif op[0] == "save":
                    saved[op[1]] = x
                elif op[0] == "branch":
                    saved[op[1]] = self.run(op[2], saved[op[1]], saved)
                elif op[0] == "load":
                    x = saved[op[1]]
                elif op[0] in ("add", "mul", "matmul"):
                    x = getattr(self, op[1])(x, saved[op[2]])
                elif op[0] == "softmax":
                    x = i8ie.softmax(x)
                elif op[0] == "attention":
                    x = getattr(self, op[1])(x, *[saved[t] for t in op[3:]])
                elif op[0] == "concat":
                    x = getattr(self, op[1])([x] + [saved[t] for t in op[2]])
                elif op[0] == "act":
                    x = getattr(self, op[1])(x)
                elif op[0] == "upsample":
                    x = i8ie.upsample(x, op[1], op[2])
                elif op[0] == "flatten":
                    x = x.reshape(-1, op[1])
            return x

        def forward(self, x):
            return self.run(spec, x, {})

    SpecNet.__name__ = "SpecNet_" + name
    return SpecNet()


def calibrated(name, state_dict=None, calib_batch=None, seed=42, calib_seed=7, per_channel=False, calibration=None):
    """The reference workflow (notebook cells 'prepare -> one FP32 batch -> convert'); per_channel=True converts
    with one weight scale per output feature (Module.convert).  calibration: None for the setting in force (the reservoir
    unless i8ie.set_calibration chose otherwise), or "minmax", ("percentile", p) or "mse": that histogram method around this
    call alone, the earlier setting put back afterwards, also on an exception."""
    import _CXX_i8ie as cx
    import i8ie

    net = build(name)
    net.load(state_dict if state_dict is not None else synthetic_state_dict(name, seed))
    cx.set_calibration_seed(calib_seed)  # the reference's calibrator is unseeded (std::random_device)
    before = i8ie.calibration()
    if calibration is not None:
        method, p = calibration if isinstance(calibration, (tuple, list)) else (calibration, before["percentile"])
        i8ie.set_calibration(method, p)
    try:
        net.prepare()
        x = calib_batch if calib_batch is not None else synthetic_input(name, 100 if not name.startswith("alexnet") else 32, seed=99)
        net(i8ie.tensor(x))
        net.convert(per_channel)
    finally:
        if calibration is not None:
            i8ie.set_calibration(before["method"], before["percentile"])
    return net


def op_names(name, *kinds):
    """the attribute names of the ops of the given kinds, in the order the spec names them, those of a branch included"""
    return [op[1] for op in _walk(network(name)[1]) if op[0] in kinds]


def layer_names(name):
    """the layers of the `layers` dict (Conv2d / ConvTranspose2d / Linear / LayerNorm / GroupNorm)"""
    return op_names(name, "layer")


def add_names(name):
    return op_names(name, "add")


def mul_names(name):
    return op_names(name, "mul")


def concat_names(name):
    return op_names(name, "concat")


def activation_names(name):
    return op_names(name, "act")


def attention_names(name):
    """the Attentions: the joins that have score_qparams() too"""
    return op_names(name, "attention")


def join_names(name):
    """every op that is a module without weights (Add, Mul, Concat, Activation, MatMul, Attention): those with
    output_qparams() beside the layers"""
    return op_names(name, "add", "mul", "concat", "act", "matmul", "attention")
