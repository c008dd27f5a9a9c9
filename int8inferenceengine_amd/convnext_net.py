"""ConvNeXt-style networks (Liu et al. 2022): the first users of `i8ie.LayerNorm`.  They are hand-written here and are not
entries of `workloads.NETWORKS` (the registry and its op set are closed); the layer tuples are the registry's, ("conv", in,
out, k, stride, pad[, groups]) and ("fc", in, out), plus ("ln", channels), and the plan is a spec of the registry's ops plus
three of its own:

    ("ln", attr)       x = <attr>(x), an i8ie.LayerNorm: over c per pixel of [n, c, h, w], over f of [n, f]
    ("cnblock", p)     with x [n, c, h, w] the current tensor:
                           y = <p>ln(<p>dw(x))                   depthwise 7x7 p3 groups = c, LayerNorm(c)
                           y = <p>pw2(<p>act(<p>pw1(y)))         1x1 c -> 4c, hardswish, 1x1 4c -> c
                           x = <p>add(y, x)
                       The layer-scale factor LAYER_SCALE is folded into pw2's weights (synthetic_state_dict).
    ("attn", p)        a pre-LN single-head attention block, t = h * w, d the projection width:
                           y = <p>ln(x);  theta, phi, g = <p>theta(y), <p>phi(y), <p>g(y)      one LN feeds three 1x1 convs c -> d
                           s = <p>mm1(theta, phi)      transpose_a: [n, t, t];   pr = softmax(s)
                           z = <p>mm2(g, pr)           transpose_b: [n, d, h, w]
                           x = <p>add(<p>out(z), x)    1x1 conv d -> c
                       A 1/sqrt(d) factor is folded into theta's weights.

    "tiny"    3x32x32: stem conv 3->16 4x4 s4 (8x8), LayerNorm(16), a block at c = 16, a downsample LayerNorm(16) -> conv 16->20
              3x3 s2 p1 (an LN result that carries a border; 4x4), a block at c = 20 (rows that are no multiple of 16), an
              attention block at c = 20, d = 12, global average pool, LayerNorm(20) on [n, 20], fc 20->10.
    "cifar"   3x32x32: patchify stem 3->64 2x2 s2 + LN (16x16), stages of (2, 2, 2, 2) blocks at 64 / 128 / 256 / 512 with
              LN + 2x2 s2 conv between them, global average pool, LN, fc 512->10: for the example and benchmarks."""
import numpy as np

import i8ie  # (the package's __init__ has put it on the path)

LAYER_SCALE = 0.5


def _cnblock(layers, spec, p, c):
    layers[p + "dw"] = ("conv", c, c, 7, 1, 3, c)
    layers[p + "ln"] = ("ln", c)
    layers[p + "pw1"] = ("conv", c, 4 * c, 1, 1, 0)
    layers[p + "pw2"] = ("conv", 4 * c, c, 1, 1, 0)
    spec.append(("cnblock", p))


def _attn(layers, spec, p, c, d):
    layers[p + "ln"] = ("ln", c)
    for r in ("theta", "phi", "g"):
        layers[p + r] = ("conv", c, d, 1, 1, 0)
    layers[p + "out"] = ("conv", d, c, 1, 1, 0)
    spec.append(("attn", p))


def _tiny():
    layers = {"stem": ("conv", 3, 16, 4, 4, 0), "stem_ln": ("ln", 16)}
    spec = [("layer", "stem"), ("ln", "stem_ln")]
    _cnblock(layers, spec, "a_", 16)
    layers["down_ln"] = ("ln", 16)
    layers["down"] = ("conv", 16, 20, 3, 2, 1)
    spec += [("ln", "down_ln"), ("layer", "down")]
    _cnblock(layers, spec, "b_", 20)
    _attn(layers, spec, "t_", 20, 12)
    layers["head_ln"] = ("ln", 20)
    layers["fc"] = ("fc", 20, 10)
    spec += [("gap",), ("flatten", 20), ("ln", "head_ln"), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _cifar():
    layers = {"stem": ("conv", 3, 64, 2, 2, 0), "stem_ln": ("ln", 64)}
    spec = [("layer", "stem"), ("ln", "stem_ln")]
    c = 64
    for s in range(4):
        if s:
            layers["d%d_ln" % s] = ("ln", c)
            layers["d%d" % s] = ("conv", c, 2 * c, 2, 2, 0)
            spec += [("ln", "d%d_ln" % s), ("layer", "d%d" % s)]
            c *= 2
        for b in range(2):
            _cnblock(layers, spec, "s%db%d_" % (s, b), c)
    layers["head_ln"] = ("ln", c)
    layers["fc"] = ("fc", c, 10)
    spec += [("gap",), ("flatten", c), ("ln", "head_ln"), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


CONFIGS = {"tiny": _tiny(), "cifar": _cifar()}


def layer_names(config):
    """the convs, LayerNorms and the fc, in the order the module holds them"""
    return list(CONFIGS[config][0])


def join_names(config):
    """the layers without weights: every block's Activation and Add, an attention block's two MatMuls and its Add"""
    out = []
    for op in CONFIGS[config][1]:
        if op[0] == "cnblock":
            out += [op[1] + "act", op[1] + "add"]
        elif op[0] == "attn":
            out += [op[1] + "mm1", op[1] + "mm2", op[1] + "add"]
    return out


def synthetic_state_dict(config, seed=42):
    """workloads.synthetic_state_dict's rule for the convs and the fc (He-uniform weights, U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    biases), LAYER_SCALE folded into every block's pw2 and 1/sqrt(d) into every theta; a LayerNorm gets gamma from U(0.5, 1.5)
    and beta from U(-0.3, 0.3)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for attr, L in CONFIGS[config][0].items():
        if L[0] == "ln":
            sd[attr + ".weight"] = rng.uniform(0.5, 1.5, L[1]).astype(np.float32)
            sd[attr + ".bias"] = rng.uniform(-0.3, 0.3, L[1]).astype(np.float32)
            continue
        groups = L[6] if len(L) > 6 else 1
        shape = (L[2], L[1] // groups, L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
        fan_in = int(np.prod(shape[1:]))
        fold = 1.0 / np.sqrt(L[2]) if attr.endswith("theta") else (LAYER_SCALE if attr.endswith("pw2") else 1.0)
        sd[attr + ".weight"] = (rng.uniform(-1, 1, shape) * np.sqrt(6.0 / fan_in) * fold).astype(np.float32)
        sd[attr + ".bias"] = (rng.uniform(-1, 1, shape[0]) / np.sqrt(fan_in) * fold).astype(np.float32)
    return sd


def synthetic_input(config, batch, seed=1234):
    """workloads.synthetic_input's normalised-image-like batch"""
    c, h, w = CONFIGS[config][2]
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (batch, c, h, w)).astype(np.float32)
    a = rng.uniform(0.2, 1.0, (batch, c, 1, 1)).astype(np.float32)
    return ((u * a - np.float32(0.45)) / np.float32(0.226)).astype(np.float32)


class ConvNeXt(i8ie.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        layers, spec, _ = CONFIGS[config]
        for attr, L in layers.items():
            if L[0] == "conv":
                setattr(self, attr, i8ie.Conv2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5], groups=L[6] if len(L) > 6 else 1))
            elif L[0] == "ln":
                setattr(self, attr, i8ie.LayerNorm(L[1]))
            else:
                setattr(self, attr, i8ie.Linear(L[1], L[2]))
        for op in spec:
            if op[0] == "cnblock":
                setattr(self, op[1] + "act", i8ie.Activation("hardswish"))
                setattr(self, op[1] + "add", i8ie.Add())
            elif op[0] == "attn":
                setattr(self, op[1] + "mm1", i8ie.MatMul(transpose_a=True))
                setattr(self, op[1] + "mm2", i8ie.MatMul(transpose_b=True))
                setattr(self, op[1] + "add", i8ie.Add())

    def cnblock(self, p, x):
        L = lambda r: getattr(self, p + r)  # noqa: E731
        y = L("ln")(L("dw")(x))
        y = L("pw2")(L("act")(L("pw1")(y)))
        return L("add")(y, x)

    def attn(self, p, x):
        L = lambda r: getattr(self, p + r)  # noqa: E731
        y = L("ln")(x)
        s = L("mm1")(L("theta")(y), L("phi")(y))
        z = L("mm2")(L("g")(y), i8ie.softmax(s))
        return L("add")(L("out")(z), x)

    def run(self, ops, x):
        for op in ops:
            if op[0] in ("layer", "ln"):
                x = getattr(self, op[1])(x)
            elif op[0] == "cnblock":
                x = self.cnblock(op[1], x)
            elif op[0] == "attn":
                x = self.attn(op[1], x)
            elif op[0] == "gap":
                x = i8ie.global_avg_pool2d(x)
            elif op[0] == "flatten":
                x = x.reshape(-1, op[1])
            else:
                raise ValueError("ConvNeXt: unknown op %r" % (op[0],))
        return x

    def forward(self, x):
        return self.run(CONFIGS[self.config][1], x)


def build(config):
    """ConvNeXt(config) on the GPU"""
    return ConvNeXt(config)


def calibrated(config, state_dict=None, calib_batch=None, seed=42, calib_seed=7, per_channel=False):
    """workloads.calibrated's flow: prepare -> one FP32 batch -> convert"""
    import _CXX_i8ie as cx

    net = build(config)
    net.load(state_dict if state_dict is not None else synthetic_state_dict(config, seed))
    cx.set_calibration_seed(calib_seed)
    net.prepare()
    net(i8ie.tensor(calib_batch if calib_batch is not None else synthetic_input(config, 100, seed=99)))
    net.convert(per_channel)
    return net
