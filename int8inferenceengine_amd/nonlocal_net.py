"""Networks with a non-local (self-attention) block (Wang et al. 2018) behind a CNN backbone: the first users of
`i8ie.MatMul` and `i8ie.softmax`.  They are hand-written here and are not entries of `workloads.NETWORKS` (the registry and
its op set are closed); the layer tuples are the registry's, ("conv", in, out, k, stride, pad) and ("fc", in, out), and the
plan is a spec of the registry's ops plus one op of its own:

    ("nonlocal", p)    with x [n, c, h, w] the current tensor, t = h * w and d the projection width:
                           theta, phi, g = <p>theta(x), <p>phi(x), <p>g(x)          1x1 convs c -> d
                           s = <p>mm1(theta, phi)      transpose_a: [n, t, t], s[i, j] = sum_c theta[c, i] phi[c, j]
                           p = softmax(s)              over j
                           y = <p>mm2(g, p)            transpose_b: [n, d, h, w], y[c, i] = sum_j g[c, j] p[i, j]
                           x = <p>add(<p>out(y), x)    1x1 conv d -> c, residual Add (a relu follows in the plan)
                       A 1/sqrt(d) factor is folded into theta's weights (synthetic_state_dict).

    "tiny"    3x32x32: conv 3->16 3x3 s2 p1, relu, max-pool 2/2 (8x8, t = 64), block A (c = 16, d = 16), relu, conv 16->20 3x3
              s2 p1 (a bordered consumer), relu (4x4, t = 16), block B (c = 20, d = 12: k = 12 takes bmm_direct), relu, global
              average pool, fc 20->10.
    "cifar"   resnet18_cifar's layers with one block (c = 256, d = 128) after stage 3 (8x8): for the example and benchmarks."""
import numpy as np

import i8ie  # (the package's __init__ has put it on the path)

from . import workloads as wl


def _nonlocal(layers, spec, p, c, d):
    for r in ("theta", "phi", "g"):
        layers[p + r] = ("conv", c, d, 1, 1, 0)
    layers[p + "out"] = ("conv", d, c, 1, 1, 0)
    spec.append(("nonlocal", p))


def _tiny():
    layers = {"stem": ("conv", 3, 16, 3, 2, 1)}
    spec = [("layer", "stem"), ("relu",), ("pool", 2, 2)]
    _nonlocal(layers, spec, "a_", 16, 16)
    layers["down"] = ("conv", 16, 20, 3, 2, 1)
    spec += [("relu",), ("layer", "down"), ("relu",)]
    _nonlocal(layers, spec, "b_", 20, 12)
    layers["fc"] = ("fc", 20, 10)
    spec += [("relu",), ("gap",), ("flatten", 20), ("layer", "fc")]
    return layers, spec, (3, 32, 32)


def _cifar():
    base_layers, base_spec, shape = wl.network("resnet18_cifar")
    layers, spec = {}, []
    for op in base_spec:
        if op == ("save", "s4b1"):  # stage 3 has ended: 256 channels at 8x8
            _nonlocal(layers, spec, "nl_", 256, 128)
            spec.append(("relu",))
        spec.append(op)
    merged = {}
    for attr, L in base_layers.items():  # (keeps the registry's layer order, the block's layers where stage 4 begins)
        if attr == "s4b1c1":
            merged.update(layers)
        merged[attr] = L
    return merged, spec, shape


CONFIGS = {"tiny": _tiny(), "cifar": _cifar()}


def blocks(config):
    """the prefixes of the non-local blocks, in plan order"""
    return [op[1] for op in CONFIGS[config][1] if op[0] == "nonlocal"]


def layer_names(config):
    return list(CONFIGS[config][0])


def join_names(config):
    """the layers without weights: every block's two MatMuls and its Add, and the backbone's Adds"""
    out = []
    for op in wl._walk(CONFIGS[config][1]):
        if op[0] == "nonlocal":
            out += [op[1] + "mm1", op[1] + "mm2", op[1] + "add"]
        elif op[0] == "add":
            out.append(op[1])
    return out


def synthetic_state_dict(config, seed=42):
    """workloads.synthetic_state_dict's rule (He-uniform weights, U(-1/sqrt(fan_in), 1/sqrt(fan_in)) biases), with the
    attention's 1/sqrt(d) folded into every theta projection"""
    rng = np.random.default_rng(seed)
    sd = {}
    for attr, L in CONFIGS[config][0].items():
        shape = (L[2], L[1], L[3], L[3]) if L[0] == "conv" else (L[2], L[1])
        fan_in = int(np.prod(shape[1:]))
        fold = 1.0 / np.sqrt(L[2]) if attr.endswith("theta") else 1.0
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


class NonLocalNet(i8ie.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        layers, spec, _ = CONFIGS[config]
        for attr, L in layers.items():
            if L[0] == "conv":
                setattr(self, attr, i8ie.Conv2d(L[1], L[2], kernel_size=L[3], stride=L[4], padding=L[5]))
            else:
                setattr(self, attr, i8ie.Linear(L[1], L[2]))
        for op in wl._walk(spec):
            if op[0] == "add":
                setattr(self, op[1], i8ie.Add())
            elif op[0] == "nonlocal":
                setattr(self, op[1] + "mm1", i8ie.MatMul(transpose_a=True))
                setattr(self, op[1] + "mm2", i8ie.MatMul(transpose_b=True))
                setattr(self, op[1] + "add", i8ie.Add())

    def nonlocal_block(self, p, x):
        s = getattr(self, p + "mm1")(getattr(self, p + "theta")(x), getattr(self, p + "phi")(x))
        y = getattr(self, p + "mm2")(getattr(self, p + "g")(x), i8ie.softmax(s))
        return getattr(self, p + "add")(getattr(self, p + "out")(y), x)

    def run(self, ops, x, saved):
        for op in ops:
            if op[0] == "layer":
                x = getattr(self, op[1])(x)
            elif op[0] == "relu":
                x = i8ie.relu(x)
            elif op[0] == "pool":
                x = i8ie.max_pool2d(x, op[1], op[2])
            elif op[0] == "gap":
                x = i8ie.global_avg_pool2d(x)
            elif op[0] == "save":
                saved[op[1]] = x
            elif op[0] == "branch":
                saved[op[1]] = self.run(op[2], saved[op[1]], saved)
            elif op[0] == "add":
                x = getattr(self, op[1])(x, saved[op[2]])
            elif op[0] == "flatten":
                x = x.reshape(-1, op[1])
            elif op[0] == "nonlocal":
                x = self.nonlocal_block(op[1], x)
            else:
                raise ValueError("NonLocalNet: unknown op %r" % (op[0],))
        return x

    def forward(self, x):
        return self.run(CONFIGS[self.config][1], x, {})


def build(config):
    """NonLocalNet(config) on the GPU"""
    return NonLocalNet(config)


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
