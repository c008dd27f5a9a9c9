"""A seeded generator of well-formed `workloads` specs over the whole op grammar, for the random-network tests on the host
(tests/test_spec_fuzz_host.py) and on the GPU (tests/test_gpu_spec_fuzz.py); DESIGN.md section 2.  A helper module, not a
conftest.

  random_network(rng)   (layers, spec, (c, h, w), folds): 2-5 blocks drawn at random and a tail.  The generator tracks (c, h, w)
                        as it goes, so every spec is legal by construction; shapes(entry) is the independent walk that checks it
  case(index)           everything a test needs of default case `index`: the entry, the folds, the batch and the seeds
  features(entry)       the block kinds and options a spec holds, read from the spec itself (the coverage assertion)
  discrimination(trace) the three conditions on the expected bytes, as figures
  describe(entry)       one line per op, for failure messages
  first_divergence(...) the first top-level op whose bytes differ from the reference's trace

Sizes stay small -- input 3 x 12..32 x 12..32, maps at most 32 x 32, at most 48 channels (the packed qkv conv of an Attention
apart) -- the point is variety of composition."""
import numpy as np

import act_ref as acr
import padpool_ref as ppr
from int8inferenceengine_amd import workloads as wl

CHANNELS = (8, 12, 16, 20, 32, 35, 48)   # 16-, 4- and 1-byte items of the pointwise kernels; both forms of the norms
MAX_C, MAX_HW, MIN_HW = 48, 32, 3
MAX_TOKENS = 100                          # h * w of a map that an attention block reads: its softmax rows keep >= 16 byte values
BATCHES = (1, 3, 5)
DECONVS = ((2, 2, 0, 0), (4, 2, 1, 0), (3, 2, 1, 1))   # (k, stride, pad, output_pad): the three forms of unet_tiny
BLOCKS = ("conv", "deconv", "deconv", "deconv", "pool", "pool", "pool", "pool", "imagepool", "upsample", "residual", "se", "mul", "concat",
          "act", "act", "act", "norm", "norm", "norm", "nonlocal", "nonlocal", "attention", "attention")   # (weights: see REQUIRED)
CALIB_IMAGES = 8                          # at least; calib_images() raises it where an op's output is a short vector
SCORE_GAIN = 2.0                          # folded into phi of a non-local block, whose input is normalised: score rows with a
                                          # spread of a few units, neither flat nor one-hot
SATURATING = ("tanh", "sigmoid", "hardsigmoid")
TAILS = ("gap", "flatten", "flatten2", "head", "head_up")
# what a sweep has to meet, as (block kind, option): plan() deals them out, every one once per pass
PLAN = ([("deconv", d) for d in DECONVS] + [("norm", o) for o in ("ln", "g1", "gc", "gany")]
        + [("pool", o) for o in ("max", "avg", "maxpad", "avgpad", "avgnocip", "ceil")]
        + [("upsample", o) for o in (("nearest", False), ("nearest", True), ("bilinear", False), ("bilinear", True))]
        + [("act", k) for k in sorted(acr.KINDS)]
        + [("attention", o) for o in ((True, True), (True, False), (False, True), (False, False))]   # (packed, d % 16 == 0)
        + [("nonlocal", 8), ("nonlocal", 16), ("conv", "depthwise"), ("conv", "dilated"), ("conv", "k7"), ("conv", "grouped"),
           ("residual", "identity"), ("residual", "projection"), ("concat", (2, "pool")), ("concat", (3, "nothing")), ("concat", (2, "nothing")), ("concat", (3, "pool")), ("se", None), ("mul", None),
           ("imagepool", None)])
SEED = 1000                                  # case i: network SEED + i, weights + 100 000, calibration + 200 000, input + 300 000

def _divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def conv_out(size, k, s, p, d=1):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


class _Gen:
    def __init__(self, rng, index=None):
        self.rng, self.layers, self.spec, self.folds, self.n = rng, {}, [], {}, 0
        self.index, self.opt, self.mul_hot, self.relu, self.reuses = index, None, False, False, index or 0
        self.depth = 0   # weighted layers since the last norm (the input counts as normalised)
        self.c, self.h, self.w = 3, int(rng.integers(12, 33)), int(rng.integers(12, 33))
        self.input = (self.c, self.h, self.w)
        self.old = []    # [(tag, (c, h, w))]: saved tensors that a consumer has already read and no branch has replaced

    # ---- small helpers
    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def take(self, draw):
        """the option the plan sets for this block (once), or draw()"""
        opt, self.opt = self.opt, None
        return draw() if opt is None else opt

    def chance(self, num, den):
        return int(self.rng.integers(0, den)) < num

    def name(self, prefix):
        self.n += 1
        return "%s%d" % (prefix, self.n)

    def shape(self):
        return self.c, self.h, self.w

    def set(self, shape):
        self.c, self.h, self.w = shape

    def maybe_relu(self, ops, num=1, den=2):
        """with chance num / den a relu behind the last op of `ops`, one time in four an Activation in its place"""
        if self.chance(num, den):
            ops.append(self.act() if self.chance(1, 4) else ("relu",))

    def act(self):
        """an Activation op; a kind that saturates (SATURATING) only within two weighted layers of a norm: further on, ranges
        have grown until most input bytes lie on the flat ends, and its output and what follows hold a handful of values"""
        kind = self.pick([k for k in sorted(acr.KINDS) if self.depth < 2 or k not in SATURATING])
        return ("act", self.name("act"), kind) + ((self.pick((0.01, 0.1, 0.2)),) if kind == "leaky_relu" else ())

    def shrink(self, fits):
        """2/2 floor max-pools until fits(h, w); False, with nothing appended, where the map would fall below MIN_HW first"""
        h, w, n = self.h, self.w, 0
        while not fits(h, w):
            h, w, n = h // 2, w // 2, n + 1
            if min(h, w) < MIN_HW:
                return False
        self.spec += [("pool", 2, 2)] * n
        self.set((self.c, h, w))
        return True

    def conv(self, ops, shape, oc=None, k=None, stride=None, pad=None, dilation=None, groups=None):
        """one Conv2d behind `shape` into `ops`; what is None is drawn, until the extent fits and the map stays >= MIN_HW.
        Returns the shape behind it."""
        c, h, w = shape
        for _ in range(40):
            kk = k if k is not None else self.pick((1, 3, 3, 5, 7))
            st = stride if stride is not None else self.pick((1, 1, 2))
            dd = dilation if dilation is not None else (1 if kk == 1 else self.pick((1, 1, 2, 3)))
            pp = pad if pad is not None else int(self.rng.integers(0, kk // 2 + 1))
            oh, ow = conv_out(h, kk, st, pp, dd), conv_out(w, kk, st, pp, dd)
            if dd * (kk - 1) + 1 <= min(h, w) + 2 * pp and min(oh, ow) >= MIN_HW:
                break
        else:
            kk, st, dd, pp, oh, ow = 1, 1, 1, 0, h, w
        if oc is None and groups is None and c > 3 and self.chance(1, 3):   # depthwise
            oc, groups = c, c
        if oc is None:
            oc = self.pick(CHANNELS)
        if groups is None:
            groups = 1 if self.chance(1, 2) else self.pick([g for g in _divisors(c) if oc % g == 0])
        attr = self.name("conv")
        self.depth += 1
        self.layers[attr] = ("conv", c, oc, kk, st, pp, groups, dd)
        ops.append(("layer", attr))
        return oc, oh, ow

    def pool(self, ops, shape, padded=None, same=False, opt=None):
        """a max or average pool behind `shape` into `ops`: floor-unpadded (the reference's forms), or with padding / ceil_mode /
        count_include_pad=False, legal per padpool_ref.legal.  same: k 3, stride 1, padding 1 (the map keeps its size)"""
        c, h, w = shape
        avg = self.chance(1, 2) if opt is None else opt.startswith("avg")
        if same:
            tail = (3, 1, 1, self.chance(1, 3)) + ((self.chance(1, 2),) if avg else ())
            ops.append((("avgpool" if avg else "pool"),) + tail)
            return shape
        padded = (self.chance(2, 3) if opt is None else opt not in ("max", "avg")) if padded is None else padded
        for _ in range(40):
            if not padded:
                k, s = self.pick(((2, 2), (3, 2), (3, 1), (2, 1)))
                oh, ow = (h - k) // s + 1, (w - k) // s + 1
                if k <= min(h, w) and min(oh, ow) >= MIN_HW:
                    ops.append(("avgpool" if avg else "pool", k, s))
                    return c, oh, ow
                continue
            k, s = self.pick((2, 3, 3, 5)), self.pick((1, 2, 2, 3))
            p, ceil, cip = int(self.rng.integers(0, k // 2 + 1)), self.chance(1, 2), self.chance(1, 2)
            if not (ppr.legal(h, k, s, p) and ppr.legal(w, k, s, p)) or (p == 0 and not ceil and (cip or not avg)):
                continue
            if (opt in ("maxpad", "avgpad", "avgnocip") and p == 0) or (opt == "avgnocip" and cip) or (opt == "ceil" and not ceil):
                continue
            oh, ow = ppr.out_size(h, k, s, p, ceil), ppr.out_size(w, k, s, p, ceil)
            if min(oh, ow) >= MIN_HW:
                ops.append(("avgpool", k, s, p, ceil, cip) if avg else ("pool", k, s, p, ceil))
                return c, oh, ow
        return shape

    # ---- blocks: each appends to self.spec and moves (c, h, w); False: not applicable here, draw another
    def b_conv(self):
        opt = self.take(lambda: None)
        mid = [g for g in _divisors(self.c) if 1 < g < self.c]
        kw = {None: {}, "depthwise": {"oc": self.c, "groups": self.c}, "dilated": {"k": 3, "dilation": 2, "pad": 1, "stride": 1},
              "k7": {"k": 7}, "grouped": {"oc": self.c, "groups": self.pick(mid)} if mid else {}}[opt]
        self.set(self.conv(self.spec, self.shape(), **kw))

    def b_deconv(self):
        k, s, p, op = self.take(lambda: self.pick(DECONVS))
        if not self.shrink(lambda h, w: (max(h, w) - 1) * s - 2 * p + k + op <= MAX_HW):
            return False
        oh, ow = (self.h - 1) * s - 2 * p + k + op, (self.w - 1) * s - 2 * p + k + op
        attr, oc = self.name("deconv"), self.pick(CHANNELS)
        self.depth += 1
        self.layers[attr] = ("deconv", self.c, oc, k, s, p, op)
        self.spec.append(("layer", attr))
        self.set((oc, oh, ow))

    def b_pool(self):
        self.set(self.pool(self.spec, self.shape(), opt=self.take(lambda: None)))

    def b_imagepool(self):
        """the ASPP image-pool pattern: gap, 1x1 conv, [relu], nearest upsample back; joined with the map by Concat or Add"""
        if not self.shrink(lambda h, w: max(h, w) <= 8):
            return False
        c, h, w = self.shape()
        add = c + 16 > MAX_C or self.chance(1, 3)   # (at least 16 channels in the branch: its tensors are one value per channel)
        tag, ops = self.name("ip"), [("gap",)]
        oc = self.conv(ops, (c, 1, 1), oc=c if add else self.pick([x for x in CHANNELS if x >= 16 and c + x <= MAX_C]), k=1, stride=1, pad=0,
                       groups=1)[0]
        self.maybe_relu(ops)
        ops.append(("upsample", (h, w) if h != w else h, "nearest"))
        self.spec += [("save", tag), ("branch", tag, ops)]
        self.spec.append(("add", self.name("add"), tag) if add else ("concat", self.name("cat"), [tag]))
        self.set((c if add else c + oc, h, w))

    def b_upsample(self):
        f = [(fh, fw) for fh in (1, 2, 3) for fw in (1, 2, 3) if fh * fw > 1 and self.h * fh <= MAX_HW and self.w * fw <= MAX_HW]
        if not f:
            return False if not self.shrink(lambda h, w: 2 * max(h, w) <= MAX_HW) else self.b_upsample()
        mode, pair = self.take(lambda: (self.pick(("nearest", "bilinear")), self.chance(1, 2)))
        fh, fw = self.pick([x for x in f if pair or x[0] == x[1]] or f)
        self.spec.append(("upsample", (fh, fw) if pair or fh != fw else fh, mode))
        self.set((self.c, self.h * fh, self.w * fw))

    def b_residual(self):
        """two 3x3 pad-1 convs and the Add with the block's input: identity, or a strided 1x1 projection in the branch"""
        c, h, w = self.shape()
        form = self.take(lambda: self.pick(("identity", "projection", "projection")))
        tag, stride = self.name("res"), 1 if form == "identity" else self.pick((1, 2))
        oc = c if form == "identity" else self.pick([x for x in CHANNELS if stride == 2 or x != c])
        if stride == 2 and min(conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)) < MIN_HW:
            stride = 1
        self.spec.append(("save", tag))
        s1 = self.conv(self.spec, (c, h, w), oc=oc, k=3, stride=stride, pad=1, dilation=1)
        self.maybe_relu(self.spec, 3, 4)
        s2 = self.conv(self.spec, s1, oc=oc, k=3, stride=1, pad=1, dilation=1)
        if stride != 1 or oc != c:
            ops = []
            assert self.conv(ops, (c, h, w), oc=oc, k=1, stride=stride, pad=0, groups=1) == s2
            self.spec.append(("branch", tag, ops))
        else:
            self.old.append((tag, (c, h, w)))
        self.spec.append(("add", self.name("add"), tag))
        self.set(s2)

    def b_se(self):
        """squeeze-and-excitation: the map times a gate [n, c] of its global average"""
        self.cool()
        wl._squeeze_excite(self.layers, self.spec, self.name("se"), self.c, self.pick((8, 12, 16)))

    def b_mul(self):
        """the product of two conv outputs of one shape"""
        self.cool()
        c, h, w = self.shape()
        tag, oc, ops = self.name("m"), self.pick(CHANNELS), []
        self.spec.append(("save", tag))
        self.conv(self.spec, (c, h, w), oc=oc, k=1, stride=1, pad=0)
        self.conv(ops, (c, h, w), oc=oc, k=3, stride=1, pad=1, dilation=1)
        self.maybe_relu(ops, 1, 3)
        self.spec += [("branch", tag, ops), ("mul", self.name("mul"), tag)]
        self.set((oc, h, w))

    def b_concat(self):
        """Concat of 2-3 branches with different channel counts: each a conv, a pool or nothing, all at one stride"""
        count, must = self.take(lambda: (self.pick((2, 3)), None))
        if must and self.c > 28:   # (a pool or an empty branch keeps the channels: room for the others)
            self.set(self.conv(self.spec, self.shape(), oc=16, k=1, stride=1, pad=0, groups=1))
        c, h, w = self.shape()
        for _ in range(40):
            stride = 2 if min(conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)) >= MIN_HW and self.chance(1, 3) and must != "nothing" else 1
            kinds = [self.pick(("conv", "conv", "pool") + (("nothing",) if stride == 1 else ())) for _ in range(count)]
            if must:
                kinds[1] = must
            widths = [self.pick((8, 12, 16, 20)) if kd == "conv" else c for kd in kinds]
            if sum(widths) <= MAX_C and kinds.count("nothing") <= 1 and len(set(widths)) > 1:
                break
        else:
            return False
        tags = [self.name("cb") for _ in kinds[1:]]
        self.spec += [("save", t) for t in tags]
        out = None
        for i, (kd, oc) in enumerate(zip(kinds, widths)):
            ops = []
            if kd == "conv":
                k = self.pick((1, 3, 5)) if stride == 1 else self.pick((1, 3))
                got = self.conv(ops, (c, h, w), oc=oc, k=k, stride=stride, pad=k // 2, dilation=1)
                self.maybe_relu(ops, 1, 3)
            elif kd == "pool" and stride == 1:
                got = self.pool(ops, (c, h, w), same=True)
            elif kd == "pool":
                avg = self.chance(1, 2)
                ops.append(("avgpool", 3, 2, 1, False, self.chance(1, 2)) if avg else ("pool", 3, 2, 1))
                got = (c, conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1))
            else:
                got = (c, h, w)
            assert out is None or got[1:] == out[1:], (got, out)
            out = got
            if i == 0:
                self.spec += ops
            elif ops:
                self.spec.append(("branch", tags[i - 1], ops))
            else:
                self.old.append((tags[i - 1], (c, h, w)))
        self.spec.append(("concat", self.name("cat"), tags))
        self.set((sum(widths),) + out[1:])

    def b_act(self):
        kind = self.take(lambda: None)
        if kind in SATURATING and self.depth >= 2:
            self.norm(self.spec, self.pick(("ln", "g1", "gc", "gany")))
        op = self.act()
        self.spec.append(op if kind is None else ("act", op[1], kind) + ((self.pick((0.01, 0.1, 0.2)),) if kind == "leaky_relu" else ()))

    def b_norm(self):
        if self.c == 3:
            return False
        self.norm(self.spec, self.take(lambda: self.pick(("ln", "g1", "gc", "gany"))))

    def norm(self, ops, form):
        attr = self.name("norm")
        g = {"ln": 0, "g1": 1, "gc": self.c, "gany": self.pick(_divisors(self.c))}[form]
        self.layers[attr] = ("gn", g, self.c) if g else ("ln", self.c)
        ops.append(("layer", attr))
        self.mul_hot, self.depth = False, 0

    def cool(self):
        """a norm ahead of a Mul where the last Mul has had none behind it: a chain of products narrows every range"""
        if self.mul_hot:
            self.norm(self.spec, self.pick(("ln", "g1", "gc", "gany")))
        self.mul_hot = True

    def b_nonlocal(self):
        """workloads._nonlocal: theta / phi / g 1x1 convs, MatMul transpose_a (k = d), Softmax, MatMul transpose_b (k = h * w),
        a 1x1 conv back and the Add; d < 16 takes bmm_direct, d >= 16 bmm_mfma"""
        if not self.shrink(lambda h, w: h * w <= MAX_TOKENS):
            return False
        p, d = self.name("nl") + "_", self.take(lambda: self.pick((8, 12, 16, 20)))
        self.spec.append(("save", p + "x"))
        self.norm(self.spec, self.pick(("ln", "g1", "gc", "gany")))   # (pre-norm, as workloads._attn: scores of a known spread)
        wl._attention(self.layers, self.spec, self.folds, p, self.c, d)
        self.spec += [("load", p + "g"), ("add", p + "add", p + "x")]
        self.folds[p + "phi"] = SCORE_GAIN
        self.old.append((p + "x", self.shape()))

    def b_attention(self):
        """fused Attention behind a packed 1x1 conv (workloads._mha) or of three 1x1 convs, a 1x1 projection and the skip;
        d = c / heads on both sides of the attn_mfma (d % 16 == 0) / attn_direct line"""
        if not self.shrink(lambda h, w: h * w <= MAX_TOKENS):
            return False
        packed, d16 = self.take(lambda: (self.chance(1, 2), self.chance(1, 2)))
        if (packed and self.c > 16) or (d16 and self.c % 16):   # a 1x1 conv to a channel count the form asks for
            self.set(self.conv(self.spec, self.shape(), oc=16 if packed else 32, k=1, stride=1, pad=0, groups=1))
        c = self.c
        heads = c // 16 if d16 else self.pick([x for x in _divisors(c) if c // x >= 4 and (c // x) % 16])
        p = self.name("at")
        self.spec.append(("save", p + "x"))
        self.norm(self.spec, self.pick(("ln", "g1", "gc", "gany")))
        if packed:
            wl._mha(self.layers, self.spec, self.folds, p + "qkv", p + "attn", c, heads)
        else:
            for r in ("q", "k", "v"):
                self.layers[p + r] = ("conv", c, c, 1, 1, 0)
            self.folds[p + "q"] = 1.0 / np.sqrt(c // heads)
            self.spec += [("save", p + "k"), ("save", p + "v"), ("layer", p + "q"), ("branch", p + "k", [("layer", p + "k")]),
                          ("branch", p + "v", [("layer", p + "v")]), ("attention", p + "attn", heads, p + "k", p + "v")]
        self.maybe_relu(self.spec, 3 if self.relu else 1, 3)
        self.layers[p + "proj"] = ("conv", c, c, 1, 1, 0)
        self.spec += [("layer", p + "proj"), ("add", p + "add", p + "x")]
        self.old.append((p + "x", self.shape()))

    def reuse(self):
        """a saved tensor that an earlier consumer has read is read again: brought to the current map by a padded 3x3 conv (behind
        an upsample, or at stride 2, where the sizes ask for one) and joined by Add, Mul or Concat; where no such step fits, as
        the gate [n, c] of a Mul"""
        tag, (c0, h0, w0) = self.old.pop(int(self.rng.integers(0, len(self.old))))
        c, h, w = self.shape()
        self.reuses += 1   # (the joins in turn, from a start that moves with the index)
        join = ("add", "mul", "concat")[self.reuses % 3]
        join = join if c + 8 <= MAX_C or join != "concat" else "add"
        if join == "mul" and self.mul_hot:
            join = "add"
        oc = self.pick([x for x in (8, 12, 16, 20) if c + x <= MAX_C]) if join == "concat" else c
        ops, stride = [], None
        if (h0, w0) == (h, w):
            stride = 1
        elif (conv_out(h0, 3, 2, 1), conv_out(w0, 3, 2, 1)) == (h, w):
            stride = 2
        elif h % h0 == 0 and w % w0 == 0 and max(h // h0, w // w0) <= 3:
            ops.append(("upsample", (h // h0, w // w0), self.pick(("nearest", "bilinear"))))
            h0, w0, stride = h, w, 1
        if stride is None:
            attr = self.name("fc")
            self.layers[attr] = ("fc", c0, c)
            ops, join = [("gap",), ("flatten", c0), ("layer", attr), ("act", self.name("act"), "hardsigmoid")], "mul"
            self.cool()
        else:
            self.conv(ops, (c0, h0, w0), oc=oc, k=3, stride=stride, pad=1, dilation=1)
            self.maybe_relu(ops, 1, 3)
        self.mul_hot = self.mul_hot or join == "mul"
        self.spec.append(("branch", tag, ops))
        self.spec.append((join, self.name(join if join != "concat" else "cat"), [tag] if join == "concat" else tag))
        if join == "concat":
            self.set((c + oc, h, w))

    def tail(self, kind=None):
        """gap, flatten, fc (behind a 1x1 conv of a relu'd map: its channel means spread over many byte values, those of most other
        producers lie within a few); flatten, fc[, relu, fc]; or a 1x1 conv head to 10 maps[, bilinear x2]"""
        kind = kind or self.pick(TAILS)
        if kind.startswith("flatten") and self.c * self.h * self.w > 8192:
            self.shrink(lambda h, w: self.c * h * w <= 8192)
        if kind == "gap":
            if self.spec[-1] != ("relu",):
                self.spec.append(("relu",))
            self.set(self.conv(self.spec, self.shape(), oc=self.pick((16, 20, 32, 35, 48)), k=1, stride=1, pad=0, groups=1))
        c, h, w = self.shape()
        if kind == "gap":
            self.layers["fc"] = ("fc", c, 10)
            self.spec += [("gap",), ("flatten", c), ("layer", "fc")]
        elif kind == "flatten2":
            hidden = self.pick((32, 64))
            self.layers["fc1"], self.layers["fc2"] = ("fc", c * h * w, hidden), ("fc", hidden, 10)
            self.spec += [("flatten", c * h * w), ("layer", "fc1"), ("relu",), ("layer", "fc2")]
        elif kind == "flatten":
            self.layers["fc"] = ("fc", c * h * w, 10)
            self.spec += [("flatten", c * h * w), ("layer", "fc")]
        else:
            self.layers["head"] = ("conv", c, 10, 1, 1, 0)
            self.spec.append(("layer", "head"))
            if kind == "head_up":
                if max(h, w) * 2 > MAX_HW:
                    self.spec.insert(-1, ("pool", 2, 2))
                self.spec.append(("upsample", 2, "bilinear"))

    def run(self):
        blocks, tail = plan(self.index) if self.index is not None else ([(None, None, False)] * int(self.rng.integers(2, 6)), None)
        self.set(self.conv(self.spec, self.shape(), groups=1))   # (3 input channels: a stem first)
        self.maybe_relu(self.spec, 3, 4)
        for kind, opt, relu in blocks:
            if self.old and self.chance(1, 3):
                self.reuse()
                self.maybe_relu(self.spec)
            tag, before = self.name("t"), self.shape()
            self.spec.append(("save", tag))
            self.opt, self.relu = opt, relu
            if kind is None or getattr(self, "b_" + kind)() is False:
                self.opt = None
                while getattr(self, "b_" + self.pick(BLOCKS))() is False:
                    pass
            self.old.append((tag, before))
            if relu:
                self.spec.append(("relu",))   # (a relu directly behind every kind of block, whatever the draw)
            else:
                self.maybe_relu(self.spec, 2, 3)
            assert self.c <= MAX_C and MIN_HW <= min(self.h, self.w) and max(self.h, self.w) <= MAX_HW, self.shape()
        self.tail(tail)
        return self.layers, self.spec, self.input, self.folds


def plan(index):
    """([(block kind, option, relu behind it?)], tail kind) of case `index`: 2 + index % 4 blocks, which take the entries of PLAN
    in the order of one shuffle per pass (seeded by SEED and the pass), case after case; a relu stands behind the blocks of
    two passes in three; the tails come in turn.  So any 32 consecutive cases go through PLAN three times and through TAILS six
    times, whatever the seed, and what is left to the draw is the options PLAN does not name, the order, and the sizes."""
    first = 14 * (index // 4) + (0, 2, 5, 9)[index % 4]
    out = []
    for slot in range(first, first + 2 + index % 4):
        p, at = divmod(slot, len(PLAN))
        kind, opt = PLAN[int(np.random.default_rng([SEED, p]).permutation(len(PLAN))[at])]
        out.append((kind, opt, p % 3 != 2))
    return out, TAILS[index % len(TAILS)]


def random_network(rng, index=None):
    """(layers, spec, (c, h, w), folds) of one random network.  index: the case's place in a sweep; its block kinds, the options a
    sweep has to meet and its tail then come from plan(index) and are not drawn"""
    return _Gen(rng, index).run()


def case(index):
    """default case `index`: {"entry", "folds", "batch", "per_channel", "weight_seed", "calib_seed", "input_seed"}"""
    rng = np.random.default_rng(SEED + index)
    layers, spec, shape, folds = random_network(rng, index)
    batches = batches_of((layers, spec, shape))
    return {"entry": (layers, spec, shape), "folds": folds, "batch": int(batches[int(rng.integers(0, len(batches)))]),
            "per_channel": bool(index & 1), "weight_seed": SEED + 100_000 + index, "calib_seed": SEED + 200_000 + index,
            "input_seed": SEED + 300_000 + index}


def batches_of(entry):
    """BATCHES, restricted where the network needs rows: a vector-shaped output (a squeeze-and-excitation gate, what follows a
    global average pool) of fewer than 64 values per batch cannot be expected to hold MIN_DISTINCT byte values, and at most
    one traced output in twenty may be that small.  Where no batch does it, the largest."""
    sizes = [int(np.prod(shape)) for _, shape, _ in shapes(entry)]
    ok = [b for b in BATCHES if sum(b * n < 64 for n in sizes) * 20 <= len(sizes)]
    return ok or BATCHES[-1:]


def calib_images(entry):
    """images of the calibration batch: CALIB_IMAGES, or as many as give every calibrated op 1000 output values.  The
    calibrator is the reference's: 1000 slots that start at zero and are sorted as a whole, so an op that has produced fewer
    values is calibrated on its values and the zeros left over -- a hardsigmoid gate [n, 16] of 8 images gets the range
    [0, 0] and the scale 1.0.  (workloads.calibrated's own batch is 100 images for the same reason.)"""
    calibrated = ("layer", "act", "add", "mul", "concat", "matmul", "attention")
    least = min(int(np.prod(shape)) for op, shape, _ in shapes(entry) if op[0] in calibrated)
    return max(CALIB_IMAGES, -(-1000 // least))


def padpool_case():
    """the hand-written case: groupnorm_tiny with its max-pool padded and a padded count_include_pad=False average pool ahead
    of the head"""
    layers, spec, shape = wl.network("groupnorm_tiny")
    spec = list(spec)
    spec[spec.index(("pool", 2, 2))] = ("pool", 3, 2, 1)
    spec.insert(spec.index(("gap",)), ("avgpool", 3, 2, 1, True, False))
    return {"entry": (layers, spec, shape), "folds": wl.FOLDS["groupnorm_tiny"], "batch": 3, "per_channel": False,
            "weight_seed": SEED - 1, "calib_seed": SEED - 2, "input_seed": SEED - 3}


# ---- the independent shape walk -----------------------------------------------------------------------------------------------
def shapes(entry):
    """every op's output shape (per image), walked without the generator's bookkeeping; asserts that each op is legal on
    what it reads.  Returns [(op, shape, info)] in execution order, the ops of the branches included; info: "gate" / "elementwise" of a
    mul, the inner dimension of a matmul, else None."""
    layers, spec, shape = entry
    out = []

    def run(ops, cur, saved):
        for op in ops:
            name = op[0]
            if name == "save":
                saved[op[1]] = cur
                continue
            if name == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
                continue
            if name == "load":
                cur = saved[op[1]]
                continue
            info = None
            if name == "layer":
                L = layers[op[1]]
                if L[0] == "conv":
                    g, d = wl.conv_groups(L), wl.conv_dilation(L)
                    assert len(cur) == 3 and cur[0] == L[1] and L[1] % g == 0 and L[2] % g == 0, (op, L, cur)
                    assert d * (L[3] - 1) + 1 <= min(cur[1:]) + 2 * L[5], (op, L, cur)
                    cur = (L[2], conv_out(cur[1], L[3], L[4], L[5], d), conv_out(cur[2], L[3], L[4], L[5], d))
                elif L[0] == "deconv":
                    assert len(cur) == 3 and cur[0] == L[1] and L[3:] in DECONVS, (op, L, cur)
                    cur = (L[2],) + tuple((x - 1) * L[4] - 2 * L[5] + L[3] + L[6] for x in cur[1:])
                elif L[0] == "fc":
                    assert cur == (L[1],), (op, L, cur)
                    cur = (L[2],)
                else:
                    assert L[-1] == cur[0] and (L[0] == "ln" or cur[0] % L[1] == 0), (op, L, cur)
            elif name in ("pool", "avgpool"):
                k, s, p, ceil = (op[1:5] + (0, False))[:4]
                assert len(cur) == 3 and ppr.legal(cur[1], k, s, p) and ppr.legal(cur[2], k, s, p), (op, cur)
                cur = (cur[0], ppr.out_size(cur[1], k, s, p, ceil), ppr.out_size(cur[2], k, s, p, ceil))
            elif name == "gap":
                cur = (cur[0], 1, 1)
            elif name == "upsample":
                fh, fw = wl.upsample_factors(op[1])
                assert 1 <= min(fh, fw) and max(fh, fw) <= 8 and op[2] in ("nearest", "bilinear"), op
                cur = (cur[0], cur[1] * fh, cur[2] * fw)
            elif name == "add":
                assert saved[op[2]] == cur, (op, cur, saved[op[2]])
            elif name == "mul":
                assert saved[op[2]] in (cur, cur[:1]), (op, cur, saved[op[2]])
                info = "elementwise" if saved[op[2]] == cur else "gate"
            elif name == "concat":
                others = [saved[t] for t in op[2]]
                assert all(o[1:] == cur[1:] for o in others), (op, cur, others)
                cur = (cur[0] + sum(o[0] for o in others),) + cur[1:]
            elif name == "flatten":
                assert int(np.prod(cur)) == op[1], (op, cur)
                cur = (op[1],)
            elif name == "matmul":
                a, b = (cur[0], int(np.prod(cur[1:]))), (saved[op[2]][0], int(np.prod(saved[op[2]][1:])))
                a, b = a[::-1] if op[3] else a, b[::-1] if op[4] else b
                assert a[1] == b[0], (op, a, b)
                info = a[1]
                cur = (a[0],) + tuple(cur[1:]) if not op[3] and len(cur) == 3 and b[1] == cur[1] * cur[2] else (a[0], b[1])
            elif name == "attention":
                if len(op) == 3:
                    assert cur[0] % (3 * op[2]) == 0, (op, cur)
                    cur = (cur[0] // 3,) + cur[1:]
                else:
                    assert cur[0] % op[2] == 0 and saved[op[3]] == saved[op[4]] and saved[op[3]][0] == cur[0], (op, cur)
            else:
                assert name in ("relu", "act", "softmax"), op
            assert max(cur) <= 3 * MAX_C or len(cur) < 3, (op, cur)
            assert len(cur) < 3 or max(cur[1:]) <= MAX_HW, (op, cur)
            out.append((op, cur, info))
        return cur

    run(spec, tuple(shape), {})
    return out


# ---- coverage -------------------------------------------------------------------------------------------------------------
def features(entry):
    """the block kinds and options the spec holds, as a set of names, read from the layers and ops alone"""
    layers, spec, _ = entry
    f = set()
    walked = shapes(entry)
    for L in layers.values():
        if L[0] == "conv":
            g, d = wl.conv_groups(L), wl.conv_dilation(L)
            f |= {"conv k%d" % L[3], "conv stride %d" % L[4]}
            f |= {"conv grouped"} if 1 < g < L[1] else set()
            f |= {"conv groups == channels"} if g == L[1] and g > 1 else set()
            f |= {"conv dilation > 1"} if d > 1 else set()
        elif L[0] == "deconv":
            f |= {"deconv", "deconv %d/%d/%d/%d" % L[3:]}
        elif L[0] == "ln":
            f.add("layernorm")
        elif L[0] == "gn":
            f |= {"groupnorm"} | ({"groupnorm G == 1"} if L[1] == 1 else set()) | ({"groupnorm G == c"} if L[1] == L[2] else set())
    for op in wl._walk(spec):
        name = op[0]
        if name == "pool":
            f.add("max pool padded" if len(op) > 3 and op[3] > 0 else "max pool")
            f |= {"pool ceil_mode"} if len(op) > 4 and op[4] else set()
        elif name == "avgpool":
            f.add("avg pool padded" if len(op) > 3 and op[3] > 0 else "avg pool")
            f |= {"pool ceil_mode"} if len(op) > 4 and op[4] else set()
            f |= {"avg pool count_include_pad=False"} if len(op) > 5 and not op[5] else set()
        elif name == "act":
            f.add("act " + op[2])
        elif name == "upsample":
            f |= {"upsample " + op[2], "upsample pair" if isinstance(op[1], tuple) else "upsample int"}
        elif name == "attention":
            f.add("attention packed" if len(op) == 3 else "attention three tensors")
        elif name in ("add", "concat", "gap", "softmax", "relu", "flatten"):
            f.add(name)
    for op, shape, info in walked:
        if op[0] == "mul":
            f.add("mul " + info)
        elif op[0] == "matmul":
            f.add("matmul k < 16" if info < 16 else "matmul k >= 16")
        elif op[0] == "attention":
            f.add("attention d %% 16 %s 0" % ("==" if (shape[0] // op[2]) % 16 == 0 else "!="))
    f |= _relu_behind(layers, spec)
    # what the tags and the end of the spec say (tag prefixes are the generator's: res, cb, ip, t)
    top = [op for op in spec]
    branched = {op[1] for op in top if op[0] == "branch"}
    for i, op in enumerate(top):
        if op[0] == "save" and op[1].startswith("res"):
            f.add("residual projection" if op[1] in branched else "residual identity")
        elif op[0] == "save" and op[1].startswith("cb") and op[1] not in branched:
            f.add("concat branch nothing")
        elif op[0] == "save" and op[1].startswith("ip"):
            f.add("image pool")
        elif op[0] == "concat":
            f.add("concat %d branches" % (len(op[2]) + 1))
        elif op[0] == "branch" and op[1].startswith("cb"):
            f.add("concat branch pool" if op[2][0][0] in ("pool", "avgpool") else "concat branch conv")
        elif op[0] == "branch" and op[1].startswith("t") and op[1][1:].isdigit():
            f.add("reuse " + top[i + 1][0] + (" gate" if op[2][0] == ("gap",) else ""))
    ends = [op[0] if op[0] != "layer" else layers[op[1]][0] for op in top[-4:]]
    f.add("tail " + ("gap" if ends[-3:] == ["gap", "flatten", "fc"] else "flatten fc relu fc" if ends == ["flatten", "fc", "relu", "fc"]
                     else "flatten fc" if ends[-2:] == ["flatten", "fc"] else "head upsample" if ends[-2:] == ["conv", "upsample"]
                     else "head"))
    return f


def _relu_behind(layers, ops):
    """{"relu behind X"} of every relu that stands directly behind an op X in its own op list: what a save, a branch or a load
    separates did not run back to back on one tensor"""
    out, behind = set(), None
    for op in ops:
        if op[0] == "branch":
            out |= _relu_behind(layers, op[2])
        if op[0] == "relu" and behind is not None:
            out.add("relu behind " + behind)
        behind = None if op[0] in ("save", "branch", "load") else layers[op[1]][0] if op[0] == "layer" else op[0]
    return out


REQUIRED = frozenset(
    ["max pool", "avg pool", "max pool padded", "avg pool padded", "pool ceil_mode", "avg pool count_include_pad=False",
     "upsample nearest", "upsample bilinear", "upsample int", "upsample pair", "matmul k < 16", "matmul k >= 16",
     "attention packed", "attention three tensors", "attention d % 16 == 0", "attention d % 16 != 0", "groupnorm G == 1",
     "groupnorm G == c", "layernorm", "conv grouped", "conv groups == channels", "conv dilation > 1", "deconv", "mul gate",
     "mul elementwise", "add", "concat", "gap", "softmax", "conv k1", "conv k3", "conv k5", "conv k7", "conv stride 2"]
    + ["deconv %d/%d/%d/%d" % d for d in DECONVS] + ["act " + k for k in acr.KINDS]
    + ["relu behind " + k for k in ("conv", "deconv", "pool", "avgpool", "upsample", "add", "mul", "concat", "act", "ln", "gn", "fc",
                                    "attention")]
    + ["tail " + k for k in ("gap", "flatten fc", "flatten fc relu fc", "head", "head upsample")]
    + ["residual identity", "residual projection", "concat 2 branches", "concat 3 branches", "concat branch conv",
       "concat branch pool", "concat branch nothing", "image pool", "reuse add", "reuse mul", "reuse concat", "reuse mul gate"])


# ---- the expected bytes discriminate ----------------------------------------------------------------------------------------
MIN_DISTINCT, MIN_DISTINCT_SHARE, MAX_SATURATED = 16, 0.9, 0.5


def collect(into):
    """a spec_ref trace callback: into gets (op, output bytes) of every traced op, in order"""
    def trace(op, out, operands):
        into.append((op, np.asarray(out[0])))

    return trace


def discrimination(traced):
    """(share of the traced op outputs with at least MIN_DISTINCT distinct byte values, share of all traced bytes that are 0 or
    255) of a collect() list"""
    rich = sum(len(np.unique(q)) >= MIN_DISTINCT for _, q in traced)
    saturated = sum(int(((q == 0) | (q == 255)).sum()) for _, q in traced)
    return rich / len(traced), saturated / sum(q.size for _, q in traced)


def assert_discriminates(traced, logits, ctx=""):
    rich, saturated = discrimination(traced)
    assert len(np.unique(logits)) > 1, "constant logits\n" + ctx
    assert rich >= MIN_DISTINCT_SHARE, "%.3f of the traced outputs hold >= %d byte values\n%s" % (rich, MIN_DISTINCT, ctx)
    assert saturated < MAX_SATURATED, "%.3f of the traced bytes are 0 or 255\n%s" % (saturated, ctx)
    return rich, saturated


# ---- failure messages -------------------------------------------------------------------------------------------------------
def describe(entry):
    """one line per op: the op, the layer tuple it names, and the shape behind it"""
    layers = entry[0]
    lines = ["input %s" % (tuple(entry[2]),)]
    for op, shape, _ in shapes(entry):
        lines.append("%-60s %-48s -> %s" % (op, layers[op[1]] if op[0] == "layer" else "", shape))
    return "\n".join(lines)


def _traced_ops(ops):
    """how many entries spec_ref.forward traces for `ops`: one per op that produces bytes, those of the branches included"""
    return sum(_traced_ops(op[2]) if op[0] == "branch" else op[0] not in ("save", "load") for op in ops)


def top_level(spec, trace):
    """the entries of a collect() list of spec_ref.forward that belong to the top-level ops of `spec`, picked by position: a
    ("branch", ...) op is followed by the entries of its own ops, which are passed over.  (Not by the ops' identity: equal
    tuples of a spec, such as ("relu",), may be one object.)"""
    out, pos = [], 0
    for op in spec:
        if op[0] == "branch":
            pos += _traced_ops(op[2])
        elif op[0] not in ("save", "load"):
            assert trace[pos][0] == op, (pos, trace[pos][0], op)
            out.append(trace[pos])
            pos += 1
    assert pos == len(trace), (pos, len(trace))
    return out


def first_divergence(i8ie, net, name, x, trace, traced=None):
    """`trace`: the collect() list of spec_ref.forward on x.  Walks the product op by op (traced: net_cases.traced, the
    top-level ops) and returns a line naming the first one whose bytes differ from the reference's, or None"""
    if traced is None:
        import net_cases as nc

        traced = nc.traced
    want = top_level(wl.network(name)[1], trace)
    mine = []
    traced(i8ie, net, name, x, collect(mine))
    assert len(mine) == len(want), (len(mine), len(want))
    for i, ((op, got), (wop, exp)) in enumerate(zip(mine, want)):
        assert op == wop, (i, op, wop)
        if got.shape != exp.shape:
            return "top-level op %d %r: shape %s, expected %s" % (i, op, got.shape, exp.shape)
        if not np.array_equal(got, exp):
            bad = np.argwhere(got != exp)
            return "top-level op %d %r: %d of %d bytes differ, first at %s: %d, expected %d" % (
                i, op, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])
    return None
