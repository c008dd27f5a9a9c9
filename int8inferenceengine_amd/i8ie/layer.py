"""Layer wrappers (reference i8ie/layer.py:5-35)."""
import numbers

import _CXX_i8ie as _C

from .tensor import Tensor


CALIBRATION_METHODS = ("minmax", "percentile", "mse")  # the range methods of a histogram observer (i8ie.set_calibration)


def calibration_percentile(percentile):
    """`percentile` as a float; ValueError unless it lies in (50, 100]"""
    p = float(percentile)
    if not 50.0 < p <= 100.0:
        raise ValueError("calibration: the percentile must lie in (50, 100], got %r" % (percentile,))
    return p


def _range_args(method, percentile):
    if method not in CALIBRATION_METHODS:
        raise ValueError("calibration_range: method %r (one of %s)" % (method, ", ".join(CALIBRATION_METHODS)))
    return method, calibration_percentile(percentile)


def _histogram(d):
    return {"exponent": int(d["exponent"]), "counts": d["counts"], "min": float(d["min"]), "max": float(d["max"]),
            "nonfinite": int(d["nonfinite"])}


class Layer:
    """Common behaviour of Linear and Conv2d; `self.layer` is the extension object."""

    layer = None

    def __call__(self, x):
        # FP32 tensor -> FP32 path; uint8 tensor -> INT8 path (after convert())
        return Tensor(self.layer(x.data))

    def load_weight(self, weight):
        self.layer.load_weight(weight)

    def load_bias(self, bias):
        self.layer.load_bias(bias)

    def prepare(self):
        """Start collecting output samples for calibration (reference src/layer.cc:28-35)."""
        self.layer.prepare()

    def convert(self, per_channel=False):
        """Quantise weights, fix the output (scale, zero_point) (reference src/layer.cc:36-54).

        per_channel=True (additive, not the reference's rule): one symmetric max-abs weight scale per output
        feature, rounded to nearest even (include/i8ie_hip.h, i8ie_quantize_weight_per_channel)."""
        self.layer.convert(bool(per_channel))

    # ---- additive (the reference cannot inject or read these) ----------------
    def set_output_qparams(self, scale, zero_point):
        """Use a given output (scale, zero_point) instead of the randomised calibrator's."""
        self.layer.set_output_qparams(float(scale), int(zero_point))

    def output_qparams(self):
        return self.layer.output_qparams()

    def calibration_histogram(self):
        """The histogram this layer's observer holds right now: {"exponent": e, "counts": np.uint64[2048], "min", "max",
        "nonfinite"} (include/i8ie_hip.h, "Histogram calibration"; min / max are +inf / -inf before the first finite value).
        RuntimeError unless the layer is preparing and prepared under a histogram method of i8ie.set_calibration."""
        return _histogram(self.layer._calib_histogram())

    def calibration_range(self, method, percentile=99.99):
        """(scale, zero_point, lo, hi) that `method` ("minmax", "percentile" or "mse") reads from the live histogram, without
        converting: one calibration pass can compare the methods.  Errors as calibration_histogram and i8ie.set_calibration."""
        return tuple(self.layer._calib_range(*_range_args(method, percentile)))

    def weight_scale(self):
        """The per-tensor weight scale (raises for a per-channel layer)."""
        return self.layer.weight_scale()

    def weight_scales(self):
        """np.float32[out]: s_w[j] of every output feature (a per-tensor layer repeats its one scale)."""
        return self.layer.weight_scales()

    def is_per_channel(self):
        return self.layer.is_per_channel()

    def groups(self):
        """Groups of a Conv2d (1 for a dense Conv2d and for Linear)."""
        return self.layer.groups() if hasattr(self.layer, "groups") else 1

    def dilation(self):
        """Dilation of a Conv2d as it was constructed: the int where both axes agree, the pair (h, w) otherwise (1 for every
        other layer)."""
        return self.layer.dilation() if hasattr(self.layer, "dilation") else 1

    def geometry(self):
        """The four geometry pairs of a Conv2d, {"kernel_size", "stride", "padding", "dilation"}: each (h, w), equal values for
        a layer constructed from ints.  None for every other layer."""
        ask = getattr(self.layer, "geometry", None) or getattr(self.layer, "_geometry", None)  # (the extension's Conv2d binds it privately)
        return None if ask is None else dict(ask())

    def forward_debug(self, x):
        """INT8 forward that also returns the INT32 pre-requant accumulators (numpy)."""
        out, acc = self.layer.forward_debug(x.data)
        return Tensor(out), acc


def _pair(value, name):
    """(h, w) of a geometry argument given as an int or as a pair of ints; anything else is a TypeError"""
    def is_int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if is_int(value):
        return (int(value), int(value))
    if isinstance(value, (tuple, list)) and len(value) == 2 and all(is_int(v) for v in value):
        return (int(value[0]), int(value[1]))
    raise TypeError("Conv2d: %s must be an int or a pair of ints (h, w), got %r" % (name, value))


class Linear(Layer):
    def __init__(self, in_channels, out_channels):
        self.layer = _C.Linear(in_channels, out_channels)


class Conv2d(Layer):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, groups=1, dilation=1):
        """groups (additive, not in the reference): output features [g*out/groups, (g+1)*out/groups) see input channels
        [g*in/groups, (g+1)*in/groups); the weight is [out, in/groups, k, k].  groups == in_channels is depthwise.
        dilation (additive as well; one integer >= 1, torch.nn.Conv2d's): tap (ky, kx) reads the input dilation * ky rows and
        dilation * kx columns from the window's origin, so the output is (h + 2 * padding - dilation * (k - 1) - 1) // stride
        + 1 high.  The weight keeps its shape; save / load are unchanged (dilation is a constructor argument like stride).
        kernel_size, stride, padding and dilation each take an int or a pair (h, w) (additive; torch.nn.Conv2d's; anything
        else is a TypeError): tap (ky, kx) of output pixel (oy, ox) reads input pixel (oy * stride_h - padding_h + ky *
        dilation_h, ox * stride_w - padding_w + kx * dilation_w), and the weight is [out, in/groups, kh, kw].  Ints and pairs of
        equal values construct exactly the layer the ints always did; geometry() gives the four pairs either way."""
        pairs = [_pair(v, n) for v, n in ((kernel_size, "kernel_size"), (stride, "stride"), (padding, "padding"), (dilation, "dilation"))]
        if all(h == w for h, w in pairs):
            self.layer = _C.Conv2d(in_channels, out_channels, pairs[0][0], pairs[1][0], pairs[2][0], groups, pairs[3][0])
        else:
            self.layer = _C._Conv2dRect(in_channels, out_channels, pairs[0], pairs[1], pairs[2], groups, pairs[3])


class ConvTranspose2d(Layer):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0):
        """Learned upsampling (additive, not in the reference): torch.nn.ConvTranspose2d with a square kernel, groups = 1 and
        dilation = 1.  The weight is torch's [in, out, k, k], the bias [out]; the output is (h - 1) * stride - 2 * padding +
        k + output_padding high.  stride >= 1, 0 <= padding <= k - 1, 0 <= output_padding < stride (RuntimeError otherwise).
        In INT8 it is the reference convolution of the zero-inserted input with the flipped kernel (include/i8ie_hip.h,
        i8ie_conv_transpose2d_create): convert(per_channel=True) gives one weight scale per OUTPUT feature."""
        self.layer = _C.ConvTranspose2d(in_channels, out_channels, kernel_size, stride, padding, output_padding)


class Norm(Layer):
    """Common behaviour of the normalisation layers (LayerNorm, GroupNorm): fp32 `weight` / `bias`, a calibrated output (scale,
    zero_point) and no INT8 weights.  Module.load() takes `<attr>.weight` / `<attr>.bias`; quantized_state_dict() keeps both as
    float32 beside `<attr>.qparams`.  weight_scale, weight_scales, q_weight, q_bias and forward_debug raise RuntimeError."""

    def convert(self, per_channel=False):
        """per_channel is accepted and ignored: there are no INT8 weights."""
        self.layer.convert()

    def is_per_channel(self):
        return False

    def _no_int8_weights(self, *args, **kwargs):
        raise RuntimeError("i8ie: %s has no INT8 weights (weight and bias stay float32)" % type(self).__name__)

    weight_scale = weight_scales = q_weight = q_bias = forward_debug = _no_int8_weights


class LayerNorm(Norm):
    """Quantized LayerNorm `y = self.norm1(x)` (additive, not in the reference): a layer with fp32 `weight` (gamma, default
    ones) and `bias` (beta, default zeros) of `channels` values each, and no INT8 weights.

    [n, c, h, w] is normalised over c per pixel (torch's channels-first "LayerNorm2d" of a ConvNeXt), c == channels; [m, f]
    and [b, t, f] over the last axis, f == channels; any other shape raises RuntimeError.  1 <= channels <= 16384.  FP32
    tensors go through the fp32 sequence of include/i8ie_hip.h (i8ie_layernorm_f32; sampled by the calibrator while
    preparing, as a layer's FP32 output is); uint8 tensors, after convert(), through i8ie_layernorm_u8 with this layer's
    output (scale, zero_point).  Module.load() takes `<attr>.weight` / `<attr>.bias`; quantized_state_dict() keeps both as
    float32 beside `<attr>.qparams`.  weight_scale, weight_scales, q_weight, q_bias and forward_debug raise RuntimeError."""

    def __init__(self, channels, eps=1e-5):
        self.channels, self.eps = int(channels), float(eps)
        self.layer = _C.LayerNorm(self.channels, self.eps)


class GroupNorm(Norm):
    """Quantized GroupNorm `y = self.gn1(x)` (additive, not in the reference), with torch.nn.GroupNorm's argument order: a layer
    with fp32 `weight` (gamma, default ones) and `bias` (beta, default zeros) of `num_channels` values each, and no INT8
    weights.

    [n, c, h, w] (c == num_channels) is normalised per image over the h * w pixels and the c / num_groups channels of each
    group; [n, c] counts as h = w = 1; any other shape raises RuntimeError.  num_groups == num_channels is InstanceNorm,
    num_groups == 1 a LayerNorm over (c, h, w) of one image: there are no extra classes for them.  num_channels must be a
    multiple of num_groups, 1 <= num_channels <= 16384, and a group of one image holds at most 65536 values.  FP32 tensors go
    through the fp32 sequence of include/i8ie_hip.h (i8ie_groupnorm_f32; sampled by the calibrator while preparing); uint8
    tensors, after convert(), through i8ie_groupnorm_u8_nhwc with this layer's output (scale, zero_point)."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        self.num_groups, self.num_channels, self.eps = int(num_groups), int(num_channels), float(eps)
        self.layer = _C._GroupNorm(self.num_groups, self.num_channels, self.eps)


class BatchNorm2d(Norm):
    """Inference BatchNorm `y = self.bn1(x)` (additive, not in the reference): torch.nn.BatchNorm2d in eval mode, a layer with
    fp32 `weight` (gamma, default ones), `bias` (beta, default zeros), `running_mean` (default zeros) and `running_var`
    (default ones) of `num_features` values each, and no INT8 weights.  There is no momentum, no training mode and no
    track_running_stats: the statistics are the stored ones.

    [n, c, h, w] (c == num_features) is normalised per channel; [n, c] as well (torch's BatchNorm1d on rows); any other shape
    raises RuntimeError.  1 <= num_features <= 16384.  FP32 tensors go through the fp32 sequence of include/i8ie_hip.h
    (i8ie_batchnorm_f32; sampled by the calibrator while preparing); uint8 tensors, after convert(), through
    i8ie_batchnorm_u8_nhwc with this layer's output (scale, zero_point).  Module.load() takes `<attr>.weight`, `.bias`,
    `.running_mean` and `.running_var`; quantized_state_dict() keeps the four as float32 beside `<attr>.qparams`.

    `i8ie.fold_batchnorm(layer, bn)` folds it into the Conv2d, Linear or ConvTranspose2d in front of it.  A folded BatchNorm is
    the identity: `bn(x)` returns `x` itself (no launch, nothing sampled), prepare() and convert() do nothing,
    quantized_state_dict() writes no key for it, and loading a parameter into it raises RuntimeError (so a Module.load() of a
    state dict that holds its keys is refused after the fold: load first, then fold)."""

    def __init__(self, num_features, eps=1e-5):
        self.num_features, self.eps = int(num_features), float(eps)
        self.layer = _C._BatchNorm2d(self.num_features, self.eps)
        self._folded = False

    def __call__(self, x):
        if self._folded:
            return x
        return Tensor(self.layer(x.data))

    def is_folded(self):
        return self._folded

    def _not_folded(self, what):
        if self._folded:
            raise RuntimeError("i8ie: BatchNorm2d: %s after the fold (the parameters are inside the neighbouring layer's weights)" % what)

    def load_weight(self, weight):
        self._not_folded("load_weight")
        self.layer.load_weight(weight)

    def load_bias(self, bias):
        self._not_folded("load_bias")
        self.layer.load_bias(bias)

    def load_running_mean(self, mean):
        self._not_folded("load_running_mean")
        self.layer.load_running_mean(mean)

    def load_running_var(self, var):
        self._not_folded("load_running_var")
        self.layer.load_running_var(var)

    def running_mean(self):
        return self.layer.running_mean()

    def running_var(self):
        return self.layer.running_var()

    def prepare(self):
        if not self._folded:
            self.layer.prepare()

    def convert(self, per_channel=False):
        """per_channel is accepted and ignored: there are no INT8 weights.  A folded BatchNorm stays as it is."""
        if not self._folded:
            self.layer.convert()


class PositionEmbedding(Norm):
    """Learned position embedding with an optional class token `y = self.pos(x)` (additive, not in the reference): a layer
    with an fp32 `weight` [T', channels] (torch's pos_embedding[0], default zeros), in the class form an fp32 `bias` [channels]
    (the class token, default zeros; load_bias raises RuntimeError without class_token), and no INT8 weights.

    The input is [n, channels, height, width], counted as n sequences of T = height * width tokens: token j is pixel
    (j // width, j % width), the order in which Attention and LayerNorm count a rank-4 tensor.  class_token=False: T' = T and
    y[i, ch, j] = x[i, ch, j] + weight[j, ch], shape unchanged.  class_token=True: T' = T + 1 and the result is
    [n, channels, 1, T + 1]: column 0 is bias[ch] + weight[0, ch], column 1 + j is x[i, ch, j] + weight[1 + j, ch] -- torchvision's
    cat([class_token.expand(n, -1, -1), tokens], 1) + pos_embedding in the engine's NHWC storage.  Any other input shape raises
    RuntimeError.  FP32 tensors add in FP32 (include/i8ie_hip.h, i8ie_posembed_f32; sampled by the calibrator while preparing);
    uint8 tensors, after convert(), go through i8ie_posembed_u8_nhwc with this layer's output (scale, zero_point).
    Module.load() takes `<attr>.weight` / `<attr>.bias`; quantized_state_dict() keeps them as float32 beside `<attr>.qparams`
    (`<attr>.bias` in the class form only).  `i8ie.crop(y, 0, 0, 1, 1).reshape(-1, channels)` picks the class column for a
    Linear head."""

    def __init__(self, channels, height, width, class_token=False):
        self.channels, self.height, self.width, self.class_token = int(channels), int(height), int(width), bool(class_token)
        self.layer = _C._PositionEmbedding(self.channels, self.height, self.width, self.class_token)

    def set_output_qparams(self, scale, zero_point):
        self.layer._set_output_qparams(float(scale), int(zero_point))  # (bound under a private name: csrc/binding/ops_posembed.cc)


def fold_batchnorm(layer, bn):
    """Fold the BatchNorm2d `bn` into the Conv2d (any groups, dilation or rectangular geometry), Linear or ConvTranspose2d
    `layer` whose output it normalises, in FP32 and before prepare().  With k[o] = gamma[o] / sqrt(var[o] + eps) in double:
        W'[o, ...] = (float)((double)W[o, ...] * k[o])
        b'[o]      = (float)(((double)b[o] - (double)mean[o]) * k[o] + (double)beta[o])
    (for ConvTranspose2d the output feature is axis 1 of torch's [in, out, k, k]).  W' and b' are loaded into `layer`, and `bn`
    becomes the identity (BatchNorm2d.is_folded()).  RuntimeError if either object is preparing, is converted or `bn` is already
    folded, and if the layer's output feature count is not bn.num_features; TypeError for any other layer class.  The fold is
    one-way: load_weight / load_bias on `layer` afterwards replace the folded parameters like any others."""
    import numpy as np

    if not isinstance(bn, BatchNorm2d):
        raise TypeError("fold_batchnorm: the second argument must be a BatchNorm2d, got %s" % type(bn).__name__)
    if not isinstance(layer, (Conv2d, Linear, ConvTranspose2d)):
        raise TypeError("fold_batchnorm: the first argument must be a Conv2d, a Linear or a ConvTranspose2d, got %s" % type(layer).__name__)
    if bn.is_folded():
        raise RuntimeError("fold_batchnorm: the BatchNorm2d is already folded")
    for what, obj in (("layer", layer), ("BatchNorm2d", bn)):
        if obj.layer.is_quantized():
            raise RuntimeError("fold_batchnorm: the %s is already converted" % what)
        if obj.layer._is_preparing():
            raise RuntimeError("fold_batchnorm: the %s is preparing (fold before prepare())" % what)
    w, b = np.asarray(layer.layer._weight(), np.float32), np.asarray(layer.layer._bias(), np.float32)
    axis = 1 if isinstance(layer, ConvTranspose2d) else 0
    if w.shape[axis] != bn.num_features or b.shape != (bn.num_features,):
        raise RuntimeError("fold_batchnorm: the layer has %d output features, the BatchNorm2d %d" % (w.shape[axis], bn.num_features))
    f64 = np.float64
    k = np.asarray(bn.layer.weight(), np.float32).astype(f64) / np.sqrt(np.asarray(bn.running_var(), np.float32).astype(f64) + f64(np.float32(bn.eps)))
    shape = [1] * w.ndim
    shape[axis] = -1
    layer.load_weight((w.astype(f64) * k.reshape(shape)).astype(np.float32))
    layer.load_bias(((b.astype(f64) - np.asarray(bn.running_mean(), np.float32).astype(f64)) * k
                     + np.asarray(bn.layer.bias(), np.float32).astype(f64)).astype(np.float32))
    bn._folded = True


class Weightless(Layer):
    """Common behaviour of the layers without weights (Add, Mul, Concat, Activation): `self.layer` has only the prepare / convert state
    machine around an output (scale, zero_point).  Takes part in Module.prepare() / convert() / quantized_state_dict()
    (`<attr>.qparams` only); Module.load() ignores it.  groups() is 1 and is_per_channel() False (the neutral values);
    load_weight, load_bias, weight_scale, weight_scales and forward_debug raise RuntimeError: there are no weights."""

    def convert(self, per_channel=False):
        """per_channel is accepted and ignored."""
        self.layer.convert()

    def is_per_channel(self):
        return False

    def _no_weights(self, *args, **kwargs):
        raise RuntimeError("i8ie: %s has no weights" % type(self).__name__)

    load_weight = load_bias = weight_scale = weight_scales = forward_debug = _no_weights


class Add(Weightless):
    """Quantized residual add `y = self.add1(a, b)` (additive, not in the reference): a layer without weights.

    FP32 tensors add in FP32 (sampled by the calibrator while preparing, as a layer's FP32 output is); uint8 tensors,
    after convert(), by the arithmetic of include/i8ie_hip.h (i8ie_add_u8) with this Add's output (scale, zero_point).
    Shapes must be equal (no broadcasting)."""

    def __init__(self):
        self.layer = _C.Add()

    def __call__(self, a, b):
        return Tensor(self.layer(a.data, b.data))


class Mul(Weightless):
    """Quantized broadcast multiply `y = self.mul1(x, g)` (additive, not in the reference): a layer without weights.

    `g` has `x`'s shape, or is a gate of an [n, c, h, w] `x`: one value per image and channel, [n, c, 1, 1] or [n, c], as a
    squeeze-and-excitation block makes it.  Only the second operand broadcasts.  FP32 tensors multiply in FP32 (sampled by
    the calibrator while preparing, as a layer's FP32 output is); uint8 tensors, after convert(), by the arithmetic of
    include/i8ie_hip.h (i8ie_mul_u8) with this Mul's output (scale, zero_point)."""

    def __init__(self):
        self.layer = _C.Mul()

    def __call__(self, a, b):
        return Tensor(self.layer(a.data, b.data))


class MatMul(Weightless):
    """Quantized batched matmul of two activation tensors `y = self.mm1(a, b)` (additive, not in the reference): a layer
    without weights.

    Operands are rank 3 [b, r, c], or rank 4 [n, c, h, w] counted as [n, c, h * w].  `a` is [b, m, k] ([b, k, m] with
    transpose_a), `b` is [b, k, n] ([b, n, k] with transpose_b), the same b on both sides (no broadcasting), k <= 32768.  The
    result is [b, m, n], or [b, m, h, w] when `a` was given as rank 4 [b, m, h, w], untransposed, and n == h * w.  Anything else
    raises RuntimeError.  FP32 tensors multiply in FP32 (sampled by the calibrator while preparing, as a layer's FP32 output
    is); uint8 tensors, after convert(), by the arithmetic of include/i8ie_hip.h (i8ie_bmm_u8) with this MatMul's output
    (scale, zero_point).  There is no bias and no alpha: fold a 1/sqrt(d) factor into the projection that makes an operand."""

    def __init__(self, transpose_a=False, transpose_b=False):
        self.transpose_a, self.transpose_b = bool(transpose_a), bool(transpose_b)
        self.layer = _C.MatMul(self.transpose_a, self.transpose_b)

    def __call__(self, a, b):
        return Tensor(self.layer(a.data, b.data))


def window_pair(window):
    """None, or (wh, ww) of an attention window given as an int or a pair of ints; anything else is a TypeError"""
    if window is None:
        return None
    is_int = lambda a: isinstance(a, numbers.Integral) and not isinstance(a, bool)  # noqa: E731
    if is_int(window):
        return int(window), int(window)
    if isinstance(window, (tuple, list)) and len(window) == 2 and all(is_int(a) for a in window):
        return int(window[0]), int(window[1])
    raise TypeError("window must be None, an int or a pair of ints (wh, ww)")


class Attention(Weightless):
    """Quantized multi-head attention `y = self.attn(q, k, v)` or, packed, `y = self.attn(qkv)` (additive, not in the
    reference): a layer without weights and with two calibrated parameter sets, the scores' and the output's.

    Operands are rank 3 [b, t, c], or rank 4 [n, c, h, w] counted as [n, h * w, c]; q is [b, tq, c], k and v are [b, tk, c],
    c = heads * d.  In the packed form the tensor has 3 * heads * d channels (q, k, v are its thirds, as one 1x1 conv or Linear
    c -> 3c makes them) and all three operands share its scale and zero point.  The result has q's rank.  Anything else raises
    RuntimeError.  There is no alpha, mask, bias or dropout: the 1/sqrt(d) factor folds into the weights of the projection
    that makes q.  FP32 tensors go through matmul, softmax, matmul per head in FP32; while preparing, the calibrator samples
    the FP32 scores and the FP32 result, and convert() fixes score_qparams() and output_qparams().  uint8 tensors, after
    convert(), take one launch (include/i8ie_hip.h, i8ie_attention_u8): per head exactly i8ie_bmm_u8, i8ie_softmax_u8,
    i8ie_bmm_u8.  quantized_state_dict() writes `<attr>.qparams` and `<attr>.score_qparams` = (scale, zero_point).

    `window`: None, or an int / a pair (wh, ww): attention inside the non-overlapping wh x ww windows of rank-4 maps (see
    `i8ie.attention`), one launch as well (i8ie_attention_window_u8).  While preparing, the calibrator samples the windowed
    scores [n * windows, heads, wh * ww, wh * ww].  The window is a constructor argument and not part of the saved state."""

    def __init__(self, heads, window=None):
        self.heads = int(heads)
        self.window = window_pair(window)
        self.layer = _C.Attention(self.heads)
        if self.window is not None:
            self.layer._set_window(*self.window)

    def __call__(self, q, k=None, v=None):
        if (k is None) != (v is None):
            raise TypeError("Attention takes q, k and v, or one packed qkv tensor")
        if k is None:
            return Tensor(self.layer(q.data))
        return Tensor(self.layer(q.data, k.data, v.data))

    def score_qparams(self):
        return self.layer.score_qparams()

    def set_score_qparams(self, scale, zero_point):
        self.layer.set_score_qparams(float(scale), int(zero_point))

    def score_calibration_histogram(self):
        """calibration_histogram() of the observer of the FP32 scores."""
        return _histogram(self.layer._score_calib_histogram())

    def score_calibration_range(self, method, percentile=99.99):
        """calibration_range() of the observer of the FP32 scores."""
        return tuple(self.layer._score_calib_range(*_range_args(method, percentile)))


class Concat(Weightless):
    """Quantized channel concatenation `y = self.cat1([a, b, ...])` (additive, not in the reference): a layer without weights.

    Joins 1 to 8 tensors [n, c_i, h, w] (or [m, f_i]) along axis 1.  FP32 tensors are copied (the result is sampled by
    the calibrator while preparing); uint8 tensors, after convert(), are brought to this Concat's output (scale,
    zero_point) by the arithmetic of include/i8ie_hip.h (i8ie_concat_u8): an input already in that quantisation is
    copied byte for byte, any other is requantised."""

    def __init__(self):
        self.layer = _C.Concat()

    def __call__(self, tensors):
        return Tensor(self.layer([t.data for t in tensors]))


# the kinds of a table-driven activation (include/i8ie_hip.h, I8IE_ACT_*)
ACTIVATION_KINDS = {"relu6": 0, "leaky_relu": 1, "hardsigmoid": 2, "hardswish": 3, "sigmoid": 4, "tanh": 5}
LEAKY_RELU_DEFAULT_SLOPE = 0.01


def activation_kind(kind, param):
    """(I8IE_ACT_* code, param) of a kind given by name.  `param` is leaky_relu's slope (default 0.01) and must be None for
    every other kind."""
    if kind not in ACTIVATION_KINDS:
        raise ValueError("unknown activation %r (one of %s)" % (kind, ", ".join(sorted(ACTIVATION_KINDS))))
    if kind == "leaky_relu":
        return ACTIVATION_KINDS[kind], float(LEAKY_RELU_DEFAULT_SLOPE if param is None else param)
    if param is not None:
        raise TypeError("activation %r takes no param" % kind)
    return ACTIVATION_KINDS[kind], 0.0


class Activation(Weightless):
    """Quantized activation `y = self.act1(x)` (additive, not in the reference): a layer without weights.

    kind: "relu6", "leaky_relu" (param: the slope, default 0.01), "hardsigmoid", "hardswish", "sigmoid" or "tanh".  FP32
    tensors go through f in FP32 (sampled by the calibrator while preparing, as a layer's FP32 output is); uint8 tensors,
    after convert(), through one 256-entry table from the input tensor's (scale, zero_point) to this layer's own output
    (scale, zero_point), by the arithmetic of include/i8ie_hip.h (i8ie_activation_table)."""

    def __init__(self, kind, param=None):
        self.kind = kind
        code, self.param = activation_kind(kind, param)
        self.layer = _C.Activation(code, self.param)

    def __call__(self, x):
        return Tensor(self.layer(x.data))
