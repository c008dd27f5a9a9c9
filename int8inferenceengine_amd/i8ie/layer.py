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

    def convert(self, per_channel=False, weight_bits=8, sparsity=None, group_size=None, spatial=False, conv_sparsity=None):
        """Quantise weights, fix the output (scale, zero_point) (reference src/layer.cc:36-54).

        per_channel=True (additive, not the reference's rule): one symmetric max-abs weight scale per output
        feature, rounded to nearest even (include/i8ie_hip.h, i8ie_quantize_weight_per_channel).
        weight_bits=4 (additive; i8ie.Linear and a pointwise i8ie.Conv2d -- kernel 1 x 1, stride 1, padding 0, groups 1, any
        dilation -- only, ValueError for every other layer; any value but 4 or 8 is a ValueError): 4-bit weights with one
        scale per output feature, whatever per_channel says (include/i8ie_hip.h, i8ie_quantize_weight_w4, on the [out, in]
        view of a conv's weight).  The layer is then per-channel in every respect: is_per_channel() is True,
        weight_scales() works and weight_scale() raises.
        sparsity="2:4" (additive; i8ie.Linear with weight_bits=8 only, ValueError for every other layer class, with
        weight_bits=4, and for any value but None or "2:4"): quantise as per_channel says, then keep in every aligned group
        of four along in_features the two integers of largest magnitude, ties to the lower index, and zero the rest
        (include/i8ie_hip.h, i8ie_prune_2_4).  The scales are those of the dense layer.
        group_size=64, 128 or 256 (additive; i8ie.Linear with weight_bits=4 only, ValueError for every other layer class, for
        weight_bits=8, with sparsity, and for any other value): every group of that many weights along in_features gets an
        integer multiplier in [1, 32] of the row's scale / 32, so a group of small weights keeps its sixteen levels
        (include/i8ie_hip.h, i8ie_quantize_weight_w4g).  weight_scales() then gives the row's scale / 32.
        spatial=True (additive; with weight_bits=4 on an i8ie.Conv2d with groups 1 whose kernel, stride, padding and dilation
        are each an int or a pair of equal values; ValueError for every other layer, with weight_bits=8, sparsity or
        group_size): 4-bit weights for a k x k layer, quantised on the [out, in * k * k] view of the weight.  On a pointwise
        layer it does what the call without the keyword does.
        conv_sparsity="2:4" (additive; a pointwise i8ie.Conv2d with weight_bits=8, sparsity=None, group_size=None and
        spatial=False only, under either per_channel; ValueError for every other layer, value or combination): quantise as
        per_channel says, then prune the [out, in] view of the weight by sparsity="2:4"'s rule along in_channels."""
        if check_conv_sparsity(self, conv_sparsity, weight_bits, sparsity, group_size, spatial):
            return self.layer._convert_sp24(bool(per_channel))
        if check_spatial(self, spatial, weight_bits, sparsity, group_size):
            return self.layer._convert_w4() if is_pointwise(self) else self.layer._convert_w4_spatial()
        sparse = check_sparsity(self, sparsity, weight_bits)
        grouped = check_group_size(self, group_size, weight_bits, sparsity)
        if check_weight_bits(self, weight_bits) == 4:
            if grouped:
                self.layer._convert_w4g(grouped)
            else:
                self.layer._convert_w4()
        elif sparse:
            self.layer._convert_sp24(bool(per_channel))
        else:
            self.layer.convert(bool(per_channel))

    def sparsity(self):
        """"2:4" for a Linear or a pointwise Conv2d converted or loaded with 2:4 structured-sparse weights, None for every other layer."""
        ask = getattr(self.layer, "_sparse24", None)
        return "2:4" if ask is not None and ask() else None

    def load_quantized(self, q_weight, q_bias, weight_scale, out_scale, out_zero_point, sparsity=None, conv_sparsity=None):
        """Restore a converted layer from dense INT8 weights (what convert() would have left behind); weight_scale is a number
        or one scale per output feature.  sparsity="2:4" (i8ie.Linear only) installs them as a 2:4 layer and raises
        ValueError unless every aligned group of four along in_features holds at most two non-zeros: nothing is pruned here.
        conv_sparsity="2:4" (a pointwise i8ie.Conv2d only, and without sparsity) does the same along in_channels."""
        if check_conv_sparsity(self, conv_sparsity, 8, sparsity) or check_sparsity(self, sparsity, 8):
            self.layer._load_quantized_sp24(q_weight, q_bias, weight_scale, out_scale, out_zero_point)
        else:
            self.layer.load_quantized(q_weight, q_bias, weight_scale, out_scale, out_zero_point)

    def weight_bits(self):
        """4 for a Linear or a Conv2d converted or loaded with 4-bit weights, 8 for every other layer."""
        ask = getattr(self.layer, "_weight_bits", None)
        return 8 if ask is None else int(ask())

    def group_size(self):
        """64, 128 or 256 for a Linear converted or loaded with group-wise 4-bit scales, None for every other layer."""
        ask = getattr(self.layer, "_group_size", None)
        return (int(ask()) or None) if ask is not None else None

    def group_scales(self):
        """np.uint8[out, ceil(in / group_size)]: the integer multiplier m[j, g] of every group (RuntimeError for a layer
        without group-wise scales).  Weight (j, k) stands for m[j, k // group_size] * q_weight()[j, k] * weight_scales()[j]."""
        if self.group_size() is None:
            raise RuntimeError("i8ie: group_scales: the layer has no group-wise scales")
        return self.layer._group_scales()

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


def is_pointwise(layer):
    """an i8ie.Conv2d with kernel 1 x 1, stride 1, padding 0 and groups 1 (any dilation: at k = 1 it is the undilated layer)"""
    if not isinstance(layer, Conv2d):
        return False
    g = layer.geometry()
    return tuple(g["kernel_size"]) == (1, 1) and tuple(g["stride"]) == (1, 1) and tuple(g["padding"]) == (0, 0) and layer.groups() == 1


def is_spatial(layer):
    """an i8ie.Conv2d that takes 4-bit weights at any kernel size: groups 1, every geometry pair of equal values"""
    if not isinstance(layer, Conv2d):
        return False
    g = layer.geometry()
    return layer.groups() == 1 and all(g[k][0] == g[k][1] for k in ("kernel_size", "stride", "padding", "dilation"))


def check_spatial(layer, spatial, weight_bits=8, sparsity=None, group_size=None):
    """spatial as convert() takes it: False, or True with weight_bits=4 alone on a layer of is_spatial; ValueError otherwise"""
    if not spatial:
        return False
    if weight_bits != 4 or isinstance(weight_bits, bool) or sparsity is not None or group_size is not None:
        raise ValueError("convert: spatial=True needs weight_bits=4 and neither sparsity nor group_size")
    if not is_spatial(layer):
        raise ValueError("convert: spatial=True is for an i8ie.Conv2d with groups 1 and equal kernel, stride, padding and dilation "
                         "on both axes, not this %s" % type(layer).__name__)
    return True


def check_weight_bits(layer, weight_bits):
    """weight_bits as convert() takes it: 8, or 4 on a Linear or a pointwise Conv2d; ValueError otherwise"""
    if weight_bits not in (4, 8) or isinstance(weight_bits, bool):
        raise ValueError("convert: weight_bits must be 4 or 8, got %r" % (weight_bits,))
    if weight_bits == 4 and not (isinstance(layer, Linear) or is_pointwise(layer)):
        raise ValueError("convert: weight_bits=4 is for i8ie.Linear and a pointwise i8ie.Conv2d (kernel 1 x 1, stride 1, padding 0, "
                         "groups 1) only, not this %s" % type(layer).__name__)
    return weight_bits


def check_conv_sparsity(layer, conv_sparsity, weight_bits=8, sparsity=None, group_size=None, spatial=False):
    """conv_sparsity as convert() takes it: None, or "2:4" alone on a pointwise Conv2d with 8-bit weights; ValueError otherwise.
    True for "2:4"."""
    if conv_sparsity is None:
        return False
    if not isinstance(conv_sparsity, str) or conv_sparsity != "2:4":
        raise ValueError("convert: conv_sparsity must be None or \"2:4\", got %r" % (conv_sparsity,))
    if not is_pointwise(layer):
        raise ValueError("convert: conv_sparsity=\"2:4\" is for a pointwise i8ie.Conv2d (kernel 1 x 1, stride 1, padding 0, groups 1) "
                         "only, not this %s" % type(layer).__name__)
    if weight_bits != 8 or isinstance(weight_bits, bool) or sparsity is not None or group_size is not None or spatial:
        raise ValueError("convert: conv_sparsity=\"2:4\" needs weight_bits=8 and none of sparsity, group_size and spatial")
    return True


def check_sparsity(layer, sparsity, weight_bits=8):
    """sparsity as convert() takes it: None, or "2:4" on a Linear with 8-bit weights; ValueError otherwise.  True for "2:4"."""
    if sparsity is None:
        return False
    if not isinstance(sparsity, str) or sparsity != "2:4":
        raise ValueError("convert: sparsity must be None or \"2:4\", got %r" % (sparsity,))
    if not isinstance(layer, Linear):
        raise ValueError("convert: sparsity=\"2:4\" is for i8ie.Linear only, not %s" % type(layer).__name__)
    if weight_bits == 4:
        raise ValueError("convert: sparsity=\"2:4\" keeps 8-bit weights; it does not combine with weight_bits=4")
    return True


def check_group_size(layer, group_size, weight_bits=8, sparsity=None):
    """group_size as convert() takes it: None, or 64 / 128 / 256 on a Linear with weight_bits=4 and no sparsity; ValueError
    otherwise.  The int, or 0 for None."""
    if group_size is None:
        return 0
    if isinstance(group_size, bool) or group_size not in (64, 128, 256):
        raise ValueError("convert: group_size must be None, 64, 128 or 256, got %r" % (group_size,))
    if not isinstance(layer, Linear):
        raise ValueError("convert: group_size is for i8ie.Linear only, not %s" % type(layer).__name__)
    if weight_bits != 4 or sparsity is not None:
        raise ValueError("convert: group_size needs weight_bits=4 and no sparsity")
    return int(group_size)


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
        self._in_channels = int(in_channels)  # (Module.convert(spatial=True) asks: the MFMA kernel wants a multiple of 32)
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

    def convert(self, per_channel=False, weight_bits=8, sparsity=None, group_size=None, spatial=False, conv_sparsity=None):
        """per_channel is accepted and ignored: there are no INT8 weights."""
        check_conv_sparsity(self, conv_sparsity, weight_bits, sparsity, group_size, spatial)
        check_spatial(self, spatial, weight_bits, sparsity, group_size)
        check_weight_bits(self, weight_bits)
        check_sparsity(self, sparsity, weight_bits)
        check_group_size(self, group_size, weight_bits, sparsity)
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

    def convert(self, per_channel=False, weight_bits=8, sparsity=None, group_size=None, spatial=False, conv_sparsity=None):
        """per_channel is accepted and ignored: there are no INT8 weights.  A folded BatchNorm stays as it is."""
        check_conv_sparsity(self, conv_sparsity, weight_bits, sparsity, group_size, spatial)
        check_spatial(self, spatial, weight_bits, sparsity, group_size)
        check_weight_bits(self, weight_bits)
        check_sparsity(self, sparsity, weight_bits)
        check_group_size(self, group_size, weight_bits, sparsity)
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

    def convert(self, per_channel=False, weight_bits=8, sparsity=None, group_size=None, spatial=False, conv_sparsity=None):
        """per_channel is accepted and ignored."""
        check_conv_sparsity(self, conv_sparsity, weight_bits, sparsity, group_size, spatial)
        check_spatial(self, spatial, weight_bits, sparsity, group_size)
        check_weight_bits(self, weight_bits)
        check_sparsity(self, sparsity, weight_bits)
        check_group_size(self, group_size, weight_bits, sparsity)
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


def shift_pair(shift):
    """(sh, sw) of a window shift given as an int or a pair of ints; anything else is a TypeError"""
    try:
        pair = window_pair(shift)
    except TypeError:
        pair = None
    if pair is None:
        raise TypeError("shift must be an int or a pair of ints (sh, sw)")
    return pair


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
    scores [n * windows, heads, wh * ww, wh * ww].  The window is a constructor argument and not part of the saved state.

    `shift`: an int or a pair (sh, sw), 0 <= sh < wh and 0 <= sw < ww: the windows are cut from the map rolled by (-sh, -sw),
    with Swin's region mask, and the result is rolled back (include/i8ie_hip.h, i8ie_attention_swin_u8): still one launch,
    and no roll.  `relative_position_bias=True`: the layer owns Swin's fp32 table [(2 wh - 1)(2 ww - 1), heads], zero until
    `load_relative_position_bias(table)` (Module.load routes `<attr>.relative_position_bias_table` to it); its expansion
    B[h][i][j] is added to the scores before the softmax, in FP32 and in INT8.  quantized_state_dict() keeps the table as
    float32 `<attr>.relative_position_bias_table`.  A non-zero shift or a bias without a window is a RuntimeError; a shift
    that is no int or pair of ints a TypeError.  shift and relative_position_bias are constructor arguments like window."""

    def __init__(self, heads, window=None, shift=0, relative_position_bias=False):
        self.heads = int(heads)
        self.window = window_pair(window)
        self.shift = shift_pair(shift)
        self.has_relative_position_bias = bool(relative_position_bias)
        if self.window is None and (self.shift != (0, 0) or self.has_relative_position_bias):
            raise RuntimeError("i8ie: Attention: a shift or a relative position bias needs a window")
        self.layer = _C.Attention(self.heads)
        if self.window is not None:
            self.layer._set_window(*self.window)
        if self.shift != (0, 0):
            self.layer._set_shift(*self.shift)
        self._table = None
        if self.has_relative_position_bias:
            import numpy as np

            wh, ww = self.window
            self.load_relative_position_bias(np.zeros(((2 * wh - 1) * (2 * ww - 1), self.heads), np.float32))

    def load_relative_position_bias(self, table):
        """Swin's table, float32 [(2 wh - 1)(2 ww - 1), heads]: expanded to B[heads][T][T] and uploaded once."""
        if not self.has_relative_position_bias:
            raise RuntimeError("i8ie: Attention: built without relative_position_bias=True")
        import numpy as np

        table = np.ascontiguousarray(table, np.float32)
        self.layer._set_score_bias(table)
        self._table = table.copy()

    def relative_position_bias(self):
        """the table as loaded (zeros until then); None without relative_position_bias=True"""
        return None if self._table is None else self._table.copy()

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
