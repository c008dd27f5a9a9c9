"""i8ie -- the reference engine's Python surface, backed by MI355X HIP kernels.

Mirrors reference i8ie/__init__.py:1-32: `tensor`, `argmax`, `relu`,
`max_pool2d`, `quantize`, `dequantize`, `Linear`, `Conv2d`, `Tensor`, `Module`.
Every op forwards to the rebuilt extension `_CXX_i8ie`; tensors are
device-resident and `.numpy()` copies back to the host.
"""
import numbers

import _CXX_i8ie as _C

from .layer import window_pair as _window_pair
from .layer import CALIBRATION_METHODS, Activation, Add, Attention, BatchNorm2d, Concat, Conv2d, ConvTranspose2d, GroupNorm, Layer, LayerNorm, Linear, MatMul, Mul, PositionEmbedding, activation_kind, fold_batchnorm
from .layer import calibration_percentile as _percentile
from .module import Module
from .tensor import Tensor

_UPSAMPLE_MODES = {"nearest": 0, "bilinear": 1}  # I8IE_UPSAMPLE_* of include/i8ie_hip.h
_PAD_MODES = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}  # I8IE_PAD_* of include/i8ie_hip.h
FullyConnected = Linear  # BASELINE.json's name for the same class (no such symbol in the reference)

__all__ = [
    "tensor", "argmax", "relu", "max_pool2d", "quantize", "dequantize",
    "Linear", "FullyConnected", "Conv2d", "ConvTranspose2d", "Tensor", "Module", "Add", "add", "Mul", "mul", "Concat", "cat", "Activation", "activation", "lut", "avg_pool2d", "global_avg_pool2d", "upsample",
    "MatMul", "matmul", "softmax", "LayerNorm", "layer_norm", "GroupNorm", "group_norm", "BatchNorm2d", "batch_norm", "fold_batchnorm", "Attention", "attention",
    "narrow", "split", "chunk", "channel_shuffle", "pixel_shuffle", "pixel_unshuffle", "interpolate", "adaptive_avg_pool2d", "pad", "crop", "PositionEmbedding", "position_embedding",
    "synchronize", "set_device", "pinned_empty", "from_torch", "set_calibration", "calibration",
]


def _calibration_args(method, percentile):
    if method != "reservoir" and method not in CALIBRATION_METHODS:
        raise ValueError("calibration method %r (one of reservoir, %s)" % (method, ", ".join(CALIBRATION_METHODS)))
    return method, _percentile(percentile)


def tensor(ndarray):
    """Copy an ndarray (cast to float32) into a new Tensor (reference i8ie/__init__.py:13-14)."""
    return Tensor(_C.tensor(ndarray))


def argmax(x, *args, **kwargs):
    """numpy argmax on the host copy, wrapped again as a float Tensor (reference :17-18)."""
    return tensor(x.numpy().argmax(*args, **kwargs))


def relu(x):
    return Tensor(_C.relu(x.data))


def _same_as_floor_pool(x, k, s, padding, ceil_mode):
    """Is this pool geometry the unpadded floor pool's: no padding, and ceil_mode off or changing no output size?  (The ceil
    size is the floor size exactly where (in - k) % s == 0, and the dropped-window rule never applies without padding.)"""
    shape = x.shape
    return padding == 0 and (not ceil_mode or (len(shape) == 4 and 0 < k <= min(shape[2:]) and s > 0
                                              and all((d - k) % s == 0 for d in shape[2:])))


def max_pool2d(x, kernel_size, stride, padding=0, ceil_mode=False):
    """Max pooling over kernel_size x kernel_size windows (NCHW), with torch's `padding` (0 <= padding <= kernel_size // 2,
    never part of a maximum) and `ceil_mode` (include/i8ie_hip.h, i8ie_pool_output_size).  The result carries the input's
    scale and zero point.  A call whose geometry is the unpadded floor pool's (padding 0, and ceil_mode off or changing no
    output size) is the reference's max_pool2d, on every tensor type; int8 (s8) tensors take that form only."""
    k, s, p = int(kernel_size), int(stride), int(padding)
    if _same_as_floor_pool(x, k, s, p, ceil_mode):
        return Tensor(_C.max_pool2d(x.data, kernel_size, stride))
    return Tensor(_C._max_pool2d_pad(x.data, k, s, p, bool(ceil_mode)))


def quantize(x, scale, zero_point):
    return Tensor(_C.quantize(x.data, scale, zero_point))


def dequantize(x):
    return Tensor(_C.dequantize(x.data))


# ---- additive helpers (not in the reference) ---------------------------------
def add(a, b, scale=None, zero_point=None):
    """a + b of two tensors of equal shape (no broadcasting).  FP32 tensors: plain fp32 sum, `scale` / `zero_point` must
    not be given.  uint8 tensors: the quantized add of include/i8ie_hip.h (i8ie_add_u8); the result's `scale` and
    `zero_point` are required.  `i8ie.Add` is the calibrated form for use inside a Module."""
    quantized = type(a.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("add of uint8 tensors needs the result's scale and zero_point")
        return Tensor(_C.add(a.data, b.data, float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("add of FP32 tensors takes no scale / zero_point")
    return Tensor(_C.add(a.data, b.data))


def mul(a, b, scale=None, zero_point=None):
    """a * b.  `b` has `a`'s shape, or is a gate of an [n, c, h, w] `a`: [n, c, 1, 1] or [n, c], one value per image and
    channel (only the second operand broadcasts; anything else raises RuntimeError).  FP32 tensors: plain fp32 product,
    `scale` / `zero_point` must not be given.  uint8 tensors: the quantized multiply of include/i8ie_hip.h (i8ie_mul_u8);
    the result's `scale` and `zero_point` are required.  `i8ie.Mul` is the calibrated form for use inside a Module."""
    quantized = type(a.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("mul of uint8 tensors needs the result's scale and zero_point")
        return Tensor(_C.mul(a.data, b.data, float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("mul of FP32 tensors takes no scale / zero_point")
    return Tensor(_C.mul(a.data, b.data))


def matmul(a, b, scale=None, zero_point=None, transpose_a=False, transpose_b=False):
    """Batched matmul of two activation tensors.  Operands are rank 3 [b, r, c], or rank 4 [n, c, h, w] counted as
    [n, c, h * w]; `a` is [b, m, k] ([b, k, m] with transpose_a), `b` is [b, k, n] ([b, n, k] with transpose_b), the same b on
    both sides (no broadcasting; anything else raises RuntimeError).  The result is [b, m, n], or [b, m, h, w] when `a` was
    given as rank 4 [b, m, h, w], untransposed, and n == h * w.  FP32 tensors: fp32 products added in ascending k, `scale` /
    `zero_point` must not be given.  uint8 tensors: the quantized matmul of include/i8ie_hip.h (i8ie_bmm_u8); the result's
    `scale` and `zero_point` are required.  `i8ie.MatMul` is the calibrated form for use inside a Module."""
    quantized = type(a.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("matmul of uint8 tensors needs the result's scale and zero_point")
        return Tensor(_C.matmul(a.data, b.data, float(scale), int(zero_point), bool(transpose_a), bool(transpose_b)))
    if scale is not None or zero_point is not None:
        raise TypeError("matmul of FP32 tensors takes no scale / zero_point")
    return Tensor(_C.matmul(a.data, b.data, bool(transpose_a), bool(transpose_b)))


def softmax(x):
    """Softmax over the last axis.  FP32 tensors: max-subtracted expf, fp32 sum, one division per element.  uint8 tensors:
    the integer softmax of include/i8ie_hip.h (i8ie_softmax_u8), defined from one 256-entry table of the input's scale; the
    result always carries scale 1/256 and zero point 0, so there are no parameters and no layer.  The result is a plain
    tensor in reference order; an input that is not in reference order (an NHWC activation between layers) is converted
    first."""
    return Tensor(_C.softmax(x.data))


def attention(q, k=None, v=None, heads=1, score_scale=None, score_zero_point=None, scale=None, zero_point=None, window=None):
    """Multi-head scaled-dot-product attention as one op.  Operands are rank 3 [b, t, c], or rank 4 [n, c, h, w] counted as
    [n, h * w, c] (the engine's NHWC storage as it lies); `q` is [b, tq, c], `k` and `v` are [b, tk, c] (tq != tk is allowed),
    c = heads * d, head h is channels h * d .. h * d + d - 1.  `k = v = None`: `q` is a packed qkv tensor with 3 * heads * d
    channels (q, k, v are its thirds, in this order).  The result has q's rank: [b, tq, c], or [n, heads * d, h, w].  Anything
    else raises RuntimeError.  There is no alpha, mask, bias or dropout: fold the 1/sqrt(d) factor into the weights of the
    projection that makes q.  FP32 tensors: matmul, softmax, matmul per head in FP32; no quantisation parameter may be given.
    uint8 tensors: per head exactly matmul (-> `score_scale`, `score_zero_point`), softmax, matmul (-> `scale`, `zero_point`)
    of include/i8ie_hip.h, in one launch (i8ie_attention_u8); all four parameters are required.  `i8ie.Attention` is the
    calibrated form for use inside a Module.
    `window`: None, or an int / a pair (wh, ww): attend inside the non-overlapping wh x ww windows of the map (Twins' locally
    grouped attention; no shift, mask or bias).  Every operand is then rank 4 with one h x w, the window divides the map and
    holds at most 32768 pixels (RuntimeError otherwise; TypeError for a window that is no int or pair of ints), and the result
    is attention on the windows moved into the batch axis, moved back: still one launch (i8ie_attention_window_u8)."""
    if (k is None) != (v is None):
        raise TypeError("attention takes q, k and v, or one packed qkv tensor")
    win = _window_pair(window)
    kd, vd = (None, None) if k is None else (k.data, v.data)
    params = (score_scale, score_zero_point, scale, zero_point)
    if type(q.data).__name__ == "6TensorIhE":
        if any(p is None for p in params):
            raise TypeError("attention of uint8 tensors needs score_scale, score_zero_point, scale and zero_point")
        qp = (float(score_scale), int(score_zero_point), float(scale), int(zero_point))
        if win is not None:
            return Tensor(_C._attention_window(q.data, kd, vd, int(heads), win[0], win[1], *qp))
        return Tensor(_C.attention(q.data, kd, vd, int(heads), *qp))
    if any(p is not None for p in params):
        raise TypeError("attention of FP32 tensors takes no quantisation parameters")
    if win is not None:
        return Tensor(_C._attention_window(q.data, kd, vd, int(heads), win[0], win[1]))
    return Tensor(_C.attention(q.data, kd, vd, int(heads)))


def layer_norm(x, weight=None, bias=None, eps=1e-5, scale=None, zero_point=None):
    """LayerNorm of [n, c, h, w] over c per pixel, of [m, f] and [b, t, f] over the last axis (anything else raises
    RuntimeError).  `weight` / `bias`: float32 arrays of one value per normalised entry, or None for ones / zeros.  FP32
    tensors: the fp32 sequence of include/i8ie_hip.h (i8ie_layernorm_f32), `scale` / `zero_point` must not be given.  uint8
    tensors: the quantized LayerNorm (i8ie_layernorm_u8); the result's `scale` and `zero_point` are required, and gamma /
    scale, beta / scale + zero_point are computed and uploaded at every call.  `i8ie.LayerNorm` is the calibrated form for
    use inside a Module (it uploads them once, at convert())."""
    quantized = type(x.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("layer_norm of a uint8 tensor needs the result's scale and zero_point")
        return Tensor(_C.layer_norm(x.data, weight, bias, float(eps), float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("layer_norm of an FP32 tensor takes no scale / zero_point")
    return Tensor(_C.layer_norm(x.data, weight, bias, float(eps)))


def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, scale=None, zero_point=None):
    """GroupNorm of [n, c, h, w], or of [n, c] counted as h = w = 1 (anything else raises RuntimeError): per image, the
    statistics of each of the `num_groups` groups of c / num_groups channels over all pixels.  num_groups == c is InstanceNorm,
    num_groups == 1 a LayerNorm over (c, h, w).  `weight` / `bias`: float32 arrays of c values, or None for ones / zeros.  A
    group of one image holds at most 65536 values.  FP32 tensors: the fp32 sequence of include/i8ie_hip.h
    (i8ie_groupnorm_f32), `scale` / `zero_point` must not be given.  uint8 tensors: the quantized GroupNorm
    (i8ie_groupnorm_u8_nhwc); the result's `scale` and `zero_point` are required, and gamma / scale, beta / scale +
    zero_point are computed and uploaded at every call.  `i8ie.GroupNorm` is the calibrated form for use inside a Module."""
    quantized = type(x.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("group_norm of a uint8 tensor needs the result's scale and zero_point")
        return Tensor(_C._group_norm(x.data, int(num_groups), weight, bias, float(eps), float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("group_norm of an FP32 tensor takes no scale / zero_point")
    return Tensor(_C._group_norm(x.data, int(num_groups), weight, bias, float(eps)))


def batch_norm(x, running_mean, running_var, weight=None, bias=None, eps=1e-5, scale=None, zero_point=None):
    """Inference BatchNorm of [n, c, h, w] or [n, c] per channel with the given statistics (torch.nn.functional.batch_norm with
    training=False; anything else raises RuntimeError).  `running_mean` / `running_var` / `weight` / `bias`: float32 arrays of
    c values; None is zeros / ones / ones / zeros.  FP32 tensors: the fp32 sequence of include/i8ie_hip.h (i8ie_batchnorm_f32),
    `scale` / `zero_point` must not be given.  uint8 tensors: the quantized BatchNorm (i8ie_batchnorm_u8_nhwc); the result's
    `scale` and `zero_point` are required, and the per-channel affine (i8ie_batchnorm_affine) is computed and uploaded at every
    call.  `i8ie.BatchNorm2d` is the calibrated form for use inside a Module (it uploads the affine once, at convert())."""
    quantized = type(x.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("batch_norm of a uint8 tensor needs the result's scale and zero_point")
        return Tensor(_C._batch_norm(x.data, running_mean, running_var, weight, bias, float(eps), float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("batch_norm of an FP32 tensor takes no scale / zero_point")
    return Tensor(_C._batch_norm(x.data, running_mean, running_var, weight, bias, float(eps)))


def position_embedding(x, weight, class_token=None, scale=None, zero_point=None):
    """x + weight over the tokens of an [n, c, h, w] tensor, token j being pixel (j // w, j % w): `weight` is a float32 array
    [T', c] shared by every image.  class_token=None: T' = h * w, the shape is unchanged.  `class_token`, a float32 array [c]:
    T' = h * w + 1 and the result is [n, c, 1, h * w + 1], column 0 being class_token + weight[0] and column 1 + j token j plus
    weight[1 + j] (torchvision's cat + pos_embedding).  FP32 tensors: one fp32 add, `scale` / `zero_point` must not be given.
    uint8 tensors: the quantized op of include/i8ie_hip.h (i8ie_posembed_u8_nhwc); the result's `scale` and `zero_point` are
    required, and the table is made and uploaded at every call.  `i8ie.PositionEmbedding` is the calibrated form for use inside
    a Module (it uploads the table once)."""
    quantized = type(x.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("position_embedding of a uint8 tensor needs the result's scale and zero_point")
        return Tensor(_C._position_embedding(x.data, weight, class_token, float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("position_embedding of an FP32 tensor takes no scale / zero_point")
    return Tensor(_C._position_embedding(x.data, weight, class_token))


def cat(tensors, scale=None, zero_point=None):
    """Join 1 to 8 tensors [n, c_i, h, w] (or [m, f_i]) along axis 1.  FP32 tensors: a copy, `scale` / `zero_point` must not
    be given.  uint8 tensors: the quantized concat of include/i8ie_hip.h (i8ie_concat_u8); the result's `scale` and
    `zero_point` are required, an input that already has them is copied byte for byte and any other is requantised.
    `i8ie.Concat` is the calibrated form for use inside a Module."""
    tensors = list(tensors)
    quantized = bool(tensors) and type(tensors[0].data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("cat of uint8 tensors needs the result's scale and zero_point")
        return Tensor(_C.cat([t.data for t in tensors], float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("cat of FP32 tensors takes no scale / zero_point")
    return Tensor(_C.cat([t.data for t in tensors]))


def activation(x, kind, scale=None, zero_point=None, param=None):
    """f(x) for kind "relu6", "leaky_relu" (param: the slope, default 0.01), "hardsigmoid", "hardswish", "sigmoid" or "tanh".
    FP32 tensors: f in FP32, `scale` / `zero_point` must not be given.  uint8 tensors: one 256-entry table from x's
    (scale, zero_point) to the result's `scale` and `zero_point`, which are required (include/i8ie_hip.h,
    i8ie_activation_table).  `i8ie.Activation` is the calibrated form for use inside a Module."""
    code, p = activation_kind(kind, param)
    quantized = type(x.data).__name__ == "6TensorIhE"
    if quantized:
        if scale is None or zero_point is None:
            raise TypeError("activation of a uint8 tensor needs the result's scale and zero_point")
        return Tensor(_C.activation(x.data, code, p, float(scale), int(zero_point)))
    if scale is not None or zero_point is not None:
        raise TypeError("activation of an FP32 tensor takes no scale / zero_point")
    return Tensor(_C.activation(x.data, code, p))


def lut(x, table, scale, zero_point):
    """y = table[x] on a uint8 tensor: `table` is 256 uint8 entries from x's bytes to the result's, which carries `scale`
    and `zero_point` (include/i8ie_hip.h, i8ie_lut_u8)."""
    import numpy as np

    t = np.asarray(table)
    if t.dtype != np.uint8 or t.shape != (256,):
        raise TypeError("lut needs a uint8 table of 256 entries")
    if type(x.data).__name__ != "6TensorIhE":
        raise TypeError("lut needs a uint8 tensor")
    return Tensor(_C.lut(x.data, np.ascontiguousarray(t), float(scale), int(zero_point)))


def avg_pool2d(x, kernel_size, stride=None, padding=0, ceil_mode=False, count_include_pad=True):
    """Average pooling over kernel_size x kernel_size windows (NCHW, as max_pool2d); `stride` defaults to `kernel_size`.
    uint8 tensors: the integer mean rounded to nearest, ties up, (sum + n // 2) // n (include/i8ie_hip.h,
    i8ie_avgpool2d_u8); the result carries the input's scale and zero point.  FP32 tensors: the fp32 sum of the window
    divided by n.  `padding` (0 <= padding <= kernel_size // 2), `ceil_mode` and `count_include_pad` are torch's
    (include/i8ie_hip.h, i8ie_pool_output_size): a padded tap is the value zero (the byte zero_point) and counts in n
    unless count_include_pad is False; a ceil-mode overhang beyond the padding never counts."""
    k, s, p = int(kernel_size), int(kernel_size if stride is None else stride), int(padding)
    if _same_as_floor_pool(x, k, s, p, ceil_mode):
        return Tensor(_C.avg_pool2d(x.data, k, s))
    return Tensor(_C._avg_pool2d_pad(x.data, k, s, p, bool(ceil_mode), bool(count_include_pad)))


def global_avg_pool2d(x):
    """avg_pool2d over the whole image: [n, c, h, w] -> [n, c, 1, 1].  `.reshape(-1, c)` of the result feeds a Linear layer."""
    return Tensor(_C.global_avg_pool2d(x.data))


def upsample(x, scale_factor, mode="nearest"):
    """Upsampling of an [n, c, h, w] tensor by integer factors: `scale_factor` is an int or (fh, fw), each in 1..8; `mode` is
    "nearest" or "bilinear" (torch's align_corners=False).  uint8 tensors: exact integers, the blend rounded to nearest, ties
    up (include/i8ie_hip.h, i8ie_upsample2d_u8); the result carries the input's scale and zero point.  FP32 tensors: a copy
    (nearest) or the fp32 blend, rows first."""
    if isinstance(scale_factor, (tuple, list)):
        if len(scale_factor) != 2:
            raise TypeError("upsample: scale_factor is an int or a pair (fh, fw)")
        fh, fw = scale_factor
    else:
        fh = fw = scale_factor
    for f in (fh, fw):
        if isinstance(f, bool) or not isinstance(f, numbers.Integral):
            raise TypeError("upsample: scale factors must be integers (there is no fractional resizing)")
    if mode not in _UPSAMPLE_MODES:
        raise RuntimeError("upsample: mode must be 'nearest' or 'bilinear'")
    return Tensor(_C.upsample(x.data, int(fh), int(fw), _UPSAMPLE_MODES[mode]))


def _integer(op, what, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError("%s: %s must be an integer" % (op, what))
    return int(v)


def _int_pair(op, what, v, none_ok=False):
    """(a, b) of an int or a pair of ints (None allowed in a pair with none_ok); TypeError for anything else"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise TypeError("%s: %s is an int or a pair" % (op, what))
        pair = tuple(v)
    else:
        pair = (v, v)
    return tuple(None if (none_ok and p is None) else _integer(op, what, p) for p in pair)


def _nchw_dims(op, x):
    """(h, w) of a uint8 or FP32 [n, c, h, w] tensor; RuntimeError for int8 (s8) tensors and any other rank"""
    if type(x.data).__name__ not in ("6TensorIhE", "6TensorIfE"):
        raise RuntimeError("%s: int8 (s8) tensors are not supported (uint8 and FP32 tensors are)" % op)
    shape = x.shape
    if len(shape) != 4:
        raise RuntimeError("%s expects an NCHW tensor" % op)
    return int(shape[2]), int(shape[3])


def interpolate(x, size=None, scale_factor=None, mode="nearest", align_corners=None):
    """torch.nn.functional.interpolate of an [n, c, h, w] tensor to any size, up or down.  Exactly one of `size` (an int or
    (oh, ow)) and `scale_factor` (an int or a pair of ints, meaning size = (h f, w f); pass `size` for anything fractional).
    `mode` is "nearest" or "bilinear"; `align_corners` (None / False / True) belongs to "bilinear" alone.  uint8 tensors: exact
    integers -- per axis the taps and weights of include/i8ie_hip.h (i8ie_resize2d_u8), the blend rounded to nearest, ties up;
    the result carries the input's scale and zero point.  Nearest takes in[(o * L) // O] per axis, which differs from torch's
    float rule at a few indices where o * L is a multiple of O.  FP32 tensors: a copy (nearest) or the fp32 blend, rows first.
    An output that is an integer multiple 1..8 of the input on both axes, align_corners not True, is `upsample` (same bytes by
    definition, and the same launch)."""
    if (size is None) == (scale_factor is None):
        raise ValueError("interpolate: exactly one of size and scale_factor")
    if mode not in _UPSAMPLE_MODES:
        raise RuntimeError("interpolate: mode must be 'nearest' or 'bilinear'")
    if align_corners is not None and not isinstance(align_corners, bool):
        raise TypeError("interpolate: align_corners is None, False or True")
    if align_corners is not None and mode == "nearest":
        raise ValueError("interpolate: align_corners goes with mode 'bilinear' only")
    if size is not None:
        oh, ow = _int_pair("interpolate", "size", size)
    else:
        try:
            fh, fw = _int_pair("interpolate", "scale_factor", scale_factor)
        except TypeError:
            raise TypeError("interpolate: scale_factor must be an int or a pair of ints; pass size= for any other ratio") from None
    h, w = _nchw_dims("interpolate", x)
    if size is None:
        oh, ow = h * fh, w * fw
    if h > 0 and w > 0 and oh % h == 0 and ow % w == 0 and 1 <= oh // h <= 8 and 1 <= ow // w <= 8 and not align_corners:
        return Tensor(_C.upsample(x.data, oh // h, ow // w, _UPSAMPLE_MODES[mode]))
    code = 0 if mode == "nearest" else (2 if align_corners else 1)  # I8IE_RESIZE_* of include/i8ie_hip.h
    return Tensor(_C._interpolate(x.data, oh, ow, code))


def adaptive_avg_pool2d(x, output_size):
    """torch's adaptive_avg_pool2d of an [n, c, h, w] tensor: `output_size` is an int or (oh, ow), None in a pair keeps that
    dim; output i of an axis averages inputs floor(i L / O) .. ceil((i + 1) L / O) - 1.  uint8 tensors: the integer mean of
    each window rounded to nearest, ties up, (sum + n // 2) // n with the window's own n (include/i8ie_hip.h,
    i8ie_adaptive_avgpool2d_u8); the result carries the input's scale and zero point.  FP32 tensors: the fp32 sum of the window
    divided by n.  (1, 1) is `global_avg_pool2d`, and where the windows are uniform squares it is `avg_pool2d` (same bytes by
    definition, and the same launch)."""
    oh, ow = _int_pair("adaptive_avg_pool2d", "output_size", output_size, none_ok=True)
    h, w = _nchw_dims("adaptive_avg_pool2d", x)
    oh, ow = h if oh is None else oh, w if ow is None else ow
    if oh < 1 or ow < 1:
        raise RuntimeError("adaptive_avg_pool2d: the output size must be at least 1 x 1")
    if h > 0 and w > 0:
        if oh == 1 and ow == 1:
            return Tensor(_C.global_avg_pool2d(x.data))
        if h % oh == 0 and w % ow == 0 and h // oh == w // ow:
            return Tensor(_C.avg_pool2d(x.data, h // oh, h // oh))
    return Tensor(_C._adaptive_avg_pool2d(x.data, oh, ow))


def narrow(x, start, length):
    """Channels start .. start + length - 1 of axis 1 of an [n, c, h, w] or [m, f] tensor (torch.narrow(x, 1, start, length)).
    uint8 tensors: the bytes are copied and the result carries the input's scale and zero point (include/i8ie_hip.h,
    i8ie_rearrange_u8_nhwc); FP32 tensors: bits copied; int8 (s8) tensors raise RuntimeError.  The result is recorded, not
    launched: it launches when something consumes it."""
    return Tensor(_C._narrow(x.data, _integer("narrow", "start", start), _integer("narrow", "length", length)))


def split(x, split_size_or_sections):
    """torch.split along axis 1: an int gives parts of that many channels (the last one may be smaller), a list gives parts
    of exactly those sizes and must sum to the channel count.  A list of tensors, each a `narrow` of x: a part nobody
    consumes launches nothing."""
    shape = x.shape
    if len(shape) not in (2, 4):
        raise RuntimeError("split expects [n, c, h, w] or [m, f]")
    c = int(shape[1])
    if isinstance(split_size_or_sections, (tuple, list)):
        sizes = [_integer("split", "every size", s) for s in split_size_or_sections]
        if not sizes or any(s <= 0 for s in sizes) or sum(sizes) != c:
            raise RuntimeError("split: the sizes must be positive and sum to the %d channels" % c)
    else:
        size = _integer("split", "the size", split_size_or_sections)
        if size <= 0:
            raise RuntimeError("split: the size must be positive")
        sizes = [min(size, c - at) for at in range(0, c, size)]
    parts, at = [], 0
    for s in sizes:
        parts.append(narrow(x, at, s))
        at += s
    return parts


def chunk(x, chunks):
    """torch.chunk along axis 1: parts of ceil(c / chunks) channels, the last one may be smaller (and there may be fewer
    than `chunks` parts).  A list of tensors, as `split` returns it."""
    chunks = _integer("chunk", "chunks", chunks)
    if chunks <= 0:
        raise RuntimeError("chunk: chunks must be positive")
    shape = x.shape
    if len(shape) not in (2, 4):
        raise RuntimeError("chunk expects [n, c, h, w] or [m, f]")
    return split(x, -(-int(shape[1]) // chunks))


def channel_shuffle(x, groups):
    """torch.nn.ChannelShuffle on an [n, c, h, w] tensor, c % groups == 0: x.view(n, g, c / g, h, w).transpose(1, 2), i.e.
    out[:, j * g + i] = in[:, i * (c / g) + j].  uint8 tensors: bytes moved, the input's scale and zero point; FP32 tensors:
    bits moved; int8 (s8) tensors raise RuntimeError (include/i8ie_hip.h, i8ie_rearrange_u8_nhwc)."""
    return Tensor(_C._channel_shuffle(x.data, _integer("channel_shuffle", "groups", groups)))


def pixel_shuffle(x, upscale_factor):
    """torch's pixel_shuffle: [n, c r r, h, w] -> [n, c, h r, w r], out[n, co, h r + i, w r + j] = in[n, co r r + i r + j, h, w],
    r an integer in 1..8.  uint8 tensors: bytes moved, the input's scale and zero point; FP32 tensors: bits moved; int8 (s8)
    tensors raise RuntimeError (include/i8ie_hip.h, i8ie_rearrange_u8_nhwc)."""
    return Tensor(_C._pixel_shuffle(x.data, _integer("pixel_shuffle", "upscale_factor", upscale_factor)))


def pixel_unshuffle(x, downscale_factor):
    """torch's pixel_unshuffle, the inverse of pixel_shuffle: [n, c, h, w] -> [n, c r r, h / r, w / r], r an integer in 1..8
    that divides h and w.  Tensor types as pixel_shuffle."""
    return Tensor(_C._pixel_unshuffle(x.data, _integer("pixel_unshuffle", "downscale_factor", downscale_factor)))


def pad(x, pad, mode="constant", value=0.0):
    """torch.nn.functional.pad on the last two axes of an [n, c, h, w] tensor: `pad` is (left, right, top, bottom), or
    (left, right) for the width alone, Python integers with |amount| <= 65535; `mode` is "constant", "reflect", "replicate"
    or "circular".  Per axis of length L, output index o reads input index i = o - before, and outside [0, L): the fill value;
    -i or 2 (L - 1) - i (amounts <= L - 1); the edge pixel; i mod L (amounts <= L) -- torch's rules and limits
    (include/i8ie_hip.h, "Spatial padding").  Negative amounts cut pixels off, in "constant" mode only.  `value` belongs to
    "constant" alone: FP32 tensors take the float itself, uint8 tensors the byte `quantize` gives it at the input's
    (scale, zero_point), so 0 is the byte zero_point.  uint8 tensors: bytes copied, the result carries the input's scale and
    zero point and is recorded, not launched (it launches when something consumes it); FP32 tensors: bits copied; int8 (s8)
    tensors and any other rank raise RuntimeError, and so does every violation of the rules above, before any device call.
    All-zero amounts return `x` itself."""
    if not isinstance(pad, (tuple, list)) or len(pad) not in (2, 4):
        raise TypeError("pad: pad is (left, right) or (left, right, top, bottom)")
    amounts = [_integer("pad", "every amount", a) for a in pad] + [0] * (4 - len(pad))
    if mode not in _PAD_MODES:
        raise RuntimeError("pad: mode must be 'constant', 'reflect', 'replicate' or 'circular'")
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise TypeError("pad: value must be a number")
    if mode != "constant" and value != 0:
        raise TypeError("pad: value goes with mode 'constant' only")
    _nchw_dims("pad", x)
    if not any(amounts):
        return x
    return Tensor(_C._pad(x.data, *amounts, _PAD_MODES[mode], float(value)))


def crop(x, top, left, height, width):
    """The window x[:, :, top:top + height, left:left + width] of an [n, c, h, w] tensor, integers, inside the map and at
    least 1 x 1 (anything else raises RuntimeError).  It is `pad` in "constant" mode with the negative amounts the window
    implies: the same bytes and the same launch."""
    top, left = _integer("crop", "top", top), _integer("crop", "left", left)
    height, width = _integer("crop", "height", height), _integer("crop", "width", width)
    h, w = _nchw_dims("crop", x)
    if top < 0 or left < 0 or height < 1 or width < 1 or top + height > h or left + width > w:
        raise RuntimeError("crop: the window %d x %d at (%d, %d) must be at least 1 x 1 and lie inside the %d x %d map"
                           % (height, width, top, left, h, w))
    return pad(x, (-left, left + width - w, -top, top + height - h))


def set_calibration(method="reservoir", percentile=99.99):
    """Choose the observer that `prepare()` gives every layer from now on, and how `convert()` turns it into an output (scale,
    zero_point).  "reservoir" (the default) is the reference's calibrator: 1000 slots, random overwrites, the smallest and
    largest slot.  The other three observe every value of a layer's FP32 output on the device in a 2048-bin histogram
    (include/i8ie_hip.h, "Histogram calibration") and read it as
        "minmax"      the exact minimum and maximum (also of an output of fewer than 1000 values),
        "percentile"  the range that leaves floor((1 - percentile / 100) * count) values outside on either side,
        "mse"         the fraction j / 64, j = 16..64, of the minmax range with the smallest quantisation error.
    The observer is fixed at prepare(); the method and percentile are those in force at convert(), so one calibration pass may
    be converted under any of the three.  set_output_qparams still overrides every observer.  ValueError for an unknown method
    and for a percentile outside (50, 100]."""
    method, percentile = _calibration_args(method, percentile)
    _C._set_calibration(method, percentile)


def calibration():
    """The setting of set_calibration as {"method", "percentile"}."""
    method, percentile = _C._calibration()
    return {"method": method, "percentile": percentile}


def synchronize():
    """Wait for all queued device work (ops are asynchronous on one HIP stream)."""
    _C.synchronize()


def pinned_empty(shape):
    """float32 ndarray in pinned host memory.  `tensor()` of it (or of a contiguous slice) uploads on
    the transfer stream, beside the kernels of the batch before; keep the contents unchanged until
    `Tensor.wait_upload()` returns."""
    return _C.pinned_empty([int(d) for d in shape])


def from_torch(t, synchronize=True):
    """Additive: wrap a contiguous float32 torch tensor on this GPU as a Tensor without copying (the reference's
    `tensor()` copies an ndarray).  `synchronize` waits for torch's current stream first; pass False when the
    engine was put on that stream with `_CXX_i8ie.use_stream`."""
    import torch

    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError("from_torch: need a contiguous float32 CUDA tensor")
    if synchronize:
        torch.cuda.current_stream(t.device).synchronize()
    return Tensor(_C.tensor_from_device(t.data_ptr(), [int(d) for d in t.shape], t))


def set_device(index):
    """Choose the GPU before the first op (default: $I8IE_DEVICE, else $LOCAL_RANK, else 0)."""
    _C.set_device(int(index))
