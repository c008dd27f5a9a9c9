"""Module base class (reference i8ie/module.py:6-35)."""
import _CXX_i8ie as _C

from .layer import Attention, BatchNorm2d, Layer, Linear, Norm, PositionEmbedding, Weightless, fold_batchnorm, is_pointwise, is_spatial
from .tensor import Tensor

# Hard-coded input quantisation of the reference (i8ie/module.py:20).
INPUT_SCALE = 0.025
INPUT_ZERO_POINT = 127


class Module:
    """Subclass, create layers as attributes in __init__, define forward(x)."""

    def __init__(self):
        self.is_quant = False

    def _layers(self):
        return [(k, v) for k, v in self.__dict__.items() if isinstance(v, Layer)]

    def load(self, state_dict):
        """Load a torch-style state dict with keys '<attr>.weight' / '<attr>.bias' (reference :10-16); a BatchNorm2d also takes
        '<attr>.running_mean' / '<attr>.running_var', an Attention with a bias '<attr>.relative_position_bias_table' (additive).  Every other key ('<attr>.num_batches_tracked') is ignored."""
        for key in state_dict:
            name, attr = key.split(".")
            if attr == "weight":
                self.__dict__[name].load_weight(state_dict[key])
            elif attr == "bias":
                self.__dict__[name].load_bias(state_dict[key])
            elif attr == "running_mean":
                self.__dict__[name].load_running_mean(state_dict[key])
            elif attr == "running_var":
                self.__dict__[name].load_running_var(state_dict[key])
            elif attr == "relative_position_bias_table":
                self.__dict__[name].load_relative_position_bias(state_dict[key])

    def fold_batchnorm(self, pairs):
        """i8ie.fold_batchnorm(layer, bn) for every (layer attribute, BatchNorm2d attribute) pair of names, in FP32 and before
        prepare(): `net.fold_batchnorm([("conv1", "bn1"), ("conv2", "bn2")])`."""
        for layer_name, bn_name in pairs:
            fold_batchnorm(self.__dict__[layer_name], self.__dict__[bn_name])

    def __call__(self, x):
        if self.is_quant:
            x = Tensor(_C.quantize(x.data, INPUT_SCALE, INPUT_ZERO_POINT))
        x = self.forward(x)
        if self.is_quant:
            x = Tensor(_C.dequantize(x.data))
        return x

    def prepare(self):
        for _, layer in self._layers():
            layer.prepare()

    def convert(self, per_channel=False, weight_bits=8, sparsity=None, group_size=None, pointwise=False, spatial=False, conv_sparsity=None):
        """per_channel=True: every layer with one weight scale per output feature (Layer.convert).  weight_bits=4: every
        Linear converts to 4-bit weights, every other layer as with 8 under the given per_channel; any value but 4 or 8 is a
        ValueError.  pointwise=True (with weight_bits=4 and neither sparsity nor group_size; anything else is a ValueError):
        every pointwise Conv2d -- kernel 1 x 1, stride 1, padding 0, groups 1 -- converts to 4-bit weights as well.  sparsity="2:4": every Linear converts to 2:4 structured-sparse 8-bit weights, every other layer as
        before; any value but None or "2:4", or weight_bits=4 with it, is a ValueError.  group_size=64, 128 or 256 (with
        weight_bits=4 and no sparsity; anything else is a ValueError): every Linear gets group-wise 4-bit scales along
        in_features (Layer.convert), every other layer converts as before.  spatial=True (with weight_bits=4 and neither
        sparsity nor group_size; anything else is a ValueError): every pointwise Conv2d and every Conv2d with groups 1, equal
        geometry pairs and in_channels % 32 == 0 converts to 4-bit weights as well (Layer.convert(spatial=True)); the stem,
        grouped, rectangular and transposed layers convert as with 8 bits.  conv_sparsity="2:4" (any other value but None, or
        pointwise=True or spatial=True with it, is a ValueError: both claim the same layers): every pointwise Conv2d with
        in_channels % 32 == 0 converts to 2:4 structured-sparse 8-bit weights (Layer.convert(conv_sparsity="2:4")), every other
        layer exactly as the remaining arguments say -- sparsity="2:4", conv_sparsity="2:4" sparsifies a whole transformer."""
        if weight_bits not in (4, 8) or isinstance(weight_bits, bool):
            raise ValueError("convert: weight_bits must be 4 or 8, got %r" % (weight_bits,))
        if sparsity is not None and (not isinstance(sparsity, str) or sparsity != "2:4" or weight_bits == 4):
            raise ValueError("convert: sparsity must be None or \"2:4\" (with weight_bits=8), got %r" % (sparsity,))
        if group_size is not None and (isinstance(group_size, bool) or group_size not in (64, 128, 256) or weight_bits != 4):
            raise ValueError("convert: group_size must be None or 64, 128, 256 (with weight_bits=4), got %r" % (group_size,))
        if pointwise and (weight_bits != 4 or sparsity is not None or group_size is not None):
            raise ValueError("convert: pointwise=True needs weight_bits=4 and neither sparsity nor group_size")
        if spatial and (weight_bits != 4 or sparsity is not None or group_size is not None):
            raise ValueError("convert: spatial=True needs weight_bits=4 and neither sparsity nor group_size")
        if conv_sparsity is not None and (not isinstance(conv_sparsity, str) or conv_sparsity != "2:4" or pointwise or spatial):
            raise ValueError("convert: conv_sparsity must be None or \"2:4\" (without pointwise and spatial), got %r" % (conv_sparsity,))
        for _, layer in self._layers():
            linear = isinstance(layer, Linear)
            if conv_sparsity and is_pointwise(layer) and layer._in_channels % 32 == 0:
                layer.convert(per_channel, conv_sparsity=conv_sparsity)
                continue
            if spatial and not linear and (is_pointwise(layer) or (is_spatial(layer) and layer._in_channels % 32 == 0)):
                layer.convert(per_channel, 4, spatial=True)
                continue
            four = linear or (pointwise and is_pointwise(layer))
            layer.convert(per_channel, weight_bits if four else 8, sparsity if linear else None, group_size if linear else None)
        self.is_quant = True

    # ---- additive: save / restore the converted (INT8) model ------------------
    # The reference can only load FP32 state dicts (module.py:10-16) and loses the
    # quantised state when the process ends; these keep it as plain arrays.
    def quantized_state_dict(self):
        """{'<attr>.q_weight' int8, '<attr>.q_bias' int8, '<attr>.qparams' float64[3] =
        (weight_scale, out_scale, out_zero_point)} for every converted layer; a per-channel layer also has
        '<attr>.w_scales' float32[out] (its weight_scale entry is then 0 and unused).  An Add, a Mul, a Concat or an Activation contributes only
        '<attr>.qparams' = (0, out_scale, out_zero_point), an Attention that and '<attr>.score_qparams' float64[2] = (scale, zero_point)
        (and its float32 '<attr>.relative_position_bias_table' where it has one);
        a LayerNorm or a GroupNorm '<attr>.qparams' and '<attr>.weight', '<attr>.bias' as float32 (a PositionEmbedding the same,
        '<attr>.bias' with class_token only); a BatchNorm2d those and
        '<attr>.running_mean', '<attr>.running_var', or no key at all once it is folded into its neighbour."""
        import numpy as np

        out = {}
        for name, layer in self._layers():
            L = layer.layer
            if isinstance(layer, BatchNorm2d) and layer.is_folded():
                continue
            if not L.is_quantized():
                raise RuntimeError("layer %r is not converted" % name)
            s_out, zp_out = L.output_qparams()
            if isinstance(layer, Attention):
                out[name + ".qparams"] = np.array([0.0, s_out, zp_out], np.float64)
                out[name + ".score_qparams"] = np.array(L.score_qparams(), np.float64)
                if layer.has_relative_position_bias:
                    out[name + ".relative_position_bias_table"] = layer.relative_position_bias()
                continue
            if isinstance(layer, Weightless):
                out[name + ".qparams"] = np.array([0.0, s_out, zp_out], np.float64)
                continue
            if isinstance(layer, Norm):
                out[name + ".weight"] = np.asarray(L.weight(), np.float32)
                if not isinstance(layer, PositionEmbedding) or layer.class_token:  # (a plain PositionEmbedding has no bias)
                    out[name + ".bias"] = np.asarray(L.bias(), np.float32)
                if isinstance(layer, BatchNorm2d):
                    out[name + ".running_mean"] = np.asarray(L.running_mean(), np.float32)
                    out[name + ".running_var"] = np.asarray(L.running_var(), np.float32)
                out[name + ".qparams"] = np.array([0.0, s_out, zp_out], np.float64)
                continue
            if layer.weight_bits() == 4:  # uint8 [out, ceil(in / 2)]: element 2i in the low nibble of byte i (i8ie_pack_w4); a conv's too
                out[name + ".q_weight4"] = L._q_weight4()
                if not isinstance(layer, Linear) and not is_pointwise(layer):  # a k x k conv: int32 [2], the kernel the rows were packed for
                    out[name + ".q_weight4_kernel"] = np.array(layer.geometry()["kernel_size"], np.int32)
                if layer.group_size() is not None:  # uint8 [out, ceil(in / group_size)] multipliers and int32 [1] (i8ie_linear_create_w4g)
                    out[name + ".q_group_scales"] = L._group_scales()
                    out[name + ".group_size"] = np.array([layer.group_size()], np.int32)
            elif layer.sparsity() == "2:4":  # int8 [out, K4 / 2] and uint8 [out, K4 / 8], one nibble per group (i8ie_pack_2_4)
                out[name + ".q_weight24"], out[name + ".q_index24"] = L._q_weight24()
            else:
                out[name + ".q_weight"] = L.q_weight()
            out[name + ".q_bias"] = L.q_bias()
            if L.is_per_channel():
                out[name + ".qparams"] = np.array([0.0, s_out, zp_out], np.float64)
                out[name + ".w_scales"] = np.asarray(L.weight_scales(), np.float32)
            else:
                out[name + ".qparams"] = np.array([L.weight_scale(), s_out, zp_out], np.float64)
        return out

    def load_quantized(self, state):
        """Inverse of quantized_state_dict(); marks the module as quantised.  A BatchNorm2d without '<attr>.qparams' in the
        state was folded in the saved model and is marked folded here."""
        import numpy as np

        for name, layer in self._layers():
            if isinstance(layer, BatchNorm2d):
                if name + ".qparams" not in state:
                    layer._folded = True
                    continue
                _, s_out, zp_out = (float(v) for v in state[name + ".qparams"])
                layer._folded = False   # (the state carries this BatchNorm: it runs, whatever this object was before)
                layer.layer.load_quantized(*(np.asarray(state[name + k], np.float32) for k in (".weight", ".bias", ".running_mean", ".running_var")),
                                           float(np.float32(s_out)), int(zp_out))
                continue
            w_scale, s_out, zp_out = (float(v) for v in state[name + ".qparams"])
            if isinstance(layer, Attention):
                s_s, zp_s = (float(v) for v in state[name + ".score_qparams"])
                layer.layer.load_quantized(float(np.float32(s_out)), int(zp_out), float(np.float32(s_s)), int(zp_s))
                if layer.has_relative_position_bias:
                    layer.load_relative_position_bias(state[name + ".relative_position_bias_table"])
                continue
            if isinstance(layer, Weightless):
                layer.layer.load_quantized(float(np.float32(s_out)), int(zp_out))
                continue
            if isinstance(layer, Norm):
                bias = state.get(name + ".bias") if isinstance(layer, PositionEmbedding) and not layer.class_token else state[name + ".bias"]
                layer.layer.load_quantized(np.asarray(state[name + ".weight"], np.float32), None if bias is None else np.asarray(bias, np.float32),
                                           float(np.float32(s_out)), int(zp_out))
                continue
            if name + ".q_weight4_kernel" in state:  # 4-bit k x k Conv2d
                kernel = tuple(int(v) for v in np.asarray(state[name + ".q_weight4_kernel"]).reshape(-1))
                if not is_spatial(layer) or kernel != tuple(layer.geometry()["kernel_size"]):
                    raise ValueError("i8ie: load_quantized: %r carries 4-bit weights packed for kernel %r (.q_weight4_kernel), which "
                                     "disagrees with the layer" % (name, kernel))
                load = layer.layer._load_quantized_w4 if is_pointwise(layer) else layer.layer._load_quantized_w4_spatial
                load(np.asarray(state[name + ".q_weight4"], np.uint8), np.asarray(state[name + ".q_bias"], np.int8),
                     np.ascontiguousarray(state[name + ".w_scales"], np.float32), float(np.float32(s_out)), int(zp_out))
                continue
            if name + ".q_weight4" in state:  # 4-bit Linear or pointwise Conv2d
                if not (isinstance(layer, Linear) or is_pointwise(layer)):
                    raise RuntimeError("i8ie: load_quantized: %r carries 4-bit weights (.q_weight4), which only a Linear or a pointwise "
                                       "Conv2d takes; the layer is a %s" % (name, type(layer).__name__))
                rest = (np.asarray(state[name + ".q_bias"], np.int8), np.ascontiguousarray(state[name + ".w_scales"], np.float32),
                        float(np.float32(s_out)), int(zp_out))
                if (name + ".q_group_scales" in state) != (name + ".group_size" in state):
                    raise ValueError("i8ie: load_quantized: %r needs both .q_group_scales and .group_size, or neither" % name)
                if name + ".group_size" in state and not isinstance(layer, Linear):
                    raise ValueError("i8ie: load_quantized: %r carries group-wise scales, which only a Linear takes" % name)
                if name + ".group_size" in state:  # ... with group-wise scales
                    layer.layer._load_quantized_w4g(np.asarray(state[name + ".q_weight4"], np.uint8), np.asarray(state[name + ".q_group_scales"], np.uint8),
                                                    int(np.asarray(state[name + ".group_size"]).reshape(-1)[0]), *rest)
                else:
                    layer.layer._load_quantized_w4(np.asarray(state[name + ".q_weight4"], np.uint8), *rest)
                continue
            if name + ".w_scales" in state:  # per-channel layer
                w_scale = np.ascontiguousarray(state[name + ".w_scales"], np.float32)
            else:
                w_scale = float(np.float32(w_scale))
            if name + ".q_weight24" in state:  # 2:4 Linear or pointwise Conv2d
                if not (isinstance(layer, Linear) or is_pointwise(layer)):
                    raise RuntimeError("i8ie: load_quantized: %r carries 2:4 weights (.q_weight24), which only a Linear or a pointwise "
                                       "Conv2d takes; the layer is a %s" % (name, type(layer).__name__))
                layer.layer._load_compressed_sp24(np.asarray(state[name + ".q_weight24"], np.int8), np.asarray(state[name + ".q_index24"], np.uint8),
                                                  np.asarray(state[name + ".q_bias"], np.int8), w_scale, float(np.float32(s_out)), int(zp_out))
                continue
            layer.layer.load_quantized(np.asarray(state[name + ".q_weight"], np.int8),
                                       np.asarray(state[name + ".q_bias"], np.int8),
                                       w_scale, float(np.float32(s_out)), int(zp_out))
        self.is_quant = True

    def save_quantized(self, path):
        """Write quantized_state_dict() as an .npz (no pickle)."""
        import numpy as np

        np.savez(path, **self.quantized_state_dict())

    def load_quantized_file(self, path):
        import numpy as np

        with np.load(path, allow_pickle=False) as f:
            self.load_quantized({k: f[k] for k in f.files})
