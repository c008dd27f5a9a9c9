"""Module base class (reference i8ie/module.py:6-35)."""
import _CXX_i8ie as _C

from .layer import Attention, BatchNorm2d, Layer, Norm, PositionEmbedding, Weightless, fold_batchnorm
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
        '<attr>.running_mean' / '<attr>.running_var' (additive).  Every other key ('<attr>.num_batches_tracked') is ignored."""
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

    def convert(self, per_channel=False):
        """per_channel=True: every layer with one weight scale per output feature (Layer.convert)."""
        for _, layer in self._layers():
            layer.convert(per_channel)
        self.is_quant = True

    # ---- additive: save / restore the converted (INT8) model ------------------
    # The reference can only load FP32 state dicts (module.py:10-16) and loses the
    # quantised state when the process ends; these keep it as plain arrays.
    def quantized_state_dict(self):
        """{'<attr>.q_weight' int8, '<attr>.q_bias' int8, '<attr>.qparams' float64[3] =
        (weight_scale, out_scale, out_zero_point)} for every converted layer; a per-channel layer also has
        '<attr>.w_scales' float32[out] (its weight_scale entry is then 0 and unused).  An Add, a Mul, a Concat or an Activation contributes only
        '<attr>.qparams' = (0, out_scale, out_zero_point), an Attention that and '<attr>.score_qparams' float64[2] = (scale, zero_point);
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
                continue
            if isinstance(layer, Weightless):
                layer.layer.load_quantized(float(np.float32(s_out)), int(zp_out))
                continue
            if isinstance(layer, Norm):
                bias = state.get(name + ".bias") if isinstance(layer, PositionEmbedding) and not layer.class_token else state[name + ".bias"]
                layer.layer.load_quantized(np.asarray(state[name + ".weight"], np.float32), None if bias is None else np.asarray(bias, np.float32),
                                           float(np.float32(s_out)), int(zp_out))
                continue
            if name + ".w_scales" in state:  # per-channel layer
                w_scale = np.ascontiguousarray(state[name + ".w_scales"], np.float32)
            else:
                w_scale = float(np.float32(w_scale))
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
