// ops_posembed.cc -- position embedding with an optional class token (no counterpart in the reference; arithmetic:
// include/i8ie_hip.h, i8ie_posembed_u8_nhwc): the op, the PositionEmbedding layer and bind_posembed.  Both entries are private to
// the i8ie package (tests/golden/binding_surface.json stays as it is): it exposes them as i8ie.position_embedding and
// i8ie.PositionEmbedding.
#include "layers.h"

namespace i8ie_py {

namespace {

// [n, c, h, w] -> [n, c, h, w], or [n, c, 1, h * w + 1] with a class token; anything else is a RuntimeError (before any
// device call)
template <typename T>
std::vector<ssize_t> posembed_shape(const Tensor<T>& x, ssize_t channels, ssize_t height, ssize_t width, bool cls) {
  if (x.shape.size() != 4) throw std::runtime_error("i8ie: position_embedding expects [n, c, h, w]");
  for (ssize_t d : x.shape)
    if (d <= 0 || d > 0x7FFFFFFF) throw std::runtime_error("i8ie: position_embedding: empty tensor");
  if (x.shape[1] != channels || x.shape[2] != height || x.shape[3] != width)
    throw std::runtime_error("i8ie: position_embedding: the tensor is [.., " + std::to_string(x.shape[1]) + ", " + std::to_string(x.shape[2]) +
                             ", " + std::to_string(x.shape[3]) + "], the table was made for [.., " + std::to_string(channels) + ", " +
                             std::to_string(height) + ", " + std::to_string(width) + "]");
  if (cls) return {x.shape[0], channels, 1, height * width + 1};
  return x.shape;
}
void posembed_dims(ssize_t channels, ssize_t height, ssize_t width) {
  if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: position_embedding: channels must be in 1..16384");
  if (height < 1 || width < 1 || height * width >= 0x40000000) throw std::runtime_error("i8ie: position_embedding: height and width must be positive (fewer than 2^30 tokens)");
}
// a float32 [rows, channels] parameter (None: zeros)
std::vector<float> posembed_param(const py::object& a, ssize_t rows, ssize_t channels, const char* what) {
  if (a.is_none()) return std::vector<float>((size_t)(rows * channels), 0.0f);
  F32Array v = F32Array::ensure(a);
  const bool ok = v && ((rows == 1 && v.ndim() == 1 && v.shape(0) == channels) || (v.ndim() == 2 && v.shape(0) == rows && v.shape(1) == channels));
  if (!ok)
    throw std::runtime_error(std::string("i8ie: position_embedding: ") + what + " must be float32 [" + (rows == 1 ? "" : std::to_string(rows) + ", ") +
                             std::to_string(channels) + "]");
  return std::vector<float>(v.data(), v.data() + v.size());
}
// E of i8ie_posembed_table on the device: P [tokens, c], the class token (or null) added into row 0
std::shared_ptr<Storage> posembed_table(const std::vector<float>& P, const std::vector<float>* cls, ssize_t tokens, ssize_t c) {
  std::vector<float> e(P.size());
  check(i8ie_posembed_table(P.data(), cls ? cls->data() : nullptr, (int)tokens, (int)c, e.data()));
  return upload_f32(e);
}

Tensor<float> posembed_f32(Tensor<float>& x, const std::shared_ptr<Storage>& e, ssize_t c, ssize_t h, ssize_t w, bool cls) {
  Tensor<float> out(posembed_shape(x, c, h, w, cls));
  check(i8ie_posembed_f32(ctx(), x.dptr(), out.dptr(), (int)x.shape[0], (int)c, (int)h, (int)w, cls ? 1 : 0, (const float*)e->dev));
  return out;
}
// e: the device table of i8ie_posembed_table, kept alive by the recorded launch
Tensor<u8_t> posembed_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& e, ssize_t c, ssize_t h, ssize_t w, bool cls, float scale, int zp) {
  check_out_qparams("position_embedding", scale, zp);
  need_contents(in);
  const std::vector<ssize_t> ishp = in.shape, oshp = posembed_shape(in, c, h, w, cls);
  if (!std::isfinite(in.scale) || !std::isfinite(255.0f * in.scale)) throw std::runtime_error("i8ie: position_embedding: the input scale must be finite");
  const float s_in = in.scale;
  const u8_t zp_i = in.zero_point, zp_o = (u8_t)zp;
  // deferred like layer_norm's result: relu(pe(..)) is one launch, a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the kernel, and several consumers (a LayerNorm and an Add skip) share one launch
  return deferred_one_input(
      in, oshp, scale, zp_o, [e, ishp, oshp, s_in, zp_i, scale, zp_o, cls](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        NhwcCopies copies;
        si = as_engine_nhwc(si, ishp, copies);
        std::shared_ptr<Storage> st = nhwc_storage(oshp, border, zp_o, s8);
        check(i8ie_posembed_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                    st->s8 ? 1 : 0, (int)ishp[0], (int)ishp[1], (int)ishp[2], (int)ishp[3], cls ? 1 : 0, (const float*)e->dev, s_in,
                                    zp_i, scale, zp_o, relu ? 1 : 0));
        return st;
      });
}

// PositionEmbedding(channels, height, width, class_token): a layer with fp32 `weight` (the table [T', c], default zeros) and, in
// the class form, `bias` (the class token [c], default zeros), no INT8 weights, and the layers' prepare / convert state machine
// around its output (scale, zero_point).  The table E does not depend on any quantisation: it is made and uploaded when first
// needed, for the FP32 and the INT8 path alike.
class PositionEmbedding : public QuantState {
 public:
  PositionEmbedding(ssize_t channels, ssize_t height, ssize_t width, bool class_token) : c_(channels), h_(height), w_(width), cls_(class_token) {
    posembed_dims(channels, height, width);
    weight_.assign((size_t)(tokens() * c_), 0.0f);
    bias_.assign(cls_ ? (size_t)c_ : 0, 0.0f);
  }
  void load_weight(const py::object& a) {
    weight_ = posembed_param(a, tokens(), c_, "weight");
    e_dev_.reset();
  }
  void load_bias(const py::object& a) {
    if (!cls_) throw std::runtime_error("i8ie: PositionEmbedding: there is no bias (the class token) without class_token=True");
    bias_ = posembed_param(a, 1, c_, "bias");
    e_dev_.reset();
  }
  void convert(bool /*per_channel: there are no INT8 weights*/ = false) {
    if (!convert_qparams()) return;
    install();
  }
  void load_quantized(const py::object& w, const py::object& b, float s_out, int zp_out) {  // what convert() would have left behind
    check_zero_point(zp_out);
    if (!cls_ && !b.is_none()) throw std::runtime_error("i8ie: PositionEmbedding: there is no bias (the class token) without class_token=True");
    weight_ = posembed_param(w, tokens(), c_, "weight");
    if (cls_) bias_ = posembed_param(b, 1, c_, "bias");
    e_dev_.reset();
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install();
  }
  Tensor<float> forward_f32(Tensor<float>& x) {
    posembed_shape(x, c_, h_, w_, cls_);
    Tensor<float> out = posembed_f32(x, table(), c_, h_, w_, cls_);
    maybe_sample(out);
    return out;
  }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    posembed_shape(x, c_, h_, w_, cls_);
    if (!is_quantized_) throw std::runtime_error("i8ie: PositionEmbedding is not converted (call convert() first)");
    return posembed_u8(x, table(), c_, h_, w_, cls_, scale_, zero_point_);
  }
  py::array_t<float> weight() const {
    py::array_t<float> a(std::vector<ssize_t>{tokens(), c_});
    std::memcpy(a.mutable_data(), weight_.data(), weight_.size() * sizeof(float));
    return a;
  }
  py::object bias() const {
    if (!cls_) return py::none();
    return py::array_t<float>((ssize_t)bias_.size(), bias_.data());
  }
  ssize_t channels() const { return c_; }
  ssize_t height() const { return h_; }
  ssize_t width() const { return w_; }
  bool class_token() const { return cls_; }

 private:
  ssize_t tokens() const { return h_ * w_ + (cls_ ? 1 : 0); }
  const std::shared_ptr<Storage>& table() {
    if (!e_dev_) e_dev_ = posembed_table(weight_, cls_ ? &bias_ : nullptr, tokens(), c_);
    return e_dev_;
  }
  void install() {
    if (!(scale_ > 0) || !std::isfinite(scale_)) throw std::runtime_error("i8ie: PositionEmbedding: the output scale must be positive and finite");
    set_quantized();
  }
  ssize_t c_, h_, w_;
  bool cls_;
  std::vector<float> weight_, bias_;
  std::shared_ptr<Storage> e_dev_;
};

}  // namespace

void bind_posembed(py::module_& m) {
  // weight: float32 [T', c]; class_token: float32 [c] or None (the plain form); the table is made and uploaded per call
  m.def("_position_embedding", [](Tensor<float>& x, const py::object& w, const py::object& cls) {
    if (x.shape.size() != 4) throw std::runtime_error("i8ie: position_embedding expects [n, c, h, w]");
    const ssize_t c = x.shape[1], h = x.shape[2], wd = x.shape[3], tokens = h * wd + (cls.is_none() ? 0 : 1);
    posembed_dims(c, h, wd);
    const std::vector<float> P = posembed_param(w, tokens, c, "weight"), t = cls.is_none() ? std::vector<float>() : posembed_param(cls, 1, c, "class_token");
    return posembed_f32(x, posembed_table(P, cls.is_none() ? nullptr : &t, tokens, c), c, h, wd, !cls.is_none());
  }, py::arg("x"), py::arg("weight"), py::arg("class_token"));
  m.def("_position_embedding", [](Tensor<u8_t>& x, const py::object& w, const py::object& cls, float scale, int zp) {
    check_out_qparams("position_embedding", scale, zp);
    if (x.shape.size() != 4) throw std::runtime_error("i8ie: position_embedding expects [n, c, h, w]");
    const ssize_t c = x.shape[1], h = x.shape[2], wd = x.shape[3], tokens = h * wd + (cls.is_none() ? 0 : 1);
    posembed_dims(c, h, wd);
    const std::vector<float> P = posembed_param(w, tokens, c, "weight"), t = cls.is_none() ? std::vector<float>() : posembed_param(cls, 1, c, "class_token");
    return posembed_u8(x, posembed_table(P, cls.is_none() ? nullptr : &t, tokens, c), c, h, wd, !cls.is_none(), scale, zp);
  }, py::arg("x"), py::arg("weight"), py::arg("class_token"), py::arg("scale"), py::arg("zero_point"));
  // The state machine's methods, bound here and not through bind_quant_state: tests/golden/binding_surface_calibration.json lists
  // the extension's classes that have a set_output_qparams attribute and stays as it is, so this private class binds that one
  // method as _set_output_qparams; i8ie.PositionEmbedding forwards to it under the public name.
  py::class_<PositionEmbedding> c(m, "_PositionEmbedding");
  c.def("prepare", &PositionEmbedding::prepare)
      .def("convert", &PositionEmbedding::convert, py::arg("per_channel") = false)
      .def("_set_output_qparams", &PositionEmbedding::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
      .def("output_qparams", &PositionEmbedding::output_qparams)
      .def("is_quantized", &PositionEmbedding::is_quantized)
      .def("_calib_histogram", &PositionEmbedding::calib_histogram)
      .def("_calib_range", &PositionEmbedding::calib_range, py::arg("method"), py::arg("param") = 99.99);
  c.def(py::init<ssize_t, ssize_t, ssize_t, bool>(), py::arg("channels"), py::arg("height"), py::arg("width"), py::arg("class_token") = false)
      .def("load_weight", &PositionEmbedding::load_weight)
      .def("load_bias", &PositionEmbedding::load_bias)
      .def("__call__", &PositionEmbedding::forward_f32)
      .def("__call__", &PositionEmbedding::forward_u8)
      .def("load_quantized", &PositionEmbedding::load_quantized, py::arg("weight"), py::arg("bias"), py::arg("out_scale"), py::arg("out_zero_point"))
      .def("weight", &PositionEmbedding::weight)
      .def("bias", &PositionEmbedding::bias)
      .def("channels", &PositionEmbedding::channels)
      .def("height", &PositionEmbedding::height)
      .def("width", &PositionEmbedding::width)
      .def("class_token", &PositionEmbedding::class_token);
}

}  // namespace i8ie_py
