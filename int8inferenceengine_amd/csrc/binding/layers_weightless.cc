// layers_weightless.cc -- the layers without INT8 weights (Add ... Activation, LayerNorm, GroupNorm, BatchNorm2d) and their bindings.
#include "layers.h"

namespace i8ie_py {

// A layer without weights (the residual Add, the channel Concat): the layers' prepare / convert state machine
// (src/layer.cc:28-54) around its output (scale, zero_point); FP32 tensors join in FP32 (and are sampled while preparing),
// u8 tensors after convert().
class Weightless : public QuantState {
 public:
  void convert(bool /*per_channel: there are no weights*/ = false) {
    if (convert_qparams()) set_quantized();
  }
  void load_quantized(float s_out, int zp_out) {  // what convert() would have left behind
    set_output_qparams(s_out, zp_out);
    set_quantized();
  }

 protected:
  Tensor<float> sampled(Tensor<float> out) {  // what a preparing layer does with its FP32 result
    maybe_sample(out);
    return out;
  }
  void need_quantized(const char* what) const {
    if (!is_quantized_) throw std::runtime_error(std::string("i8ie: ") + what + " is not converted (call convert() first)");
  }
};
class Add : public Weightless {
 public:
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(add_f32(a, b)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    need_quantized("Add");
    return add_u8(a, b, scale_, zero_point_);
  }
};
// a * b; b has a's shape or is a's gate [n, c, 1, 1] / [n, c]
class Mul : public Weightless {
 public:
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(mul_f32(a, b)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    mul_is_gate(a, b);
    need_quantized("Mul");
    return mul_u8(a, b, scale_, zero_point_);
  }
};
// a . b of two activation tensors (matmul_shape's rules), each optionally given transposed
class MatMul : public Weightless {
 public:
  MatMul(bool transpose_a, bool transpose_b) : ta_(transpose_a), tb_(transpose_b) {}
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(matmul_f32(a, b, ta_, tb_)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    matmul_shape(a, b, ta_, tb_);
    need_quantized("MatMul");
    return matmul_u8(a, b, scale_, zero_point_, ta_, tb_);
  }
  bool transpose_a() const { return ta_; }
  bool transpose_b() const { return tb_; }

 private:
  bool ta_, tb_;
};
// multi-head attention of q, k, v (or one packed qkv tensor; attention_shape's rules): two calibrated parameter sets, the
// scores' (scale, zero_point) beside the output's.  While preparing, the FP32 scores are sampled by a calibrator of their own.
class Attention : public Weightless {
 public:
  explicit Attention(ssize_t heads) : heads_(heads) {
    if (heads < 1) throw std::runtime_error("i8ie: Attention: heads must be >= 1");
  }
  void prepare() {
    if (!is_quantized_) score_cal_ = std::make_unique<Calibrator>(rt().calib_histogram);
    QuantState::prepare();
  }
  void convert(bool /*per_channel: there are no weights*/ = false) {
    if (!is_quantized_ && is_preparing_ && score_cal_ && score_cal_->cnt > 0) {
      float s;
      u8_t z;
      std::tie(s, z) = score_cal_->get_range(1);
      if (!score_overridden_) {
        score_scale_ = s;
        score_zp_ = z;
      }
    }
    score_cal_.reset();
    Weightless::convert();
  }
  void set_score_qparams(float s, int zp) {  // inject what calibration would produce
    check_zero_point(zp);
    score_scale_ = s;
    score_zp_ = (u8_t)zp;
    score_overridden_ = true;
  }
  py::dict score_calib_histogram() { return histogram_dict(score_cal_.get(), is_preparing_); }
  py::tuple score_calib_range(const std::string& method, double param) { return histogram_range_tuple(score_cal_.get(), is_preparing_, method, param); }
  std::tuple<float, int> score_qparams() const { return std::make_tuple(score_scale_, (int)score_zp_); }
  void load_quantized(float s_out, int zp_out, float s_score, int zp_score) {  // what convert() would have left behind
    set_score_qparams(s_score, zp_score);
    Weightless::load_quantized(s_out, zp_out);
  }
  Tensor<float> forward_f32(Tensor<float>& q, Tensor<float>& k, Tensor<float>& v) { return run_f32(q, &k, &v); }
  Tensor<float> forward_f32_packed(Tensor<float>& qkv) { return run_f32(qkv, nullptr, nullptr); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& q, Tensor<u8_t>& k, Tensor<u8_t>& v) { return run_u8(q, &k, &v); }
  Tensor<u8_t> forward_u8_packed(Tensor<u8_t>& qkv) { return run_u8(qkv, nullptr, nullptr); }
  ssize_t heads() const { return heads_; }
  // attend inside win_h x win_w windows of rank-4 maps from now on (i8ie.Attention(heads, window=): a constructor argument, not state)
  void set_window(ssize_t wh, ssize_t ww) {
    if (wh < 1 || ww < 1) throw std::runtime_error("i8ie: Attention: the window must be at least 1 x 1");
    wh_ = wh;
    ww_ = ww;
  }

 private:
  Tensor<float> run_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v) {
    if (wh_ > 0) return run_window_f32(q, k, v);
    if (!is_preparing_ || !score_cal_) return attention_f32(q, k, v, heads_, nullptr);
    const AttnShape s = attention_shape(q, k, v, heads_);
    Tensor<float> scores(std::vector<ssize_t>{s.b, s.heads, s.tq, s.tk});
    Tensor<float> out = attention_f32(q, k, v, heads_, &scores);
    calib_sample(*score_cal_, scores);
    return sampled(out);
  }
  Tensor<float> run_window_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v) {
    if (!is_preparing_ || !score_cal_) return attention_window_f32(q, k, v, heads_, wh_, ww_, nullptr);
    const AttnWindowShape s = attention_window_shape(q, k, v, heads_, wh_, ww_);
    Tensor<float> scores(std::vector<ssize_t>{s.b * s.windows, s.heads, s.tq, s.tk});
    Tensor<float> out = attention_window_f32(q, k, v, heads_, wh_, ww_, &scores);
    calib_sample(*score_cal_, scores);
    return sampled(out);
  }
  Tensor<u8_t> run_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v) {
    if (wh_ > 0) {
      attention_window_shape(q, k, v, heads_, wh_, ww_);
      need_quantized("Attention");
      return attention_window_u8(q, k, v, heads_, wh_, ww_, score_scale_, score_zp_, scale_, zero_point_);
    }
    attention_shape(q, k, v, heads_);
    need_quantized("Attention");
    return attention_u8(q, k, v, heads_, score_scale_, score_zp_, scale_, zero_point_);
  }
  ssize_t heads_;
  ssize_t wh_ = 0, ww_ = 0;   // 0: the global form
  std::unique_ptr<Calibrator> score_cal_;
  float score_scale_ = 1;
  u8_t score_zp_ = 0;
  bool score_overridden_ = false;
};
// cat along axis 1: a list of FP32 tensors before convert(), of u8 tensors after it
class Concat : public Weightless {
 public:
  py::object forward(const py::list& tensors) {
    if (!tensors.empty() && py::isinstance<Tensor<u8_t>>(tensors[0])) {
      std::vector<Tensor<u8_t>> ts = cat_list<u8_t>(tensors);
      cat_shape(ts);
      need_quantized("Concat");
      return py::cast(cat_u8(std::move(ts), scale_, zero_point_));
    }
    return py::cast(sampled(cat_f32(cat_list<float>(tensors))));
  }
};
// a table-driven activation (I8IE_ACT_*): f in FP32 before convert(), one table lookup from the input tensor's
// (scale, zero_point) to this layer's own output qparams after it
class Activation : public Weightless {
 public:
  Activation(int kind, float param) : kind_(kind), param_(param) {
    LutBytes probe;  // (an unknown kind or a slope that is not finite is refused here)
    check(i8ie_activation_table(kind, param, 1.0f, 0, 1.0f, 0, probe.data()));
  }
  Tensor<float> forward_f32(Tensor<float>& x) { return sampled(activation_f32(x, kind_, param_)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    need_quantized("Activation");
    return activation_u8(x, kind_, param_, scale_, zero_point_);
  }
  int kind() const { return kind_; }
  float param() const { return param_; }

 private:
  int kind_;
  float param_;
};
// LayerNorm over the channel axis of [n, c, h, w] or the last axis of [m, f] / [b, t, f]: a layer with fp32 weight (gamma) and
// bias (beta) and the layers' prepare / convert state machine around its output (scale, zero_point).  There are no INT8
// weights: convert() computes g = gamma / s_out and b = beta / s_out + zp_out (i8ie_layernorm_affine) and uploads them once.
class LayerNorm : public QuantState {
 public:
  LayerNorm(ssize_t channels, float eps) : channels_(channels), eps_(eps) {
    if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: LayerNorm: channels must be in 1..16384");
    if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: LayerNorm: eps must be positive and finite");
    gamma_.assign((size_t)channels, 1.0f);
    beta_.assign((size_t)channels, 0.0f);
  }
  void load_weight(const py::object& w) { gamma_ = layer_norm_param(w, channels_, 1.0f, "weight"); params_changed(); }
  void load_bias(const py::object& b) { beta_ = layer_norm_param(b, channels_, 0.0f, "bias"); params_changed(); }
  void convert(bool /*per_channel: there are no INT8 weights*/ = false) {
    if (!convert_qparams()) return;
    install();
  }
  void load_quantized(const py::object& w, const py::object& b, float s_out, int zp_out) {  // what convert() would have left behind
    check_zero_point(zp_out);
    gamma_ = layer_norm_param(w, channels_, 1.0f, "weight");
    beta_ = layer_norm_param(b, channels_, 0.0f, "bias");
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install();
  }
  Tensor<float> forward_f32(Tensor<float>& x) {
    layer_norm_rows(x, channels_);
    if (!gamma_dev_) {
      gamma_dev_ = upload_f32(gamma_);
      beta_dev_ = upload_f32(beta_);
    }
    Tensor<float> out = layer_norm_f32(x, gamma_dev_, beta_dev_, channels_, eps_);
    maybe_sample(out);
    return out;
  }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    layer_norm_rows(x, channels_);
    if (!is_quantized_) throw std::runtime_error("i8ie: LayerNorm is not converted (call convert() first)");
    return layer_norm_u8(x, g_dev_, b_dev_, channels_, eps_, scale_, zero_point_);
  }
  py::array_t<float> weight() const { return py::array_t<float>((ssize_t)gamma_.size(), gamma_.data()); }
  py::array_t<float> bias() const { return py::array_t<float>((ssize_t)beta_.size(), beta_.data()); }
  ssize_t channels() const { return channels_; }
  float eps() const { return eps_; }

 protected:
  void output_qparams_changed() override {
    if (is_quantized_) install();
  }

 private:
  void params_changed() {
    gamma_dev_.reset();
    beta_dev_.reset();
    if (is_quantized_) install();
  }
  void install() {
    if (!(scale_ > 0) || !std::isfinite(scale_)) throw std::runtime_error("i8ie: LayerNorm: the output scale must be positive and finite");
    std::tie(g_dev_, b_dev_) = layer_norm_affine(gamma_, beta_, scale_, zero_point_);
    set_quantized();
  }
  ssize_t channels_;
  float eps_;
  std::vector<float> gamma_, beta_;
  std::shared_ptr<Storage> gamma_dev_, beta_dev_;  // FP32 path
  std::shared_ptr<Storage> g_dev_, b_dev_;         // after convert()
};
// GroupNorm of [n, c, h, w] or [n, c] (torch.nn.GroupNorm): LayerNorm's state machine and parameters, the statistics taken per
// image over the pixels and the c / groups channels of a group (include/i8ie_hip.h, i8ie_groupnorm_u8_nhwc).
class GroupNorm : public QuantState {
 public:
  GroupNorm(ssize_t groups, ssize_t channels, float eps) : groups_(groups), channels_(channels), eps_(eps) {
    if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: GroupNorm: num_channels must be in 1..16384");
    if (groups < 1 || channels % groups != 0) throw std::runtime_error("i8ie: GroupNorm: num_channels must be a multiple of num_groups");
    if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: GroupNorm: eps must be positive and finite");
    gamma_.assign((size_t)channels, 1.0f);
    beta_.assign((size_t)channels, 0.0f);
  }
  void load_weight(const py::object& w) { gamma_ = layer_norm_param(w, channels_, 1.0f, "weight"); params_changed(); }
  void load_bias(const py::object& b) { beta_ = layer_norm_param(b, channels_, 0.0f, "bias"); params_changed(); }
  void convert(bool /*per_channel: there are no INT8 weights*/ = false) {
    if (!convert_qparams()) return;
    install();
  }
  void load_quantized(const py::object& w, const py::object& b, float s_out, int zp_out) {  // what convert() would have left behind
    check_zero_point(zp_out);
    gamma_ = layer_norm_param(w, channels_, 1.0f, "weight");
    beta_ = layer_norm_param(b, channels_, 0.0f, "bias");
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install();
  }
  Tensor<float> forward_f32(Tensor<float>& x) {
    group_norm_pixels(x, groups_, channels_);
    if (!gamma_dev_) {
      gamma_dev_ = upload_f32(gamma_);
      beta_dev_ = upload_f32(beta_);
    }
    Tensor<float> out = group_norm_f32(x, gamma_dev_, beta_dev_, groups_, channels_, eps_);
    maybe_sample(out);
    return out;
  }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    group_norm_pixels(x, groups_, channels_);
    if (!is_quantized_) throw std::runtime_error("i8ie: GroupNorm is not converted (call convert() first)");
    return group_norm_u8(x, g_dev_, b_dev_, groups_, channels_, eps_, scale_, zero_point_);
  }
  py::array_t<float> weight() const { return py::array_t<float>((ssize_t)gamma_.size(), gamma_.data()); }
  py::array_t<float> bias() const { return py::array_t<float>((ssize_t)beta_.size(), beta_.data()); }
  ssize_t num_groups() const { return groups_; }
  ssize_t channels() const { return channels_; }
  float eps() const { return eps_; }

 protected:
  void output_qparams_changed() override {
    if (is_quantized_) install();
  }

 private:
  void params_changed() {
    gamma_dev_.reset();
    beta_dev_.reset();
    if (is_quantized_) install();
  }
  void install() {
    if (!(scale_ > 0) || !std::isfinite(scale_)) throw std::runtime_error("i8ie: GroupNorm: the output scale must be positive and finite");
    std::tie(g_dev_, b_dev_) = layer_norm_affine(gamma_, beta_, scale_, zero_point_);
    set_quantized();
  }
  ssize_t groups_, channels_;
  float eps_;
  std::vector<float> gamma_, beta_;
  std::shared_ptr<Storage> gamma_dev_, beta_dev_;  // FP32 path
  std::shared_ptr<Storage> g_dev_, b_dev_;         // after convert()
};
// Inference BatchNorm of [n, c, h, w] or [n, c] (torch.nn.BatchNorm2d / BatchNorm1d in eval mode): fp32 weight (gamma), bias
// (beta), running_mean and running_var of num_features values each and the layers' prepare / convert state machine around its
// output (scale, zero_point).  convert() computes g and b (i8ie_batchnorm_affine) and uploads them once; they do not depend on
// the input's quantisation, which is an argument of every launch.
class BatchNorm2d : public QuantState {
 public:
  BatchNorm2d(ssize_t channels, float eps) : channels_(channels), eps_(eps) {
    if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: BatchNorm2d: num_features must be in 1..16384");
    if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: BatchNorm2d: eps must be positive and finite");
    gamma_.assign((size_t)channels, 1.0f);
    beta_.assign((size_t)channels, 0.0f);
    mean_.assign((size_t)channels, 0.0f);
    var_.assign((size_t)channels, 1.0f);
  }
  void load_weight(const py::object& a) { gamma_ = layer_norm_param(a, channels_, 1.0f, "weight"); params_changed(); }
  void load_bias(const py::object& a) { beta_ = layer_norm_param(a, channels_, 0.0f, "bias"); params_changed(); }
  void load_running_mean(const py::object& a) { mean_ = layer_norm_param(a, channels_, 0.0f, "running_mean"); params_changed(); }
  void load_running_var(const py::object& a) { var_ = layer_norm_param(a, channels_, 1.0f, "running_var"); params_changed(); }
  void convert(bool /*per_channel: there are no INT8 weights*/ = false) {
    if (!convert_qparams()) return;
    install();
  }
  void load_quantized(const py::object& w, const py::object& b, const py::object& mean, const py::object& var, float s_out,
                      int zp_out) {  // what convert() would have left behind
    check_zero_point(zp_out);
    gamma_ = layer_norm_param(w, channels_, 1.0f, "weight");
    beta_ = layer_norm_param(b, channels_, 0.0f, "bias");
    mean_ = layer_norm_param(mean, channels_, 0.0f, "running_mean");
    var_ = layer_norm_param(var, channels_, 1.0f, "running_var");
    dev_ = BatchNormF32();
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install();
  }
  Tensor<float> forward_f32(Tensor<float>& x) {
    batch_norm_pixels(x, channels_);
    if (!dev_.gamma) dev_ = BatchNormF32{upload_f32(gamma_), upload_f32(beta_), upload_f32(mean_), upload_f32(var_)};
    Tensor<float> out = batch_norm_f32(x, dev_, channels_, eps_);
    maybe_sample(out);
    return out;
  }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    batch_norm_pixels(x, channels_);
    if (!is_quantized_) throw std::runtime_error("i8ie: BatchNorm2d is not converted (call convert() first)");
    return batch_norm_u8(x, g_dev_, b_dev_, channels_, scale_, zero_point_);
  }
  static py::array_t<float> array_of(const std::vector<float>& v) { return py::array_t<float>((ssize_t)v.size(), v.data()); }
  py::array_t<float> weight() const { return array_of(gamma_); }
  py::array_t<float> bias() const { return array_of(beta_); }
  py::array_t<float> running_mean() const { return array_of(mean_); }
  py::array_t<float> running_var() const { return array_of(var_); }
  ssize_t num_features() const { return channels_; }
  float eps() const { return eps_; }

 protected:
  void output_qparams_changed() override {
    if (is_quantized_) install();
  }

 private:
  void params_changed() {
    dev_ = BatchNormF32();
    if (is_quantized_) install();
  }
  void install() {
    if (!(scale_ > 0) || !std::isfinite(scale_)) throw std::runtime_error("i8ie: BatchNorm2d: the output scale must be positive and finite");
    std::tie(g_dev_, b_dev_) = batch_norm_affine(gamma_, beta_, mean_, var_, eps_, scale_, zero_point_);
    set_quantized();
  }
  ssize_t channels_;
  float eps_;
  std::vector<float> gamma_, beta_, mean_, var_;
  BatchNormF32 dev_;                        // FP32 path
  std::shared_ptr<Storage> g_dev_, b_dev_;  // after convert()
};
template <typename L>
void bind_weightless_state(py::class_<L>& c) {
  bind_quant_state(c);
  c.def("load_quantized", &L::load_quantized, py::arg("out_scale"), py::arg("out_zero_point"));
}
template <typename L>
void bind_weightless_common(py::class_<L>& c) {
  c.def(py::init<>());
  bind_weightless_state(c);
}

void bind_weightless_layers(py::module_& m) {
  {
    py::class_<Add> c(m, "Add");
    bind_weightless_common(c);
    c.def("__call__", &Add::forward_f32).def("__call__", &Add::forward_u8);
  }
  {
    py::class_<Mul> c(m, "Mul");
    bind_weightless_common(c);
    c.def("__call__", &Mul::forward_f32).def("__call__", &Mul::forward_u8);
  }
  {
    py::class_<MatMul> c(m, "MatMul");
    c.def(py::init<bool, bool>(), py::arg("transpose_a") = false, py::arg("transpose_b") = false);
    bind_weightless_state(c);
    c.def("__call__", &MatMul::forward_f32).def("__call__", &MatMul::forward_u8)
        .def("transpose_a", &MatMul::transpose_a).def("transpose_b", &MatMul::transpose_b);
  }
  {
    py::class_<Attention> c(m, "Attention");
    bind_quant_state(c);
    c.def(py::init<ssize_t>(), py::arg("heads"))
        .def("set_score_qparams", &Attention::set_score_qparams, py::arg("scale"), py::arg("zero_point"))
        .def("score_qparams", &Attention::score_qparams)
        .def("_score_calib_histogram", &Attention::score_calib_histogram)
        .def("_score_calib_range", &Attention::score_calib_range, py::arg("method"), py::arg("param") = 99.99)
        .def("load_quantized", &Attention::load_quantized, py::arg("out_scale"), py::arg("out_zero_point"), py::arg("score_scale"),
             py::arg("score_zero_point"))
        .def("heads", &Attention::heads)
        .def("_set_window", &Attention::set_window, py::arg("win_h"), py::arg("win_w"))
        .def("__call__", &Attention::forward_f32).def("__call__", &Attention::forward_f32_packed)
        .def("__call__", &Attention::forward_u8).def("__call__", &Attention::forward_u8_packed);
  }
  {
    py::class_<Concat> c(m, "Concat");
    bind_weightless_common(c);
    c.def("__call__", &Concat::forward, py::arg("tensors"));
  }
  {
    py::class_<Activation> c(m, "Activation");
    c.def(py::init<int, float>(), py::arg("kind"), py::arg("param") = 0.0f);
    bind_weightless_state(c);
    c.def("__call__", &Activation::forward_f32).def("__call__", &Activation::forward_u8).def("kind", &Activation::kind).def("param", &Activation::param);
  }

  {
    py::class_<LayerNorm> c(m, "LayerNorm");
    bind_quant_state(c);
    c.def(py::init<ssize_t, float>(), py::arg("channels"), py::arg("eps") = 1e-5f)
        .def("load_weight", &LayerNorm::load_weight)
        .def("load_bias", &LayerNorm::load_bias)
        .def("__call__", &LayerNorm::forward_f32)
        .def("__call__", &LayerNorm::forward_u8)
        .def("load_quantized", &LayerNorm::load_quantized, py::arg("weight"), py::arg("bias"), py::arg("out_scale"),
             py::arg("out_zero_point"))
        .def("weight", &LayerNorm::weight)
        .def("bias", &LayerNorm::bias)
        .def("channels", &LayerNorm::channels)
        .def("eps", &LayerNorm::eps);
  }
  {
    py::class_<GroupNorm> c(m, "_GroupNorm");  // (private to the i8ie package: see _group_norm in ops.cc)
    bind_quant_state(c);
    c.def(py::init<ssize_t, ssize_t, float>(), py::arg("num_groups"), py::arg("num_channels"), py::arg("eps") = 1e-5f)
        .def("load_weight", &GroupNorm::load_weight)
        .def("load_bias", &GroupNorm::load_bias)
        .def("__call__", &GroupNorm::forward_f32)
        .def("__call__", &GroupNorm::forward_u8)
        .def("load_quantized", &GroupNorm::load_quantized, py::arg("weight"), py::arg("bias"), py::arg("out_scale"),
             py::arg("out_zero_point"))
        .def("weight", &GroupNorm::weight)
        .def("bias", &GroupNorm::bias)
        .def("num_groups", &GroupNorm::num_groups)
        .def("channels", &GroupNorm::channels)
        .def("eps", &GroupNorm::eps);
  }
  {
    py::class_<BatchNorm2d> c(m, "_BatchNorm2d");  // (private to the i8ie package: see _batch_norm in ops.cc)
    bind_quant_state(c);
    c.def(py::init<ssize_t, float>(), py::arg("num_features"), py::arg("eps") = 1e-5f)
        .def("load_weight", &BatchNorm2d::load_weight)
        .def("load_bias", &BatchNorm2d::load_bias)
        .def("load_running_mean", &BatchNorm2d::load_running_mean)
        .def("load_running_var", &BatchNorm2d::load_running_var)
        .def("__call__", &BatchNorm2d::forward_f32)
        .def("__call__", &BatchNorm2d::forward_u8)
        .def("load_quantized", &BatchNorm2d::load_quantized, py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
             py::arg("running_var"), py::arg("out_scale"), py::arg("out_zero_point"))
        .def("weight", &BatchNorm2d::weight)
        .def("bias", &BatchNorm2d::bias)
        .def("running_mean", &BatchNorm2d::running_mean)
        .def("running_var", &BatchNorm2d::running_var)
        .def("num_features", &BatchNorm2d::num_features)
        .def("eps", &BatchNorm2d::eps)
        .def("_is_preparing", &BatchNorm2d::is_preparing);
  }
}

}  // namespace i8ie_py
