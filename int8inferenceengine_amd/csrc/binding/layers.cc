// layers.cc -- the layers with weights and their bindings.
#include "layers.h"

namespace i8ie_py {

class Linear : public BaseLayer {
 public:
  Linear(ssize_t in_channel, ssize_t out_channel) : BaseLayer({out_channel, in_channel}, out_channel) {}
  using BaseLayer::BaseLayer;

  Tensor<float> forward_f32(Tensor<float>& in) {  // src/fully_connected.cc:5-21
    need_fp32();
    check_shapes();
    const ssize_t n = wshape_[0], k = wshape_[1];
    if (in.shape.empty() || in.size % k != 0 || in.shape.back() != k)
      throw std::runtime_error("i8ie: Linear: input's last dimension must equal in_features");
    const ssize_t m = in.size / k;
    upload_fp32();
    Tensor<float> out({m, n});
    check(i8ie_linear_f32(ctx(), in.dptr(), (int)m, (int)k, w_dev_, b_dev_, (int)n, out.dptr()));
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {  // src/fully_connected.cc:22-52
    need_quantized();
    const ssize_t n = wshape_[0], k = wshape_[1];
    if (in.shape.empty() || in.shape.back() != k)
      throw std::runtime_error("i8ie: Linear: input's last dimension must equal in_features");
    const ssize_t m = in.size / k;
    if (!want_acc) return std::make_tuple(defer(in, {m, n}, (int)m, 0, 0, false), py::object(py::none()));
    return forward_acc(in, {m, n}, {m, n}, (int)m, 0, 0);
  }

 protected:
  void check_shapes() const override {
    if (wshape_.size() != 2) throw std::runtime_error("i8ie: Linear weight must be [out_features, in_features]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: Linear bias size mismatch");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (per_channel_)
      check(i8ie_linear_create_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                           reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1],
                                           w_scales_.data(), &l));
    else
      check(i8ie_linear_create(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                               reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1], w_scale_, &l));
    return l;
  }
};

class Conv2d : public BaseLayer {
 public:
  using Pair = std::pair<ssize_t, ssize_t>;
  // groups: not in the reference (src/conv2d.cc:100-142 per group); the weight is [out, in / groups, k, k]
  // dilation: not in the reference either (torch.nn.Conv2d's dilation=, one integer)
  Conv2d(ssize_t in_channel, ssize_t out_channel, ssize_t kernel_size, ssize_t stride, ssize_t padding, ssize_t groups = 1,
         ssize_t dilation = 1)
      : BaseLayer({out_channel, checked_cg(in_channel, out_channel, groups), kernel_size, kernel_size}, out_channel),
        stride_(stride), padding_(padding), groups_(groups), dilation_(dilation), in_channels_(in_channel),
        stride_w_(stride), padding_w_(padding), dilation_w_(dilation) {
    check_axis(stride, padding, dilation);
  }
  // pairs (h, w) for the four geometry arguments (_Conv2dRect): the weight is [out, in / groups, kh, kw]
  Conv2d(ssize_t in_channel, ssize_t out_channel, Pair kernel_size, Pair stride, Pair padding, ssize_t groups, Pair dilation)
      : BaseLayer({out_channel, checked_cg(in_channel, out_channel, groups), kernel_size.first, kernel_size.second}, out_channel),
        stride_(stride.first), padding_(padding.first), groups_(groups), dilation_(dilation.first), in_channels_(in_channel),
        stride_w_(stride.second), padding_w_(padding.second), dilation_w_(dilation.second) {
    if (kernel_size.first < 1 || kernel_size.second < 1) throw std::runtime_error("i8ie: Conv2d: kernel_size must be >= 1");
    check_axis(stride_, padding_, dilation_);
    check_axis(stride_w_, padding_w_, dilation_w_);
  }
  // include/conv2d.h:16-17 leaves stride_/padding_ uninitialised for these two
  // constructors; they are 1 / 0 here.
  Conv2d(F32Array w, F32Array b) : BaseLayer(w, b) {}

  std::vector<ssize_t> out_shape(const std::vector<ssize_t>& s) const {
    if (s.size() != 4) throw std::runtime_error("i8ie: Conv2d expects an NCHW tensor");
    if (s[1] != in_channels()) throw std::runtime_error("i8ie: Conv2d: input channels do not match the weight");
    const ssize_t kh = dilation_ * (wshape_[2] - 1) + 1, kw = dilation_w_ * (wshape_[3] - 1) + 1;  // the kernel's extent
    if (s[2] - kh + 2 * padding_ < 0 || s[3] - kw + 2 * padding_w_ < 0)
      throw std::runtime_error((dilation_ > 1 || dilation_w_ > 1) ? "i8ie: Conv2d: dilated kernel larger than the padded input"
                                                                  : "i8ie: Conv2d: kernel larger than the padded input");
    return {s[0], wshape_[0], (s[2] - kh + 2 * padding_) / stride_ + 1, (s[3] - kw + 2 * padding_w_) / stride_w_ + 1};
  }
  Tensor<float> forward_f32(Tensor<float>& in) {  // src/conv2d.cc:63-98
    need_fp32();
    check_shapes();
    Tensor<float> out(out_shape(in.shape));
    upload_fp32();
    if (square())
      check(i8ie_conv2d_f32_dilated(ctx(), in.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                                    w_dev_, b_dev_, (int)wshape_[0], (int)wshape_[2], (int)wshape_[3], (int)stride_,
                                    (int)padding_, (int)groups_, (int)dilation_, out.dptr()));
    else {
      const i8ie_conv_geom g = geom();
      check(i8ie_conv2d_f32_rect(ctx(), in.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3], w_dev_,
                                 b_dev_, (int)wshape_[0], (int)groups_, &g, out.dptr()));
    }
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {  // src/conv2d.cc:100-142
    need_quantized();
    return forward_spatial_u8(in, out_shape(in.shape), want_acc);
  }

 protected:
  void check_shapes() const override {
    if (wshape_.size() != 4) throw std::runtime_error("i8ie: Conv2d weight must be [out, in, kh, kw]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: Conv2d bias size mismatch");
  }
  void check_weight_shape(const std::vector<ssize_t>& shp, const char* what) const override {
    if (in_channels_ <= 0) return;  // (built from arrays: the weight defines the layer)
    if (shp.size() != 4 || shp[0] != wshape_[0] || shp[1] != in_channels_ / groups_ || shp[2] != wshape_[2] || shp[3] != wshape_[3])
      throw std::runtime_error(std::string("i8ie: Conv2d: ") + what + ": weight must be [out, in / groups, k, k]");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (!square()) {  // (equal pairs take the entries below: constructed exactly as a layer of ints is)
      const i8ie_conv_geom g = geom();
      if (per_channel_)
        check(i8ie_conv2d_create_rect_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                                  reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)in_channels(),
                                                  (int)groups_, &g, w_scales_.data(), &l));
      else
        check(i8ie_conv2d_create_rect(ctx(), reinterpret_cast<const int8_t*>(qw_.data()), reinterpret_cast<const int8_t*>(qb_.data()),
                                      (int)n, (int)in_channels(), (int)groups_, &g, w_scale_, &l));
      return l;
    }
    if (per_channel_)
      check(i8ie_conv2d_create_dilated_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                                   reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)in_channels(),
                                                   (int)wshape_[2], (int)wshape_[3], (int)stride_, (int)padding_,
                                                   (int)groups_, (int)dilation_, w_scales_.data(), &l));
    else
      check(i8ie_conv2d_create_dilated(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                       reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)in_channels(),
                                       (int)wshape_[2], (int)wshape_[3], (int)stride_, (int)padding_, (int)groups_,
                                       (int)dilation_, w_scale_, &l));
    return l;
  }

 public:
  ssize_t groups() const { return groups_; }
  ssize_t dilation() const { return dilation_; }
  Pair dilation_pair() const { return {dilation_, dilation_w_}; }
  py::dict geometry() const {
    py::dict d;
    d["kernel_size"] = py::make_tuple(wshape_[2], wshape_[3]);
    d["stride"] = py::make_tuple(stride_, stride_w_);
    d["padding"] = py::make_tuple(padding_, padding_w_);
    d["dilation"] = py::make_tuple(dilation_, dilation_w_);
    return d;
  }

 private:
  static void check_axis(ssize_t stride, ssize_t padding, ssize_t dilation) {
    if (dilation < 1) throw std::runtime_error("i8ie: Conv2d: dilation must be >= 1");
    if (stride == 0) throw std::runtime_error("i8ie: Conv2d: stride must not be 0");  // include/conv2d.h:12-14
    if (stride < 0 || padding < 0) throw std::runtime_error("i8ie: Conv2d: negative stride/padding");
  }
  bool square() const {
    return wshape_[2] == wshape_[3] && stride_ == stride_w_ && padding_ == padding_w_ && dilation_ == dilation_w_;
  }
  i8ie_conv_geom geom() const {
    return i8ie_conv_geom{(int)wshape_[2], (int)wshape_[3], (int)stride_, (int)stride_w_, (int)padding_, (int)padding_w_,
                          (int)dilation_, (int)dilation_w_};
  }
  static ssize_t checked_cg(ssize_t in_channel, ssize_t out_channel, ssize_t groups) {
    if (groups < 1) throw std::runtime_error("i8ie: Conv2d: groups must be >= 1");
    if (in_channel % groups != 0 || out_channel % groups != 0)
      throw std::runtime_error("i8ie: Conv2d: groups must divide in_channels and out_channels");
    return in_channel / groups;
  }
  ssize_t in_channels() const { return wshape_[1] * groups_; }
  ssize_t stride_ = 1;
  ssize_t padding_ = 0;
  ssize_t groups_ = 1;
  ssize_t dilation_ = 1;
  ssize_t in_channels_ = 0;  // as constructed from sizes (0: constructed from arrays)
  ssize_t stride_w_ = 1, padding_w_ = 0, dilation_w_ = 1;  // the w axis (stride_ / padding_ / dilation_: the h axis)
};

// Conv2d constructed from pairs (i8ie.Conv2d with a pair whose values differ): a class of its own, private to the package, so
// that the extension's Conv2d keeps its recorded surface
class Conv2dRect : public Conv2d {
 public:
  using Conv2d::Conv2d;
};

// ConvTranspose2d (additive, not in the reference): torch.nn.ConvTranspose2d with a square kernel, groups = 1, dilation = 1.
// The layer is the reference convolution of the equivalent zero-inserted problem (include/i8ie_hip.h,
// i8ie_conv_transpose2d_create), so the weights are held as the equivalent kernel W~ [out, in, k, k],
// W~[oc][ic][ky][kx] = W[ic][oc][k-1-ky][k-1-kx]: convert() quantises W~ by the layers' own rules (per tensor over weight and
// bias; per row of W~ with row_len = in*k*k).  load_weight / load_quantized take and q_weight gives torch's [in, out, k, k].
class ConvTranspose2d : public BaseLayer {
 public:
  ConvTranspose2d(ssize_t in_channel, ssize_t out_channel, ssize_t kernel_size, ssize_t stride, ssize_t padding, ssize_t output_padding)
      : BaseLayer({checked(out_channel, in_channel, kernel_size, stride, padding, output_padding), in_channel, kernel_size, kernel_size},
                  out_channel),
        stride_(stride), padding_(padding), opad_(output_padding) {}

  // torch's [in, out, k, k] <-> the equivalent [out, in, k, k] (the same map both ways round, with the outer sizes swapped)
  template <typename T>
  static std::vector<T> swap_flip(const T* src, ssize_t a, ssize_t b, ssize_t k) {  // src [a][b][k][k] -> [b][a][k][k], flipped
    std::vector<T> dst((size_t)(a * b * k * k));
    for (ssize_t i = 0; i < a; ++i)
      for (ssize_t j = 0; j < b; ++j)
        for (ssize_t y = 0; y < k; ++y)
          for (ssize_t x = 0; x < k; ++x)
            dst[(size_t)(((j * a + i) * k + (k - 1 - y)) * k + (k - 1 - x))] = src[(size_t)(((i * b + j) * k + y) * k + x)];
    return dst;
  }
  void check_torch_shape(const std::vector<ssize_t>& shp, const char* what) const {
    if (shp.size() != 4 || shp[0] != wshape_[1] || shp[1] != wshape_[0] || shp[2] != wshape_[2] || shp[3] != wshape_[3])
      throw std::runtime_error(std::string("i8ie: ConvTranspose2d: ") + what + ": weight must be [in, out, k, k]");
  }
  void load_weight(F32Array w) {
    if (!has_fp32_) throw std::runtime_error("i8ie: load_weight: layer is already converted");
    check_torch_shape(std::vector<ssize_t>(w.shape(), w.shape() + w.ndim()), "load_weight");
    w_ = swap_flip<float>(w.data(), wshape_[1], wshape_[0], wshape_[2]);
    wt_.assign(w.data(), w.data() + w.size());
    release_fp32_dev();
  }
  void load_quantized(S8Array qw, S8Array qb, py::object w_scale, float s_out, int zp_out) {
    check_torch_shape(std::vector<ssize_t>(qw.shape(), qw.shape() + qw.ndim()), "load_quantized");
    std::vector<s8_t> eq = swap_flip<s8_t>(qw.data(), wshape_[1], wshape_[0], wshape_[2]);
    py::array_t<s8_t> a(wshape_);
    std::memcpy(a.mutable_data(), eq.data(), eq.size());
    BaseLayer::load_quantized(a, qb, w_scale, s_out, zp_out);
    std::vector<float>().swap(wt_);
  }
  void convert(bool per_channel = false) {
    BaseLayer::convert(per_channel);
    if (is_quantized_) std::vector<float>().swap(wt_);
  }
  py::array_t<s8_t> q_weight() const {
    need_quantized();
    std::vector<s8_t> t = swap_flip<s8_t>(qw_.data(), wshape_[0], wshape_[1], wshape_[2]);
    py::array_t<s8_t> a(std::vector<ssize_t>{wshape_[1], wshape_[0], wshape_[2], wshape_[3]});
    std::memcpy(a.mutable_data(), t.data(), t.size());
    return a;
  }

  py::array_t<float> fp32_weight() override {  // torch's [in, out, k, k]
    need_fp32_params();
    const std::vector<float>& t = fp32_kernel_weight();
    py::array_t<float> a(std::vector<ssize_t>{wshape_[1], wshape_[0], wshape_[2], wshape_[3]});
    std::memcpy(a.mutable_data(), t.data(), t.size() * sizeof(float));
    return a;
  }

  std::vector<ssize_t> out_shape(const std::vector<ssize_t>& s) const {
    if (s.size() != 4) throw std::runtime_error("i8ie: ConvTranspose2d expects an NCHW tensor");
    if (s[1] != wshape_[1]) throw std::runtime_error("i8ie: ConvTranspose2d: input channels do not match the weight");
    const ssize_t k = wshape_[2];
    const ssize_t oh = (s[2] - 1) * stride_ - 2 * padding_ + k + opad_, ow = (s[3] - 1) * stride_ - 2 * padding_ + k + opad_;
    if (s[2] < 1 || s[3] < 1 || oh < 1 || ow < 1) throw std::runtime_error("i8ie: ConvTranspose2d: empty output");
    return {s[0], wshape_[0], oh, ow};
  }
  Tensor<float> forward_f32(Tensor<float>& in) {
    need_fp32();
    Tensor<float> out(out_shape(in.shape));
    upload_fp32();
    check(i8ie_conv_transpose2d_f32(ctx(), in.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                                    w_dev_, b_dev_, (int)wshape_[0], (int)wshape_[2], (int)stride_, (int)padding_, (int)opad_,
                                    out.dptr()));
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {
    need_quantized();
    return forward_spatial_u8(in, out_shape(in.shape), want_acc);
  }

 protected:
  const std::vector<float>& fp32_kernel_weight() override {  // (the FP32 kernel reads torch's layout)
    if (wt_.empty()) wt_ = swap_flip<float>(w_.data(), wshape_[0], wshape_[1], wshape_[2]);
    return wt_;
  }
  void check_shapes() const override {
    if (wshape_.size() != 4) throw std::runtime_error("i8ie: ConvTranspose2d weight must be [in, out, k, k]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: ConvTranspose2d bias size mismatch");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (per_channel_)
      check(i8ie_conv_transpose2d_create_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                                     reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1],
                                                     (int)wshape_[2], (int)stride_, (int)padding_, (int)opad_,
                                                     w_scales_.data(), &l));
    else
      check(i8ie_conv_transpose2d_create(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                         reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1], (int)wshape_[2],
                                         (int)stride_, (int)padding_, (int)opad_, w_scale_, &l));
    return l;
  }

 private:
  // the rules of the C entries (I8IE_ERR_ARG there), raised where Conv2d raises for bad groups
  static ssize_t checked(ssize_t out_channel, ssize_t in_channel, ssize_t k, ssize_t stride, ssize_t padding, ssize_t opad) {
    if (in_channel < 1 || out_channel < 1 || k < 1) throw std::runtime_error("i8ie: ConvTranspose2d: non-positive size");
    if (stride < 1) throw std::runtime_error("i8ie: ConvTranspose2d: stride must be >= 1");
    if (padding < 0 || padding > k - 1) throw std::runtime_error("i8ie: ConvTranspose2d: padding must be in [0, kernel_size - 1]");
    if (opad < 0 || opad >= stride) throw std::runtime_error("i8ie: ConvTranspose2d: output_padding must be in [0, stride)");
    return out_channel;
  }
  ssize_t stride_ = 1, padding_ = 0, opad_ = 0;
  std::vector<float> wt_;  // the FP32 weight as loaded (torch's layout), for the FP32 kernel
};

template <typename L>
void bind_layer_common(py::class_<L>& c) {
  c.def("load_weight", &L::load_weight)
      .def("load_bias", &L::load_bias)
      .def("__call__", [](L& l, Tensor<float>& x) { return l.forward_f32(x); })
      .def("__call__", [](L& l, Tensor<u8_t>& x) { return std::get<0>(l.forward_u8(x, false)); })
      .def("forward_debug", [](L& l, Tensor<u8_t>& x) { return l.forward_u8(x, true); })
      .def("load_quantized", &L::load_quantized, py::arg("q_weight"), py::arg("q_bias"), py::arg("weight_scale"),
           py::arg("out_scale"), py::arg("out_zero_point"))
      .def("q_weight", &L::q_weight)
      .def("q_bias", &L::q_bias)
      .def("weight_scale", &L::weight_scale)
      .def("weight_scales", &L::weight_scales)
      .def("is_per_channel", &L::is_per_channel)
      // (private: the classes keep their recorded public surface; i8ie.fold_batchnorm reads the FP32 parameters through these)
      .def("_weight", [](L& l) { return l.fp32_weight(); })
      .def("_bias", [](L& l) { return l.fp32_bias(); })
      .def("_is_preparing", [](const L& l) { return l.is_preparing(); });
  bind_quant_state(c);
}

void bind_layers(py::module_& m) {
  {
    py::class_<Linear> c(m, "Linear");  // src/fully_connected.cc:54-72
    c.def(py::init<F32Array, F32Array>())
        .def(py::init([](Tensor<float>& w, Tensor<float>& b) { return new Linear(w.numpy(), b.numpy()); }))
        .def(py::init<ssize_t, ssize_t>());
    bind_layer_common(c);
  }
  {
    py::class_<Conv2d> c(m, "Conv2d");  // src/conv2d.cc:144-165
    c.def(py::init<F32Array, F32Array>())
        .def(py::init([](Tensor<float>& w, Tensor<float>& b) { return new Conv2d(w.numpy(), b.numpy()); }))
        .def(py::init<ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t>(), py::arg("in_channels"),
             py::arg("out_channels"), py::arg("kernel_size"), py::arg("stride") = 1, py::arg("padding") = 0,
             py::arg("groups") = 1, py::arg("dilation") = 1)
        .def("groups", &Conv2d::groups)
        .def("dilation", &Conv2d::dilation)
        .def("_geometry", &Conv2d::geometry);  // (private: the class keeps its recorded public surface; i8ie.Layer.geometry() asks it)
    bind_layer_common(c);
  }

  {
    using Pair = Conv2d::Pair;
    py::class_<Conv2dRect> c(m, "_Conv2dRect");
    c.def(py::init<ssize_t, ssize_t, Pair, Pair, Pair, ssize_t, Pair>(), py::arg("in_channels"), py::arg("out_channels"),
          py::arg("kernel_size"), py::arg("stride") = Pair(1, 1), py::arg("padding") = Pair(0, 0), py::arg("groups") = 1,
          py::arg("dilation") = Pair(1, 1))
        .def("groups", &Conv2dRect::groups)
        .def("dilation", [](const Conv2dRect& l) -> py::object {
          const Pair d = l.dilation_pair();
          return d.first == d.second ? py::object(py::int_(d.first)) : py::object(py::make_tuple(d.first, d.second));
        })
        .def("geometry", &Conv2dRect::geometry);
    bind_layer_common(c);
  }
  {
    py::class_<ConvTranspose2d> c(m, "ConvTranspose2d");
    c.def(py::init<ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t>(), py::arg("in_channels"), py::arg("out_channels"),
          py::arg("kernel_size"), py::arg("stride") = 1, py::arg("padding") = 0, py::arg("output_padding") = 0);
    bind_layer_common(c);
  }
  bind_weightless_layers(m);
}

}  // namespace i8ie_py
