// layers.h -- BaseLayer: what Linear, Conv2d and ConvTranspose2d share (weights, convert, the deferred INT8 forward).
#pragma once
#include "calibrator.h"
#include "ops.h"

namespace i8ie_py {

// x.reshape(n, -1) of a border-free NHWC activation of m images that still lies as its conv left it: its storage (a Linear
// layer then walks K in (h, w, c) order instead of asking for the reference's order), or null
inline const Storage* flattened_nhwc(const Tensor<u8_t>& t, int m) {
  const Storage* s = t.st.get();
  const bool yes = s && s->layout == I8IE_LAYOUT_NHWC && s->border == 0 && s->dn == m && s->dh * s->dw > 1 &&
                   (ssize_t)s->dn * s->dc * s->dh * s->dw == t.size;
  return yes ? s : nullptr;
}

class BaseLayer : public QuantState {
 public:
  BaseLayer(std::vector<ssize_t> wshape, ssize_t out_channel) : wshape_(std::move(wshape)) {
    ssize_t n = 1;
    for (ssize_t d : wshape_) n *= d;
    w_.assign((size_t)n, 0.0f);
    b_.assign((size_t)out_channel, 0.0f);
    has_fp32_ = true;
  }
  BaseLayer(F32Array w, F32Array b) {
    has_fp32_ = true;
    load_weight(w);
    load_bias(b);
  }
  virtual ~BaseLayer() { release_fp32_dev(); }

  void load_weight(F32Array w) {  // include/layer.h:15-20
    if (!has_fp32_) throw std::runtime_error("i8ie: load_weight: layer is already converted");
    check_weight_shape(std::vector<ssize_t>(w.shape(), w.shape() + w.ndim()), "load_weight");
    wshape_.assign(w.shape(), w.shape() + w.ndim());
    w_.assign(w.data(), w.data() + w.size());
    release_fp32_dev();
  }
  void load_bias(F32Array b) {  // include/layer.h:21-26
    if (!has_fp32_) throw std::runtime_error("i8ie: load_bias: layer is already converted");
    b_.assign(b.data(), b.data() + b.size());
    release_fp32_dev();
  }
  void convert(bool per_channel = false) {  // src/layer.cc:36-54 (per_channel: the opt-in per-output-channel rule)
    if (!convert_qparams()) return;
    check_shapes();
    const ssize_t n = (ssize_t)b_.size();
    qw_.resize(w_.size());
    qb_.resize(b_.size());
    per_channel_ = per_channel;
    if (per_channel) {
      w_scales_.assign((size_t)n, 0.0f);
      check(i8ie_quantize_weight_per_channel(w_.data(), (int)n, (int64_t)(w_.size() / n), b_.data(),
                                             reinterpret_cast<int8_t*>(qw_.data()), reinterpret_cast<int8_t*>(qb_.data()),
                                             w_scales_.data()));
      w_scale_ = 1;
    } else {
      check(i8ie_quantize_weight(w_.data(), (int64_t)w_.size(), b_.data(), (int64_t)b_.size(),
                                 reinterpret_cast<int8_t*>(qw_.data()), reinterpret_cast<int8_t*>(qb_.data()),
                                 &w_scale_));
    }
    install_handle();
  }
  // additive: restore a converted layer from saved INT8 weights (what convert() would have produced)
  // w_scale: a number (per-tensor layer) or an array of one scale per output feature (per-channel layer)
  void load_quantized(S8Array qw, S8Array qb, py::object w_scale, float s_out, int zp_out) {
    check_zero_point(zp_out);
    std::vector<ssize_t> shp(qw.shape(), qw.shape() + qw.ndim());
    if (shp.size() != wshape_.size()) throw std::runtime_error("i8ie: load_quantized: weight rank mismatch");
    check_weight_shape(shp, "load_quantized");
    wshape_ = shp;
    if (qb.size() != wshape_[0]) throw std::runtime_error("i8ie: load_quantized: bias size mismatch");
    const bool pc = py::isinstance<py::array>(w_scale) ? py::array(w_scale).ndim() > 0
                                                        : (py::isinstance<py::list>(w_scale) || py::isinstance<py::tuple>(w_scale));
    std::vector<float> scales;
    if (pc) {
      auto a = F32Array::ensure(w_scale);
      if (!a || a.ndim() != 1 || a.size() != wshape_[0])
        throw std::runtime_error("i8ie: load_quantized: weight_scale array must hold one scale per output feature");
      scales.assign(a.data(), a.data() + a.size());
    }
    qw_.assign(qw.data(), qw.data() + qw.size());
    qb_.assign(qb.data(), qb.data() + qb.size());
    per_channel_ = pc;
    w_scales_ = scales;
    w_scale_ = pc ? 1.0f : w_scale.cast<float>();
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install_handle();
  }
  py::array_t<s8_t> q_weight() const {
    need_quantized();
    py::array_t<s8_t> a(wshape_);
    std::memcpy(a.mutable_data(), qw_.data(), qw_.size());
    return a;
  }
  py::array_t<s8_t> q_bias() const {
    need_quantized();
    py::array_t<s8_t> a((ssize_t)qb_.size());
    std::memcpy(a.mutable_data(), qb_.data(), qb_.size());
    return a;
  }
  float weight_scale() const {
    need_quantized();
    if (per_channel_) throw std::runtime_error("i8ie: weight_scale: per-channel layer (use weight_scales())");
    return w_scale_;
  }
  py::array_t<float> weight_scales() const {  // float32 [out] in both modes (i8ie_layer_weight_scales)
    need_quantized();
    py::array_t<float> a((ssize_t)qb_.size());
    int pc = 0;
    check(i8ie_layer_weight_scales(q_.get(), a.mutable_data(), (int)qb_.size(), &pc));
    return a;
  }
  bool is_per_channel() const { return is_quantized_ && per_channel_; }
  // the FP32 parameters as loaded (what i8ie.fold_batchnorm reads); gone once convert() has released them
  virtual py::array_t<float> fp32_weight() {
    need_fp32_params();
    py::array_t<float> a(wshape_);
    std::memcpy(a.mutable_data(), w_.data(), w_.size() * sizeof(float));
    return a;
  }
  py::array_t<float> fp32_bias() {
    need_fp32_params();
    return py::array_t<float>((ssize_t)b_.size(), b_.data());
  }

 protected:
  void output_qparams_changed() override {
    if (q_) check(i8ie_layer_set_output_qparams(q_.get(), scale_, zero_point_));
  }
  // the tail convert() and load_quantized() share: the library's layer from the INT8 weights, the output qparams into it,
  // the FP32 weights released (src/layer.cc:52-53), the state flipped
  void install_handle() {
    i8ie_layer* raw = make_handle((ssize_t)qb_.size());
    q_ = std::shared_ptr<i8ie_layer>(raw, [](i8ie_layer* l) { i8ie_layer_destroy(l); });
    check(i8ie_layer_set_output_qparams(q_.get(), scale_, zero_point_));
    set_quantized();
    std::vector<float>().swap(w_);
    std::vector<float>().swap(b_);
    has_fp32_ = false;
    release_fp32_dev();
  }
  virtual void check_shapes() const = 0;
  // a layer that was given its channel counts refuses a weight of another shape (Conv2d with groups: [out, in/groups, k, k])
  virtual void check_weight_shape(const std::vector<ssize_t>&, const char*) const {}
  virtual i8ie_layer* make_handle(ssize_t n) = 0;
  // Deferred INT8 forward: returns a tensor whose launch happens when it is first needed.
  Tensor<u8_t> defer(Tensor<u8_t>& in, std::vector<ssize_t> oshape, int m, int h, int w, bool spatial) {
    Tensor<u8_t> out = pending_u8(std::move(oshape), scale_, zero_point_);
    std::shared_ptr<i8ie_layer> handle = q_;
    Tensor<u8_t> src = in;  // shares the input's storage / pending launch
    const float s_in = in.scale;
    const u8_t zp_in = in.zero_point;
    const int zp_out = zero_point_;
    const std::vector<ssize_t> oshp = out.shape;
    const size_t obytes = (size_t)out.size;
    // One recorded conv / linear forward, with or without a max-pool folded in behind it (pk > 1).  Negotiates the
    // layouts at both ends with the library: a conv whose kernel reads re-biased bytes asks its producer for them, and
    // stores re-biased itself when its consumer asked and its kernel can (i8ie_layer_rebiased_io).
    auto run = [handle, s_in, zp_in, zp_out, m, spatial, oshp, obytes](Tensor<u8_t>& src, int h, int w, bool relu, int border, bool s8,
                                                                        int pk, int ps) -> std::shared_ptr<Storage> {
      int out_layout = I8IE_LAYOUT_NCHW, pad = 0;
      if (spatial) {
        check(i8ie_layer_preferred_layout(handle.get(), &out_layout));
        check(i8ie_layer_padding(handle.get(), &pad));
      }
      const bool pool = pk > 1 || (pk == 1 && ps > 1);  // (a subsampling 1 x 1 window is a pool: the library runs it unfused)
      if (pool && out_layout != I8IE_LAYOUT_NHWC) return nullptr;  // (the caller pools the unfused result)
      std::vector<ssize_t> rshp = oshp;
      if (pool) {
        rshp[2] = (oshp[2] - pk) / ps + 1;
        rshp[3] = (oshp[3] - pk) / ps + 1;
      }
      int reads = 0, stores = 0;
      if (spatial && out_layout == I8IE_LAYOUT_NHWC) check(i8ie_layer_rebiased_io(handle.get(), m, h, w, pool ? pk : 0, ps, &reads, &stores));
      const bool st_s8 = s8 && stores;
      if (spatial && out_layout == I8IE_LAYOUT_NHWC && src.pend && src.qsrc && !src.pend_relu) {
        int yes = 0;
        check(i8ie_layer_accepts_f32_input(handle.get(), h, w, &yes));
        if (yes) {  // quantize + conv (+ relu) (+ max-pool) in one kernel, reading the FP32 input
          auto st = nhwc_storage(rshp, border, zp_out, st_s8);
          check(i8ie_layer_forward_f32_input_pool(handle.get(), (const float*)src.qsrc->device_ptr(), m, h, w, src.qscale, src.qzp,
                                                  relu ? 1 : 0, pool ? pk : 0, ps, (uint8_t*)st->dev,
                                                  st_s8 ? I8IE_LAYOUT_NHWC_S8 : I8IE_LAYOUT_NHWC, border, nullptr));
          return st;
        }
      }
      const uint8_t* ip;
      if (spatial) {
        // ask a still-pending producer for a zero-point border that covers this conv's padding (and for re-biased bytes
        // when this layer's kernel reads them as they are)
        src.realize(out_layout == I8IE_LAYOUT_NHWC ? pad : 0, reads != 0);
        ip = (src.st && src.st->s8 && reads) ? src.dptr_raw() : src.dptr_any();
      } else {
        src.realize(0);
        if (const Storage* s = flattened_nhwc(src, m)) {
          ip = src.dptr_any();
          h = s->dh;
          w = s->dw;
        } else {
          ip = src.dptr();
        }
      }
      const int in_layout = src.st->s8 ? I8IE_LAYOUT_NHWC_S8 : src.st->layout, in_border = src.st->border;
      const int ob = out_layout == I8IE_LAYOUT_NHWC ? border : 0;
      auto st = out_layout == I8IE_LAYOUT_NHWC ? nhwc_storage(rshp, ob, zp_out, st_s8) : device_storage(obytes);
      const int ol = st_s8 ? I8IE_LAYOUT_NHWC_S8 : out_layout;
      if (pool)
        check(i8ie_layer_forward_pool(handle.get(), ip, in_layout, in_border, m, h, w, s_in, zp_in, relu ? 1 : 0, pk, ps,
                                      (uint8_t*)st->dev, ol, ob, nullptr));
      else
        check(i8ie_layer_forward_fused(handle.get(), ip, in_layout, in_border, m, h, w, s_in, zp_in, relu ? 1 : 0,
                                       (uint8_t*)st->dev, ol, ob, nullptr));
      // (the input is released when the last tensor holding this closure lets go of it: right after the
      // launch in `x = relu(layer(x))`, later if the un-fused result is observed as well)
      return st;
    };
    out.pend = make_pend([run, src, h, w](bool relu, int border, bool s8) mutable { return run(src, h, w, relu, border, s8, 0, 0); },
                         {in.pend});
    if (spatial) {
      // max_pool2d right behind this (relu'd) conv: one call of the library, which folds the pool into the convolution's
      // epilogue where a kernel of its can and runs the max-pool kernel behind it otherwise
      Tensor<u8_t> srcp = in;
      out.pend->fn_pool = [run, srcp, h, w](bool relu, int border, bool s8, int pk, int ps) mutable {
        return run(srcp, h, w, relu, border, s8, pk, ps);
      };
    }
    if (!spatial && out.shape.size() == 2 && out.shape[1] <= 16) {
      // dequantize(layer(x)) of a classifier head: one fused launch (i8ie_layer_forward_dequant)
      Tensor<u8_t> src2 = in;
      out.pend_f32 = std::make_shared<std::function<std::shared_ptr<Storage>(bool)>>(
          [handle, src2, s_in, zp_in, m, obytes](bool relu) mutable {
            src2.realize(0);
            const uint8_t* ip;
            int lay = I8IE_LAYOUT_NCHW, hh = 0, ww = 0;
            if (const Storage* s = flattened_nhwc(src2, m)) {
              ip = src2.dptr_any();
              lay = I8IE_LAYOUT_NHWC;
              hh = s->dh;
              ww = s->dw;
            } else {
              ip = src2.dptr();
            }
            auto f = device_storage(obytes * sizeof(float));
            auto q = device_storage(obytes);  // u8 side output: only written when the fused kernel does not apply
            check(i8ie_layer_forward_dequant(handle.get(), ip, lay, m, hh, ww, s_in, zp_in, relu ? 1 : 0,
                                             (uint8_t*)q->dev, (float*)f->dev));
            return f;
          });
    }
    return out;
  }
  // forward_debug: the eager forward in the reference's order, with the int32 accumulators (shape `ashape`) beside the result
  std::tuple<Tensor<u8_t>, py::object> forward_acc(Tensor<u8_t>& in, std::vector<ssize_t> oshape, std::vector<ssize_t> ashape, int m, int h,
                                                   int w) {
    Tensor<u8_t> out = pending_u8(std::move(oshape), scale_, zero_point_);
    out.st = device_storage((size_t)out.size);
    Tensor<int32_t> acc(std::move(ashape));
    check(i8ie_layer_forward(q_.get(), in.dptr(), m, h, w, in.scale, in.zero_point, out.dptr(), acc.dptr()));
    py::object acc_np = acc.numpy();
    return std::make_tuple(std::move(out), acc_np);
  }
  // Conv2d / ConvTranspose2d on a u8 tensor: recorded, or the debug forward
  std::tuple<Tensor<u8_t>, py::object> forward_spatial_u8(Tensor<u8_t>& in, std::vector<ssize_t> oshape, bool want_acc) {
    const int n = (int)in.shape[0], h = (int)in.shape[2], w = (int)in.shape[3];
    if (!want_acc) return std::make_tuple(defer(in, oshape, n, h, w, true), py::object(py::none()));
    return forward_acc(in, oshape, {oshape[0], oshape[2] * oshape[3], oshape[1]}, n, h, w);
  }
  void need_quantized() const {
    if (!is_quantized_) throw std::runtime_error("i8ie: layer is not converted (call convert() first)");
  }
  void need_fp32() const {
    if (!has_fp32_)
      throw std::runtime_error("i8ie: FP32 input given to a converted layer (its FP32 weights were released)");
  }
  void need_fp32_params() const {
    if (!has_fp32_) throw std::runtime_error("i8ie: the layer is converted: its FP32 weight and bias were released");
  }
  virtual const std::vector<float>& fp32_kernel_weight() { return w_; }  // the host weight the FP32 kernel reads
  void upload_fp32() {
    if (w_dev_) return;
    const std::vector<float>& w = fp32_kernel_weight();
    check(i8ie_malloc(ctx(), w.size() * 4, (void**)&w_dev_));
    check(i8ie_malloc(ctx(), b_.size() * 4, (void**)&b_dev_));
    check(i8ie_memcpy_h2d(ctx(), w_dev_, w.data(), w.size() * 4));
    check(i8ie_memcpy_h2d(ctx(), b_dev_, b_.data(), b_.size() * 4));
  }
  void release_fp32_dev() {
    if (rt().ctx) {
      if (w_dev_) i8ie_free(rt().ctx, w_dev_);
      if (b_dev_) i8ie_free(rt().ctx, b_dev_);
    }
    w_dev_ = b_dev_ = nullptr;
  }

  std::vector<ssize_t> wshape_;
  std::vector<float> w_, b_;
  bool has_fp32_ = false;
  float* w_dev_ = nullptr;
  float* b_dev_ = nullptr;
  std::vector<s8_t> qw_, qb_;
  float w_scale_ = 1;
  bool per_channel_ = false;
  std::vector<float> w_scales_;  // per-channel layers: s_w[j]
  std::shared_ptr<i8ie_layer> q_;
};

void bind_layers(py::module_& m);             // layers.cc: Linear, Conv2d, ConvTranspose2d, then the weightless ones
void bind_weightless_layers(py::module_& m);  // layers_weightless.cc: Add ... Activation, LayerNorm, GroupNorm, BatchNorm2d

}  // namespace i8ie_py
