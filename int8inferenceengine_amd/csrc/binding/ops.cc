// ops.cc -- quantize / dequantize / relu / the pools / upsample / activation and lut, the s8 instantiations, and bind_ops.
#include "ops.h"

namespace i8ie_py {

// ------------------------------------------------------------ elementwise ----
Tensor<u8_t> quantize(Tensor<float>& in, float scale, u8_t zp) {  // src/quantize_utils.cc:44-52
  Tensor<u8_t> out = pending_u8(in.shape, scale, zp);
  (void)in.dptr();  // make sure the FP32 source is on the device
  std::shared_ptr<Storage> src = in.st;
  const ssize_t n = in.size;
  out.qsrc = src;
  out.qscale = scale;
  out.qzp = zp;
  // deferred: a first conv layer that accepts FP32 input consumes `src` directly (fused quantize)
  out.pend = make_pend(
      [src, n, scale, zp](bool relu, int, bool) {
        auto st = device_storage((size_t)n);
        check(i8ie_quantize_f32_u8(ctx(), (const float*)src->device_ptr(), (uint8_t*)st->dev, n, scale, zp));
        if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, n, zp));
        return st;
      });
  return out;
}
Tensor<float> dequantize(Tensor<u8_t>& in) {  // src/quantize_utils.cc:54-58
  if (in.pend && in.pend_f32) {  // classifier head still pending: layer + (relu) + dequantize in one launch
    Tensor<float> out;
    out.shape = in.shape;
    out.size = in.size;
    out.st = (*in.pend_f32)(in.pend_relu);
    return out;
  }
  Tensor<float> out(in.shape);
  check(i8ie_dequantize_u8_f32(ctx(), in.dptr(), out.dptr(), in.size, in.scale, in.zero_point));
  return out;
}
Tensor<u8_t> relu_u8(Tensor<u8_t>& in) {  // src/functional.cc:15-26
  if (in.pend && !in.pend_relu) {
    // `in` is a layer output that has not been launched: record layer+relu as one launch.
    // `in` itself stays pending (if it is ever observed it launches without the relu).
    Tensor<u8_t> out = pending_u8(in.shape, in.scale, in.zero_point);
    out.pend = in.pend;
    out.pend_f32 = in.pend_f32;
    out.pend_relu = true;  // (qsrc is not carried over: relu(quantize(x)) is not a plain quantize)
    return out;
  }
  const uint8_t* src = in.shape.size() == 4 ? in.dptr_any() : in.dptr();
  Tensor<u8_t> out(in.shape);
  out.scale = in.scale;
  out.zero_point = in.zero_point;
  if (in.st->layout == I8IE_LAYOUT_NHWC) {  // elementwise over the physical buffer (border bytes = zp stay zp)
    out.st = device_storage(in.st->bytes);
    out.st->set_nhwc(in.shape, in.st->border);
  }
  check(i8ie_relu_u8(ctx(), src, (uint8_t*)out.st->dev, (int64_t)in.st->bytes, in.zero_point));
  return out;
}
Tensor<float> relu_f32(Tensor<float>& in) {  // src/functional.cc:5-13
  Tensor<float> out(in.shape);
  check(i8ie_relu_f32(ctx(), in.dptr(), out.dptr(), in.size));
  return out;
}
template <typename T>
std::vector<ssize_t> pool_shape(const Tensor<T>& in, ssize_t k, ssize_t s) {
  if (in.shape.size() != 4) throw std::runtime_error("i8ie: max_pool2d expects an NCHW tensor");
  if (k <= 0 || s <= 0) throw std::runtime_error("i8ie: max_pool2d: kernel_size and stride must be positive");
  if (k > in.shape[2] || k > in.shape[3]) throw std::runtime_error("i8ie: max_pool2d: window larger than input");
  return {in.shape[0], in.shape[1], (in.shape[2] - k) / s + 1, (in.shape[3] - k) / s + 1};
}
Tensor<u8_t> max_pool2d_u8(Tensor<u8_t>& in, ssize_t k, ssize_t s) {  // src/functional.cc:36-64
  Tensor<u8_t> out = pending_u8(pool_shape(in, k, s), in.scale, in.zero_point);
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> ishp = in.shape, oshp = out.shape;
  const u8_t zp = in.zero_point;
  const int kk = (int)k, ss = (int)s;
  // deferred so that a consuming conv can ask for a zero-point border around the result
  out.pend = make_pend(
      [src, ishp, oshp, zp, kk, ss](bool relu, int border, bool s8) mutable {
        if (src.pend && src.pend->fn_pool && src.pend.use_count() == 1 && src.pend->made.empty()) {
          // relu(layer(x)) still pending, nobody else holds it (no second consumer, not observable any more), and its
          // kernel pools in the epilogue: one launch, no unpooled tensor.  With another holder the layer launches once,
          // unfused, and every consumer reads that result (a recorded launch never runs twice).
          // (a relu behind the pool folds in as well: max-pool and relu commute, both are monotone)
          std::shared_ptr<Storage> st = src.pend->fn_pool(src.pend_relu || relu, border, s8, kk, ss);
          if (st) return st;
        }
        const uint8_t* ip = src.dptr_any();
        std::shared_ptr<Storage> st;
        const size_t logical = (size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3];
        if (src.st->layout == I8IE_LAYOUT_NHWC && ishp[1] % 16 == 0) {
          st = nhwc_storage(oshp, border, zp);
          check(i8ie_maxpool2d_u8_nhwc(ctx(), ip, src.st->border, (uint8_t*)st->dev, border, (int)ishp[0], (int)ishp[1],
                                       (int)ishp[2], (int)ishp[3], kk, ss));
        } else {
          st = device_storage(logical);
          check(i8ie_maxpool2d_u8(ctx(), src.dptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                  (int)ishp[3], kk, ss));
        }
        if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        return st;
      }, {in.pend});
  return out;
}
// ---- avg_pool2d / global_avg_pool2d (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_avgpool2d_u8) ---
// kh x kw window; the global pool is the whole image at stride 1
template <typename T>
std::vector<ssize_t> avg_pool_shape(const Tensor<T>& in, ssize_t kh, ssize_t kw, ssize_t s, bool global) {
  const std::string what = global ? "i8ie: global_avg_pool2d" : "i8ie: avg_pool2d";
  if (in.shape.size() != 4) throw std::runtime_error(what + " expects an NCHW tensor");
  if (global) {
    kh = in.shape[2];
    kw = in.shape[3];
  }
  if (kh <= 0 || kw <= 0 || s <= 0) throw std::runtime_error(what + ": kernel_size and stride must be positive");
  if (kh > in.shape[2] || kw > in.shape[3]) throw std::runtime_error(what + ": window larger than input");
  if (kh * kw > 65536) throw std::runtime_error(what + ": window of more than 65536 elements");
  return {in.shape[0], in.shape[1], (in.shape[2] - kh) / s + 1, (in.shape[3] - kw) / s + 1};
}
Tensor<float> avg_pool_f32(Tensor<float>& in, ssize_t k, ssize_t s, bool global) {
  Tensor<float> out(avg_pool_shape(in, k, k, s, global));
  const ssize_t kh = global ? in.shape[2] : k, kw = global ? in.shape[3] : k;
  check(i8ie_avgpool2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                           (int)kh, (int)kw, (int)s));
  return out;
}
Tensor<u8_t> avg_pool_u8(Tensor<u8_t>& in, ssize_t k, ssize_t s, bool global) {
  const std::vector<ssize_t> ishp = in.shape, oshp = avg_pool_shape(in, k, k, s, global);
  const u8_t zp = in.zero_point;
  const int kh = (int)(global ? in.shape[2] : k), kw = (int)(global ? in.shape[3] : k), ss = (int)s;
  // deferred like max_pool2d's and add's results: relu(avg_pool2d(..)) is one launch, and a consuming conv gets its
  // zero-point border and, where it reads them, re-biased bytes straight from the pool kernel
  return deferred_one_input(  // (as max_pool2d: the input's qparams; like add, no check for an empty tensor)
      in, oshp, in.scale, zp, [ishp, oshp, zp, kh, kw, ss](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        const size_t logical = (size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3];
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          // a plain border-free [n, c, 1, 1] result is the same bytes in both orders: it is labelled NCHW, so that its
          // reshape to [n, c] reaches a Linear layer (or the host) without a layout conversion
          const bool both_orders = oshp[2] == 1 && oshp[3] == 1 && border == 0 && !s8;
          st = both_orders ? device_storage(logical) : nhwc_storage(oshp, border, zp, s8);
          check(i8ie_avgpool2d_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev,
                                       st->border, st->s8 ? 1 : 0, (int)ishp[0], (int)ishp[1], (int)ishp[2], (int)ishp[3], kh, kw, ss,
                                       relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage(logical);
          check(i8ie_avgpool2d_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                  (int)ishp[3], kh, kw, ss));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}
// ---- the pools with torch's padding and ceil_mode (no counterpart in the reference; geometry and arithmetic:
// include/i8ie_hip.h, i8ie_pool_output_size).  The i8ie package sends a call here only where the geometry differs from the
// unpadded floor pool's; that one keeps the entries above, and with them the conv + max-pool fusion.
struct PadPool {
  int k, s, p, ceil_mode, include_pad;
  bool avg;
  std::vector<ssize_t> oshp;
};
// the checked arguments of one call, and the result's shape
template <typename T>
PadPool pad_pool_args(const Tensor<T>& in, ssize_t k, ssize_t s, ssize_t p, bool ceil_mode, bool include_pad, bool avg) {
  const std::string what = avg ? "i8ie: avg_pool2d" : "i8ie: max_pool2d";
  if (in.shape.size() != 4) throw std::runtime_error(what + " expects an NCHW tensor");
  if (k <= 0 || s <= 0) throw std::runtime_error(what + ": kernel_size and stride must be positive");
  if (p < 0 || p > k / 2) throw std::runtime_error(what + ": padding must be at least 0 and at most half the kernel_size");
  if (k > in.shape[2] + 2 * p || k > in.shape[3] + 2 * p) throw std::runtime_error(what + ": window larger than the padded input");
  if (k * k > 65536) throw std::runtime_error(what + ": window of more than 65536 elements");
  for (ssize_t d : in.shape)
    if (d <= 0 || d > 0x7FFFFFFF) throw std::runtime_error(what + ": empty tensor");
  const int oh = i8ie_pool_output_size((int)in.shape[2], (int)k, (int)s, (int)p, ceil_mode ? 1 : 0);
  const int ow = i8ie_pool_output_size((int)in.shape[3], (int)k, (int)s, (int)p, ceil_mode ? 1 : 0);
  if (oh < 0 || ow < 0) throw std::runtime_error(std::string("i8ie: ") + i8ie_last_error());
  return PadPool{(int)k, (int)s, (int)p, ceil_mode ? 1 : 0, include_pad ? 1 : 0, avg, {in.shape[0], in.shape[1], oh, ow}};
}
Tensor<float> pad_pool_f32(Tensor<float>& in, const PadPool& g) {
  Tensor<float> out(g.oshp);
  const int n = (int)in.shape[0], c = (int)in.shape[1], h = (int)in.shape[2], w = (int)in.shape[3];
  if (g.avg) check(i8ie_avgpool2d_f32_pad(ctx(), in.dptr(), out.dptr(), n, c, h, w, g.k, g.s, g.p, g.ceil_mode, g.include_pad));
  else check(i8ie_maxpool2d_f32_pad(ctx(), in.dptr(), out.dptr(), n, c, h, w, g.k, g.s, g.p, g.ceil_mode));
  return out;
}
Tensor<u8_t> pad_pool_u8(Tensor<u8_t>& in, const PadPool& g) {
  const std::vector<ssize_t> ishp = in.shape, oshp = g.oshp;
  need_contents(in);
  const u8_t zp = in.zero_point;
  // deferred like avg_pool2d's result: relu(pool(..)) is one launch, and a consuming conv gets its zero-point border and,
  // where it reads them, re-biased bytes straight from the pool kernel
  return deferred_one_input(  // (as the unpadded pools: the input's qparams)
      in, oshp, in.scale, zp, [ishp, zp, g](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        const std::vector<ssize_t>& oshp = g.oshp;
        const int n = (int)ishp[0], c = (int)ishp[1], h = (int)ishp[2], w = (int)ishp[3];
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != ishp[0] || si->dc != ishp[1] || si->dh != ishp[2] || si->dw != ishp[3])) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage(oshp, border, zp, s8);
          const uint8_t* ip = (const uint8_t*)si->device_ptr();
          if (g.avg)
            check(i8ie_avgpool2d_u8_nhwc_pad(ctx(), ip, si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, n, c, h, w,
                                             g.k, g.s, g.p, g.ceil_mode, g.include_pad, relu ? 1 : 0, zp));
          else
            check(i8ie_maxpool2d_u8_nhwc_pad(ctx(), ip, si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, n, c, h, w,
                                             g.k, g.s, g.p, g.ceil_mode, relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage((size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3]);
          const uint8_t* ip = (const uint8_t*)si->device_ptr();
          if (g.avg) check(i8ie_avgpool2d_u8_pad(ctx(), ip, (uint8_t*)st->dev, n, c, h, w, g.k, g.s, g.p, g.ceil_mode, g.include_pad, zp));
          else check(i8ie_maxpool2d_u8_pad(ctx(), ip, (uint8_t*)st->dev, n, c, h, w, g.k, g.s, g.p, g.ceil_mode));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}
// ---- upsample (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_upsample2d_u8) -----------------------
template <typename T>
std::vector<ssize_t> upsample_shape(const Tensor<T>& in, ssize_t fh, ssize_t fw, int mode) {
  if (in.shape.size() != 4) throw std::runtime_error("i8ie: upsample expects an NCHW tensor");
  for (ssize_t d : in.shape)
    if (d <= 0) throw std::runtime_error("i8ie: upsample: empty tensor");
  if (fh < 1 || fh > 8 || fw < 1 || fw > 8) throw std::runtime_error("i8ie: upsample: scale factors must be integers in 1..8");
  if (mode != I8IE_UPSAMPLE_NEAREST && mode != I8IE_UPSAMPLE_BILINEAR) throw std::runtime_error("i8ie: upsample: unknown mode");
  return {in.shape[0], in.shape[1], in.shape[2] * fh, in.shape[3] * fw};
}
Tensor<float> upsample_f32(Tensor<float>& in, ssize_t fh, ssize_t fw, int mode) {
  Tensor<float> out(upsample_shape(in, fh, fw, mode));
  check(i8ie_upsample2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                            (int)fh, (int)fw, mode));
  return out;
}
Tensor<u8_t> upsample_u8(Tensor<u8_t>& in, ssize_t fh, ssize_t fw, int mode) {
  const std::vector<ssize_t> ishp = in.shape, oshp = upsample_shape(in, fh, fw, mode);
  need_contents(in);
  const u8_t zp = in.zero_point;
  const int f_h = (int)fh, f_w = (int)fw;
  // deferred like avg_pool2d's result: relu(upsample(..)) is one launch, and a consuming conv gets its zero-point border
  // and, where it reads them, re-biased bytes straight from the upsample kernel
  return deferred_one_input(  // (as the pools: the input's qparams)
      in, oshp, in.scale, zp, [ishp, oshp, zp, f_h, f_w, mode](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != ishp[0] || si->dc != ishp[1] || si->dh != ishp[2] || si->dw != ishp[3])) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage(oshp, border, zp, s8);
          check(i8ie_upsample2d_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                        st->s8 ? 1 : 0, (int)ishp[0], (int)ishp[1], (int)ishp[2], (int)ishp[3], f_h, f_w, mode,
                                        relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage((size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3]);
          check(i8ie_upsample2d_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                   (int)ishp[3], f_h, f_w, mode));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}
// ---- activation / lut (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_activation_table) -------
Tensor<float> activation_f32(Tensor<float>& in, int kind, float param) {
  Tensor<float> out(in.shape);
  check(i8ie_activation_f32(ctx(), kind, param, in.dptr(), out.dptr(), in.size));
  return out;
}
// out = table[in] with the result's (scale, zp): table maps plain bytes to plain bytes
Tensor<u8_t> lut_u8(Tensor<u8_t>& in, const LutBytes& table, float scale, int zp) {
  check_out_qparams("lut", scale, zp);
  need_contents(in);
  const std::vector<ssize_t> shp = in.shape;
  const ssize_t total = in.size;
  const u8_t zp_o = (u8_t)zp;
  // deferred like add's and cat's results: relu(act(..)) is one launch (the relu is max(table[a], zp) on the host), and a
  // consuming conv gets its zero-point border and, where it reads them, re-biased bytes straight from the lookup kernel
  return deferred_one_input(
      in, shp, scale, zp_o, [table, zp_o, shp, total](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        LutBytes t = table;
        if (relu)
          for (u8_t& b : t) b = std::max(b, zp_o);
        std::shared_ptr<Storage> st;
        if (shp.size() == 4) {  // the engine keeps NHWC between layers (and a consumer that asked for a border reads NHWC)
          NhwcCopies copies;
          si = as_engine_nhwc(si, shp, copies);
          st = nhwc_storage(shp, border, zp_o, s8);
          check(i8ie_lut_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                 st->s8 ? 1 : 0, (int)shp[0], (int)shp[1], (int)shp[2], (int)shp[3], t.data()));
        } else {  // rows and other ranks (a flattened NHWC activation goes back to the reference's order): the flat form
          si->to_nchw();
          st = device_storage((size_t)total);
          check(i8ie_lut_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int64_t)total, t.data()));
        }
        return st;
      });
}
Tensor<u8_t> activation_u8(Tensor<u8_t>& in, int kind, float param, float scale, int zp) {
  check_zero_point(zp);
  LutBytes table;
  check(i8ie_activation_table(kind, param, in.scale, in.zero_point, scale, (uint8_t)zp, table.data()));
  return lut_u8(in, table, scale, zp);
}
LutBytes lut_from_array(const py::array_t<uint8_t, py::array::c_style>& a) {
  if (a.size() != 256) throw std::runtime_error("i8ie: lut: the table must hold 256 uint8 entries");
  LutBytes t;
  std::memcpy(t.data(), a.data(), 256);
  return t;
}
// the s8 instantiations of the generic templates (src/functional.cc:5-13, 36-64, registered at :78-82)
Tensor<s8_t> relu_s8(Tensor<s8_t>& in) {
  if (!in.st) return Tensor<s8_t>();  // default-constructed: nothing to do
  Tensor<s8_t> out(in.shape);  // (the generic relu does not carry scale / zero point over: src/functional.cc:7)
  if (in.size > 0) check(i8ie_relu_s8(ctx(), (const int8_t*)in.dptr(), (int8_t*)out.dptr(), in.size));
  return out;
}
Tensor<s8_t> max_pool2d_s8(Tensor<s8_t>& in, ssize_t k, ssize_t s) {
  Tensor<s8_t> out(pool_shape(in, k, s));
  out.scale = in.scale;  // src/functional.cc:43-44
  out.zero_point = in.zero_point;
  check(i8ie_maxpool2d_s8(ctx(), (const int8_t*)in.dptr(), (int8_t*)out.dptr(), (int)in.shape[0], (int)in.shape[1],
                          (int)in.shape[2], (int)in.shape[3], (int)k, (int)s));
  return out;
}
Tensor<float> max_pool2d_f32(Tensor<float>& in, ssize_t k, ssize_t s) {
  Tensor<float> out(pool_shape(in, k, s));
  check(i8ie_maxpool2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2],
                           (int)in.shape[3], (int)k, (int)s));
  return out;
}
template <typename T>
ssize_t layer_norm_axis(const Tensor<T>& x) {
  if (x.shape.size() < 2) throw std::runtime_error("i8ie: layer_norm expects [n, c, h, w], [m, f] or [b, t, f]");
  return x.shape.size() == 4 ? x.shape[1] : x.shape.back();
}
template <typename T>
ssize_t group_norm_channels(const Tensor<T>& x) {
  if (x.shape.size() != 2 && x.shape.size() != 4) throw std::runtime_error("i8ie: group_norm expects [n, c, h, w] or [n, c]");
  return x.shape[1];
}

void bind_ops(py::module_& m) {
  m.def("quantize", &quantize);         // src/pybind11.cc:41-45
  m.def("dequantize", &dequantize);     // src/pybind11.cc:46-48
  m.def("relu", &relu_f32);             // src/functional.cc:73-75
  m.def("relu", &relu_u8);
  m.def("max_pool2d", &max_pool2d_f32);  // src/functional.cc:68-72
  m.def("max_pool2d", &max_pool2d_u8);
  m.def("relu", &relu_s8);               // src/functional.cc:81
  m.def("max_pool2d", &max_pool2d_s8);
  // additive (the reference joins no two tensors): a + b in FP32; the quantized Add of include/i8ie_hip.h on u8 tensors
  m.def("add", &add_f32, py::arg("a"), py::arg("b"));
  m.def("add", &add_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"));
  // additive: a * b in FP32; the quantized Mul of include/i8ie_hip.h on u8 tensors.  b has a's shape or is a's gate
  m.def("mul", &mul_f32, py::arg("a"), py::arg("b"));
  m.def("mul", &mul_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"));
  // additive: the batched matmul of two activation tensors and the softmax over the last axis (include/i8ie_hip.h,
  // i8ie_bmm_u8 / i8ie_softmax_u8); a u8 softmax result always carries scale 1/256, zero point 0
  m.def("matmul", &matmul_f32, py::arg("a"), py::arg("b"), py::arg("transpose_a") = false, py::arg("transpose_b") = false);
  m.def("matmul", &matmul_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"), py::arg("transpose_a") = false,
        py::arg("transpose_b") = false);
  m.def("softmax", &softmax_f32, py::arg("x"));
  m.def("softmax", &softmax_u8, py::arg("x"));
  // additive: fused multi-head attention (include/i8ie_hip.h, i8ie_attention_u8); k and v None: q is a packed qkv tensor
  m.def("attention", [](Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads) { return attention_f32(q, k, v, heads, nullptr); },
        py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"));
  m.def("attention", &attention_u8, py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"),
        py::arg("score_scale"), py::arg("score_zero_point"), py::arg("scale"), py::arg("zero_point"));
  // ... inside win_h x win_w windows of rank-4 maps (i8ie_attention_window_u8); private: i8ie.attention(window=) is the surface
  m.def("_attention_window", [](Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, ssize_t wh, ssize_t ww) {
    return attention_window_f32(q, k, v, heads, wh, ww, nullptr);
  }, py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"), py::arg("win_h"), py::arg("win_w"));
  m.def("_attention_window", &attention_window_u8, py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"),
        py::arg("win_h"), py::arg("win_w"), py::arg("score_scale"), py::arg("score_zero_point"), py::arg("scale"), py::arg("zero_point"));
  // additive: LayerNorm over the channel axis of [n, c, h, w] or the last axis of [m, f] / [b, t, f] (include/i8ie_hip.h,
  // i8ie_layernorm_u8); weight / bias: float32 [channels] or None (ones / zeros); uploaded per call
  m.def("layer_norm", [](Tensor<float>& x, const py::object& w, const py::object& b, float eps) {
    const ssize_t c = layer_norm_axis(x);
    return layer_norm_f32(x, upload_f32(layer_norm_param(w, c, 1.0f, "weight")), upload_f32(layer_norm_param(b, c, 0.0f, "bias")), c, eps);
  }, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("eps"));
  m.def("layer_norm", [](Tensor<u8_t>& x, const py::object& w, const py::object& b, float eps, float scale, int zp) {
    check_out_qparams("layer_norm", scale, zp);
    const ssize_t c = layer_norm_axis(x);
    if (c > 16384) throw std::runtime_error("i8ie: layer_norm: rows of more than 16384 values");
    auto gb = layer_norm_affine(layer_norm_param(w, c, 1.0f, "weight"), layer_norm_param(b, c, 0.0f, "bias"), scale, zp);
    return layer_norm_u8(x, gb.first, gb.second, c, eps, scale, zp);
  }, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("scale"), py::arg("zero_point"));
  // additive: GroupNorm of [n, c, h, w] or [n, c] per image over the pixels and the c / num_groups channels of a group
  // (include/i8ie_hip.h, i8ie_groupnorm_u8_nhwc); weight / bias: float32 [c] or None (ones / zeros); uploaded per call.  The
  // extension's public names are recorded whole in tests/golden/binding_surface.json, which stays as it is: this entry and
  // the _GroupNorm class are private to the i8ie package, which exposes them as i8ie.group_norm and i8ie.GroupNorm
  m.def("_group_norm", [](Tensor<float>& x, ssize_t groups, const py::object& w, const py::object& b, float eps) {
    const ssize_t c = group_norm_channels(x);
    group_norm_pixels(x, groups, c);
    return group_norm_f32(x, upload_f32(layer_norm_param(w, c, 1.0f, "weight")), upload_f32(layer_norm_param(b, c, 0.0f, "bias")), groups, c, eps);
  }, py::arg("x"), py::arg("num_groups"), py::arg("weight"), py::arg("bias"), py::arg("eps"));
  m.def("_group_norm", [](Tensor<u8_t>& x, ssize_t groups, const py::object& w, const py::object& b, float eps, float scale, int zp) {
    check_out_qparams("group_norm", scale, zp);
    const ssize_t c = group_norm_channels(x);
    group_norm_pixels(x, groups, c);
    auto gb = layer_norm_affine(layer_norm_param(w, c, 1.0f, "weight"), layer_norm_param(b, c, 0.0f, "bias"), scale, zp);
    return group_norm_u8(x, gb.first, gb.second, groups, c, eps, scale, zp);
  }, py::arg("x"), py::arg("num_groups"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("scale"), py::arg("zero_point"));
  // additive: inference BatchNorm of [n, c, h, w] or [n, c] with the stored running statistics (include/i8ie_hip.h,
  // i8ie_batchnorm_u8_nhwc); weight / bias: float32 [c] or None (ones / zeros); the affine is computed and uploaded per call.
  // Private like _group_norm (tests/golden/binding_surface.json stays as it is): the i8ie package exposes it as i8ie.batch_norm
  m.def("_batch_norm", [](Tensor<float>& x, const py::object& mean, const py::object& var, const py::object& w, const py::object& b, float eps) {
    if (x.shape.size() != 2 && x.shape.size() != 4) throw std::runtime_error("i8ie: batch_norm expects [n, c, h, w] or [n, c]");
    const ssize_t c = x.shape[1];
    batch_norm_pixels(x, c);
    return batch_norm_f32(x, BatchNormF32{upload_f32(layer_norm_param(w, c, 1.0f, "weight")), upload_f32(layer_norm_param(b, c, 0.0f, "bias")),
                                          upload_f32(layer_norm_param(mean, c, 0.0f, "running_mean")),
                                          upload_f32(layer_norm_param(var, c, 1.0f, "running_var"))}, c, eps);
  }, py::arg("x"), py::arg("running_mean"), py::arg("running_var"), py::arg("weight"), py::arg("bias"), py::arg("eps"));
  m.def("_batch_norm", [](Tensor<u8_t>& x, const py::object& mean, const py::object& var, const py::object& w, const py::object& b, float eps,
                          float scale, int zp) {
    check_out_qparams("batch_norm", scale, zp);
    if (x.shape.size() != 2 && x.shape.size() != 4) throw std::runtime_error("i8ie: batch_norm expects [n, c, h, w] or [n, c]");
    const ssize_t c = x.shape[1];
    batch_norm_pixels(x, c);
    auto gb = batch_norm_affine(layer_norm_param(w, c, 1.0f, "weight"), layer_norm_param(b, c, 0.0f, "bias"),
                                layer_norm_param(mean, c, 0.0f, "running_mean"), layer_norm_param(var, c, 1.0f, "running_var"), eps, scale, zp);
    return batch_norm_u8(x, gb.first, gb.second, c, scale, zp);
  }, py::arg("x"), py::arg("running_mean"), py::arg("running_var"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("scale"),
     py::arg("zero_point"));
  // additive: cat along axis 1 of up to 8 tensors, a copy in FP32; the quantized concat of include/i8ie_hip.h on u8 tensors
  m.def("cat", [](const py::list& tensors) { return cat_f32(cat_list<float>(tensors)); }, py::arg("tensors"));
  m.def("cat", [](const py::list& tensors, float scale, int zp) { return cat_u8(cat_list<u8_t>(tensors), scale, zp); },
        py::arg("tensors"), py::arg("scale"), py::arg("zero_point"));
  // additive: the table-driven activations of include/i8ie_hip.h (kind: I8IE_ACT_*), f in FP32, one table lookup on u8
  // tensors; lut applies a caller's own 256-entry table
  m.def("activation", &activation_f32, py::arg("x"), py::arg("kind"), py::arg("param"));
  m.def("activation", &activation_u8, py::arg("x"), py::arg("kind"), py::arg("param"), py::arg("scale"), py::arg("zero_point"));
  m.def("lut", [](Tensor<u8_t>& x, const py::array_t<uint8_t, py::array::c_style>& table, float scale, int zp) {
    return lut_u8(x, lut_from_array(table), scale, zp);
  }, py::arg("x"), py::arg("table"), py::arg("scale"), py::arg("zero_point"));
  m.def("activation_table", [](int kind, float param, float s_in, int zp_in, float s_out, int zp_out) {
    check_zero_point(zp_in);
    check_zero_point(zp_out);
    py::array_t<uint8_t> out(256);
    check(i8ie_activation_table(kind, param, s_in, (uint8_t)zp_in, s_out, (uint8_t)zp_out, out.mutable_data()));
    return out;
  }, py::arg("kind"), py::arg("param"), py::arg("s_in"), py::arg("zp_in"), py::arg("s_out"), py::arg("zp_out"));
  // additive (the reference has no average pool): round-to-nearest integer mean on u8 tensors, fp32 sum / n on FP32 ones
  m.def("avg_pool2d", [](Tensor<float>& x, ssize_t k, ssize_t s) { return avg_pool_f32(x, k, s, false); }, py::arg("x"),
        py::arg("kernel_size"), py::arg("stride"));
  m.def("avg_pool2d", [](Tensor<u8_t>& x, ssize_t k, ssize_t s) { return avg_pool_u8(x, k, s, false); }, py::arg("x"),
        py::arg("kernel_size"), py::arg("stride"));
  m.def("global_avg_pool2d", [](Tensor<float>& x) { return avg_pool_f32(x, 0, 1, true); }, py::arg("x"));
  m.def("global_avg_pool2d", [](Tensor<u8_t>& x) { return avg_pool_u8(x, 0, 1, true); }, py::arg("x"));
  // additive: the pools with torch's padding and ceil_mode (include/i8ie_hip.h, i8ie_pool_output_size).  Private like
  // _group_norm (tests/golden/binding_surface.json stays as it is): i8ie.max_pool2d / i8ie.avg_pool2d come here where the
  // geometry is not the unpadded floor pool's.  No s8 overload: s8 tensors keep the unpadded pool only
  m.def("_max_pool2d_pad", [](Tensor<float>& x, ssize_t k, ssize_t s, ssize_t p, bool ceil_mode) {
    return pad_pool_f32(x, pad_pool_args(x, k, s, p, ceil_mode, false, false));
  }, py::arg("x"), py::arg("kernel_size"), py::arg("stride"), py::arg("padding"), py::arg("ceil_mode"));
  m.def("_max_pool2d_pad", [](Tensor<u8_t>& x, ssize_t k, ssize_t s, ssize_t p, bool ceil_mode) {
    return pad_pool_u8(x, pad_pool_args(x, k, s, p, ceil_mode, false, false));
  }, py::arg("x"), py::arg("kernel_size"), py::arg("stride"), py::arg("padding"), py::arg("ceil_mode"));
  m.def("_avg_pool2d_pad", [](Tensor<float>& x, ssize_t k, ssize_t s, ssize_t p, bool ceil_mode, bool count_include_pad) {
    return pad_pool_f32(x, pad_pool_args(x, k, s, p, ceil_mode, count_include_pad, true));
  }, py::arg("x"), py::arg("kernel_size"), py::arg("stride"), py::arg("padding"), py::arg("ceil_mode"), py::arg("count_include_pad"));
  m.def("_avg_pool2d_pad", [](Tensor<u8_t>& x, ssize_t k, ssize_t s, ssize_t p, bool ceil_mode, bool count_include_pad) {
    return pad_pool_u8(x, pad_pool_args(x, k, s, p, ceil_mode, count_include_pad, true));
  }, py::arg("x"), py::arg("kernel_size"), py::arg("stride"), py::arg("padding"), py::arg("ceil_mode"), py::arg("count_include_pad"));
  // additive (the reference has no resize op): nearest / bilinear upsampling by integer factors (mode: I8IE_UPSAMPLE_*), exact
  // integers on u8 tensors, the fp32 sequence of include/i8ie_hip.h on FP32 ones
  m.def("upsample", &upsample_f32, py::arg("x"), py::arg("factor_h"), py::arg("factor_w"), py::arg("mode"));
  m.def("upsample", &upsample_u8, py::arg("x"), py::arg("factor_h"), py::arg("factor_w"), py::arg("mode"));
}

}  // namespace i8ie_py
