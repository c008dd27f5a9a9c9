// ops_join.cc -- add, mul and cat: the ops that join tensors.
#include "ops.h"

namespace i8ie_py {

// ---- add (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_add_u8) ----------------------------
Tensor<float> add_f32(Tensor<float>& a, Tensor<float>& b) {
  if (a.shape != b.shape) throw std::runtime_error("i8ie: add: shapes differ (there is no broadcasting)");
  Tensor<float> out(a.shape);
  check(i8ie_add_f32(ctx(), a.dptr(), b.dptr(), out.dptr(), a.size));
  return out;
}
// The deferred result of a two-operand op on operands of one shape (add, the equal-shape mul), through the op's flat and NHWC
// C entries.  Deferred like max_pool2d's result: relu(op(..)) is one launch, and a consuming conv gets its zero-point border
// and, where it reads them, re-biased bytes straight from the op's kernel.  The caller has checked its arguments.
using PairFlatFn = decltype(&i8ie_add_u8);
using PairNhwcFn = decltype(&i8ie_add_u8_nhwc);
Tensor<u8_t> equal_shape_u8(PairFlatFn flat, PairNhwcFn nhwc, Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  Tensor<u8_t> out = pending_u8(a.shape, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> shp = a.shape;
  const ssize_t n = a.size;
  out.pend = make_pend(
      [flat, nhwc, ops, s_a, s_b, zp_a, zp_b, scale, zp_o, shp, n](bool relu, int border, bool s8) mutable {
        auto ss = resolve_operands(ops.data(), 2);
        NhwcCopies copies;
        reconcile_pair(ss[0], ss[1], shp, copies);
        Storage *sa = ss[0].get(), *sb = ss[1].get();
        std::shared_ptr<Storage> st;
        if (sa->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage({sa->dn, sa->dc, sa->dh, sa->dw}, shp.size() == 4 ? border : 0, zp_o, s8);
          check(nhwc(ctx(), (const uint8_t*)sa->device_ptr(), sa->border, sa->s8 ? 1 : 0, (const uint8_t*)sb->device_ptr(), sb->border,
                     sb->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, sa->dn, sa->dc, sa->dh, sa->dw, s_a, zp_a, s_b, zp_b,
                     scale, zp_o, relu ? 1 : 0));
        } else {
          st = device_storage((size_t)n);
          check(flat(ctx(), (const uint8_t*)sa->device_ptr(), (const uint8_t*)sb->device_ptr(), (uint8_t*)st->dev, (int64_t)n, s_a, zp_a,
                     s_b, zp_b, scale, zp_o, relu ? 1 : 0));
        }
        // (the operands are released with the closure's copies, as a layer's input is)
        return st;
      }, {a.pend, b.pend});
  return out;
}
Tensor<u8_t> add_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  if (a.shape != b.shape) throw std::runtime_error("i8ie: add: shapes differ (there is no broadcasting)");
  check_out_qparams("add", scale, zp);  // (add alone checks neither the operands' scales nor for an empty tensor)
  return equal_shape_u8(i8ie_add_u8, i8ie_add_u8_nhwc, a, b, scale, zp);
}
Tensor<float> mul_f32(Tensor<float>& a, Tensor<float>& b) {
  const bool gate = mul_is_gate(a, b);
  Tensor<float> out(a.shape);
  check(i8ie_mul_f32(ctx(), a.dptr(), b.dptr(), out.dptr(), a.size, gate ? (int64_t)(a.shape[2] * a.shape[3]) : 0));
  return out;
}
// i8ie_mul_u8_nhwc on operands of one shape, with the add's argument list
int mul_u8_nhwc_equal(i8ie_ctx* c, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8, uint8_t* out,
                      int out_border, int out_s8, int n, int ch, int h, int w, float s_a, uint8_t zp_a, float s_b, uint8_t zp_b,
                      float s_out, uint8_t zp_out, int relu) {
  return i8ie_mul_u8_nhwc(c, a, a_border, a_s8, b, b_border, b_s8, 0, out, out_border, out_s8, n, ch, h, w, s_a, zp_a, s_b, zp_b, s_out,
                          zp_out, relu);
}
Tensor<u8_t> mul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  const bool gate = mul_is_gate(a, b);
  check_out_qparams("mul", scale, zp);
  if (!std::isfinite(a.scale) || !std::isfinite(b.scale)) throw std::runtime_error("i8ie: mul: an operand's scale is not finite");
  need_contents(a);
  need_contents(b);
  if (!gate) return equal_shape_u8(i8ie_mul_u8, mul_u8_nhwc_equal, a, b, scale, zp);
  Tensor<u8_t> out = pending_u8(a.shape, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> shp = a.shape;
  // deferred like the equal-shape result
  out.pend = make_pend(
      [ops, s_a, s_b, zp_a, zp_b, scale, zp_o, shp](bool relu, int border, bool s8) mutable {
        // (the gate of a squeeze-and-excitation block is f(a), still pending: it launches first, and a is read as it lies)
        auto ss = resolve_operands(ops.data(), 2);
        NhwcCopies copies;
        std::shared_ptr<Storage> sa = as_engine_nhwc(ss[0], shp, copies);
        std::shared_ptr<Storage>& sb = ss[1];
        // the gate as its producer left it: an [n, c, 1, 1] NHWC buffer with its border and re-bias, or plain rows (an
        // NCHW [n, c, 1, 1] tensor is the same bytes)
        const bool g_nhwc = sb->layout == I8IE_LAYOUT_NHWC && sb->dn == shp[0] && sb->dc == shp[1] && sb->dh == 1 && sb->dw == 1;
        if (!g_nhwc) sb->to_nchw();
        std::shared_ptr<Storage> st = nhwc_storage(shp, border, zp_o, s8);
        check(i8ie_mul_u8_nhwc(ctx(), (const uint8_t*)sa->device_ptr(), sa->border, sa->s8 ? 1 : 0, (const uint8_t*)sb->device_ptr(),
                               g_nhwc ? sb->border : 0, g_nhwc && sb->s8 ? 1 : 0, 1, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0,
                               (int)shp[0], (int)shp[1], (int)shp[2], (int)shp[3], s_a, zp_a, s_b, zp_b, scale, zp_o, relu ? 1 : 0));
        return st;
      }, {a.pend, b.pend});
  return out;
}
template <typename T>
ssize_t cat_run_len(const Tensor<T>& t) { return t.shape.size() == 4 ? t.shape[1] * t.shape[2] * t.shape[3] : t.shape[1]; }
Tensor<float> cat_f32(std::vector<Tensor<float>> ts) {
  Tensor<float> out(cat_shape(ts));
  const float* in[I8IE_CONCAT_MAX_INPUTS];
  int64_t len[I8IE_CONCAT_MAX_INPUTS];
  for (size_t i = 0; i < ts.size(); ++i) {
    in[i] = ts[i].dptr();
    len[i] = (int64_t)cat_run_len(ts[i]);
  }
  check(i8ie_concat_f32(ctx(), (int)ts.size(), in, len, out.dptr(), (int64_t)out.shape[0]));
  return out;
}
Tensor<u8_t> cat_u8(std::vector<Tensor<u8_t>> ts, float scale, int zp) {
  const std::vector<ssize_t> shp = cat_shape(ts);
  check_out_qparams("cat", scale, zp);
  for (const auto& t : ts)
    if (!std::isfinite(t.scale)) throw std::runtime_error("i8ie: cat: an input's scale is not finite");
  Tensor<u8_t> out = pending_u8(shp, scale, (u8_t)zp);
  const u8_t zp_o = (u8_t)zp;
  const ssize_t total = out.size;
  // deferred like add's result: relu(cat(..)) is one launch, and a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the concat kernel.  (the closure's copies share the inputs' storage / launches)
  auto node = make_pend([ts, scale, zp_o, shp, total](bool relu, int border, bool s8) mutable {
    const int k = (int)ts.size();
    auto ss = resolve_operands(ts.data(), ts.size());
    bool any_nhwc = false;
    for (int i = 0; i < k; ++i) any_nhwc = any_nhwc || ss[i]->layout == I8IE_LAYOUT_NHWC;
    const uint8_t* in[I8IE_CONCAT_MAX_INPUTS];
    float s_in[I8IE_CONCAT_MAX_INPUTS];
    uint8_t zp_in[I8IE_CONCAT_MAX_INPUTS];
    for (int i = 0; i < k; ++i) {
      s_in[i] = ts[i].scale;
      zp_in[i] = ts[i].zero_point;
    }
    std::shared_ptr<Storage> st;
    if (shp.size() == 4 && any_nhwc) {  // the engine keeps NHWC between layers (and a consumer that asked for a border reads NHWC)
      int c_in[I8IE_CONCAT_MAX_INPUTS], b_in[I8IE_CONCAT_MAX_INPUTS], x_in[I8IE_CONCAT_MAX_INPUTS];
      NhwcCopies copies;  // (the same tensor again takes its conversion too)
      for (int i = 0; i < k; ++i) {
        ss[i] = as_engine_nhwc(ss[i], ts[i].shape, copies);
        in[i] = (const uint8_t*)ss[i]->device_ptr();
        c_in[i] = (int)ts[i].shape[1];
        b_in[i] = ss[i]->border;
        x_in[i] = ss[i]->s8 ? 1 : 0;
      }
      st = nhwc_storage(shp, border, zp_o, s8);
      check(i8ie_concat_u8_nhwc(ctx(), k, in, c_in, b_in, x_in, s_in, zp_in, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, (int)shp[0],
                                (int)shp[2], (int)shp[3], scale, zp_o, relu ? 1 : 0));
    } else {  // NCHW tensors and [m, f_i] rows (a flattened NHWC activation goes back to the reference's order): the run form
      int64_t len[I8IE_CONCAT_MAX_INPUTS];
      for (int i = 0; i < k; ++i) {
        ss[i]->to_nchw();
        in[i] = (const uint8_t*)ss[i]->device_ptr();
        len[i] = (int64_t)cat_run_len(ts[i]);
      }
      st = device_storage((size_t)total);
      check(i8ie_concat_u8(ctx(), k, in, len, s_in, zp_in, (uint8_t*)st->dev, (int64_t)shp[0], scale, zp_o, relu ? 1 : 0));
    }
    // (the inputs are released with the closure's copies, as a layer's input is)
    return st;
  });
  for (const auto& t : ts)
    if (t.pend) node->inputs.push_back(t.pend);
  out.pend = node;
  return out;
}

}  // namespace i8ie_py
