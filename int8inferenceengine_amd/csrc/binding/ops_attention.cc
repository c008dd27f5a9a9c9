// ops_attention.cc -- matmul, softmax, attention, layer_norm and group_norm.
#include "ops.h"

namespace i8ie_py {

// the [rows, cols] matrix per batch item of a tensor in reference order; `transposed`: the tensor holds [cols, rows]
i8ie_bmm_mat mat_reference_order(void* ptr, ssize_t rows, ssize_t cols, bool transposed) {
  i8ie_bmm_mat m;
  m.ptr = ptr;
  m.batch_stride = (int64_t)rows * cols;
  m.row_stride = transposed ? 1 : (int64_t)cols;
  m.col_stride = transposed ? (int64_t)rows : 1;
  m.s8 = 0;
  return m;
}
Tensor<float> matmul_f32(Tensor<float>& a, Tensor<float>& b, bool ta, bool tb) {
  const MatmulShape s = matmul_shape(a, b, ta, tb);
  Tensor<float> out(s.out);
  i8ie_bmm_args g{};
  g.b = (int)s.b; g.m = (int)s.m; g.n = (int)s.n; g.k = (int)s.k;
  g.a = mat_reference_order(a.dptr(), s.m, s.k, ta);
  g.bm = mat_reference_order(b.dptr(), s.k, s.n, tb);
  g.out = mat_reference_order(out.dptr(), s.m, s.n, false);
  check(i8ie_bmm_f32(ctx(), &g));
  return out;
}
// A u8 operand as it lies.  A rank-4 tensor stored NHWC without a border is physically [n, t, c]: its [c, t] matrix has the
// channel stride 1 and is read through the strides, re-biased or not.  One that exists with a border, and a view under other
// logical dims, goes back to the reference's order first (one layout conversion).
i8ie_bmm_mat mat_of_storage(const std::shared_ptr<Storage>& s, const std::vector<ssize_t>& shp, ssize_t rows, ssize_t cols, bool transposed) {
  const bool nhwc = s->layout == I8IE_LAYOUT_NHWC && s->border == 0 && shp.size() == 4 && s->dn == shp[0] && s->dc == shp[1] &&
                    s->dh == shp[2] && s->dw == shp[3];
  if (!nhwc) {
    s->to_nchw();
    return mat_reference_order(s->device_ptr(), rows, cols, transposed);
  }
  i8ie_bmm_mat m = mat_reference_order(s->device_ptr(), rows, cols, !transposed);  // [t, c] in memory: the transpose of [c, t]
  m.s8 = s->s8 ? 1 : 0;
  return m;
}
Tensor<u8_t> matmul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp, bool ta, bool tb) {
  const MatmulShape s = matmul_shape(a, b, ta, tb);
  check_out_qparams("matmul", scale, zp);
  if (!std::isfinite(a.scale) || !std::isfinite(b.scale)) throw std::runtime_error("i8ie: matmul: an operand's scale is not finite");
  need_contents(a);
  need_contents(b);
  Tensor<u8_t> out = pending_u8(s.out, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> sha = a.shape, shb = b.shape;
  // deferred like add's result: relu(matmul(..)) is one launch, and a rank-4 result gets the border and re-bias the next conv
  // asks for straight from the kernel.  The operands' producers are asked for border 0 (operand_as_it_lies).
  out.pend = make_pend(
      [ops, s, s_a, s_b, zp_a, zp_b, scale, zp_o, sha, shb, ta, tb](bool relu, int border, bool s8) mutable {
        auto ss = resolve_operands(ops.data(), 2);
        i8ie_bmm_args g{};
        g.b = (int)s.b; g.m = (int)s.m; g.n = (int)s.n; g.k = (int)s.k;
        g.a = mat_of_storage(ss[0], sha, s.m, s.k, ta);
        g.bm = mat_of_storage(ss[1], shb, s.k, s.n, tb);
        std::shared_ptr<Storage> st;
        if (s.out.size() == 4) {  // NHWC [b, h + 2B, w + 2B, m]: the n columns are the pixels
          st = nhwc_storage(s.out, border, zp_o, s8);
          g.out.ptr = st->dev;
          g.out.batch_stride = (int64_t)s.m * (s.out[2] + 2 * st->border) * (s.out[3] + 2 * st->border);
          g.out.row_stride = 1;
          g.out.col_stride = (int64_t)s.m;
          g.out.s8 = st->s8 ? 1 : 0;
          g.out_pix_axis = 2;
          g.out_h = (int)s.out[2]; g.out_w = (int)s.out[3]; g.out_border = st->border;
        } else {
          st = device_storage((size_t)(s.b * s.m * s.n));
          g.out = mat_reference_order(st->dev, s.m, s.n, false);
        }
        g.s_a = s_a; g.s_b = s_b; g.s_out = scale;
        g.zp_a = zp_a; g.zp_b = zp_b; g.zp_out = zp_o;
        g.relu = relu ? 1 : 0;
        check(i8ie_bmm_u8(ctx(), &g));
        return st;
      }, {a.pend, b.pend});
  return out;
}
// softmax over the last axis; the u8 result always carries scale 1/256, zero point 0.  A plain flat tensor: an input that is
// not in reference order is converted first.
Tensor<float> softmax_f32(Tensor<float>& x) {
  if (x.shape.empty() || x.size <= 0) throw std::runtime_error("i8ie: softmax: empty tensor");
  Tensor<float> out(x.shape);
  check(i8ie_softmax_f32(ctx(), x.dptr(), out.dptr(), (int64_t)(x.size / x.shape.back()), (int)x.shape.back()));
  return out;
}
Tensor<u8_t> softmax_u8(Tensor<u8_t>& x) {
  if (x.shape.empty() || x.size <= 0) throw std::runtime_error("i8ie: softmax: empty tensor");
  if (x.shape.back() > 65535) throw std::runtime_error("i8ie: softmax: rows of more than 65535 values");
  if (!std::isfinite(x.scale) || x.scale < 0) throw std::runtime_error("i8ie: softmax: the input scale must be finite and not negative");
  const uint8_t* src = x.dptr();
  Tensor<u8_t> out(x.shape);
  out.scale = 1.0f / 256.0f;
  out.zero_point = 0;
  check(i8ie_softmax_u8(ctx(), src, out.dptr(), (int64_t)(x.size / x.shape.back()), (int)x.shape.back(), x.scale));
  return out;
}
// FP32: the composition i8ie_bmm_f32, i8ie_softmax_f32, i8ie_bmm_f32 per head.  Rank-3 operands go through
// i8ie_attention_f32; an FP32 rank-4 tensor is NCHW, its token matrix has the token stride 1, so the same three entries are
// driven through strides here (the bits are the same: i8ie_bmm_f32 adds in ascending k whatever the strides are).  `scores`:
// null, or a [b, heads, tq, tk] tensor that receives the scores before the softmax (what the calibrator samples).
Tensor<float> attention_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, Tensor<float>* scores) {
  const AttnShape s = attention_shape(q, k, v, heads);
  Tensor<float> out(s.out);
  Tensor<float>* ts[3] = {&q, s.packed ? &q : k, s.packed ? &q : v};
  const ssize_t C = s.packed ? 3 * s.c : s.c;
  const bool flat = q.shape.size() == 3 && ts[1]->shape.size() == 3 && ts[2]->shape.size() == 3;
  if (flat) {
    i8ie_attention_args g{};
    g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = (int)s.tq; g.tk = (int)s.tk;
    i8ie_attn_mat* ms[3] = {&g.q, &g.k, &g.v};
    for (int i = 0; i < 3; ++i) {
      const ssize_t t = i == 0 ? s.tq : s.tk;
      *ms[i] = i8ie_attn_mat{ts[i]->dptr() + (s.packed ? i * s.c : 0), (int64_t)t * C, (int64_t)C, 0};
    }
    g.out = i8ie_attn_mat{out.dptr(), (int64_t)s.tq * s.c, (int64_t)s.c, 0};
    g.scores_out_dev = scores ? scores->dptr() : nullptr;
    check(i8ie_attention_f32(ctx(), &g));
    return out;
  }
  // element (batch, token, column) of a tensor with `ch` channels, channel offset `off`: [b, t, ch] or NCHW [b, ch, t]
  auto mat = [](Tensor<float>& t, ssize_t tokens, ssize_t ch, ssize_t off, bool tokens_are_rows) {
    const bool nchw = t.shape.size() == 4;
    i8ie_bmm_mat m;
    m.ptr = t.dptr() + (nchw ? off * tokens : off);
    m.batch_stride = (int64_t)tokens * ch;
    const int64_t tok = nchw ? 1 : (int64_t)ch, col = nchw ? (int64_t)tokens : 1;
    m.row_stride = tokens_are_rows ? tok : col;
    m.col_stride = tokens_are_rows ? col : tok;
    m.s8 = 0;
    return m;
  };
  const ssize_t per_head = s.tq * s.tk;
  Tensor<float> ws({s.b, s.tq, s.tk});
  for (ssize_t h = 0; h < s.heads; ++h) {
    i8ie_bmm_args a{};
    a.b = (int)s.b; a.m = (int)s.tq; a.n = (int)s.tk; a.k = (int)s.d;
    a.a = mat(*ts[0], s.tq, C, h * s.d, true);
    a.bm = mat(*ts[1], s.tk, C, (s.packed ? s.c : 0) + h * s.d, false);
    a.out = i8ie_bmm_mat{ws.dptr(), (int64_t)per_head, (int64_t)s.tk, 1, 0};
    check(i8ie_bmm_f32(ctx(), &a));
    if (scores) {
      a.out = i8ie_bmm_mat{scores->dptr() + h * per_head, (int64_t)(s.heads * per_head), (int64_t)s.tk, 1, 0};
      check(i8ie_bmm_f32(ctx(), &a));
    }
    check(i8ie_softmax_f32(ctx(), ws.dptr(), ws.dptr(), (int64_t)(s.b * s.tq), (int)s.tk));
    i8ie_bmm_args o{};
    o.b = (int)s.b; o.m = (int)s.tq; o.n = (int)s.d; o.k = (int)s.tk;
    o.a = i8ie_bmm_mat{ws.dptr(), (int64_t)per_head, (int64_t)s.tk, 1, 0};
    o.bm = mat(*ts[2], s.tk, C, (s.packed ? 2 * s.c : 0) + h * s.d, true);
    o.out = mat(out, s.tq, s.c, h * s.d, true);
    check(i8ie_bmm_f32(ctx(), &o));
  }
  return out;
}
// A u8 operand as it lies.  A rank-4 tensor stored NHWC without a border is physically [n, t, ch]: read in place, re-biased or
// not.  One that exists with a border, a view under other logical dims and an NCHW tensor take a layout conversion into a
// border-free NHWC buffer (`copies` keeps a temporary alive); a rank-3 tensor is read in the reference's order.
i8ie_attn_mat attn_operand(std::shared_ptr<Storage> s, const std::vector<ssize_t>& shp, ssize_t tokens, ssize_t ch, ssize_t off,
                           NhwcCopies& copies) {
  i8ie_attn_mat m{};
  if (shp.size() == 4) {
    if (s->layout == I8IE_LAYOUT_NHWC && s->border != 0) s->to_nchw();
    s = as_engine_nhwc(s, shp, copies);
    m.s8 = s->s8 ? 1 : 0;
  } else {
    s->to_nchw();
  }
  m.ptr = (uint8_t*)s->device_ptr() + off;
  m.batch_stride = (int64_t)tokens * ch;
  m.token_stride = (int64_t)ch;
  return m;
}
Tensor<u8_t> attention_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v, ssize_t heads, float s_s, int zp_s, float scale, int zp) {
  const AttnShape s = attention_shape(q, k, v, heads);
  check_out_qparams("attention", scale, zp);
  check_out_qparams("attention (scores)", s_s, zp_s);
  std::vector<Tensor<u8_t>> ops{q};  // share the operands' storage / pending launches
  if (!s.packed) {
    ops.push_back(*k);
    ops.push_back(*v);
  }
  for (const auto& t : ops) {
    if (!std::isfinite(t.scale)) throw std::runtime_error("i8ie: attention: an operand's scale is not finite");
    need_contents(t);
  }
  Tensor<u8_t> out = pending_u8(s.out, scale, (u8_t)zp);
  const u8_t zp_o = (u8_t)zp, zs = (u8_t)zp_s;
  // deferred like matmul's result: relu(attention(..)) is one launch, and a rank-4 result gets the border and re-bias the next
  // conv asks for straight from the kernel.  The operands' producers are asked for border 0 (operand_as_it_lies).
  auto run = [ops, s, s_s, zs, scale, zp_o](bool relu, int border, bool s8) mutable {
    auto ss = resolve_operands(ops.data(), ops.size());
    NhwcCopies copies;
    i8ie_attention_args g{};
    g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = (int)s.tq; g.tk = (int)s.tk;
    const ssize_t C = s.packed ? 3 * s.c : s.c;
    const Tensor<u8_t>&tq = ops[0], &tk = ops[s.packed ? 0 : 1], &tv = ops[s.packed ? 0 : 2];
    g.q = attn_operand(ss[0], tq.shape, s.tq, C, 0, copies);
    g.k = attn_operand(ss[s.packed ? 0 : 1], tk.shape, s.tk, C, s.packed ? s.c : 0, copies);
    g.v = attn_operand(ss[s.packed ? 0 : 2], tv.shape, s.tk, C, s.packed ? 2 * s.c : 0, copies);
    g.s_q = tq.scale; g.s_k = tk.scale; g.s_v = tv.scale; g.s_s = s_s; g.s_o = scale;
    g.zp_q = tq.zero_point; g.zp_k = tk.zero_point; g.zp_v = tv.zero_point; g.zp_s = zs; g.zp_o = zp_o;
    g.relu = relu ? 1 : 0;
    std::shared_ptr<Storage> st;
    if (s.out.size() == 4) {  // NHWC [b, h + 2B, w + 2B, c]: the tq tokens are the pixels
      st = nhwc_storage(s.out, border, zp_o, s8);
      g.out = i8ie_attn_mat{st->dev, (int64_t)s.c * (s.out[2] + 2 * st->border) * (s.out[3] + 2 * st->border), (int64_t)s.c, st->s8 ? 1 : 0};
      g.out_h = (int)s.out[2]; g.out_w = (int)s.out[3]; g.out_border = st->border;
    } else {
      st = device_storage((size_t)(s.b * s.tq * s.c));
      g.out = i8ie_attn_mat{st->dev, (int64_t)s.tq * s.c, (int64_t)s.c, 0};
    }
    check(i8ie_attention_u8(ctx(), &g));
    return st;
  };
  if (s.packed) out.pend = make_pend(run, {q.pend});
  else out.pend = make_pend(run, {q.pend, k->pend, v->pend});
  return out;
}
// FP32, windowed: i8ie_attention_window_f32 on the NCHW tensors (part, i8ie_attention_f32, unpart)
Tensor<float> attention_window_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, ssize_t wh, ssize_t ww,
                                   Tensor<float>* scores) {
  const AttnWindowShape s = attention_window_shape(q, k, v, heads, wh, ww);
  Tensor<float> out(s.out);
  Tensor<float>* ts[3] = {&q, s.packed ? &q : k, s.packed ? &q : v};
  const ssize_t C = s.packed ? 3 * s.c : s.c, hw = s.h * s.w;
  i8ie_attention_args g{};
  g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = g.tk = (int)s.tq;
  i8ie_attn_mat* ms[3] = {&g.q, &g.k, &g.v};
  for (int i = 0; i < 3; ++i) *ms[i] = i8ie_attn_mat{ts[i]->dptr() + (s.packed ? i * s.c * hw : 0), (int64_t)C * hw, (int64_t)hw, 0};
  g.out = i8ie_attn_mat{out.dptr(), (int64_t)s.c * hw, (int64_t)hw, 0};
  g.out_h = (int)s.h; g.out_w = (int)s.w;
  g.scores_out_dev = scores ? scores->dptr() : nullptr;
  i8ie_attention_window win{(int)s.h, (int)s.w, (int)s.wh, (int)s.ww, 0, 0, 0};
  check(i8ie_attention_window_f32(ctx(), &g, &win));
  return out;
}
// A u8 map operand of the windowed form as it lies: NHWC under its own dims is read in place, border and re-bias included
// (the kernel walks the interior); a view under other logical dims and an NCHW tensor take as_engine_nhwc's conversion.
i8ie_attn_mat attn_window_operand(std::shared_ptr<Storage> s, const std::vector<ssize_t>& shp, ssize_t ch, ssize_t off, NhwcCopies& copies,
                                  int* border) {
  s = as_engine_nhwc(s, shp, copies);
  *border = s->border;
  i8ie_attn_mat m{};
  m.ptr = (uint8_t*)s->device_ptr() + off;
  m.batch_stride = (int64_t)ch * (shp[2] + 2 * s->border) * (shp[3] + 2 * s->border);
  m.token_stride = (int64_t)ch;
  m.s8 = s->s8 ? 1 : 0;
  return m;
}
Tensor<u8_t> attention_window_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v, ssize_t heads, ssize_t wh, ssize_t ww, float s_s, int zp_s,
                                 float scale, int zp) {
  const AttnWindowShape s = attention_window_shape(q, k, v, heads, wh, ww);
  check_out_qparams("attention", scale, zp);
  check_out_qparams("attention (scores)", s_s, zp_s);
  std::vector<Tensor<u8_t>> ops{q};  // share the operands' storage / pending launches
  if (!s.packed) {
    ops.push_back(*k);
    ops.push_back(*v);
  }
  for (const auto& t : ops) {
    if (!std::isfinite(t.scale)) throw std::runtime_error("i8ie: attention: an operand's scale is not finite");
    need_contents(t);
  }
  Tensor<u8_t> out = pending_u8(s.out, scale, (u8_t)zp);
  const u8_t zp_o = (u8_t)zp, zs = (u8_t)zp_s;
  // deferred like the global form's result (relu folds in, the consumer's border and re-bias come from the kernel); an operand
  // that another consumer made bordered is read with its border: no conversion launch
  auto run = [ops, s, s_s, zs, scale, zp_o](bool relu, int border, bool s8) mutable {
    auto ss = resolve_operands(ops.data(), ops.size());
    NhwcCopies copies;
    i8ie_attention_args g{};
    i8ie_attention_window win{(int)s.h, (int)s.w, (int)s.wh, (int)s.ww, 0, 0, 0};
    g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = g.tk = (int)s.tq;
    const ssize_t C = s.packed ? 3 * s.c : s.c;
    const Tensor<u8_t>&tq = ops[0], &tk = ops[s.packed ? 0 : 1], &tv = ops[s.packed ? 0 : 2];
    g.q = attn_window_operand(ss[0], tq.shape, C, 0, copies, &win.q_border);
    g.k = attn_window_operand(ss[s.packed ? 0 : 1], tk.shape, C, s.packed ? s.c : 0, copies, &win.k_border);
    g.v = attn_window_operand(ss[s.packed ? 0 : 2], tv.shape, C, s.packed ? 2 * s.c : 0, copies, &win.v_border);
    g.s_q = tq.scale; g.s_k = tk.scale; g.s_v = tv.scale; g.s_s = s_s; g.s_o = scale;
    g.zp_q = tq.zero_point; g.zp_k = tk.zero_point; g.zp_v = tv.zero_point; g.zp_s = zs; g.zp_o = zp_o;
    g.relu = relu ? 1 : 0;
    std::shared_ptr<Storage> st = nhwc_storage(s.out, border, zp_o, s8);
    g.out = i8ie_attn_mat{st->dev, (int64_t)s.c * (s.h + 2 * st->border) * (s.w + 2 * st->border), (int64_t)s.c, st->s8 ? 1 : 0};
    g.out_h = (int)s.h; g.out_w = (int)s.w; g.out_border = st->border;
    check(i8ie_attention_window_u8(ctx(), &g, &win));
    return st;
  };
  if (s.packed) out.pend = make_pend(run, {q.pend});
  else out.pend = make_pend(run, {q.pend, k->pend, v->pend});
  return out;
}
Tensor<float> layer_norm_f32(Tensor<float>& x, const std::shared_ptr<Storage>& gamma, const std::shared_ptr<Storage>& beta, ssize_t channels,
                             float eps) {
  const auto ri = layer_norm_rows(x, channels);
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: layer_norm: eps must be positive and finite");
  Tensor<float> out(x.shape);
  check(i8ie_layernorm_f32(ctx(), x.dptr(), out.dptr(), ri.first, (int)channels, (const float*)gamma->dev, (const float*)beta->dev, eps,
                           ri.second));
  return out;
}
// g, b: the device arrays of i8ie_layernorm_affine for (scale, zp), kept alive by the recorded launch
Tensor<u8_t> layer_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t channels, float eps,
                           float scale, int zp) {
  check_out_qparams("layer_norm", scale, zp);
  need_contents(in);
  const int64_t rows = layer_norm_rows(in, channels).first;
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: layer_norm: eps must be positive and finite");
  if (!(in.scale > 0) || !std::isfinite(in.scale)) throw std::runtime_error("i8ie: layer_norm: the input scale must be positive and finite");
  const std::vector<ssize_t> shp = in.shape;
  const float s_in = in.scale;
  const u8_t zp_o = (u8_t)zp;
  const int C = (int)channels;
  // deferred like add's and the activations' results: relu(ln(..)) is one launch, a consuming conv gets its zero-point border
  // and, where it reads them, re-biased bytes straight from the kernel, and several consumers share one launch (PendNode)
  return deferred_one_input(
      in, shp, scale, zp_o, [g, b, shp, rows, s_in, eps, zp_o, C](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        std::shared_ptr<Storage> st;
        if (shp.size() == 4) {
          NhwcCopies copies;
          si = as_engine_nhwc(si, shp, copies);
          st = nhwc_storage(shp, border, zp_o, s8);
          check(i8ie_layernorm_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                       st->s8 ? 1 : 0, (int)shp[0], C, (int)shp[2], (int)shp[3], (const float*)g->dev, (const float*)b->dev,
                                       s_in, eps, relu ? 1 : 0, zp_o));
        } else {  // rows (a flattened NHWC activation goes back to the reference's order; one pixel per image is in it already)
          if (si->layout == I8IE_LAYOUT_NHWC && si->dh * si->dw == 1 && si->border == 0) si->unbias();
          else si->to_nchw();
          st = device_storage((size_t)rows * C);
          check(i8ie_layernorm_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, rows, C, (const float*)g->dev,
                                  (const float*)b->dev, s_in, eps, relu ? 1 : 0, zp_o));
        }
        return st;
      });
}
Tensor<float> group_norm_f32(Tensor<float>& x, const std::shared_ptr<Storage>& gamma, const std::shared_ptr<Storage>& beta, ssize_t groups,
                             ssize_t channels, float eps) {
  const int64_t hw = group_norm_pixels(x, groups, channels);
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: group_norm: eps must be positive and finite");
  Tensor<float> out(x.shape);
  check(i8ie_groupnorm_f32(ctx(), x.dptr(), out.dptr(), (int)x.shape[0], (int)channels, (int)groups, hw, (const float*)gamma->dev,
                           (const float*)beta->dev, eps));
  return out;
}
// g, b: the device arrays of i8ie_layernorm_affine for (scale, zp), kept alive by the recorded launch
Tensor<u8_t> group_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t groups,
                           ssize_t channels, float eps, float scale, int zp) {
  check_out_qparams("group_norm", scale, zp);
  need_contents(in);
  group_norm_pixels(in, groups, channels);
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: group_norm: eps must be positive and finite");
  if (!(in.scale > 0) || !std::isfinite(in.scale)) throw std::runtime_error("i8ie: group_norm: the input scale must be positive and finite");
  const std::vector<ssize_t> shp = in.shape;
  const float s_in = in.scale;
  const u8_t zp_o = (u8_t)zp;
  const int C = (int)channels, G = (int)groups;
  // deferred like layer_norm's result: relu(gn(..)) is one launch (two in the split form), a consuming conv gets its zero-point
  // border and, where it reads them, re-biased bytes straight from the kernel
  return deferred_one_input(
      in, shp, scale, zp_o, [g, b, shp, s_in, eps, zp_o, C, G](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        const int n = (int)shp[0], h = shp.size() == 4 ? (int)shp[2] : 1, w = shp.size() == 4 ? (int)shp[3] : 1;
        std::shared_ptr<Storage> st;
        int in_border = 0, in_s8 = 0;
        if (shp.size() == 4) {
          NhwcCopies copies;
          si = as_engine_nhwc(si, shp, copies);
          st = nhwc_storage(shp, border, zp_o, s8);
          in_border = si->border;
          in_s8 = si->s8 ? 1 : 0;
        } else {  // [n, c] rows: one pixel per image (a flattened NHWC activation of one pixel per image is in that order already)
          if (si->layout == I8IE_LAYOUT_NHWC && si->dh * si->dw == 1 && si->border == 0) si->unbias();
          else si->to_nchw();
          st = device_storage((size_t)n * C);
        }
        // the split form's partial sums come from the allocator the result came from (stream-ordered, so a capture sees no
        // allocation of its own kind); the block goes back behind the two launches
        const int64_t ws_bytes = i8ie_groupnorm_workspace_bytes(n, C, G, h, w);
        if (ws_bytes < 0) check(-1);
        std::shared_ptr<Storage> ws = ws_bytes > 0 ? device_storage((size_t)ws_bytes) : nullptr;
        check(i8ie_groupnorm_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), in_border, in_s8, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, n,
                                     C, G, h, w, (const float*)g->dev, (const float*)b->dev, s_in, eps, relu ? 1 : 0, zp_o,
                                     ws ? ws->dev : nullptr));
        return st;
      });
}
Tensor<float> batch_norm_f32(Tensor<float>& x, const BatchNormF32& p, ssize_t channels, float eps) {
  const int64_t hw = batch_norm_pixels(x, channels);
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: batch_norm: eps must be positive and finite");
  Tensor<float> out(x.shape);
  check(i8ie_batchnorm_f32(ctx(), x.dptr(), out.dptr(), (int64_t)x.shape[0] * hw, (int)channels, hw, (const float*)p.gamma->dev,
                           (const float*)p.beta->dev, (const float*)p.mean->dev, (const float*)p.var->dev, eps));
  return out;
}
// g, b: the device arrays of i8ie_batchnorm_affine for (scale, zp), kept alive by the recorded launch
Tensor<u8_t> batch_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t channels, float scale,
                           int zp) {
  check_out_qparams("batch_norm", scale, zp);
  need_contents(in);
  const int64_t hw = batch_norm_pixels(in, channels);
  if (!std::isfinite(in.scale) || !std::isfinite(255.0f * in.scale)) throw std::runtime_error("i8ie: batch_norm: the input scale must be finite");
  const std::vector<ssize_t> shp = in.shape;
  const float s_in = in.scale;
  const u8_t zp_i = in.zero_point, zp_o = (u8_t)zp;
  const int C = (int)channels;
  // deferred like layer_norm's result: relu(bn(..)) is one launch, a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the kernel, and several consumers share one launch (PendNode)
  return deferred_one_input(
      in, shp, scale, zp_o, [g, b, shp, hw, s_in, zp_i, zp_o, C](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        const int64_t n = (int64_t)shp[0];
        std::shared_ptr<Storage> st;
        if (shp.size() == 4) {
          // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
          if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != shp[0] || si->dc != shp[1] || si->dh != shp[2] || si->dw != shp[3])) si->to_nchw();
          if (si->layout == I8IE_LAYOUT_NHWC) {
            st = nhwc_storage(shp, border, zp_o, s8);
            check(i8ie_batchnorm_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                         st->s8 ? 1 : 0, (int)n, C, (int)shp[2], (int)shp[3], (const float*)g->dev, (const float*)b->dev, s_in,
                                         zp_i, relu ? 1 : 0, zp_o));
            return st;
          }
        } else {  // [n, c] rows (a flattened NHWC activation of one pixel per image is in that order already)
          if (si->layout == I8IE_LAYOUT_NHWC && si->dh * si->dw == 1 && si->border == 0) si->unbias();
          else si->to_nchw();
        }
        // reference order (a user-made tensor, an im2col-route conv's result, rows): the flat entry, no layout conversion
        st = device_storage((size_t)(n * C * hw));
        check(i8ie_batchnorm_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, n * hw, C, hw, (const float*)g->dev,
                                (const float*)b->dev, s_in, zp_i, relu ? 1 : 0, zp_o));
        return st;
      });
}
// (g, b) of i8ie_batchnorm_affine on the device
std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>> batch_norm_affine(const std::vector<float>& gamma, const std::vector<float>& beta,
                                                                                 const std::vector<float>& mean, const std::vector<float>& var,
                                                                                 float eps, float scale, int zp) {
  std::vector<float> g(gamma.size()), b(gamma.size());
  check(i8ie_batchnorm_affine(gamma.data(), beta.data(), mean.data(), var.data(), (int)gamma.size(), eps, scale, (uint8_t)zp, g.data(), b.data()));
  return {upload_f32(g), upload_f32(b)};
}
std::vector<float> layer_norm_param(const py::object& a, ssize_t channels, float fill, const char* what) {
  if (a.is_none()) return std::vector<float>((size_t)channels, fill);
  F32Array v = F32Array::ensure(a);
  if (!v || v.ndim() != 1 || v.shape(0) != channels)
    throw std::runtime_error(std::string("i8ie: layer_norm: ") + what + " must hold one float per normalised value");
  return std::vector<float>(v.data(), v.data() + v.size());
}
// (g, b) of i8ie_layernorm_affine on the device
std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>> layer_norm_affine(const std::vector<float>& gamma, const std::vector<float>& beta,
                                                                                 float scale, int zp) {
  std::vector<float> g(gamma.size()), b(gamma.size());
  check(i8ie_layernorm_affine(gamma.data(), beta.data(), (int)gamma.size(), scale, (uint8_t)zp, g.data(), b.data()));
  return {upload_f32(g), upload_f32(b)};
}

}  // namespace i8ie_py
