// ops.h -- the functional ops: the shape rules the layer classes share with them (templates) and the ops the layers call.
#pragma once
#include "operands.h"

namespace i8ie_py {

// ---- mul (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_mul_u8) ----------------------------
// b has a's shape (false), or is a gate [n, c, 1, 1] / [n, c] of a rank-4 a (true); anything else is a RuntimeError
// (before any device call).  Only the second operand broadcasts.
template <typename T>
bool mul_is_gate(const Tensor<T>& a, const Tensor<T>& b) {
  if (a.shape.size() != 2 && a.shape.size() != 4) throw std::runtime_error("i8ie: mul: the first operand must be [n, c, h, w] or [m, f]");
  for (ssize_t d : a.shape)
    if (d <= 0) throw std::runtime_error("i8ie: mul: empty tensor");
  if (a.shape == b.shape) return false;
  const bool gate = a.shape.size() == 4 && b.shape.size() >= 2 && b.shape[0] == a.shape[0] && b.shape[1] == a.shape[1] &&
                    (b.shape.size() == 2 || (b.shape.size() == 4 && b.shape[2] == 1 && b.shape[3] == 1));
  if (!gate)
    throw std::runtime_error("i8ie: mul: the second operand must have the first one's shape or be its gate [n, c, 1, 1] / [n, c] "
                             "(no other broadcasting)");
  return true;
}
// ---- matmul / softmax (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_bmm_u8, i8ie_softmax_u8) ----
// Operands are rank 3 [b, r, c], or rank 4 [n, c, h, w] counted as [n, c, h * w] (the last two dimensions merged in reference
// order).  a is [b, m, k] ([b, k, m] when transpose_a), b is [b, k, n] ([b, n, k] when transpose_b); the same b on both sides.
// The result is [b, m, n] -- or [b, m, h, w] when a was given as rank 4 [b, m, h, w], untransposed, and n == h * w.  Anything
// else is a RuntimeError (before any device call).
struct MatmulShape {
  ssize_t b = 0, m = 0, n = 0, k = 0;
  std::vector<ssize_t> out;
};
template <typename T>
MatmulShape matmul_shape(const Tensor<T>& a, const Tensor<T>& b, bool ta, bool tb) {
  auto rc = [](const Tensor<T>& t, const char* which) {
    if (t.shape.size() != 3 && t.shape.size() != 4)
      throw std::runtime_error(std::string("i8ie: matmul: the ") + which + " operand must be [b, r, c] or [n, c, h, w]");
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: matmul: empty tensor");
    return std::array<ssize_t, 3>{t.shape[0], t.shape[1], t.shape.size() == 4 ? t.shape[2] * t.shape[3] : t.shape[2]};
  };
  const auto A = rc(a, "first"), B = rc(b, "second");
  MatmulShape s;
  s.b = A[0];
  s.m = ta ? A[2] : A[1];
  s.k = ta ? A[1] : A[2];
  s.n = tb ? B[1] : B[2];
  if (B[0] != s.b) throw std::runtime_error("i8ie: matmul: the operands' batch sizes differ (there is no broadcasting)");
  if ((tb ? B[2] : B[1]) != s.k) throw std::runtime_error("i8ie: matmul: the operands' inner dimensions differ");
  if (s.k > 32768) throw std::runtime_error("i8ie: matmul: inner dimension above 32768");
  if (a.shape.size() == 4 && !ta && s.n == a.shape[2] * a.shape[3]) s.out = {s.b, s.m, a.shape[2], a.shape[3]};
  else s.out = {s.b, s.m, s.n};
  return s;
}
// ---- attention (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_attention_u8) -----------------------
// Operands are rank 3 [b, t, c], or rank 4 [n, c, h, w] counted as [n, h * w, c] (the engine's NHWC storage as it lies).  q is
// [b, tq, c], k and v are [b, tk, c], c = heads * d; or one packed tensor with 3 * heads * d channels (k == v == nullptr): q, k, v
// are then its channels [0, c), [c, 2c), [2c, 3c).  The result has q's rank: [b, tq, c] or [n, c, h, w].  Anything else is a
// RuntimeError (before any device call).
struct AttnShape {
  ssize_t b = 0, heads = 0, d = 0, c = 0, tq = 0, tk = 0;
  bool packed = false;
  std::vector<ssize_t> out;
};
template <typename T>
AttnShape attention_shape(const Tensor<T>& q, const Tensor<T>* k, const Tensor<T>* v, ssize_t heads) {
  auto btc = [](const Tensor<T>& t, const char* which) {
    if (t.shape.size() != 3 && t.shape.size() != 4)
      throw std::runtime_error(std::string("i8ie: attention: ") + which + " must be [b, t, c] or [n, c, h, w]");
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: attention: empty tensor");
    if (t.shape.size() == 4) return std::array<ssize_t, 3>{t.shape[0], t.shape[2] * t.shape[3], t.shape[1]};
    return std::array<ssize_t, 3>{t.shape[0], t.shape[1], t.shape[2]};
  };
  if ((k == nullptr) != (v == nullptr)) throw std::runtime_error("i8ie: attention takes q, k and v, or one packed qkv tensor");
  if (heads < 1) throw std::runtime_error("i8ie: attention: heads must be >= 1");
  AttnShape s;
  s.heads = heads;
  s.packed = k == nullptr;
  const auto Q = btc(q, s.packed ? "qkv" : "q");
  s.b = Q[0];
  s.tq = s.tk = Q[1];
  if (s.packed) {
    if (Q[2] % (3 * heads) != 0) throw std::runtime_error("i8ie: attention: a packed qkv tensor needs 3 * heads * d channels");
    s.c = Q[2] / 3;
  } else {
    const auto K = btc(*k, "k"), V = btc(*v, "v");
    if (K[0] != s.b || V[0] != s.b) throw std::runtime_error("i8ie: attention: the operands' batch sizes differ (there is no broadcasting)");
    if (K[2] != Q[2] || V[2] != Q[2]) throw std::runtime_error("i8ie: attention: q, k and v must have the same channel count");
    if (K[1] != V[1]) throw std::runtime_error("i8ie: attention: k and v must have the same token count");
    if (Q[2] % heads != 0) throw std::runtime_error("i8ie: attention: the channel count is not heads * d");
    s.c = Q[2];
    s.tk = K[1];
  }
  s.d = s.c / heads;
  if (s.tk > 32768) throw std::runtime_error("i8ie: attention: more than 32768 key tokens");
  if (q.shape.size() == 4) s.out = {s.b, s.c, q.shape[2], q.shape[3]};
  else s.out = {s.b, s.tq, s.c};
  return s;
}
// The windowed form (include/i8ie_hip.h, i8ie_attention_window_u8): every operand is a rank-4 map [n, c, h, w] of one h x w,
// the window (wh, ww) divides it and holds at most 32768 pixels.  b is the image count, tq == tk == wh * ww, and `windows` the
// windows per image.  Anything else is a RuntimeError (before any device call).
struct AttnWindowShape : AttnShape {
  ssize_t h = 0, w = 0, wh = 0, ww = 0, windows = 0;
};
template <typename T>
AttnWindowShape attention_window_shape(const Tensor<T>& q, const Tensor<T>* k, const Tensor<T>* v, ssize_t heads, ssize_t wh, ssize_t ww) {
  if ((k == nullptr) != (v == nullptr)) throw std::runtime_error("i8ie: attention takes q, k and v, or one packed qkv tensor");
  if (heads < 1) throw std::runtime_error("i8ie: attention: heads must be >= 1");
  if (wh < 1 || ww < 1) throw std::runtime_error("i8ie: attention: the window must be at least 1 x 1");
  for (const Tensor<T>* t : {&q, k, v}) {
    if (!t) continue;
    if (t->shape.size() != 4) throw std::runtime_error("i8ie: attention: the windowed form takes [n, c, h, w] operands");
    for (ssize_t d : t->shape)
      if (d <= 0) throw std::runtime_error("i8ie: attention: empty tensor");
  }
  AttnWindowShape s;
  s.heads = heads;
  s.packed = k == nullptr;
  s.b = q.shape[0];
  s.h = q.shape[2]; s.w = q.shape[3]; s.wh = wh; s.ww = ww;
  if (s.packed) {
    if (q.shape[1] % (3 * heads) != 0) throw std::runtime_error("i8ie: attention: a packed qkv tensor needs 3 * heads * d channels");
    s.c = q.shape[1] / 3;
  } else {
    for (const Tensor<T>* t : {k, v}) {
      if (t->shape[0] != s.b) throw std::runtime_error("i8ie: attention: the operands' batch sizes differ (there is no broadcasting)");
      if (t->shape[1] != q.shape[1]) throw std::runtime_error("i8ie: attention: q, k and v must have the same channel count");
      if (t->shape[2] != s.h || t->shape[3] != s.w) throw std::runtime_error("i8ie: attention: the windowed form needs q, k and v maps of one size");
    }
    if (q.shape[1] % heads != 0) throw std::runtime_error("i8ie: attention: the channel count is not heads * d");
    s.c = q.shape[1];
  }
  s.d = s.c / heads;
  if (s.h % wh != 0 || s.w % ww != 0)
    throw std::runtime_error("i8ie: attention: the window does not divide the map (pad it first)");
  if (wh * ww > 32768) throw std::runtime_error("i8ie: attention: more than 32768 pixels in a window");
  s.tq = s.tk = wh * ww;
  s.windows = (s.h / wh) * (s.w / ww);
  s.out = {s.b, s.c, s.h, s.w};
  return s;
}
// ---- layer_norm (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_layernorm_u8) ---------------------
// [n, c, h, w] is normalised over c per pixel, [m, f] and [b, t, f] over the last axis: (rows, inner) of the FP32 entry, or
// a RuntimeError (before any device call)
template <typename T>
std::pair<int64_t, int64_t> layer_norm_rows(const Tensor<T>& x, ssize_t channels) {
  const size_t r = x.shape.size();
  if (x.size <= 0 || (r != 2 && r != 3 && r != 4)) throw std::runtime_error("i8ie: layer_norm expects [n, c, h, w], [m, f] or [b, t, f]");
  if ((r == 4 ? x.shape[1] : x.shape.back()) != channels)
    throw std::runtime_error("i8ie: layer_norm: the normalised axis has " + std::to_string(r == 4 ? x.shape[1] : x.shape.back()) +
                             " values, the layer " + std::to_string(channels));
  if (channels > 16384) throw std::runtime_error("i8ie: layer_norm: rows of more than 16384 values");
  return {(int64_t)(x.size / channels), r == 4 ? (int64_t)(x.shape[2] * x.shape[3]) : 1};
}
// ---- group_norm (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_groupnorm_u8_nhwc) ----------------
// [n, c, h, w] is normalised per image over the pixels and the c / groups channels of a group, [n, c] is h = w = 1: the pixels
// per image, or a RuntimeError (before any device call)
template <typename T>
int64_t group_norm_pixels(const Tensor<T>& x, ssize_t groups, ssize_t channels) {
  const size_t r = x.shape.size();
  if (x.size <= 0 || (r != 2 && r != 4)) throw std::runtime_error("i8ie: group_norm expects [n, c, h, w] or [n, c]");
  if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: group_norm: channels must be in 1..16384");
  if (groups < 1 || channels % groups != 0) throw std::runtime_error("i8ie: group_norm: the channel count must be a multiple of the group count");
  if (x.shape[1] != channels)
    throw std::runtime_error("i8ie: group_norm: the tensor has " + std::to_string(x.shape[1]) + " channels, the layer " + std::to_string(channels));
  const int64_t hw = r == 4 ? (int64_t)(x.shape[2] * x.shape[3]) : 1;
  if ((int64_t)(channels / groups) * hw > I8IE_GROUPNORM_MAX_N)
    throw std::runtime_error("i8ie: group_norm: a group of one image has more than 65536 values");
  return hw;
}
// ---- batch_norm (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_batchnorm_u8_nhwc) ----------------
// [n, c, h, w] or [n, c], normalised per channel with the stored statistics: the pixels per image, or a RuntimeError (before
// any device call)
template <typename T>
int64_t batch_norm_pixels(const Tensor<T>& x, ssize_t channels) {
  const size_t r = x.shape.size();
  if (x.size <= 0 || (r != 2 && r != 4)) throw std::runtime_error("i8ie: batch_norm expects [n, c, h, w] or [n, c]");
  if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: batch_norm: channels must be in 1..16384");
  if (x.shape[1] != channels)
    throw std::runtime_error("i8ie: batch_norm: the tensor has " + std::to_string(x.shape[1]) + " channels, the layer " + std::to_string(channels));
  return r == 4 ? (int64_t)(x.shape[2] * x.shape[3]) : 1;
}
// ---- cat (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_concat_u8) --------------------------
// axis 1 of k rank-4 [n, c_i, h, w] or k rank-2 [m, f_i] tensors: the result's shape, or a RuntimeError (before any device call)
template <typename T>
std::vector<ssize_t> cat_shape(const std::vector<Tensor<T>>& ts) {
  if (ts.empty() || ts.size() > I8IE_CONCAT_MAX_INPUTS) throw std::runtime_error("i8ie: cat: between 1 and 8 tensors");
  std::vector<ssize_t> shp = ts[0].shape;
  if (shp.size() != 2 && shp.size() != 4) throw std::runtime_error("i8ie: cat: tensors must be [n, c, h, w] or [m, f] (joined along axis 1)");
  for (size_t i = 1; i < ts.size(); ++i) {
    const std::vector<ssize_t>& s = ts[i].shape;
    if (s.size() != shp.size()) throw std::runtime_error("i8ie: cat: ranks differ");
    for (size_t d = 0; d < s.size(); ++d)
      if (d != 1 && s[d] != ts[0].shape[d]) throw std::runtime_error("i8ie: cat: shapes differ outside axis 1");
    shp[1] += s[1];
  }
  for (const auto& t : ts)
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: cat: empty tensor");
  return shp;
}
// a Python list of tensors of one dtype; anything else (a mix included) is a RuntimeError
template <typename T>
std::vector<Tensor<T>> cat_list(const py::list& l) {
  std::vector<Tensor<T>> ts;
  for (const py::handle& h : l) {
    if (!py::isinstance<Tensor<T>>(h)) throw std::runtime_error("i8ie: cat: every tensor must have the same dtype (float32, or uint8 with scale and zero_point)");
    ts.push_back(h.cast<Tensor<T>&>());
  }
  return ts;
}
using LutBytes = std::array<u8_t, 256>;

// the ops a layer class calls (ops_join.cc, ops_attention.cc, ops.cc); every other op is reached through bind_ops alone
Tensor<float> add_f32(Tensor<float>& a, Tensor<float>& b);
Tensor<u8_t> add_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp);
Tensor<float> mul_f32(Tensor<float>& a, Tensor<float>& b);
Tensor<u8_t> mul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp);
Tensor<float> cat_f32(std::vector<Tensor<float>> ts);
Tensor<u8_t> cat_u8(std::vector<Tensor<u8_t>> ts, float scale, int zp);
Tensor<float> matmul_f32(Tensor<float>& a, Tensor<float>& b, bool ta, bool tb);
Tensor<u8_t> matmul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp, bool ta, bool tb);
Tensor<float> softmax_f32(Tensor<float>& x);
Tensor<u8_t> softmax_u8(Tensor<u8_t>& x);
Tensor<float> attention_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, Tensor<float>* scores);
Tensor<u8_t> attention_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v, ssize_t heads, float s_s, int zp_s, float scale, int zp);
// ... inside wh x ww windows of rank-4 maps; `scores` is then [n * windows, heads, wh * ww, wh * ww]
Tensor<float> attention_window_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, ssize_t wh, ssize_t ww,
                                   Tensor<float>* scores);
Tensor<u8_t> attention_window_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v, ssize_t heads, ssize_t wh, ssize_t ww, float s_s, int zp_s,
                                 float scale, int zp);
Tensor<float> layer_norm_f32(Tensor<float>& x, const std::shared_ptr<Storage>& gamma, const std::shared_ptr<Storage>& beta, ssize_t channels, float eps);
Tensor<u8_t> layer_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t channels, float eps,
                           float scale, int zp);
std::vector<float> layer_norm_param(const py::object& a, ssize_t channels, float fill, const char* what);
std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>> layer_norm_affine(const std::vector<float>& gamma, const std::vector<float>& beta,
                                                                                 float scale, int zp);
Tensor<float> group_norm_f32(Tensor<float>& x, const std::shared_ptr<Storage>& gamma, const std::shared_ptr<Storage>& beta, ssize_t groups,
                             ssize_t channels, float eps);
Tensor<u8_t> group_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t groups,
                           ssize_t channels, float eps, float scale, int zp);
// the four device arrays gamma, beta, mean, var of the FP32 form
struct BatchNormF32 {
  std::shared_ptr<Storage> gamma, beta, mean, var;
};
Tensor<float> batch_norm_f32(Tensor<float>& x, const BatchNormF32& p, ssize_t channels, float eps);
Tensor<u8_t> batch_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t channels, float scale,
                           int zp);
std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>> batch_norm_affine(const std::vector<float>& gamma, const std::vector<float>& beta,
                                                                                 const std::vector<float>& mean, const std::vector<float>& var,
                                                                                 float eps, float scale, int zp);
Tensor<float> activation_f32(Tensor<float>& in, int kind, float param);
Tensor<u8_t> activation_u8(Tensor<u8_t>& in, int kind, float param, float scale, int zp);
void bind_ops(py::module_& m);
void bind_rearrange(py::module_& m);  // ops_rearrange.cc: _narrow, _channel_shuffle, _pixel_shuffle, _pixel_unshuffle
void bind_resize(py::module_& m);     // ops_resize.cc: _interpolate, _adaptive_avg_pool2d
void bind_pad(py::module_& m);        // ops_pad.cc: _pad
void bind_posembed(py::module_& m);   // ops_posembed.cc: _position_embedding, _PositionEmbedding

}  // namespace i8ie_py
