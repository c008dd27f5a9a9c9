// i8ie_layer_create.hip -- how a layer handle is made: every create entry of the C-ABI fills one
// LayerSpec, runs its argument checks and calls layer_build: spec -> checks -> route -> pack -> upload.  Also here: what a
// handle answers about itself, i8ie_layer_destroy, the stateless i8ie_*_u8s8 entries (the grouped / dilated / transposed ones
// build a temporary handle) and the host-side weight quantizers.  Host code only: no kernel in this file.
//   reference: src/fully_connected.cc:22-52, src/conv2d.cc:100-142, src/layer.cc:6-26,36-54
// The routes A / B / F / G / T are listed at the top of i8ie_layer.hip; route_of below is the ONE place that chooses among them.
#include <cmath>
#include <new>
#include <vector>

#include "i8ie_layer.h"
#include "i8ie_stem.h"
#include "i8ie_requant.h"
#include "i8ie_gconv.h"
#include "i8ie_deconv.h"

namespace {

// ---- spec ---------------------------------------------------------------------------------------------------------------------
enum { KIND_LINEAR, KIND_CONV, KIND_DECONV };
// A layer as its create entry describes it.  Linear: c input features under a 1 x 1 kernel.  ConvTranspose2d: kh = kw = k, and the
// weights are the equivalent matrix [n][c * k * k] (i8ie_deconv.h).
struct LayerSpec {
  int kind = KIND_CONV;
  int n = 0, c = 0, kh = 1, kw = 1, stride = 1, pad = 0, groups = 1, dilation = 1, output_pad = 0;
  // the w axis of a Conv2d: stride / pad / dilation above are the h axis' numbers.  Only
  // i8ie_conv2d_create_rect gives unequal pairs; `rect`: it did (or kh != kw came with it), and the layer is route G's
  int stride_w = 1, pad_w = 0, dilation_w = 1;
  bool rect = false;
  float s_w = 1.0f;
  const float* s_w_pc = nullptr;  // [n] per-channel scales; null: per tensor (s_w)
  int K() const { return (c / groups) * kh * kw; }  // the reduction length of one output feature (after the checks: groups >= 1)
};
LayerSpec conv_spec(int kc, int c, int kh, int kw, int stride, int pad) {
  LayerSpec s;
  s.n = kc; s.c = c; s.kh = kh; s.kw = kw; s.stride = s.stride_w = stride; s.pad = s.pad_w = pad;
  return s;
}
LayerSpec dilated_spec(int kc, int c, int kh, int kw, int stride, int pad, int groups, int dilation) {
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.groups = groups; s.dilation = s.dilation_w = dilation;
  return s;
}
// the eight integers of i8ie_conv2d_create_rect; all four pairs equal: the spec of i8ie_conv2d_create_dilated
LayerSpec rect_spec(int kc, int c, int groups, const i8ie_conv_geom& g) {
  LayerSpec s = dilated_spec(kc, c, g.kh, g.kw, g.stride_h, g.pad_h, groups, g.dilation_h);
  s.stride_w = g.stride_w; s.pad_w = g.pad_w; s.dilation_w = g.dilation_w;
  s.rect = g.kh != g.kw || g.stride_h != g.stride_w || g.pad_h != g.pad_w || g.dilation_h != g.dilation_w;
  return s;
}
LayerSpec deconv_spec(int kc, int c, int k, int stride, int pad, int output_pad) {
  LayerSpec s = conv_spec(kc, c, k, k, stride, pad);
  s.kind = KIND_DECONV; s.output_pad = output_pad;
  return s;
}
LayerSpec linear_spec(int n, int k) {
  LayerSpec s;
  s.kind = KIND_LINEAR; s.n = n; s.c = k;
  return s;
}

// ---- checks: the argument rules, each a named piece; an entry lists the ones it applies, in its order ----------------------------
// All of them answer before any device call.  Code and text of every answer are pinned (tests/golden/create_arg_rules.json), and
// the text names the function that has always given it -- so a piece whose rule used to live in an entry reports under that
// entry's name (REQUIRE_AS), and the pieces name their locals as the texts quote them.
#define REQUIRE_AS(who, cond, msg)                           \
  do {                                                       \
    if (!(cond)) {                                           \
      i8ie_set_error("%s: %s (%s)", who, msg, #cond);        \
      return I8IE_ERR_ARG;                                   \
    }                                                        \
  } while (0)

// geometry of the plain Conv2d entries
int check_geometry(const LayerSpec& s) {
  const int c = s.c, kh = s.kh, kw = s.kw, stride = s.stride, pad = s.pad;
  REQUIRE_AS("i8ie_conv2d_create", c > 0 && kh > 0 && kw > 0, "non-positive dimension");
  REQUIRE_AS("i8ie_conv2d_create", stride > 0, "stride must be positive");
  REQUIRE_AS("i8ie_conv2d_create", pad >= 0, "negative padding");
  return I8IE_OK;
}
// groups (not in the reference; src/conv2d.cc:100-142 per group): geometry and the rules on groups of every entry that takes them
int check_groups(const LayerSpec& s) {
  const int kc = s.n, c = s.c, kh = s.kh, kw = s.kw, stride = s.stride, pad = s.pad, groups = s.groups;
  I8IE_REQUIRE(kc > 0 && c > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0, "stride must be positive");
  I8IE_REQUIRE(pad >= 0, "negative padding");
  I8IE_REQUIRE(groups >= 1, "groups must be >= 1");
  I8IE_REQUIRE(c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  I8IE_REQUIRE(groups <= 65535, "at most 65535 groups");
  return I8IE_OK;
}
// dilation (not in the reference; the kernel inflated by zeros)
int check_dilation(int dilation) {
  I8IE_REQUIRE(dilation >= 1, "dilation must be >= 1");
  return I8IE_OK;
}
// the w axis of a rect geometry: the rules check_groups and check_dilation apply to the h axis' numbers
int check_rect(const LayerSpec& s) {
  const int stride_w = s.stride_w, pad_w = s.pad_w, dilation_w = s.dilation_w;
  REQUIRE_AS("i8ie_conv2d_create_rect", stride_w > 0, "stride must be positive");
  REQUIRE_AS("i8ie_conv2d_create_rect", pad_w >= 0, "negative padding");
  REQUIRE_AS("i8ie_conv2d_create_rect", dilation_w >= 1, "dilation must be >= 1");
  return I8IE_OK;
}
// ConvTranspose2d (not in the reference): i8ie_deconv_check_args is the rule
int check_deconv(const LayerSpec& s) { return i8ie_deconv_check_args(s.n, s.c, s.kh, s.stride, s.pad, s.output_pad); }
// scales from the caller: finite and >= 0 (pooling the INT32 accumulators before the requantiser needs a monotone
// map per channel, DESIGN.md "Per-channel weight scales")
int check_scales(const float* s_w, int n) {
  I8IE_REQUIRE(s_w != nullptr, "null argument");
  for (int j = 0; j < n; ++j) {
    if (!(s_w[j] >= 0.0f && s_w[j] <= 3.402823466e+38f)) {
      i8ie_set_error("per-channel weight scale %d is negative or not finite", j);
      return I8IE_ERR_ARG;
    }
  }
  return I8IE_OK;
}
// null pointers and the sizes nothing above has looked at: layer_build's own first step
int check_build_args(const i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, i8ie_layer** out, const LayerSpec& s) {
  const int n = s.n, K = s.K();
  REQUIRE_AS("layer_create", ctx && qw_host && qb_host && out, "null argument");
  REQUIRE_AS("layer_create", n > 0 && K > 0, "non-positive dimension");
  return I8IE_OK;
}

// ---- route --------------------------------------------------------------------------------------------------------------------
struct Route {
  int path;   // PATH_*
  int dil;    // the effective dilation: what the kernels walk (the handle's dil_arg remembers the number of the spec)
  bool stem;  // route B: the first-stage kernel's packing is made as well
  int dil_w;  // a rect layer's effective dilation on the w axis (every other layer: dil)
};
// the geometry a forward of the spec walks (conv_geom of i8ie_layer.h)
i8ie_conv_geom geom_of(const LayerSpec& s, const Route& r) {
  return i8ie_conv_geom{s.kh, s.kw, s.stride, s.stride_w, s.pad, s.pad_w, r.dil, r.dil_w};
}
Route route_of(const LayerSpec& s) {
  if (s.kind == KIND_LINEAR) return {PATH_F, 1, false, 1};  // (a Linear handle has no route: PATH_F is the field's rest value)
  if (s.kind == KIND_DECONV) return {PATH_T, 1, false, 1};
  // an unequal pair: the grouped route with any groups >= 1, the pairs in the gather; one tap on an axis has no dilation there
  if (s.rect) return {PATH_G, s.kh == 1 ? 1 : s.dilation, false, s.kw == 1 ? 1 : s.dilation_w};
  // dilation 1 or a 1 x 1 kernel is exactly the undilated layer: same route, same kernels
  const int dil = (s.dilation == 1 || (s.kh == 1 && s.kw == 1)) ? 1 : s.dilation;
  if (s.groups > 1 || dil > 1) return {PATH_G, dil, false, dil};  // (a dilated layer with any groups >= 1: the dilation is in the gather)
  if (s.c % 16 == 0) return {PATH_A, 1, false, 1};
  if (s.c <= 4 && s.stride % 4 == 0)
    return {PATH_B, 1, s.c <= 3 && s.n % 32 == 0 && s.n <= 96 && (s.kh + 3) / 4 * ((s.kw + 3) / 4) * 48 <= 14 * 32, 1};
  return {PATH_F, 1, false, 1};
}

// ---- pack: the weights in the K orders of the kernels, built on the host once -----------------------------------------------------
struct WeightShape { int n, cg, kh, kw; };  // qw [n][cg][kh][kw]
// The one walk: tap (ch, y, x) of feature j goes to at(j, ch, y, x) of a zeroed panel of `size` bytes.
template <class At>
std::vector<int8_t> pack_walk(const int8_t* qw, const WeightShape& w, size_t size, At at) {
  std::vector<int8_t> panel(size, 0);
  for (int j = 0; j < w.n; ++j)
    for (int ch = 0; ch < w.cg; ++ch)
      for (int y = 0; y < w.kh; ++y)
        for (int x = 0; x < w.kw; ++x) panel[at(j, ch, y, x)] = *qw++;
  return panel;
}
// route A: [Npad][Kpad2], K ordered (kh, kw, c)
std::vector<int8_t> pack_khwc(const int8_t* qw, const WeightShape& w, int Npad, int Kpad2) {
  return pack_walk(qw, w, (size_t)Npad * Kpad2,
                   [&](int j, int ch, int y, int x) { return (size_t)j * Kpad2 + ((size_t)y * w.kw + x) * w.cg + ch; });
}
// route B: [Npad][Kpad2], a row of taps in kwg groups of 4 pixels x 4 channels
std::vector<int8_t> pack_small_c(const int8_t* qw, const WeightShape& w, int Npad, int Kpad2) {
  const int kwg = (w.kw + 3) / 4;
  return pack_walk(qw, w, (size_t)Npad * Kpad2, [&](int j, int ch, int y, int x) {
    return (size_t)j * Kpad2 + ((size_t)y * kwg + x / 4) * 16 + (x % 4) * 4 + ch;
  });
}
// route B, the first-stage kernel: [n][KpadStem], K in its space-to-depth order
std::vector<int8_t> pack_stem(const int8_t* qw, const WeightShape& w, int KpadStem) {
  return pack_walk(qw, w, (size_t)w.n * KpadStem,
                   [&](int j, int ch, int y, int x) { return (size_t)j * KpadStem + i8ie_stem_kindex(w.kw, ch, y, x); });
}
// route G: [groups][Ngp][Kgp]; group g's n / groups rows go to panel g, K ordered (kh, kw, cg)
std::vector<int8_t> pack_grouped(const int8_t* qw, const WeightShape& w, int groups, int Ngp, int Kgp) {
  const int Ng = w.n / groups;
  return pack_walk(qw, w, (size_t)groups * Ngp * Kgp, [&](int j, int ch, int y, int x) {
    return ((size_t)(j / Ng) * Ngp + j % Ng) * Kgp + ((size_t)y * w.kw + x) * w.cg + ch;
  });
}

// ---- upload -------------------------------------------------------------------------------------------------------------------
// a host vector as a buffer of the handle; an empty one (a packing the route does not make) leaves *dev null
template <class T, class D>
int upload(i8ie_layer* L, D** dev, const std::vector<T>& v) {
  return v.empty() ? I8IE_OK : i8ie_layer_buffer(L, (void**)dev, v.size() * sizeof(T), v.data());
}

// what every handle holds: the weights as converted, the v1 panel (routes G and T never read theirs: known, kept), the sums
int upload_common(i8ie_layer* L, const int8_t* qw_host, const int8_t* qb_host) {
  i8ie_ctx* ctx = L->ctx;
  const int n = L->n, K = L->K;
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->qw, (size_t)n * K, qw_host));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->qb, (size_t)n, qb_host));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->Bpack, (size_t)L->Npad * L->Kpad));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->wsum, (size_t)n * 4));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->oc, (size_t)n * 4));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->ocp, (size_t)L->Npad * 4));  // padded: vector loads
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->biasf, (size_t)L->Npad * 4));
  I8IE_TRY(i8ie_memset(ctx, L->ocp, 0, (size_t)L->Npad * 4));
  I8IE_TRY(i8ie_memset(ctx, L->biasf, 0, (size_t)L->Npad * 4));
  I8IE_TRY(i8ie_launch_pad_rows(ctx, L->qw, n, K, L->Bpack, L->Npad, L->Kpad, 0));
  return i8ie_launch_offsets(ctx, L->conv, L->qw, nullptr, n, K, 1.0f, 0, nullptr, L->wsum);
}

// the route's own packings: their pitches into the handle, their bytes onto the device
int upload_route(i8ie_layer* L, const Route& r, const int8_t* qw_host) {
  const int n = L->n, c = L->c, kh = L->kh, kw = L->kw;
  const WeightShape w{n, c / L->groups, kh, kw};
  if (r.path == PATH_T) {
    std::vector<int8_t> panels;
    std::vector<int32_t> tph;
    std::vector<int> ttab;
    L->Ngp = round_up(n, 16);
    L->Kpp = i8ie_deconv_kpitch(c, kh, L->stride);
    i8ie_deconv_pack(qw_host, n, c, kh, L->stride, panels, tph);
    i8ie_deconv_ktab(c, kh, L->stride, ttab);
    I8IE_TRY(upload(L, &L->Bt, panels));
    I8IE_TRY(upload(L, &L->ttab, ttab));
    return upload(L, &L->tph, tph);
  }
  if (r.path == PATH_G) {
    std::vector<int> gtab;
    L->Ngp = round_up(n / L->groups, 16);
    L->Kgp = round_up(L->K, 64);
    i8ie_gconv_ktab(w.cg, kh, kw, L->Kgp, gtab);
    I8IE_TRY(upload(L, &L->Bg, pack_grouped(qw_host, w, L->groups, L->Ngp, L->Kgp)));
    return upload(L, &L->gtab, gtab);
  }
  if (r.path == PATH_A) {
    L->K2 = kh * kw * c;
    L->Kpad2 = round_up(L->K2, 128);
    return upload(L, &L->Bpack2, pack_khwc(qw_host, w, L->Npad, L->Kpad2));
  }
  if (r.path == PATH_B) {
    L->kwg = (kw + 3) / 4;
    L->K2 = kh * L->kwg * 16;
    L->Kpad2 = round_up(L->K2, 128);
    I8IE_TRY(upload(L, &L->Bpack2, pack_small_c(qw_host, w, L->Npad, L->Kpad2)));
    if (!r.stem) return I8IE_OK;
    L->KpadStem = i8ie_stem_kpad(kh, kw);
    return upload(L, &L->Bstem, pack_stem(qw_host, w, L->KpadStem));
  }
  return I8IE_OK;  // Linear, route F: the v1 panel is all
}

// per-channel layers: s_w[n] (host copy, device [Npad]) and the multiplier buffer (filled per (s_in, s_out) by the forward)
int upload_scales(i8ie_layer* L, const float* s_w_pc) {
  L->pc = true;
  L->sw_host.assign(s_w_pc, s_w_pc + L->n);
  std::vector<float> sw((size_t)L->Npad, 1.0f);
  for (int j = 0; j < L->n; ++j) sw[j] = s_w_pc[j];
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->swv, sw.size() * 4));
  I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->msv, sw.size() * 4));
  I8IE_TRY(i8ie_memcpy_h2d(L->ctx, L->swv, sw.data(), sw.size() * 4));
  return i8ie_memset(L->ctx, L->msv, 0, sw.size() * 4);
}

// ---- build: a checked spec and its host weights into a handle, or nothing ---------------------------------------------------------
int layer_build(i8ie_ctx* ctx, const LayerSpec& s, const int8_t* qw_host, const int8_t* qb_host, i8ie_layer** out) {
  I8IE_TRY(check_build_args(ctx, qw_host, qb_host, out, s));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  i8ie_layer* L = new (std::nothrow) i8ie_layer();
  if (!L) return I8IE_ERR_OOM;
  const Route r = route_of(s);
  L->ctx = ctx; L->conv = s.kind != KIND_LINEAR; L->n = s.n; L->K = s.K();
  if (L->conv) {
    L->c = s.c; L->kh = s.kh; L->kw = s.kw; L->stride = s.stride; L->pad = s.pad;
    L->groups = s.groups; L->opad = s.output_pad;
    L->rect = s.rect; L->stride_w = s.stride_w; L->pad_w = s.pad_w;
  }
  L->path = r.path; L->dil = r.dil; L->dil_arg = s.dilation; L->dil_w = r.dil_w; L->dil_arg_w = s.dilation_w;
  L->s_w = s.s_w_pc ? 1.0f : s.s_w;  // (unused by a per-channel layer)
  L->Kpad = round_up(L->K, 128);
  L->Npad = round_up(L->n, 128);
  int rc = upload_common(L, qw_host, qb_host);
  if (rc == I8IE_OK) rc = upload_route(L, r, qw_host);
  if (rc == I8IE_OK && s.s_w_pc) rc = upload_scales(L, s.s_w_pc);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

// ---- the stateless grouped / dilated / transposed calls -----------------------------------------------------------------------------
// what such a call gets besides the layer: device tensors, the weights on the device, the caller's offset vector
struct OnceCall {
  const uint8_t* in;
  int n, h, w;
  const int8_t* qw;
  uint8_t zp_in;
  const int32_t* oc;
  float s_in, s_out;
  uint8_t zp_out;
  uint8_t* out;
  int32_t* acc;
};
int check_once(const char* who, const i8ie_ctx* ctx, const OnceCall& q) {
  const void *in = q.in, *qw = q.qw, *oc = q.oc, *out = q.out;
  const int n = q.n;
  REQUIRE_AS(who, ctx && in && qw && oc && out, "null argument");
  REQUIRE_AS(who, n > 0, "non-positive batch");
  return I8IE_OK;
}
int check_once_geometry(const LayerSpec& s, const OnceCall& q) {
  ConvGeom cg;
  if (s.kind == KIND_DECONV) return deconv_geom(s.c, q.h, q.w, s.n, s.kh, s.stride, s.pad, s.output_pad, &cg);
  return conv_geom(s.c, q.h, q.w, s.n, geom_of(s, route_of(s)), &cg);
}
// The weights are packed for this one call: read back from the device, built into a temporary handle (zero bias: the caller's
// oc[] carries the bias term) that runs one NCHW forward with that oc[] instead of its own, and is destroyed.
int run_once(i8ie_ctx* ctx, const LayerSpec& s, const OnceCall& q) {
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  std::vector<int8_t> qw_host((size_t)s.n * s.K()), qb_host((size_t)s.n, 0);
  I8IE_TRY(i8ie_memcpy_d2h(ctx, qw_host.data(), q.qw, qw_host.size()));
  i8ie_layer* L = nullptr;
  I8IE_TRY(layer_build(ctx, s, qw_host.data(), qb_host.data(), &L));
  L->s_out = q.s_out;
  L->zp_out = q.zp_out;
  int rc = i8ie_launch_finish_offsets(ctx, q.oc, L->wsum, L->qb, q.s_in, L->n, L->ocp, nullptr);
  L->oc_valid = rc == I8IE_OK;
  L->oc_s_in = q.s_in;
  L->oc_zp_in = q.zp_in;
  if (rc == I8IE_OK) rc = i8ie_layer_forward(L, q.in, q.n, q.h, q.w, q.s_in, q.zp_in, q.out, q.acc);
  i8ie_layer_destroy(L);
  return rc;
}

}  // namespace

int i8ie_layer_buffer(i8ie_layer* L, void** dev, size_t bytes, const void* host) {
  I8IE_TRY(i8ie_malloc(L->ctx, bytes, dev));
  L->owned.push_back(*dev);
  return host ? i8ie_memcpy_h2d(L->ctx, *dev, host, bytes) : I8IE_OK;
}

extern "C" {

// ---- create entries: spec, this entry's checks in this entry's order, layer_build ---------------------------------------------------
int i8ie_linear_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k, float s_w,
                       i8ie_layer** out) {
  LayerSpec s = linear_spec(n, k);
  s.s_w = s_w;
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_linear_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k,
                                   const float* s_w_host, i8ie_layer** out) {
  LayerSpec s = linear_spec(n, k);
  s.s_w_pc = s_w_host;
  I8IE_REQUIRE(out != nullptr && n > 0, "bad argument");
  I8IE_TRY(check_scales(s_w_host, n));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh, int kw,
                       int stride, int pad, float s_w, i8ie_layer** out) {
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.s_w = s_w;
  I8IE_TRY(check_geometry(s));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh,
                                   int kw, int stride, int pad, const float* s_w_host, i8ie_layer** out) {
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.s_w_pc = s_w_host;
  I8IE_REQUIRE(out != nullptr && kc > 0, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  I8IE_TRY(check_geometry(s));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_grouped(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh, int kw,
                               int stride, int pad, int groups, float s_w, i8ie_layer** out) {
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.groups = groups; s.s_w = s_w;
  I8IE_TRY(check_groups(s));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_grouped_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                                           int kh, int kw, int stride, int pad, int groups, const float* s_w_host,
                                           i8ie_layer** out) {
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.groups = groups; s.s_w_pc = s_w_host;
  I8IE_TRY(check_groups(s));
  if (groups == 1)  // (the dense layer has always answered as the plain per-channel entry)
    REQUIRE_AS("i8ie_conv2d_create_per_channel", out != nullptr && kc > 0, "bad argument");
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_dilated(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh, int kw,
                               int stride, int pad, int groups, int dilation, float s_w, i8ie_layer** out) {
  LayerSpec s = dilated_spec(kc, c, kh, kw, stride, pad, groups, dilation);
  s.s_w = s_w;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(dilation));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_dilated_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh,
                                           int kw, int stride, int pad, int groups, int dilation, const float* s_w_host,
                                           i8ie_layer** out) {
  LayerSpec s = dilated_spec(kc, c, kh, kw, stride, pad, groups, dilation);
  s.s_w_pc = s_w_host;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(dilation));
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

// a geometry of eight integers; all four pairs equal: what the two entries above make
int i8ie_conv2d_create_rect(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int groups,
                            const i8ie_conv_geom* geom, float s_w, i8ie_layer** out) {
  I8IE_REQUIRE(geom != nullptr, "null geometry");
  LayerSpec s = rect_spec(kc, c, groups, *geom);
  s.s_w = s_w;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(s.dilation));
  I8IE_TRY(check_rect(s));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv2d_create_rect_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int groups,
                                        const i8ie_conv_geom* geom, const float* s_w_host, i8ie_layer** out) {
  I8IE_REQUIRE(geom != nullptr, "null geometry");
  LayerSpec s = rect_spec(kc, c, groups, *geom);
  s.s_w_pc = s_w_host;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(s.dilation));
  I8IE_TRY(check_rect(s));
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv_transpose2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int k, int stride,
                                 int pad, int output_pad, float s_w, i8ie_layer** out) {
  LayerSpec s = deconv_spec(kc, c, k, stride, pad, output_pad);
  s.s_w = s_w;
  I8IE_TRY(check_deconv(s));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

int i8ie_conv_transpose2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int k,
                                             int stride, int pad, int output_pad, const float* s_w_host, i8ie_layer** out) {
  LayerSpec s = deconv_spec(kc, c, k, stride, pad, output_pad);
  s.s_w_pc = s_w_host;
  I8IE_TRY(check_deconv(s));
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  return layer_build(ctx, s, qw_host, qb_host, out);
}

// ---- what a handle answers about itself ---------------------------------------------------------------------------------------------
int i8ie_layer_weight_scales(const i8ie_layer* L, float* out, int n, int* per_channel) {
  I8IE_REQUIRE(L && out && per_channel, "null argument");
  I8IE_REQUIRE(n == L->n, "n must be the layer's out features");
  for (int j = 0; j < n; ++j) out[j] = L->pc ? L->sw_host[j] : L->s_w;
  *per_channel = L->pc ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_groups(const i8ie_layer* L, int* groups) {
  I8IE_REQUIRE(L && groups, "null argument");
  *groups = L->groups;
  return I8IE_OK;
}

int i8ie_layer_dilation(const i8ie_layer* L, int* dilation) {
  I8IE_REQUIRE(L && dilation, "null argument");
  I8IE_REQUIRE(L->dil_arg == L->dil_arg_w, "the layer's dilations differ per axis: ask i8ie_layer_geometry");
  *dilation = L->dil_arg;
  return I8IE_OK;
}

int i8ie_layer_geometry(const i8ie_layer* L, i8ie_conv_geom* geom) {
  I8IE_REQUIRE(L && geom, "null argument");
  I8IE_REQUIRE(L->conv, "a Linear layer has no geometry");
  *geom = i8ie_conv_geom{L->kh, L->kw, L->stride, L->stride_w, L->pad, L->pad_w, L->dil_arg, L->dil_arg_w};
  return I8IE_OK;
}

int i8ie_layer_set_output_qparams(i8ie_layer* L, float s_out, uint8_t zp_out) {
  I8IE_REQUIRE(L != nullptr, "null layer");
  L->s_out = s_out;
  L->zp_out = zp_out;
  L->ms_valid = false;  // (per-channel multipliers depend on s_out)
  return I8IE_OK;
}

int i8ie_layer_get_output_qparams(const i8ie_layer* L, float* s_out, uint8_t* zp_out) {
  I8IE_REQUIRE(L && s_out && zp_out, "null argument");
  *s_out = L->s_out;
  *zp_out = L->zp_out;
  return I8IE_OK;
}

int i8ie_layer_preferred_layout(const i8ie_layer* L, int* layout) {
  I8IE_REQUIRE(L && layout, "null argument");
  const bool fast = L->conv && L->path != PATH_F && !force_fallback(L->ctx) && (L->n % 16 == 0);
  *layout = fast ? I8IE_LAYOUT_NHWC : I8IE_LAYOUT_NCHW;
  return I8IE_OK;
}

int i8ie_layer_padding(const i8ie_layer* L, int* pad) {
  I8IE_REQUIRE(L && pad, "null argument");
  // (a transposed layer reads no border; a dilated one needs none and accepts any: its taps are bounds-checked, and a
  // border of `pad` pixels around a small map would multiply its bytes)
  // (a rect layer, like a dilated one, needs no border and accepts any)
  *pad = (L->conv && L->path != PATH_T && L->dil == 1 && !L->rect) ? L->pad : 0;
  return I8IE_OK;
}

int i8ie_layer_destroy(i8ie_layer* L) {
  if (!L) return I8IE_OK;
  for (void* p : L->owned) i8ie_free(L->ctx, p);
  for (const I8ieWCache::Ent& e : L->wc.ents) i8ie_free(L->ctx, e.buf);
  delete L;
  return I8IE_OK;
}

// ---- stateless entry points: any geometry, v1 kernels, no handle; the caller supplies oc -----------------------------------------------
int i8ie_conv_offsets(i8ie_ctx* ctx, const int8_t* qw, const int8_t* qb, int kc, int K, float s_in, uint8_t zp_in,
                      int32_t* oc) {
  I8IE_REQUIRE(ctx && qw && qb && oc, "null argument");
  I8IE_REQUIRE(kc > 0 && K > 0, "non-positive dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return i8ie_launch_offsets(ctx, true, qw, qb, kc, K, s_in, zp_in, oc, nullptr);
}

int i8ie_linear_offsets(i8ie_ctx* ctx, const int8_t* qw, int n, int k, uint8_t zp_in, int32_t* oc) {
  I8IE_REQUIRE(ctx && qw && oc, "null argument");
  I8IE_REQUIRE(n > 0 && k > 0, "non-positive dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return i8ie_launch_offsets(ctx, false, qw, nullptr, n, k, 0.0f, zp_in, oc, nullptr);
}

int i8ie_linear_u8s8(i8ie_ctx* ctx, const uint8_t* in, int m, int k, const int8_t* qw, const int8_t* qb, int n,
                     const int32_t* oc, float s_in, float s_w, float s_out, uint8_t zp_out, uint8_t* out,
                     int32_t* acc) {
  I8IE_REQUIRE(ctx && in && qw && qb && oc && out, "null argument");
  I8IE_REQUIRE(m > 0 && k > 0 && n > 0, "non-positive dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int Kpad = round_up(k, 128), Npad = round_up(n, 128);
  const size_t b_bytes = i8ie_align_up((size_t)Npad * Kpad, 256);
  const size_t s_bytes = i8ie_align_up((size_t)n * 4, 256);
  const size_t a_bytes = (size_t)m * Kpad;
  I8IE_TRY(i8ie_ws_reserve(ctx, b_bytes + s_bytes + a_bytes));
  uint8_t* ws = (uint8_t*)ctx->ws;
  int8_t* Bpack = (int8_t*)ws;
  int32_t* wsum = (int32_t*)(ws + b_bytes);
  uint8_t* scratch = ws + b_bytes + s_bytes;
  I8IE_TRY(i8ie_launch_pad_rows(ctx, qw, n, k, Bpack, Npad, Kpad, 0));
  I8IE_TRY(i8ie_launch_offsets(ctx, false, qw, nullptr, n, k, 0.0f, 0, nullptr, wsum));
  return linear_run_v1(ctx, in, m, k, Bpack, Kpad, qb, n, oc, wsum, s_in, s_w, s_out, zp_out, out, acc, scratch);
}

int i8ie_conv2d_u8s8(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int kh,
                     int kw, int stride, int pad, uint8_t zp_in, const int32_t* oc, float s_in, float s_w,
                     float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  I8IE_REQUIRE(ctx && in && qw && oc && out, "null argument");
  I8IE_REQUIRE(n > 0, "non-positive batch");
  ConvGeom cg;
  I8IE_TRY(conv_geom(c, h, w, kc, kh, kw, stride, pad, &cg));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int Npad = round_up(kc, 128);
  const int ipc = chunk_images(cg, n);
  const size_t b_bytes = i8ie_align_up((size_t)Npad * cg.Kpad, 256);
  const size_t s_bytes = i8ie_align_up((size_t)kc * 4, 256);
  const size_t col_bytes = (size_t)ipc * cg.oh * cg.ow * cg.Kpad;
  I8IE_TRY(i8ie_ws_reserve(ctx, b_bytes + s_bytes + col_bytes));
  uint8_t* ws = (uint8_t*)ctx->ws;
  int8_t* Bpack = (int8_t*)ws;
  int32_t* wsum = (int32_t*)(ws + b_bytes);
  uint8_t* col = ws + b_bytes + s_bytes;
  I8IE_TRY(i8ie_launch_pad_rows(ctx, qw, kc, cg.K, Bpack, Npad, cg.Kpad, 0));
  I8IE_TRY(i8ie_launch_offsets(ctx, true, qw, nullptr, kc, cg.K, 1.0f, 0, nullptr, wsum));
  return conv_run_v1(ctx, in, n, cg, Bpack, oc, wsum, zp_in, s_in, s_w, s_out, zp_out, out, acc, col, ipc);
}

// ---- ... and the three that build a temporary handle (run_once); an identity case goes to the form it equals -----------------------------
int i8ie_conv2d_u8s8_grouped(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int kh,
                             int kw, int stride, int pad, int groups, uint8_t zp_in, const int32_t* oc, float s_in,
                             float s_w, float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  I8IE_REQUIRE(groups >= 1, "groups must be >= 1");
  I8IE_REQUIRE(c > 0 && kc > 0 && c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  if (groups == 1)
    return i8ie_conv2d_u8s8(ctx, in, n, c, h, w, qw, kc, kh, kw, stride, pad, zp_in, oc, s_in, s_w, s_out, zp_out, out, acc);
  LayerSpec s = conv_spec(kc, c, kh, kw, stride, pad);
  s.groups = groups; s.s_w = s_w;
  const OnceCall q{in, n, h, w, qw, zp_in, oc, s_in, s_out, zp_out, out, acc};
  I8IE_TRY(check_once(__func__, ctx, q));
  I8IE_TRY(check_once_geometry(s, q));
  return run_once(ctx, s, q);
}

int i8ie_conv2d_u8s8_dilated(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int kh,
                             int kw, int stride, int pad, int groups, int dilation, uint8_t zp_in, const int32_t* oc, float s_in,
                             float s_w, float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  LayerSpec s = dilated_spec(kc, c, kh, kw, stride, pad, groups, dilation);
  s.s_w = s_w;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(dilation));
  if (route_of(s).dil == 1)
    return i8ie_conv2d_u8s8_grouped(ctx, in, n, c, h, w, qw, kc, kh, kw, stride, pad, groups, zp_in, oc, s_in, s_w, s_out, zp_out,
                                    out, acc);
  const OnceCall q{in, n, h, w, qw, zp_in, oc, s_in, s_out, zp_out, out, acc};
  I8IE_TRY(check_once_geometry(s, q));
  I8IE_TRY(check_once(__func__, ctx, q));
  return run_once(ctx, s, q);
}

int i8ie_conv2d_u8s8_rect(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int groups,
                          const i8ie_conv_geom* geom, uint8_t zp_in, const int32_t* oc, float s_in, float s_w, float s_out,
                          uint8_t zp_out, uint8_t* out, int32_t* acc) {
  I8IE_REQUIRE(geom != nullptr, "null geometry");
  LayerSpec s = rect_spec(kc, c, groups, *geom);
  s.s_w = s_w;
  I8IE_TRY(check_groups(s));
  I8IE_TRY(check_dilation(s.dilation));
  I8IE_TRY(check_rect(s));
  if (!s.rect)
    return i8ie_conv2d_u8s8_dilated(ctx, in, n, c, h, w, qw, kc, s.kh, s.kw, s.stride, s.pad, groups, s.dilation, zp_in, oc, s_in,
                                    s_w, s_out, zp_out, out, acc);
  const OnceCall q{in, n, h, w, qw, zp_in, oc, s_in, s_out, zp_out, out, acc};
  I8IE_TRY(check_once_geometry(s, q));
  I8IE_TRY(check_once(__func__, ctx, q));
  return run_once(ctx, s, q);
}

int i8ie_conv_transpose2d_u8s8(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int k,
                               int stride, int pad, int output_pad, uint8_t zp_in, const int32_t* oc, float s_in, float s_w,
                               float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  LayerSpec s = deconv_spec(kc, c, k, stride, pad, output_pad);
  s.s_w = s_w;
  const OnceCall q{in, n, h, w, qw, zp_in, oc, s_in, s_out, zp_out, out, acc};
  I8IE_TRY(check_deconv(s));
  I8IE_TRY(check_once(__func__, ctx, q));
  I8IE_TRY(check_once_geometry(s, q));
  return run_once(ctx, s, q);
}

// ---- host-side weight quantizers ------------------------------------------------------------------------------------------------------
// quantize_weight, src/layer.cc:6-26 (one-shot at convert())
int i8ie_quantize_weight(const float* w, int64_t nw, const float* b, int64_t nb, int8_t* qw, int8_t* qb,
                         float* scale_out) {
  I8IE_REQUIRE(w && b && qw && qb && scale_out, "null argument");
  I8IE_REQUIRE(nw > 0 && nb > 0, "empty tensor");
  float mx = -3.402823466e+38f, mn = 3.402823466e+38f;
  for (int64_t i = 0; i < nw; ++i) {
    mn = w[i] < mn ? w[i] : mn;
    mx = w[i] > mx ? w[i] : mx;
  }
  for (int64_t i = 0; i < nb; ++i) {
    mn = b[i] < mn ? b[i] : mn;
    mx = b[i] > mx ? b[i] : mx;
  }
  const float s = (mx - mn) / 127;
  for (int64_t i = 0; i < nw; ++i) qw[i] = (int8_t)(int32_t)(w[i] / s);
  for (int64_t i = 0; i < nb; ++i) qb[i] = (int8_t)(int32_t)(b[i] / s);
  *scale_out = s;
  return I8IE_OK;
}

// per-output-channel quantize (DESIGN.md "Per-channel weight scales"): row j = w[j * row_len ..], bias b[j] (may be null:
// zero); symmetric max-abs over the row and its bias, round half to even, clamp to [-127, 127]
int i8ie_quantize_weight_per_channel(const float* w, int rows, int64_t row_len, const float* b, int8_t* qw, int8_t* qb,
                                     float* scales) {
  I8IE_REQUIRE(w && qw && qb && scales, "null argument");
  I8IE_REQUIRE(rows > 0 && row_len > 0, "empty tensor");
  auto q8 = [](float x, float s) {
    float r = std::nearbyint(x / s);  // (the default rounding mode: to nearest, ties to even)
    r = r > 127.0f ? 127.0f : (r < -127.0f ? -127.0f : r);
    return (int8_t)(int32_t)r;
  };
  for (int j = 0; j < rows; ++j) {
    const float* row = w + (size_t)j * row_len;
    const float bj = b ? b[j] : 0.0f;
    float a = std::fabs(bj);
    for (int64_t k = 0; k < row_len; ++k) a = std::fabs(row[k]) > a ? std::fabs(row[k]) : a;
    const float s = a == 0.0f ? 1.0f : a / 127.0f;
    for (int64_t k = 0; k < row_len; ++k) qw[(size_t)j * row_len + k] = q8(row[k], s);
    qb[j] = q8(bj, s);
    scales[j] = s;
  }
  return I8IE_OK;
}

}  // extern "C"
