// i8ie_layer.h -- the layer handle as its two translation units see it: i8ie_layer_create.hip makes and frees it (DESIGN.md
// section 4b), i8ie_layer.hip runs it (section 4a).  Internal: nothing here is part of the C-ABI.
#pragma once
#include <vector>

#include "i8ie_internal.h"
#include "i8ie_calls.h"

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }
inline bool force_fallback(const i8ie_ctx* ctx) { return (ctx->options & 1) != 0; }

enum { PATH_F = 0, PATH_A = 1, PATH_B = 2, PATH_G = 3, PATH_T = 4 };  // PATH_G: grouped (i8ie_gconv.hip), PATH_T: transposed (i8ie_deconv.hip)

// stride / pad: the h axis' numbers, which a square layer (every route but G) has on both axes; stride_w / pad_w / dil_h / dil_w:
// the rest of the per-axis geometry, read by route G alone
struct ConvGeom {
  int c, h, w, kc, kh, kw, stride, pad, oh, ow, K, Kpad;
  int stride_w, pad_w, dil_h, dil_w;
};

// The geometry of one forward from the eight integers of i8ie_conv_geom (`e`: the EFFECTIVE dilations, what the kernels walk;
// DESIGN.md sections 8j, 8p): per axis the kernel spans dil (k - 1) + 1 pixels; 1 = the reference's geometry
inline int conv_geom(int c, int h, int w, int kc, const i8ie_conv_geom& e, ConvGeom* g) {
  // (the h axis' numbers under the names the square entries' error texts quote)
  const int kh = e.kh, kw = e.kw, stride = e.stride_h, pad = e.pad_h, dil = e.dilation_h;
  const int stride_w = e.stride_w, pad_w = e.pad_w, dil_w = e.dilation_w;
  I8IE_REQUIRE(c > 0 && h > 0 && w > 0 && kc > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0, "stride must be positive");  // include/conv2d.h:12-14
  I8IE_REQUIRE(stride_w > 0, "stride must be positive");
  I8IE_REQUIRE(pad >= 0, "negative padding");
  I8IE_REQUIRE(pad_w >= 0, "negative padding");
  I8IE_REQUIRE(dil >= 1, "dilation must be >= 1");
  I8IE_REQUIRE(dil_w >= 1, "dilation must be >= 1");
  const long long eh = (long long)dil * (kh - 1) + 1, ew = (long long)dil_w * (kw - 1) + 1;  // the kernel's extent
  const char* larger = (dil > 1 || dil_w > 1) ? "dilated kernel larger than padded input" : "kernel larger than padded input";
  // I8IE_REQUIRE quotes its condition in the error text, and the text of a square layer is pinned (tests/golden/
  // create_arg_rules.json) with the one `pad` on both axes: equal paddings answer with that wording, unequal ones with their own
  if (pad == pad_w) {
    I8IE_REQUIRE(h - eh + 2 * pad >= 0 && w - ew + 2 * pad >= 0, larger);
  } else {
    I8IE_REQUIRE(h - eh + 2 * pad >= 0 && w - ew + 2 * pad_w >= 0, larger);
  }
  g->c = c; g->h = h; g->w = w; g->kc = kc; g->kh = kh; g->kw = kw; g->stride = stride; g->pad = pad;
  g->stride_w = stride_w; g->pad_w = pad_w; g->dil_h = dil; g->dil_w = dil_w;
  g->oh = (int)((h - eh + 2 * pad) / stride) + 1;  // src/conv2d.cc:108-109
  g->ow = (int)((w - ew + 2 * pad_w) / stride_w) + 1;
  g->K = c * kh * kw;
  g->Kpad = round_up(g->K, 128);
  return I8IE_OK;
}
// ... and from the one number per argument of the square entries
inline int conv_geom(int c, int h, int w, int kc, int kh, int kw, int stride, int pad, ConvGeom* g, int dil = 1) {
  return conv_geom(c, h, w, kc, i8ie_conv_geom{kh, kw, stride, stride, pad, pad, dil, dil}, g);
}

// ConvTranspose2d: kh = kw = k, OH = (H - 1) s - 2 p + k + output_padding (torch.nn.ConvTranspose2d)
inline int deconv_geom(int c, int h, int w, int kc, int k, int stride, int pad, int opad, ConvGeom* g) {
  I8IE_REQUIRE(c > 0 && h > 0 && w > 0 && kc > 0 && k > 0, "non-positive dimension");
  g->c = c; g->h = h; g->w = w; g->kc = kc; g->kh = k; g->kw = k; g->stride = g->stride_w = stride; g->pad = g->pad_w = pad;
  g->dil_h = g->dil_w = 1;
  const long long oh = (long long)(h - 1) * stride - 2 * pad + k + opad, ow = (long long)(w - 1) * stride - 2 * pad + k + opad;
  I8IE_REQUIRE(oh > 0 && ow > 0 && oh < (1 << 30) && ow < (1 << 30), "transposed conv: empty or oversized output");
  g->oh = (int)oh;
  g->ow = (int)ow;
  g->K = c * k * k;
  g->Kpad = round_up(g->K, 128);
  return I8IE_OK;
}

struct i8ie_layer {
  i8ie_ctx* ctx = nullptr;
  bool conv = false;
  int n = 0, K = 0;  // out features, reduction length (reference K order)
  int c = 0, kh = 0, kw = 0, stride = 1, pad = 0;
  int Kpad = 0, Npad = 0;
  float s_w = 1.0f;
  float s_out = 1.0f;   // include/layer.h:46
  uint8_t zp_out = 0;   // include/layer.h:47
  // Every device buffer below is made by i8ie_layer_buffer, which puts it on `owned`; i8ie_layer_destroy frees that list and
  // the re-packs in `wc`, nothing by name.
  std::vector<void*> owned;
  int8_t* qw = nullptr;     // [n][K] as converted, K ordered (c, kh, kw)
  int8_t* qb = nullptr;     // [n]
  int8_t* Bpack = nullptr;  // [Npad][Kpad] zero padded, reference K order (Linear; conv path F)
  int8_t* Bperm = nullptr;  // Linear fed by an NHWC-flattened activation: Bpack with K reordered (h, w, c); made on first use
  int perm_c = 0, perm_hw = 0;
  int path = PATH_F;        // conv: PATH_A / PATH_B / PATH_F / PATH_G / PATH_T
  int dil = 1, dil_arg = 1; // conv: the effective dilation (1 when the kernel is 1 x 1) and the number the layer was created with;
                            // dil > 1 is PATH_G as well, with groups >= 1
  // a layer of i8ie_conv2d_create_rect with an unequal pair: PATH_G with any groups >= 1.  stride / pad /
  // dil / dil_arg above are then the h axis' numbers and these the w axis'; a square layer holds equal values
  bool rect = false;
  int stride_w = 1, pad_w = 0, dil_w = 1, dil_arg_w = 1;
  int groups = 1;           // conv, groups > 1 (PATH_G): K above is the reduction length INSIDE a group, (c / groups) * kh * kw,
  int Ngp = 0, Kgp = 0;     // and the weights are [groups][Ngp][Kgp], K ordered (kh, kw, cg) (i8ie_gconv.h)
  int8_t* Bg = nullptr;
  int* gtab = nullptr;      // the MFMA kernel's gather table (i8ie_gconv_ktab)
  int opad = 0;             // ConvTranspose2d (PATH_T): output_padding; qw / K above are the EQUIVALENT matrix [n][c * k * k];
  int Kpp = 0;              // the phase panels [stride^2][Ngp][Kpp], their gather table and the per-(phase, feature) sums of
  int8_t* Bt = nullptr;     // the taps a phase does not see (i8ie_deconv.h)
  int* ttab = nullptr;
  int32_t* tph = nullptr;
  int8_t* Bpack2 = nullptr; // conv paths A/B: [Npad][Kpad2], K ordered (kh, kw, c) / grouped
  int K2 = 0, Kpad2 = 0;    // valid / padded K of Bpack2 (bytes)
  I8ieWCache wc;            // Bpack2 in the fragment orders of i8ie_pconv.hip / i8ie_tconv.hip: one buffer per packing
                            // key, made on first use, never overwritten (captured graphs replay their addresses)
  int kwg = 0;              // path B: taps per row in 4-pixel groups
  int8_t* Bstem = nullptr;  // path B, when the first-stage kernel (i8ie_stem.hip) takes the layer: [n][KpadStem], K in its
  int KpadStem = 0;         // space-to-depth order (i8ie_stem_kindex), zero padded
  int32_t* wsum = nullptr;  // [n]
  int32_t* oc = nullptr;    // [n], valid for (oc_s_in, oc_zp_in)
  int32_t* ocp = nullptr;   // [n] oc + 128 * wsum
  float* biasf = nullptr;   // [n] (float)qb / s_in (Linear)
  bool oc_valid = false;
  float oc_s_in = 0.0f;
  int oc_zp_in = -1;
  // per-channel weight scales (i8ie_*_create_per_channel): s_w[j] per output feature, and the per-column multipliers of
  // i8ie_requant.h cached like oc' per (s_in, s_out); every kernel then runs its PC instance (s_w above is unused)
  bool pc = false;
  std::vector<float> sw_host;  // [n]
  float* swv = nullptr;        // [Npad] s_w[j] (padding 1)
  float* msv = nullptr;        // [Npad] fl(s_in * s_w[j] / s_out) (padding 0), valid for (ms_s_in, ms_s_out)
  bool ms_valid = false;
  bool ms_fast = false;        // every column allows the guarded estimate (i8ie_requant_pc_fast)
  float ms_s_in = 0.0f, ms_s_out = 0.0f;
};

// the geometry the kernels walk: the handle's numbers with the effective dilations
inline i8ie_conv_geom layer_geom(const i8ie_layer* L) {
  return i8ie_conv_geom{L->kh, L->kw, L->stride, L->stride_w, L->pad, L->pad_w, L->dil, L->dil_w};
}

// one device buffer of the handle: `bytes` allocated into *dev and onto L->owned, filled from `host` when that is given
int i8ie_layer_buffer(i8ie_layer* L, void** dev, size_t bytes, const void* host = nullptr);

// what the launchers get as s_w: the layer's scale, or for a per-channel layer the switch between the guarded estimate
// (1) and the exact sequence (0) that i8ie_make_requant reads off it (I8ieIgemmCall::msv)
inline float sw_arg(const i8ie_layer* L) { return L->pc ? (L->ms_fast ? 1.0f : 0.0f) : L->s_w; }
inline const float* msv_arg(const i8ie_layer* L) { return L->pc ? L->msv : nullptr; }
inline const float* sbv_arg(const i8ie_layer* L) { return L->pc ? L->swv : nullptr; }

// ---- the v1 (any-geometry) runners of i8ie_layer.hip: route F of a handle, and the stateless i8ie_*_u8s8 entries -----------
constexpr size_t kColBudget = (size_t)192 << 20;  // im2col scratch per chunk
inline int chunk_images(const ConvGeom& g, int n) {
  const size_t per_img = (size_t)g.oh * g.ow * g.Kpad;
  size_t imgs = kColBudget / per_img;
  if (imgs < 1) imgs = 1;
  return imgs > (size_t)n ? n : (int)imgs;
}
int conv_run_v1(i8ie_ctx* ctx, const uint8_t* in, int n, const ConvGeom& cg, const int8_t* Bpack, const int32_t* oc,
                const int32_t* wsum, uint8_t zp_in, float s_in, float s_w, float s_out, uint8_t zp_out, uint8_t* out,
                int32_t* acc, uint8_t* col, int imgs_per_chunk, const float* sbv = nullptr);
int linear_run_v1(i8ie_ctx* ctx, const uint8_t* in, int m, int k, const int8_t* Bpack, int Kpad, const int8_t* qb,
                  int n, const int32_t* oc, const int32_t* wsum, float s_in, float s_w, float s_out, uint8_t zp_out,
                  uint8_t* out, int32_t* acc, uint8_t* scratch, const float* sbv = nullptr);
