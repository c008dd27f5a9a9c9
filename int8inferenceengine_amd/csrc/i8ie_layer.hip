// i8ie_layer.hip -- Linear / Conv2d INT8 forward entry points of the C-ABI:
// the stateless calls on raw device pointers and the layer handles that keep
// the converted weights resident (packed for the MFMA kernels) and cache the
// zero-point offset vector per (s_in, zp_in).
//   reference: src/fully_connected.cc:22-52, src/conv2d.cc:100-142,
//              src/layer.cc:6-26,36-54
//
// Conv2d has four execution paths, all producing the reference's bytes:
//   A  channels % 16 == 0: implicit GEMM over NHWC activations (i8ie_igemm.hip)
//   B  channels <= 4 and stride % 4 == 0 (AlexNet conv1): the NCHW input is repacked
//      once into a physically padded, 4-pixel-grouped NHWC image; then path A's kernel
//   F  anything else: materialised im2col + v1 GEMM (i8ie_gemm.hip)
//   G  groups > 1 (i8ie_conv2d_create_grouped; not in the reference): one reference convolution per group, in the
//      grouped kernels of i8ie_gconv.hip over NHWC activations
//   T  ConvTranspose2d (i8ie_conv_transpose2d_create; not in the reference): the reference convolution of the equivalent
//      zero-inserted problem, computed phase by phase in the kernels of i8ie_deconv.hip over NHWC activations
// Activations cross the ABI as NCHW (the reference's layout) or, on request, as
// NHWC so that consecutive layers skip the layout conversion.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "i8ie_internal.h"
#include "i8ie_calls.h"
#include "i8ie_first.h"
#include "i8ie_stem.h"
#include "i8ie_requant.h"
#include "i8ie_gconv.h"
#include "i8ie_deconv.h"

namespace {

constexpr size_t kColBudget = (size_t)192 << 20;  // im2col scratch per chunk (fallback path F)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }

enum { PATH_F = 0, PATH_A = 1, PATH_B = 2, PATH_G = 3, PATH_T = 4 };  // PATH_G: grouped (i8ie_gconv.hip), PATH_T: transposed (i8ie_deconv.hip)

struct ConvGeom {
  int c, h, w, kc, kh, kw, stride, pad, oh, ow, K, Kpad;
};

int conv_geom(int c, int h, int w, int kc, int kh, int kw, int stride, int pad, ConvGeom* g) {
  I8IE_REQUIRE(c > 0 && h > 0 && w > 0 && kc > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0, "stride must be positive");  // include/conv2d.h:12-14
  I8IE_REQUIRE(pad >= 0, "negative padding");
  I8IE_REQUIRE(h - kh + 2 * pad >= 0 && w - kw + 2 * pad >= 0, "kernel larger than padded input");
  g->c = c; g->h = h; g->w = w; g->kc = kc; g->kh = kh; g->kw = kw; g->stride = stride; g->pad = pad;
  g->oh = (h - kh + 2 * pad) / stride + 1;  // src/conv2d.cc:108-109
  g->ow = (w - kw + 2 * pad) / stride + 1;
  g->K = c * kh * kw;
  g->Kpad = round_up(g->K, 128);
  return I8IE_OK;
}

// ConvTranspose2d: kh = kw = k, OH = (H - 1) s - 2 p + k + output_padding (torch.nn.ConvTranspose2d)
int deconv_geom(int c, int h, int w, int kc, int k, int stride, int pad, int opad, ConvGeom* g) {
  I8IE_REQUIRE(c > 0 && h > 0 && w > 0 && kc > 0 && k > 0, "non-positive dimension");
  g->c = c; g->h = h; g->w = w; g->kc = kc; g->kh = k; g->kw = k; g->stride = stride; g->pad = pad;
  const long long oh = (long long)(h - 1) * stride - 2 * pad + k + opad, ow = (long long)(w - 1) * stride - 2 * pad + k + opad;
  I8IE_REQUIRE(oh > 0 && ow > 0 && oh < (1 << 30) && ow < (1 << 30), "transposed conv: empty or oversized output");
  g->oh = (int)oh;
  g->ow = (int)ow;
  g->K = c * k * k;
  g->Kpad = round_up(g->K, 128);
  return I8IE_OK;
}

inline int chunk_images(const ConvGeom& g, int n) {
  const size_t per_img = (size_t)g.oh * g.ow * g.Kpad;
  size_t imgs = kColBudget / per_img;
  if (imgs < 1) imgs = 1;
  return imgs > (size_t)n ? n : (int)imgs;
}

// ---- v1 (fallback) runners ------------------------------------------------------------------
int conv_run_v1(i8ie_ctx* ctx, const uint8_t* in, int n, const ConvGeom& cg, const int8_t* Bpack, const int32_t* oc,
                const int32_t* wsum, uint8_t zp_in, float s_in, float s_w, float s_out, uint8_t zp_out, uint8_t* out,
                int32_t* acc, uint8_t* col, int imgs_per_chunk, const float* sbv = nullptr) {
  const int P = cg.oh * cg.ow;
  for (int i0 = 0; i0 < n; i0 += imgs_per_chunk) {
    const int nb = (n - i0) < imgs_per_chunk ? (n - i0) : imgs_per_chunk;
    I8IE_TRY(i8ie_launch_im2col(ctx, in + (size_t)i0 * cg.c * cg.h * cg.w, col, nb, cg.c, cg.h, cg.w, cg.kh, cg.kw,
                                cg.oh, cg.ow, cg.stride, cg.pad, cg.K, cg.Kpad, zp_in));
    I8ieGemmArgs g{};
    g.A = col;
    g.lda = cg.Kpad;
    g.Ka = cg.Kpad;
    g.M = nb * P;
    g.B = Bpack;
    g.Kpad = cg.Kpad;
    g.N = cg.kc;
    g.oc = oc;
    g.wsum = wsum;
    g.qb = nullptr;  // conv folds the bias into oc (src/conv2d.cc:123)
    g.s_in = s_in;
    g.s_w = s_w;
    g.s_out = s_out;
    g.zp_out = zp_out;
    g.out = out + (size_t)i0 * cg.kc * P;
    g.out_mode = I8IE_OUT_NCHW;
    g.P = P;
    g.acc = acc ? acc + (size_t)i0 * P * cg.kc : nullptr;
    g.Ktrue = cg.K;
    g.sbv = sbv;
    I8IE_TRY(i8ie_gemm_launch(ctx, g));
  }
  return I8IE_OK;
}

int linear_run_v1(i8ie_ctx* ctx, const uint8_t* in, int m, int k, const int8_t* Bpack, int Kpad, const int8_t* qb,
                  int n, const int32_t* oc, const int32_t* wsum, float s_in, float s_w, float s_out, uint8_t zp_out,
                  uint8_t* out, int32_t* acc, uint8_t* scratch, const float* sbv = nullptr) {
  I8ieGemmArgs g{};
  if (k % 16 != 0 || !aligned16(in)) {
    I8IE_TRY(i8ie_launch_pad_rows(ctx, in, m, k, scratch, m, Kpad, 0));
    g.A = scratch;
    g.lda = Kpad;
    g.Ka = Kpad;
  } else {
    g.A = in;
    g.lda = k;
    g.Ka = k;
  }
  g.M = m; g.B = Bpack; g.Kpad = Kpad; g.N = n; g.oc = oc; g.wsum = wsum; g.qb = qb;
  g.s_in = s_in; g.s_w = s_w; g.s_out = s_out; g.zp_out = zp_out;
  g.out = out; g.out_mode = I8IE_OUT_ROWMAJOR; g.P = 1; g.acc = acc; g.Ktrue = k; g.sbv = sbv;
  return i8ie_gemm_launch(ctx, g);
}

}  // namespace

struct i8ie_layer {
  i8ie_ctx* ctx = nullptr;
  bool conv = false;
  int n = 0, K = 0;  // out features, reduction length (reference K order)
  int c = 0, kh = 0, kw = 0, stride = 1, pad = 0;
  int Kpad = 0, Npad = 0;
  float s_w = 1.0f;
  float s_out = 1.0f;   // include/layer.h:46
  uint8_t zp_out = 0;   // include/layer.h:47
  int8_t* qw = nullptr;     // [n][K] as converted, K ordered (c, kh, kw)
  int8_t* qb = nullptr;     // [n]
  int8_t* Bpack = nullptr;  // [Npad][Kpad] zero padded, reference K order (Linear; conv path F)
  int8_t* Bperm = nullptr;  // Linear fed by an NHWC-flattened activation: Bpack with K reordered (h, w, c)
  int perm_c = 0, perm_hw = 0;
  int path = PATH_F;        // conv: PATH_A / PATH_B / PATH_F / PATH_G / PATH_T
  int groups = 1;           // conv, groups > 1 (PATH_G): K above is the reduction length INSIDE a group, (c / groups) * kh * kw,
  int Ngp = 0, Kgp = 0;     // and the weights live in `wc` as [groups][Ngp][Kgp], K ordered (kh, kw, cg) (i8ie_gconv.h)
  int8_t* Bg = nullptr;
  int* gtab = nullptr;      // the MFMA kernel's gather table (i8ie_gconv_ktab), in `wc` as well
  int opad = 0;             // ConvTranspose2d (PATH_T): output_padding; qw / K above are the EQUIVALENT matrix [n][c * k * k];
  int Kpp = 0;              // the phase panels [stride^2][Ngp][Kpp], their gather table and the per-(phase, feature) sums of
  int8_t* Bt = nullptr;     // the taps a phase does not see (i8ie_deconv.h), all three in `wc`
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

namespace {

int ensure_offsets(i8ie_layer* L, float s_in, uint8_t zp_in) {
  uint32_t a, b;
  memcpy(&a, &s_in, 4);
  memcpy(&b, &L->oc_s_in, 4);
  if (L->oc_valid && L->oc_zp_in == (int)zp_in && a == b) return I8IE_OK;
  // the reference recomputes this on every call (src/conv2d.cc:117-124); it only depends on
  // (s_in, zp_in), which are fixed once the network is converted
  i8ie_ctx* ctx = L->ctx;
  I8IE_TRY(i8ie_launch_offsets(ctx, L->conv, L->qw, L->qb, L->n, L->K, s_in, zp_in, L->oc, nullptr));
  I8IE_TRY(i8ie_launch_finish_offsets(ctx, L->oc, L->wsum, L->qb, s_in, L->n, L->ocp, L->conv ? nullptr : L->biasf));
  L->oc_valid = true;
  L->oc_s_in = s_in;
  L->oc_zp_in = zp_in;
  return I8IE_OK;
}

// per-channel layers: the multipliers for (s_in, s_out), computed on the host in double (as i8ie_make_requant does) and
// copied over the same buffer -- built by the eager run before a graph capture, never reallocated
int ensure_multipliers(i8ie_layer* L, float s_in) {
  if (!L->pc) return I8IE_OK;
  if (L->ms_valid && memcmp(&s_in, &L->ms_s_in, 4) == 0 && memcmp(&L->s_out, &L->ms_s_out, 4) == 0) return I8IE_OK;
  std::vector<float> ms((size_t)L->Npad, 0.0f);
  for (int j = 0; j < L->n; ++j) ms[j] = i8ie_requant_ms(s_in, L->sw_host[j], L->s_out);
  I8IE_TRY(i8ie_memcpy_h2d(L->ctx, L->msv, ms.data(), ms.size() * 4));
  L->ms_fast = i8ie_requant_pc_fast(s_in, L->sw_host.data(), L->n, L->s_out);
  L->ms_valid = true;
  L->ms_s_in = s_in;
  L->ms_s_out = L->s_out;
  return I8IE_OK;
}
// what the launchers get as s_w: the layer's scale, or for a per-channel layer the switch between the guarded estimate
// (1) and the exact sequence (0) that i8ie_make_requant reads off it (I8ieIgemmCall::msv)
inline float sw_arg(const i8ie_layer* L) { return L->pc ? (L->ms_fast ? 1.0f : 0.0f) : L->s_w; }
inline const float* msv_arg(const i8ie_layer* L) { return L->pc ? L->msv : nullptr; }
inline const float* sbv_arg(const i8ie_layer* L) { return L->pc ? L->swv : nullptr; }

bool force_fallback(const i8ie_ctx* ctx) { return (ctx->options & 1) != 0; }

}  // namespace

extern "C" {

int i8ie_ctx_set_option(i8ie_ctx* ctx, int option, int value) {
  I8IE_REQUIRE(ctx != nullptr, "null ctx");
  I8IE_REQUIRE(option == I8IE_OPT_FORCE_FALLBACK || option == I8IE_OPT_KERNEL_VARIANT ||
                   option == I8IE_OPT_PROFILE_STRIDE || option == I8IE_OPT_CU_LIMIT,
               "unknown option");
  if (option == I8IE_OPT_CU_LIMIT) {
    I8IE_REQUIRE(value >= 0, "CU limit must be >= 0");
    ctx->cu_limit = value;
    return I8IE_OK;
  }
  if (option == I8IE_OPT_PROFILE_STRIDE) {
    I8IE_REQUIRE(value >= 1, "profile stride must be >= 1");
    ctx->prof_stride = value;
    return I8IE_OK;
  }
  if (option == I8IE_OPT_KERNEL_VARIANT) {
    ctx->pick = i8ie_decode_variant(value);
    return I8IE_OK;
  }
  if (value)
    ctx->options |= 1;
  else
    ctx->options &= ~1;
  return I8IE_OK;
}

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

// ---- stateless entry points: any geometry, v1 kernels, caller supplies oc --------------------
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

static int layer_create(i8ie_ctx* ctx, bool conv, const int8_t* qw_host, const int8_t* qb_host, int n, int K, int c,
                        int kh, int kw, int stride, int pad, float s_w, i8ie_layer** out, int groups = 1, int opad = -1);

// the stateless form with groups (groups: not in the reference).  groups > 1 packs the weights for this one call: the
// device weights are read back, a temporary layer handle runs the call with the caller's oc[] and is destroyed.
int i8ie_conv2d_u8s8_grouped(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int kh,
                             int kw, int stride, int pad, int groups, uint8_t zp_in, const int32_t* oc, float s_in,
                             float s_w, float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  I8IE_REQUIRE(groups >= 1, "groups must be >= 1");
  I8IE_REQUIRE(c > 0 && kc > 0 && c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  if (groups == 1)
    return i8ie_conv2d_u8s8(ctx, in, n, c, h, w, qw, kc, kh, kw, stride, pad, zp_in, oc, s_in, s_w, s_out, zp_out, out, acc);
  I8IE_REQUIRE(ctx && in && qw && oc && out, "null argument");
  I8IE_REQUIRE(n > 0, "non-positive batch");
  ConvGeom cg;
  I8IE_TRY(conv_geom(c, h, w, kc, kh, kw, stride, pad, &cg));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int Kg = (c / groups) * kh * kw;
  std::vector<int8_t> qw_host((size_t)kc * Kg), qb_host((size_t)kc, 0);
  I8IE_TRY(i8ie_memcpy_d2h(ctx, qw_host.data(), qw, qw_host.size()));
  i8ie_layer* L = nullptr;
  I8IE_TRY(layer_create(ctx, true, qw_host.data(), qb_host.data(), kc, Kg, c, kh, kw, stride, pad, s_w, &L, groups));
  L->s_out = s_out;
  L->zp_out = zp_out;
  // the caller's offset vector (it carries the bias term) instead of the handle's own
  int rc = i8ie_launch_finish_offsets(ctx, oc, L->wsum, L->qb, s_in, kc, L->ocp, nullptr);
  if (rc == I8IE_OK) {
    L->oc_valid = true;
    L->oc_s_in = s_in;
    L->oc_zp_in = zp_in;
    rc = i8ie_layer_forward(L, in, n, h, w, s_in, zp_in, out, acc);
  }
  i8ie_layer_destroy(L);
  return rc;
}

// ---- NHWC helpers exposed on the ABI -----------------------------------------------------------
int i8ie_layout_convert_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int to_nhwc,
                           int border, uint8_t border_value) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && border >= 0, "bad dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  if (to_nhwc) {
    if (border > 0)
      I8IE_HIP_TRY(hipMemsetAsync(out, border_value, (size_t)n * (h + 2 * border) * (w + 2 * border) * c, ctx->stream));
    return i8ie_launch_nchw_to_nhwc(ctx, in, out, n, c, h, w, border);
  }
  return i8ie_launch_nhwc_to_nchw(ctx, in, out, n, c, h, w, border);
}

int i8ie_fill_border_u8(i8ie_ctx* ctx, uint8_t* buf, int n, int c, int h, int w, int border, uint8_t value) {
  I8IE_REQUIRE(ctx && buf, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && border >= 0, "bad dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return i8ie_launch_fill_border(ctx, buf, n, c, h, w, border, value);
}

int i8ie_maxpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, uint8_t* out, int out_border, int n,
                           int c, int h, int w, int k, int s) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(c % 16 == 0, "NHWC max-pool needs channels % 16 == 0");
  I8IE_REQUIRE(k > 0 && s > 0, "kernel_size and stride must be positive");
  I8IE_REQUIRE(k <= h && k <= w, "window larger than the input");
  I8IE_REQUIRE(aligned16(in) && aligned16(out), "buffers must be 16-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return i8ie_launch_maxpool_nhwc(ctx, in, in_border, out, out_border, n, c, h, w, k, s, 0);
}

// ---- layer handles ----------------------------------------------------------------------------
static int layer_create(i8ie_ctx* ctx, bool conv, const int8_t* qw_host, const int8_t* qb_host, int n, int K, int c,
                        int kh, int kw, int stride, int pad, float s_w, i8ie_layer** out, int groups, int opad) {
  I8IE_REQUIRE(ctx && qw_host && qb_host && out, "null argument");
  I8IE_REQUIRE(n > 0 && K > 0, "non-positive dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  i8ie_layer* L = new (std::nothrow) i8ie_layer();
  if (!L) return I8IE_ERR_OOM;
  L->ctx = ctx; L->conv = conv; L->n = n; L->K = K; L->c = c; L->kh = kh; L->kw = kw;
  L->stride = stride; L->pad = pad; L->s_w = s_w;
  L->Kpad = round_up(K, 128);
  L->Npad = round_up(n, 128);
  // MFMA-order weight panel for the implicit-GEMM conv paths, built on the host once
  std::vector<int8_t> pack2, packg;
  std::vector<int> gtab, ttab;
  std::vector<int8_t> packt;
  std::vector<int32_t> tph;
  if (conv && opad >= 0) {
    // transposed (opad: output_padding): qw_host is the equivalent matrix [n][c * k * k]
    L->path = PATH_T;
    L->opad = opad;
    L->Ngp = round_up(n, 16);
    L->Kpp = i8ie_deconv_kpitch(c, kh, stride);
    i8ie_deconv_pack(qw_host, n, c, kh, stride, packt, tph);
    i8ie_deconv_ktab(c, kh, stride, ttab);
  } else if (conv && groups > 1) {
    // grouped: qw_host is [n][Cg * kh * kw]; group g's Ng rows go to panel g in (kh, kw, cg) order
    const int Cg = c / groups, Ng = n / groups;
    L->path = PATH_G;
    L->groups = groups;
    L->Ngp = round_up(Ng, 16);
    L->Kgp = round_up(K, 64);
    packg.assign((size_t)groups * L->Ngp * L->Kgp, 0);
    for (int j = 0; j < n; ++j)
      for (int ch = 0; ch < Cg; ++ch)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x)
            packg[((size_t)(j / Ng) * L->Ngp + j % Ng) * L->Kgp + ((size_t)y * kw + x) * Cg + ch] =
                qw_host[(((size_t)j * Cg + ch) * kh + y) * kw + x];
    i8ie_gconv_ktab(Cg, kh, kw, L->Kgp, gtab);
  } else if (conv && c % 16 == 0) {
    L->path = PATH_A;
    L->K2 = kh * kw * c;
    L->Kpad2 = round_up(L->K2, 128);
    pack2.assign((size_t)L->Npad * L->Kpad2, 0);
    for (int j = 0; j < n; ++j)
      for (int ch = 0; ch < c; ++ch)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x)
            pack2[(size_t)j * L->Kpad2 + ((size_t)y * kw + x) * c + ch] = qw_host[(((size_t)j * c + ch) * kh + y) * kw + x];
  } else if (conv && c <= 4 && stride % 4 == 0) {
    L->path = PATH_B;
    L->kwg = (kw + 3) / 4;
    L->K2 = kh * L->kwg * 16;
    L->Kpad2 = round_up(L->K2, 128);
    pack2.assign((size_t)L->Npad * L->Kpad2, 0);
    for (int j = 0; j < n; ++j)
      for (int ch = 0; ch < c; ++ch)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x)
            pack2[(size_t)j * L->Kpad2 + ((size_t)y * L->kwg + x / 4) * 16 + (x % 4) * 4 + ch] =
                qw_host[(((size_t)j * c + ch) * kh + y) * kw + x];
  }
  std::vector<int8_t> packs;  // the same weights in the K order of the first-stage kernel (i8ie_stem.hip)
  if (L->path == PATH_B && c <= 3 && n % 32 == 0 && n <= 96 && (kh + 3) / 4 * ((kw + 3) / 4) * 48 <= 14 * 32) {
    L->KpadStem = i8ie_stem_kpad(kh, kw);
    packs.assign((size_t)n * L->KpadStem, 0);
    for (int j = 0; j < n; ++j)
      for (int ch = 0; ch < c; ++ch)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x)
            packs[(size_t)j * L->KpadStem + i8ie_stem_kindex(kw, ch, y, x)] = qw_host[(((size_t)j * c + ch) * kh + y) * kw + x];
  }
  int rc = I8IE_OK;
  do {
    if ((rc = i8ie_malloc(ctx, (size_t)n * K, (void**)&L->qw)) != I8IE_OK) break;
    if ((rc = i8ie_malloc(ctx, (size_t)n, (void**)&L->qb)) != I8IE_OK) break;
    if ((rc = i8ie_malloc(ctx, (size_t)L->Npad * L->Kpad, (void**)&L->Bpack)) != I8IE_OK) break;
    if ((rc = i8ie_malloc(ctx, (size_t)n * 4, (void**)&L->wsum)) != I8IE_OK) break;
    if ((rc = i8ie_malloc(ctx, (size_t)n * 4, (void**)&L->oc)) != I8IE_OK) break;
    if ((rc = i8ie_malloc(ctx, (size_t)L->Npad * 4, (void**)&L->ocp)) != I8IE_OK) break;  // padded: vector loads
    if ((rc = i8ie_malloc(ctx, (size_t)L->Npad * 4, (void**)&L->biasf)) != I8IE_OK) break;
    if ((rc = i8ie_memset(ctx, L->ocp, 0, (size_t)L->Npad * 4)) != I8IE_OK) break;
    if ((rc = i8ie_memset(ctx, L->biasf, 0, (size_t)L->Npad * 4)) != I8IE_OK) break;
    if ((rc = i8ie_memcpy_h2d(ctx, L->qw, qw_host, (size_t)n * K)) != I8IE_OK) break;
    if ((rc = i8ie_memcpy_h2d(ctx, L->qb, qb_host, (size_t)n)) != I8IE_OK) break;
    if ((rc = i8ie_launch_pad_rows(ctx, L->qw, n, K, L->Bpack, L->Npad, L->Kpad, 0)) != I8IE_OK) break;
    if ((rc = i8ie_launch_offsets(ctx, conv, L->qw, nullptr, n, K, 1.0f, 0, nullptr, L->wsum)) != I8IE_OK) break;
    if (!pack2.empty()) {
      if ((rc = i8ie_malloc(ctx, pack2.size(), (void**)&L->Bpack2)) != I8IE_OK) break;
      if ((rc = i8ie_memcpy_h2d(ctx, L->Bpack2, pack2.data(), pack2.size())) != I8IE_OK) break;
    }
    if (!packg.empty()) {  // (kept per packing key like the re-packed panels: never overwritten, freed with the layer)
      if ((rc = i8ie_malloc(ctx, packg.size(), (void**)&L->Bg)) != I8IE_OK) break;
      L->wc.ents.push_back({0x6763000000000001ull, L->Bg});
      if ((rc = i8ie_memcpy_h2d(ctx, L->Bg, packg.data(), packg.size())) != I8IE_OK) break;
      if ((rc = i8ie_malloc(ctx, gtab.size() * 4, (void**)&L->gtab)) != I8IE_OK) break;
      L->wc.ents.push_back({0x6763000000000002ull, L->gtab});
      if ((rc = i8ie_memcpy_h2d(ctx, L->gtab, gtab.data(), gtab.size() * 4)) != I8IE_OK) break;
    }
    if (!packt.empty()) {  // (per packing key as well)
      if ((rc = i8ie_malloc(ctx, packt.size(), (void**)&L->Bt)) != I8IE_OK) break;
      L->wc.ents.push_back({0x6463000000000001ull, L->Bt});
      if ((rc = i8ie_memcpy_h2d(ctx, L->Bt, packt.data(), packt.size())) != I8IE_OK) break;
      if ((rc = i8ie_malloc(ctx, ttab.size() * 4, (void**)&L->ttab)) != I8IE_OK) break;
      L->wc.ents.push_back({0x6463000000000002ull, L->ttab});
      if ((rc = i8ie_memcpy_h2d(ctx, L->ttab, ttab.data(), ttab.size() * 4)) != I8IE_OK) break;
      if ((rc = i8ie_malloc(ctx, tph.size() * 4, (void**)&L->tph)) != I8IE_OK) break;
      L->wc.ents.push_back({0x6463000000000003ull, L->tph});
      if ((rc = i8ie_memcpy_h2d(ctx, L->tph, tph.data(), tph.size() * 4)) != I8IE_OK) break;
    }
    if (!packs.empty()) {
      if ((rc = i8ie_malloc(ctx, packs.size(), (void**)&L->Bstem)) != I8IE_OK) break;
      if ((rc = i8ie_memcpy_h2d(ctx, L->Bstem, packs.data(), packs.size())) != I8IE_OK) break;
    }
  } while (0);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

// per-channel layers: the per-tensor handle plus s_w[n] (host copy, device [Npad]) and the multiplier buffer
static int layer_make_per_channel(i8ie_layer* L, const float* s_w_host) {
  const int n = L->n;
  L->pc = true;
  L->sw_host.assign(s_w_host, s_w_host + n);
  std::vector<float> sw((size_t)L->Npad, 1.0f);
  for (int j = 0; j < n; ++j) sw[j] = s_w_host[j];
  I8IE_TRY(i8ie_malloc(L->ctx, (size_t)L->Npad * 4, (void**)&L->swv));
  I8IE_TRY(i8ie_malloc(L->ctx, (size_t)L->Npad * 4, (void**)&L->msv));
  I8IE_TRY(i8ie_memcpy_h2d(L->ctx, L->swv, sw.data(), sw.size() * 4));
  return i8ie_memset(L->ctx, L->msv, 0, (size_t)L->Npad * 4);
}

// scales from the caller: finite and >= 0 (pooling the INT32 accumulators before the requantiser needs a monotone
// map per channel, DESIGN.md "Per-channel weight scales")
static int check_scales(const float* s_w, int n) {
  I8IE_REQUIRE(s_w != nullptr, "null argument");
  for (int j = 0; j < n; ++j) {
    if (!(s_w[j] >= 0.0f && s_w[j] <= 3.402823466e+38f)) {
      i8ie_set_error("per-channel weight scale %d is negative or not finite", j);
      return I8IE_ERR_ARG;
    }
  }
  return I8IE_OK;
}

int i8ie_linear_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k,
                                   const float* s_w_host, i8ie_layer** out) {
  I8IE_REQUIRE(out != nullptr && n > 0, "bad argument");
  I8IE_TRY(check_scales(s_w_host, n));
  i8ie_layer* L = nullptr;
  I8IE_TRY(i8ie_linear_create(ctx, qw_host, qb_host, n, k, 1.0f, &L));
  const int rc = layer_make_per_channel(L, s_w_host);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

int i8ie_conv2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh,
                                   int kw, int stride, int pad, const float* s_w_host, i8ie_layer** out) {
  I8IE_REQUIRE(out != nullptr && kc > 0, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  i8ie_layer* L = nullptr;
  I8IE_TRY(i8ie_conv2d_create(ctx, qw_host, qb_host, kc, c, kh, kw, stride, pad, 1.0f, &L));
  const int rc = layer_make_per_channel(L, s_w_host);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

int i8ie_layer_weight_scales(const i8ie_layer* L, float* out, int n, int* per_channel) {
  I8IE_REQUIRE(L && out && per_channel, "null argument");
  I8IE_REQUIRE(n == L->n, "n must be the layer's out features");
  for (int j = 0; j < n; ++j) out[j] = L->pc ? L->sw_host[j] : L->s_w;
  *per_channel = L->pc ? 1 : 0;
  return I8IE_OK;
}

int i8ie_linear_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k, float s_w,
                       i8ie_layer** out) {
  return layer_create(ctx, false, qw_host, qb_host, n, k, 0, 0, 0, 1, 0, s_w, out);
}

int i8ie_conv2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh, int kw,
                       int stride, int pad, float s_w, i8ie_layer** out) {
  I8IE_REQUIRE(c > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0, "stride must be positive");
  I8IE_REQUIRE(pad >= 0, "negative padding");
  return layer_create(ctx, true, qw_host, qb_host, kc, c * kh * kw, c, kh, kw, stride, pad, s_w, out);
}

// groups: not in the reference (src/conv2d.cc:100-142 per group).  Argument checks come before any device call.
static int check_groups(int kc, int c, int kh, int kw, int stride, int pad, int groups) {
  I8IE_REQUIRE(kc > 0 && c > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0, "stride must be positive");
  I8IE_REQUIRE(pad >= 0, "negative padding");
  I8IE_REQUIRE(groups >= 1, "groups must be >= 1");
  I8IE_REQUIRE(c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  I8IE_REQUIRE(groups <= 65535, "at most 65535 groups");
  return I8IE_OK;
}

int i8ie_conv2d_create_grouped(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int kh, int kw,
                               int stride, int pad, int groups, float s_w, i8ie_layer** out) {
  I8IE_TRY(check_groups(kc, c, kh, kw, stride, pad, groups));
  if (groups == 1) return i8ie_conv2d_create(ctx, qw_host, qb_host, kc, c, kh, kw, stride, pad, s_w, out);
  return layer_create(ctx, true, qw_host, qb_host, kc, (c / groups) * kh * kw, c, kh, kw, stride, pad, s_w, out, groups);
}

int i8ie_conv2d_create_grouped_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                                           int kh, int kw, int stride, int pad, int groups, const float* s_w_host,
                                           i8ie_layer** out) {
  I8IE_TRY(check_groups(kc, c, kh, kw, stride, pad, groups));
  if (groups == 1) return i8ie_conv2d_create_per_channel(ctx, qw_host, qb_host, kc, c, kh, kw, stride, pad, s_w_host, out);
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  i8ie_layer* L = nullptr;
  I8IE_TRY(i8ie_conv2d_create_grouped(ctx, qw_host, qb_host, kc, c, kh, kw, stride, pad, groups, 1.0f, &L));
  const int rc = layer_make_per_channel(L, s_w_host);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

int i8ie_layer_groups(const i8ie_layer* L, int* groups) {
  I8IE_REQUIRE(L && groups, "null argument");
  *groups = L->groups;
  return I8IE_OK;
}

// ConvTranspose2d: not in the reference (src/conv2d.cc:100-142 on the equivalent problem, include/i8ie_hip.h).  Argument
// checks (i8ie_deconv_check_args) come before any device call.
int i8ie_conv_transpose2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int k, int stride,
                                 int pad, int output_pad, float s_w, i8ie_layer** out) {
  I8IE_TRY(i8ie_deconv_check_args(kc, c, k, stride, pad, output_pad));
  return layer_create(ctx, true, qw_host, qb_host, kc, c * k * k, c, k, k, stride, pad, s_w, out, 1, output_pad);
}

int i8ie_conv_transpose2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int k,
                                             int stride, int pad, int output_pad, const float* s_w_host, i8ie_layer** out) {
  I8IE_TRY(i8ie_deconv_check_args(kc, c, k, stride, pad, output_pad));
  I8IE_REQUIRE(out != nullptr, "bad argument");
  I8IE_TRY(check_scales(s_w_host, kc));
  i8ie_layer* L = nullptr;
  I8IE_TRY(i8ie_conv_transpose2d_create(ctx, qw_host, qb_host, kc, c, k, stride, pad, output_pad, 1.0f, &L));
  const int rc = layer_make_per_channel(L, s_w_host);
  if (rc != I8IE_OK) {
    i8ie_layer_destroy(L);
    return rc;
  }
  *out = L;
  return I8IE_OK;
}

// the stateless form: qw is the equivalent matrix on the device; it is read back and packed for this one call (a temporary
// layer handle runs the call with the caller's oc[] and is destroyed), as i8ie_conv2d_u8s8_grouped does
int i8ie_conv_transpose2d_u8s8(i8ie_ctx* ctx, const uint8_t* in, int n, int c, int h, int w, const int8_t* qw, int kc, int k,
                               int stride, int pad, int output_pad, uint8_t zp_in, const int32_t* oc, float s_in, float s_w,
                               float s_out, uint8_t zp_out, uint8_t* out, int32_t* acc) {
  I8IE_TRY(i8ie_deconv_check_args(kc, c, k, stride, pad, output_pad));
  I8IE_REQUIRE(ctx && in && qw && oc && out, "null argument");
  I8IE_REQUIRE(n > 0, "non-positive batch");
  ConvGeom cg;
  I8IE_TRY(deconv_geom(c, h, w, kc, k, stride, pad, output_pad, &cg));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  std::vector<int8_t> qw_host((size_t)kc * cg.K), qb_host((size_t)kc, 0);
  I8IE_TRY(i8ie_memcpy_d2h(ctx, qw_host.data(), qw, qw_host.size()));
  i8ie_layer* L = nullptr;
  I8IE_TRY(i8ie_conv_transpose2d_create(ctx, qw_host.data(), qb_host.data(), kc, c, k, stride, pad, output_pad, s_w, &L));
  L->s_out = s_out;
  L->zp_out = zp_out;
  int rc = i8ie_launch_finish_offsets(ctx, oc, L->wsum, L->qb, s_in, kc, L->ocp, nullptr);
  if (rc == I8IE_OK) {
    L->oc_valid = true;
    L->oc_s_in = s_in;
    L->oc_zp_in = zp_in;
    rc = i8ie_layer_forward(L, in, n, h, w, s_in, zp_in, out, acc);
  }
  i8ie_layer_destroy(L);
  return rc;
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
  *pad = (L->conv && L->path != PATH_T) ? L->pad : 0;  // (a transposed layer reads no border)
  return I8IE_OK;
}

static int layer_forward_impl(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                              float s_in, uint8_t zp_in, int relu, int pool_k, int pool_s, uint8_t* out, int out_layout,
                              int out_border, int32_t* acc, float* out_f32);

int i8ie_layer_forward_fused(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                             float s_in, uint8_t zp_in, int relu, uint8_t* out, int out_layout, int out_border,
                             int32_t* acc) {
  I8IE_REQUIRE(out != nullptr, "null argument");
  return layer_forward_impl(L, in, in_layout, in_border, m, h, w, s_in, zp_in, relu, 0, 0, out, out_layout, out_border,
                            acc, nullptr);
}

int i8ie_layer_forward_pool(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                            float s_in, uint8_t zp_in, int relu, int pool_k, int pool_s, uint8_t* out, int out_layout,
                            int out_border, int32_t* acc) {
  I8IE_REQUIRE(L != nullptr && out != nullptr, "null argument");
  I8IE_REQUIRE(L->conv, "i8ie_layer_forward_pool: Conv2d layers only");
  I8IE_REQUIRE(pool_k > 0 && pool_s > 0, "kernel_size and stride must be positive");
  return layer_forward_impl(L, in, in_layout, in_border, m, h, w, s_in, zp_in, relu, pool_k, pool_s, out, out_layout,
                            out_border, acc, nullptr);
}

// dequantize(layer(x)) for a Linear layer: src/quantize_utils.cc:54-58 applied to the result of
// src/fully_connected.cc:22-52.  out_u8 may be null when the layer has at most 16 output features (the fused
// small-N kernel writes the FP32 values directly); otherwise it receives the u8 result as usual.
int i8ie_layer_forward_dequant(i8ie_layer* L, const uint8_t* in, int in_layout, int m, int h, int w, float s_in,
                               uint8_t zp_in, int relu, uint8_t* out_u8, float* out_f32) {
  I8IE_REQUIRE(L && out_f32, "null argument");
  I8IE_REQUIRE(!L->conv, "i8ie_layer_forward_dequant: Linear layers only");
  return layer_forward_impl(L, in, in_layout, 0, m, h, w, s_in, zp_in, relu, 0, 0, out_u8, I8IE_LAYOUT_NCHW, 0, nullptr,
                            out_f32);
}

// the first-stage kernel (i8ie_stem.hip) takes this conv layer at this output size (+ this pool behind it)?
static bool stem_takes(const i8ie_layer* L, const ConvGeom& cg, int pool_k, int pool_s) {
  return L->conv && L->path == PATH_B && L->Bstem != nullptr && !force_fallback(L->ctx) && !L->ctx->pick.no_stem &&
         i8ie_stem_supported(cg.c, cg.stride, L->n, cg.kh, cg.kw, cg.oh, cg.ow, pool_k, pool_s) != 0;
}

// would the patch-stationary kernel (i8ie_pconv.hip) take this conv launch, with this pool folded in and these
// re-biased layouts?  (it answers from the kernel choice, the geometry and the batch, as the dispatcher will; nothing is launched)
// (`out_border`: the border of the output the real call will write; the size limits of the kernel depend on it.  The layout
// negotiation queries below do not know it yet and ask with 0: layer_forward_impl asks again with the real one and runs the
// pool / the re-bias as launches of their own when the kernel then declines)
static bool pconv_probe(i8ie_layer* L, const ConvGeom& cg, int m, int in_border, int pool_k, int pool_s, bool a_s8, bool out_s8, int out_border = 0) {
  if (!L->conv || L->path != PATH_A || force_fallback(L->ctx) || !i8ie_conv_tries(L->ctx, I8IE_CONV_PCONV)) return false;
  const int b = in_border > cg.pad ? in_border : cg.pad;
  I8ieIgemmCall q{};
  q.amode = 1; q.M = m * cg.oh * cg.ow; q.B = L->Bpack2; q.Kpad = L->Kpad2; q.Npad = L->Npad;
  q.Kchunks = L->K2 / 16; q.N = L->n; q.wcache = &L->wc; q.OH = cg.oh; q.OW = cg.ow;
  q.Hp = cg.h + 2 * b; q.Wp = cg.w + 2 * b; q.C = cg.c; q.KH = cg.kh; q.KW = cg.kw; q.sh = q.sw = cg.stride;
  q.a_bytes = (size_t)m * q.Hp * q.Wp * cg.c;
  q.pool_k = pool_k; q.pool_s = pool_s; q.a_s8 = a_s8 ? 1 : 0; q.out_s8 = out_s8 ? 1 : 0; q.ob = out_border;
  return q.a_bytes < i8ie_igemm_chunk_limit() && i8ie_pconv_takes(L->ctx, q) == 1;
}

// route T: NHWC in and out of the kernel, one launch (no zero-insert, scatter or fill pass); the layout conversions around
// it as on the other routes.  The force-fallback option picks deconv_direct inside the launcher.  (NHWC_S8 and the pool have
// been taken off by the caller: plain bytes, no pool.)
static int forward_transposed(i8ie_layer* L, const ConvGeom& cg, const uint8_t* in, int in_layout, int in_border, int m,
                              float s_in, uint8_t zp_in, int relu, uint8_t* out, int out_layout, int out_border, int32_t* acc) {
  i8ie_ctx* ctx = L->ctx;
  const bool in_nchw = in_layout == I8IE_LAYOUT_NCHW, out_nchw = out_layout == I8IE_LAYOUT_NCHW;
  const size_t a_bytes = in_nchw ? i8ie_align_up((size_t)m * cg.c * cg.h * cg.w, 256) : 0;
  const size_t o_bytes = out_nchw ? i8ie_align_up((size_t)m * cg.kc * cg.oh * cg.ow, 256) : 0;
  if (a_bytes + o_bytes) I8IE_TRY(i8ie_ws_reserve(ctx, a_bytes + o_bytes + 256));
  uint8_t* ws = (uint8_t*)ctx->ws;
  if (in_nchw) I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, in, ws, m, cg.c, cg.h, cg.w, 0));
  I8ieDeconvCall d{};
  d.A = in_nchw ? ws : in; d.m = m; d.H = cg.h; d.W = cg.w; d.C = cg.c; d.ib = in_nchw ? 0 : in_border;
  d.OH = cg.oh; d.OW = cg.ow; d.k = cg.kh; d.s = cg.stride; d.p = cg.pad;
  d.N = L->n; d.Ngp = L->Ngp; d.Kpp = L->Kpp; d.Bp = L->Bt; d.ktab = L->ttab; d.ocp = L->ocp; d.tph = L->tph;
  d.msv = msv_arg(L); d.sbv = sbv_arg(L);
  d.s_in = s_in; d.s_w = sw_arg(L); d.s_out = L->s_out; d.zp_in = zp_in; d.zp_out = L->zp_out; d.relu = relu;
  d.out = out_nchw ? ws + a_bytes : out; d.ob = out_nchw ? 0 : out_border; d.acc = acc;
  I8IE_TRY(i8ie_deconv_launch(ctx, d));
  if (out_nchw) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, d.out, out, m, cg.kc, cg.oh, cg.ow, 0));
  return I8IE_OK;
}

static int layer_forward_impl(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                              float s_in, uint8_t zp_in, int relu, int pool_k, int pool_s, uint8_t* out, int out_layout,
                              int out_border, int32_t* acc, float* out_f32) {
  I8IE_REQUIRE(L && in, "null argument");
  I8IE_REQUIRE(out != nullptr || (out_f32 != nullptr && !L->conv), "null output");
  I8IE_REQUIRE(m > 0, "non-positive batch");
  I8IE_REQUIRE(in_layout >= I8IE_LAYOUT_NCHW && in_layout <= I8IE_LAYOUT_NHWC_S8 && out_layout >= I8IE_LAYOUT_NCHW &&
                   out_layout <= I8IE_LAYOUT_NHWC_S8,
               "bad layout tag");
  I8IE_REQUIRE(L->conv || (in_layout != I8IE_LAYOUT_NHWC_S8 && out_layout != I8IE_LAYOUT_NHWC_S8),
               "the re-biased layout applies to conv layers only");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "negative border");
  I8IE_REQUIRE(in_layout != I8IE_LAYOUT_NCHW || in_border == 0, "only NHWC tensors carry a border");
  I8IE_REQUIRE(out_layout != I8IE_LAYOUT_NCHW || out_border == 0, "only NHWC tensors carry a border");
  i8ie_ctx* ctx = L->ctx;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8IE_TRY(ensure_offsets(L, s_in, zp_in));
  I8IE_TRY(ensure_multipliers(L, s_in));

  if (!L->conv) {  // ---- Linear: row-major in / out -------------------------------------------------
    I8IE_REQUIRE(in_border == 0 && out_border == 0, "Linear tensors carry no border");
    // Rows that are a flattened NHWC activation [m][h][w][c] (the engine's layout between layers) instead of
    // the reference's flattened NCHW: same contraction with K walked in (h, w, c) order, so the weight panel
    // is permuted once per (c, h*w) and the input is used as it lies -- no transpose back to NCHW.  oc[] and
    // wsum[] are sums over all of K and keep the reference's accumulation order (they come from qw).
    const int hw = (in_layout == I8IE_LAYOUT_NHWC && h > 0 && w > 0) ? h * w : 1;
    const int8_t* panel = L->Bpack;
    if (hw > 1) {
      I8IE_REQUIRE(L->K % hw == 0, "Linear: in_features is not c * h * w for the given h, w");
      if (force_fallback(ctx) || L->K % 16 != 0 || !aligned16(in)) {
        // the any-geometry route wants reference order: transpose the input instead of the weights
        I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)m * L->K + (size_t)m * L->Kpad + (size_t)8 * m * L->n * 4 + 4096));
        uint8_t* t = (uint8_t*)ctx->ws + i8ie_align_up((size_t)m * L->Kpad + (size_t)8 * m * L->n * 4, 256) + 512;
        I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, in, t, m, L->K / hw, h, w, 0));
        return layer_forward_impl(L, t, I8IE_LAYOUT_NCHW, 0, m, 0, 0, s_in, zp_in, relu, 0, 0, out, out_layout, out_border,
                                  acc, out_f32);
      }
      if (L->Bperm == nullptr || L->perm_c != L->K / hw || L->perm_hw != hw) {
        if (L->Bperm == nullptr) I8IE_TRY(i8ie_malloc(ctx, (size_t)L->Npad * L->Kpad, (void**)&L->Bperm));
        I8IE_TRY(i8ie_launch_permute_k(ctx, L->Bpack, L->Bperm, L->Npad, L->Kpad, L->K, L->K / hw, hw));
        L->perm_c = L->K / hw;
        L->perm_hw = hw;
      }
      panel = L->Bperm;
    }
    const bool need_pad = (L->K % 16 != 0) || !aligned16(in);
    if (!force_fallback(ctx) && !need_pad && L->n <= i8ie_smalln_max_features()) {
      // classifier head: one wave per row, dot4 + wavefront reduction, epilogue (and dequantize) fused
      I8ieSmallNCall sc{};
      sc.A = in; sc.lda = (size_t)L->K; sc.M = m; sc.K = L->K; sc.B = panel; sc.Kpad = L->Kpad; sc.N = L->n;
      sc.ocp = L->ocp; sc.biasf = L->biasf; sc.s_in = s_in; sc.s_w = sw_arg(L); sc.s_out = L->s_out;
      sc.zp_out = L->zp_out; sc.relu = relu; sc.out = out; sc.acc = acc; sc.out_f32 = out_f32; sc.sbv = sbv_arg(L);
      return i8ie_launch_linear_smalln(ctx, sc);
    }
    I8IE_REQUIRE(out != nullptr, "i8ie_layer_forward_dequant: this layer needs the u8 output buffer as well");
    if (out_f32 != nullptr) {  // general shape: the ordinary forward, then the dequantize kernel
      I8IE_TRY(layer_forward_impl(L, in, in_layout, 0, m, h, w, s_in, zp_in, relu, 0, 0, out, I8IE_LAYOUT_NCHW, 0, acc, nullptr));
      return i8ie_dequantize_u8_f32(ctx, out, out_f32, (int64_t)m * L->n, L->s_out, L->zp_out);
    }
    if (force_fallback(ctx)) {
      if (need_pad) I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)m * L->Kpad));
      I8IE_TRY(linear_run_v1(ctx, in, m, L->K, L->Bpack, L->Kpad, L->qb, L->n, L->oc, L->wsum, s_in, L->s_w, L->s_out,
                             L->zp_out, out, acc, (uint8_t*)ctx->ws, sbv_arg(L)));
      if (relu) I8IE_TRY(i8ie_relu_u8(ctx, out, out, (int64_t)m * L->n, L->zp_out));
      return I8IE_OK;
    }
    I8ieIgemmCall c{};
    const int lin = ctx->pick.linear;
    // few rows: the one-launch kernel of i8ie_flin.hip
    const bool flin = !need_pad && lin != I8IE_LIN_TILED && L->K % 16 == 0 &&
                      i8ie_flin_wants(m, L->n, L->Kpad, lin == I8IE_LIN_FLIN || lin == I8IE_LIN_FLIN128);
    // split K when the output has too few tiles to fill the chip (small batch, or few features)
    const long tiles_m = (m + 127) / 128, blocks_est = tiles_m * ((L->n + 63) / 64);
    const int nk = L->Kpad / 128;
    int ksplit = 1;
    // many rows: the one-launch kernel of i8ie_mlin.hip
    const bool mlin = !need_pad && !flin && lin != I8IE_LIN_TILED && lin != I8IE_LIN_TILED_MANY && L->K % 16 == 0 &&
                      aligned16(out) && L->Npad % 128 == 0 &&
                      i8ie_mlin_wants(m, L->n, L->Kpad, lin == I8IE_LIN_MLIN || lin == I8IE_LIN_MLIN64 || lin == I8IE_LIN_MLIN128);
    if (blocks_est < 256 && nk >= 4 && !flin && !mlin) {
      ksplit = (int)((512 + blocks_est - 1) / blocks_est);
      if (ksplit > 8) ksplit = 8;
      if (ksplit > nk / 2) ksplit = nk / 2;
    }
    const size_t pad_bytes = need_pad ? i8ie_align_up((size_t)m * L->Kpad, 256) : 0;
    const size_t part_bytes = ksplit > 1 ? (size_t)ksplit * m * L->n * 4 : 0;
    if (pad_bytes + part_bytes) I8IE_TRY(i8ie_ws_reserve(ctx, pad_bytes + part_bytes));
    c.ksplit = ksplit;
    c.partial = ksplit > 1 ? (int32_t*)((uint8_t*)ctx->ws + pad_bytes) : nullptr;
    if (need_pad) {
      I8IE_TRY(i8ie_launch_pad_rows(ctx, in, m, L->K, ctx->ws, m, L->Kpad, 0));
      c.A = (const uint8_t*)ctx->ws;
      c.lda = L->Kpad;
      c.Kchunks = L->Kpad / 16;
    } else {
      c.A = in;
      c.lda = L->K;
      c.Kchunks = L->K / 16;
    }
    c.a_bytes = (size_t)m * c.lda;
    c.amode = 0; c.M = m;
    c.B = panel; c.Kpad = L->Kpad; c.Npad = L->Npad; c.N = L->n; c.ocp = L->ocp; c.biasf = L->biasf;
    c.s_in = s_in; c.s_w = sw_arg(L); c.s_out = L->s_out; c.zp_out = L->zp_out; c.relu = relu;
    c.out = out; c.ob = 0; c.acc = acc; c.Ktrue = L->K; c.msv = msv_arg(L); c.sbv = sbv_arg(L);
    if (flin) return i8ie_flin_launch(ctx, c);
    if (mlin) return i8ie_mlin_launch(ctx, c);
    return i8ie_igemm_launch(ctx, c);
  }

  // ---- Conv2d --------------------------------------------------------------------------------
  ConvGeom cg;
  if (L->path == PATH_T)
    I8IE_TRY(deconv_geom(L->c, h, w, L->n, L->kh, L->stride, L->pad, L->opad, &cg));
  else
    I8IE_TRY(conv_geom(L->c, h, w, L->n, L->kh, L->kw, L->stride, L->pad, &cg));
  const bool pool = i8ie_is_pool(pool_k, pool_s);
  if (pool) I8IE_REQUIRE(pool_k <= cg.oh && pool_k <= cg.ow, "max-pool window larger than the convolution's output");
  const bool in_s8 = in_layout == I8IE_LAYOUT_NHWC_S8, out_s8 = out_layout == I8IE_LAYOUT_NHWC_S8;
  // Which kernel folds what: the first-stage kernel (path B) pools and can store re-biased; the patch-stationary kernel
  // (path A) pools, reads and stores re-biased -- when it takes the launch at all (batch, geometry, LDS: asked below).
  // Everything else: the plain call, with the pool / the re-bias as launches of their own around it.
  const bool stem = stem_takes(L, cg, pool ? pool_k : 0, pool_s) && (acc == nullptr || aligned16(acc));
  bool pconv = false;
  if (!stem && (pool || in_s8 || out_s8) && out_layout != I8IE_LAYOUT_NCHW && aligned16(in) && aligned16(out) &&
      (acc == nullptr || aligned16(acc)))
    pconv = pconv_probe(L, cg, m, in_border, pool ? pool_k : 0, pool_s, in_s8, out_s8, out_border);
  if (in_s8 && !pconv) {  // nobody reads the re-biased bytes as they are: plain copy first
    const size_t bytes = (size_t)m * (cg.h + 2 * in_border) * (cg.w + 2 * in_border) * cg.c;
    uint8_t* tmp = nullptr;
    I8IE_TRY(i8ie_malloc(ctx, bytes, (void**)&tmp));
    int rc = i8ie_rebias_u8(ctx, in, tmp, (int64_t)bytes);
    if (rc == I8IE_OK)
      rc = layer_forward_impl(L, tmp, I8IE_LAYOUT_NHWC, in_border, m, h, w, s_in, zp_in, relu, pool_k, pool_s, out, out_layout,
                              out_border, acc, nullptr);
    i8ie_free(ctx, tmp);
    return rc;
  }
  if (out_s8 && !pconv && !stem) {  // plain result into a temporary, re-biased, then laid into `out` with its border
    const int oph = pool ? (cg.oh - pool_k) / pool_s + 1 : cg.oh, opw = pool ? (cg.ow - pool_k) / pool_s + 1 : cg.ow;
    const size_t bytes = (size_t)m * L->n * oph * opw;
    I8IE_REQUIRE(L->n % 16 == 0, "re-biased NHWC output needs out features % 16 == 0");
    uint8_t* tmp = nullptr;
    I8IE_TRY(i8ie_malloc(ctx, bytes, (void**)&tmp));
    int rc = layer_forward_impl(L, in, in_layout, in_border, m, h, w, s_in, zp_in, relu, pool_k, pool_s, tmp, I8IE_LAYOUT_NHWC, 0,
                                acc, nullptr);
    if (rc == I8IE_OK) rc = i8ie_rebias_u8(ctx, tmp, tmp, (int64_t)bytes);
    if (rc == I8IE_OK) rc = i8ie_launch_reborder(ctx, tmp, out, m, L->n, oph, opw, 0, out_border, L->zp_out ^ 0x80);
    i8ie_free(ctx, tmp);
    return rc;
  }
  if (pool && !stem && !pconv) {
    // no kernel fuses this pool: max_pool2d<u8> (src/functional.cc:36-64) as its own launch behind the convolution
    const int oph = (cg.oh - pool_k) / pool_s + 1, opw = (cg.ow - pool_k) / pool_s + 1;
    const bool nhwc = out_layout == I8IE_LAYOUT_NHWC && L->n % 16 == 0;
    uint8_t* tmp = nullptr;
    I8IE_TRY(i8ie_malloc(ctx, (size_t)m * L->n * cg.oh * cg.ow, (void**)&tmp));
    int rc = layer_forward_impl(L, in, in_layout, in_border, m, h, w, s_in, zp_in, relu, 0, 0, tmp,
                                nhwc ? I8IE_LAYOUT_NHWC : I8IE_LAYOUT_NCHW, 0, acc, nullptr);
    if (rc == I8IE_OK) {
      if (nhwc) {
        rc = i8ie_launch_maxpool_nhwc(ctx, tmp, 0, out, out_border, m, L->n, cg.oh, cg.ow, pool_k, pool_s, 0);
      } else if (out_layout == I8IE_LAYOUT_NCHW) {
        rc = i8ie_maxpool2d_u8(ctx, tmp, out, m, L->n, cg.oh, cg.ow, pool_k, pool_s);
      } else {  // NHWC result with channels % 16 != 0: pool in NCHW, then lay out
        uint8_t* tmp2 = nullptr;
        rc = i8ie_malloc(ctx, (size_t)m * L->n * oph * opw, (void**)&tmp2);
        if (rc == I8IE_OK) rc = i8ie_maxpool2d_u8(ctx, tmp, tmp2, m, L->n, cg.oh, cg.ow, pool_k, pool_s);
        if (rc == I8IE_OK) rc = i8ie_launch_nchw_to_nhwc(ctx, tmp2, out, m, L->n, oph, opw, out_border);
        i8ie_free(ctx, tmp2);
      }
    }
    i8ie_free(ctx, tmp);
    return rc;
  }
  const int ph = pool ? (cg.oh - pool_k) / pool_s + 1 : cg.oh, pw = pool ? (cg.ow - pool_k) / pool_s + 1 : cg.ow;
  const size_t in_bytes = (size_t)m * cg.c * cg.h * cg.w;
  const size_t out_bytes = (size_t)m * cg.kc * ph * pw;
  const int path = (L->path == PATH_G || L->path == PATH_T) ? L->path : (force_fallback(ctx) ? PATH_F : L->path);

  if (path == PATH_T) return forward_transposed(L, cg, in, in_layout, in_border, m, s_in, zp_in, relu, out, out_layout, out_border, acc);

  if (path == PATH_G) {
    // grouped: NHWC in and out of the kernel (the input's own border serves, or bounds checks against zp_in); the layout
    // conversions around it as on the other paths.  The force-fallback option picks gconv_direct inside the launcher.
    const bool in_nchw = in_layout == I8IE_LAYOUT_NCHW, out_nchw = out_layout == I8IE_LAYOUT_NCHW;
    const size_t a_bytes = in_nchw ? i8ie_align_up(in_bytes, 256) : 0;
    const size_t o_bytes = out_nchw ? i8ie_align_up(out_bytes, 256) : 0;
    if (a_bytes + o_bytes) I8IE_TRY(i8ie_ws_reserve(ctx, a_bytes + o_bytes + 256));
    uint8_t* ws = (uint8_t*)ctx->ws;
    if (in_nchw) I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, in, ws, m, cg.c, cg.h, cg.w, 0));
    I8ieGconvCall g{};
    g.A = in_nchw ? ws : in; g.m = m; g.H = cg.h; g.W = cg.w; g.C = cg.c; g.ib = in_nchw ? 0 : in_border;
    g.OH = cg.oh; g.OW = cg.ow; g.stride = cg.stride; g.pad = cg.pad; g.KH = cg.kh; g.KW = cg.kw;
    g.groups = L->groups; g.Cg = cg.c / L->groups; g.Ng = L->n / L->groups; g.Ngp = L->Ngp; g.Kgp = L->Kgp;
    g.Bp = L->Bg; g.ktab = L->gtab; g.ocp = L->ocp; g.msv = msv_arg(L); g.sbv = sbv_arg(L);
    g.s_in = s_in; g.s_w = sw_arg(L); g.s_out = L->s_out; g.zp_in = zp_in; g.zp_out = L->zp_out; g.relu = relu;
    g.out = out_nchw ? ws + a_bytes : out; g.ob = out_nchw ? 0 : out_border; g.acc = acc;
    I8IE_TRY(i8ie_gconv_launch(ctx, g));
    if (out_nchw) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, g.out, out, m, cg.kc, cg.oh, cg.ow, 0));
    return I8IE_OK;
  }

  if (path == PATH_F) {
    const int ipc = chunk_images(cg, m);
    const size_t col_bytes = i8ie_align_up((size_t)ipc * cg.oh * cg.ow * cg.Kpad, 256);
    const size_t a_bytes = in_layout == I8IE_LAYOUT_NHWC ? i8ie_align_up(in_bytes, 256) : 0;
    const size_t o_bytes = out_layout == I8IE_LAYOUT_NHWC ? i8ie_align_up(out_bytes, 256) : 0;
    I8IE_TRY(i8ie_ws_reserve(ctx, col_bytes + a_bytes + o_bytes));
    uint8_t* ws = (uint8_t*)ctx->ws;
    uint8_t* col = ws;
    const uint8_t* src = in;
    if (a_bytes) {
      I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, in, ws + col_bytes, m, cg.c, cg.h, cg.w, in_border));
      src = ws + col_bytes;
    }
    uint8_t* dst = o_bytes ? ws + col_bytes + a_bytes : out;
    I8IE_TRY(conv_run_v1(ctx, src, m, cg, L->Bpack, L->oc, L->wsum, zp_in, s_in, L->s_w, L->s_out, L->zp_out, dst, acc,
                         col, ipc, sbv_arg(L)));
    if (relu) I8IE_TRY(i8ie_relu_u8(ctx, dst, dst, (int64_t)out_bytes, L->zp_out));
    if (o_bytes) {
      I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, dst, out, m, cg.kc, cg.oh, cg.ow, out_border));
    }
    return I8IE_OK;
  }

  I8ieIgemmCall c{};
  c.amode = 1; c.M = m * cg.oh * cg.ow;
  c.B = L->Bpack2; c.Kpad = L->Kpad2; c.Npad = L->Npad; c.Kchunks = L->K2 / 16; c.N = L->n; c.ocp = L->ocp;
  c.biasf = nullptr; c.wcache = &L->wc;
  c.s_in = s_in; c.s_w = sw_arg(L); c.s_out = L->s_out; c.zp_out = L->zp_out; c.relu = relu;
  c.acc = acc; c.Ktrue = cg.K; c.OH = cg.oh; c.OW = cg.ow; c.msv = msv_arg(L); c.sbv = sbv_arg(L);
  if (pconv) {  // (the patch-stationary kernel said it takes this launch as it is)
    c.pool_k = pool ? pool_k : 0; c.pool_s = pool_s; c.a_s8 = in_s8 ? 1 : 0; c.out_s8 = out_s8 ? 1 : 0;
  }
  const size_t o_bytes = out_layout == I8IE_LAYOUT_NCHW ? i8ie_align_up(out_bytes, 256) : 0;

  if (path == PATH_A) {
    const int Hp = cg.h + 2 * cg.pad, Wp = cg.w + 2 * cg.pad;
    const bool direct = in_layout != I8IE_LAYOUT_NCHW && in_border >= cg.pad && aligned16(in);
    const size_t a_bytes = direct ? 0 : i8ie_align_up((size_t)m * Hp * Wp * cg.c, 256);
    I8IE_TRY(i8ie_ws_reserve(ctx, a_bytes + o_bytes + 256));
    uint8_t* ws = (uint8_t*)ctx->ws;
    if (direct) {
      const int iHp = cg.h + 2 * in_border, iWp = cg.w + 2 * in_border, d = in_border - cg.pad;
      const size_t shift = ((size_t)d * iWp + d) * cg.c;
      c.A = in + shift;
      c.a_bytes = (size_t)m * iHp * iWp * cg.c - shift;
      c.Hp = iHp; c.Wp = iWp;
    } else {
      if (in_layout != I8IE_LAYOUT_NCHW) {  // (re-biased bytes are copied as they are; their border value is zp ^ 0x80)
        I8IE_TRY(i8ie_launch_reborder(ctx, in, ws, m, cg.c, cg.h, cg.w, in_border, cg.pad, in_s8 ? (zp_in ^ 0x80) : zp_in));
      } else {
        if (cg.pad > 0) I8IE_HIP_TRY(hipMemsetAsync(ws, zp_in, (size_t)m * Hp * Wp * cg.c, ctx->stream));
        I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, in, ws, m, cg.c, cg.h, cg.w, cg.pad));
      }
      c.A = ws;
      c.a_bytes = (size_t)m * Hp * Wp * cg.c;
      c.Hp = Hp; c.Wp = Wp;
    }
    c.C = cg.c; c.KH = cg.kh; c.KW = cg.kw; c.sh = c.sw = cg.stride;
    c.out = o_bytes ? ws + a_bytes : out;
  } else {  // PATH_B: small-C, stride % 4 == 0
    const int Hp = (cg.oh - 1) * cg.stride + cg.kh;
    const int Wg = (cg.ow - 1) * (cg.stride / 4) + L->kwg;
    const size_t t_bytes = in_layout != I8IE_LAYOUT_NCHW ? i8ie_align_up(in_bytes, 256) : 0;
    const size_t r_bytes = i8ie_align_up((size_t)m * Hp * Wg * 16, 256);
    if (stem && (acc == nullptr || aligned16(acc))) {
      // first-stage kernel (i8ie_stem.hip): space-to-depth image, conv (+ relu) (+ max-pool) in one contraction launch
      const size_t s_bytes = i8ie_align_up(i8ie_stem_scratch_bytes(m, cg.kh, cg.kw, cg.stride, cg.oh, cg.ow), 256);
      I8IE_TRY(i8ie_ws_reserve(ctx, t_bytes + s_bytes + o_bytes + 256));
      uint8_t* ws = (uint8_t*)ctx->ws;
      const uint8_t* src = in;
      if (t_bytes) {
        I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, in, ws, m, cg.c, cg.h, cg.w, in_border));
        src = ws;
      }
      uint8_t* dst = o_bytes ? ws + t_bytes + s_bytes : out;
      I8ieStemCall f{};
      f.x = nullptr; f.xu8 = src; f.scratch = ws + t_bytes;
      f.n = m; f.c = cg.c; f.h = cg.h; f.w = cg.w; f.q_scale = s_in; f.q_zp = zp_in;
      f.KH = cg.kh; f.KW = cg.kw; f.stride = cg.stride; f.pad = cg.pad; f.OH = cg.oh; f.OW = cg.ow;
      f.B = L->Bstem; f.Kpad = L->KpadStem; f.N = L->n; f.ocp = L->ocp;
      f.s_in = s_in; f.s_w = sw_arg(L); f.s_out = L->s_out; f.zp_out = L->zp_out; f.relu = relu;
      f.pool_k = pool ? pool_k : 0; f.pool_s = pool_s;
      f.out = dst; f.ob = o_bytes ? 0 : out_border; f.out_s8 = out_s8 ? 1 : 0; f.acc = acc;
      f.msv = msv_arg(L); f.sbv = sbv_arg(L);
      I8IE_TRY(i8ie_stem_launch(ctx, f));
      if (o_bytes) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, dst, out, m, cg.kc, ph, pw, 0));
      return I8IE_OK;
    }
    I8IE_TRY(i8ie_ws_reserve(ctx, t_bytes + r_bytes + o_bytes + 256));
    uint8_t* ws = (uint8_t*)ctx->ws;
    const uint8_t* src = in;
    if (t_bytes) {
      I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, in, ws, m, cg.c, cg.h, cg.w, in_border));
      src = ws;
    }
    uint8_t* rep = ws + t_bytes;
    const bool wstat = (acc == nullptr || (L->n % 4 == 0 && aligned16(acc))) && i8ie_first_supported(cg.c, cg.stride, L->n, L->K2, cg.kh, L->kwg, cg.ow);
    I8IE_TRY(i8ie_launch_repack_smallc(ctx, src, rep, m, cg.c, cg.h, cg.w, Hp, Wg, cg.pad, cg.pad, zp_in, wstat));
    if (wstat) {
      // weights-stationary small-C kernel (i8ie_first.hip) on the grouped image
      uint8_t* dst = o_bytes ? ws + t_bytes + r_bytes : out;
      const int ob = o_bytes ? 0 : out_border;
      I8ieFirstCall f{};
      f.x = nullptr; f.grouped = rep; f.scratch = nullptr;
      f.n = m; f.c = cg.c; f.h = cg.h; f.w = cg.w; f.q_scale = s_in; f.q_zp = zp_in;
      f.KH = cg.kh; f.KW = cg.kw; f.KWG = L->kwg; f.stride = cg.stride; f.pad = cg.pad; f.OH = cg.oh; f.OW = cg.ow;
      f.B = L->Bpack2; f.Kpad = L->Kpad2; f.K2 = L->K2; f.N = L->n; f.ocp = L->ocp;
      f.s_in = s_in; f.s_w = sw_arg(L); f.s_out = L->s_out; f.zp_out = L->zp_out; f.relu = relu;
      f.out = dst; f.ob = ob; f.acc = acc; f.msv = msv_arg(L); f.sbv = sbv_arg(L);
      I8IE_TRY(i8ie_first_launch(ctx, f));
      if (o_bytes) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, dst, out, m, cg.kc, cg.oh, cg.ow, 0));
      return I8IE_OK;
    }
    c.A = rep;
    c.a_bytes = (size_t)m * Hp * Wg * 16;
    c.Hp = Hp; c.Wp = Wg; c.C = 16; c.KH = cg.kh; c.KW = L->kwg;
    c.sh = cg.stride; c.sw = cg.stride / 4;
    c.out = o_bytes ? ws + t_bytes + r_bytes : out;
  }
  c.ob = o_bytes ? 0 : out_border;
  I8IE_TRY(i8ie_igemm_launch(ctx, c));
  if (o_bytes) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, c.out, out, m, cg.kc, cg.oh, cg.ow, 0));
  return I8IE_OK;
}

int i8ie_layer_accepts_f32_input(const i8ie_layer* L, int h, int w, int* yes) {
  I8IE_REQUIRE(L && yes, "null argument");
  *yes = 0;
  if (!L->conv || L->path != PATH_B || force_fallback(L->ctx)) return I8IE_OK;
  ConvGeom cg;
  if (conv_geom(L->c, h, w, L->n, L->kh, L->kw, L->stride, L->pad, &cg) != I8IE_OK) return I8IE_OK;
  *yes = (stem_takes(L, cg, 0, 0) || i8ie_first_supported(L->c, L->stride, L->n, L->K2, L->kh, L->kwg, cg.ow)) ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_fuses_pool(const i8ie_layer* L, int m, int h, int w, int pool_k, int pool_s, int* yes) {
  I8IE_REQUIRE(L && yes, "null argument");
  *yes = 0;
  if (!L->conv || L->path == PATH_T || pool_k < 1 || pool_s < 1 || m < 1) return I8IE_OK;
  ConvGeom cg;
  if (conv_geom(L->c, h, w, L->n, L->kh, L->kw, L->stride, L->pad, &cg) != I8IE_OK) return I8IE_OK;
  if (pool_k > cg.oh || pool_k > cg.ow) return I8IE_OK;
  *yes = (stem_takes(L, cg, pool_k, pool_s) || pconv_probe(const_cast<i8ie_layer*>(L), cg, m, cg.pad, pool_k, pool_s, false, false)) ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_rebiased_io(const i8ie_layer* L, int m, int h, int w, int pool_k, int pool_s, int* reads, int* stores) {
  I8IE_REQUIRE(L && reads && stores, "null argument");
  *reads = *stores = 0;
  if (!L->conv || L->path == PATH_T || m < 1) return I8IE_OK;
  ConvGeom cg;
  if (conv_geom(L->c, h, w, L->n, L->kh, L->kw, L->stride, L->pad, &cg) != I8IE_OK) return I8IE_OK;
  const bool pool = i8ie_is_pool(pool_k, pool_s);
  if (pool && (pool_s < 1 || pool_k > cg.oh || pool_k > cg.ow)) return I8IE_OK;
  i8ie_layer* Lm = const_cast<i8ie_layer*>(L);
  *reads = pconv_probe(Lm, cg, m, cg.pad, pool ? pool_k : 0, pool_s, true, false) ? 1 : 0;
  *stores = (stem_takes(L, cg, pool ? pool_k : 0, pool_s) || pconv_probe(Lm, cg, m, cg.pad, pool ? pool_k : 0, pool_s, false, true)) ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_forward_f32_input_pool(i8ie_layer* L, const float* in, int m, int h, int w, float q_scale, uint8_t q_zp,
                                      int relu, int pool_k, int pool_s, uint8_t* out, int out_layout, int out_border,
                                      int32_t* acc) {
  I8IE_REQUIRE(L && in && out, "null argument");
  I8IE_REQUIRE(out_layout == I8IE_LAYOUT_NHWC || out_layout == I8IE_LAYOUT_NHWC_S8, "the fused first layer writes NHWC (plain or re-biased)");
  I8IE_REQUIRE(m > 0 && out_border >= 0, "bad argument");
  int yes = 0;
  I8IE_TRY(i8ie_layer_accepts_f32_input(L, h, w, &yes));
  if (!yes) {
    i8ie_set_error("i8ie_layer_forward_f32_input: layer/geometry not supported by the fused first-layer kernels");
    return I8IE_ERR_STATE;
  }
  i8ie_ctx* ctx = L->ctx;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8IE_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0, "output must be 16-byte aligned");
  I8IE_REQUIRE(acc == nullptr || aligned16(acc), "accumulator buffer must be 16-byte aligned");
  I8IE_TRY(ensure_offsets(L, q_scale, q_zp));
  I8IE_TRY(ensure_multipliers(L, q_scale));
  ConvGeom cg;
  I8IE_TRY(conv_geom(L->c, h, w, L->n, L->kh, L->kw, L->stride, L->pad, &cg));
  const bool pool = i8ie_is_pool(pool_k, pool_s);
  if (pool) {
    I8IE_REQUIRE(pool_s > 0 && pool_k <= cg.oh && pool_k <= cg.ow, "max-pool window larger than the convolution's output");
  }
  if (stem_takes(L, cg, pool ? pool_k : 0, pool_s)) {
    I8IE_TRY(i8ie_ws_reserve(ctx, i8ie_stem_scratch_bytes(m, cg.kh, cg.kw, cg.stride, cg.oh, cg.ow) + 256));
    I8ieStemCall f{};
    f.x = in; f.xu8 = nullptr; f.scratch = (uint8_t*)ctx->ws;
    f.n = m; f.c = cg.c; f.h = h; f.w = w; f.q_scale = q_scale; f.q_zp = q_zp;
    f.KH = cg.kh; f.KW = cg.kw; f.stride = cg.stride; f.pad = cg.pad; f.OH = cg.oh; f.OW = cg.ow;
    f.B = L->Bstem; f.Kpad = L->KpadStem; f.N = L->n; f.ocp = L->ocp;
    f.s_in = q_scale; f.s_w = sw_arg(L); f.s_out = L->s_out; f.zp_out = L->zp_out; f.relu = relu;
    f.pool_k = pool ? pool_k : 0; f.pool_s = pool_s;
    f.out = out; f.ob = out_border; f.out_s8 = out_layout == I8IE_LAYOUT_NHWC_S8 ? 1 : 0; f.acc = acc;
    f.msv = msv_arg(L); f.sbv = sbv_arg(L);
    return i8ie_stem_launch(ctx, f);
  }
  if (pool || out_layout == I8IE_LAYOUT_NHWC_S8) {
    // the older first-layer kernel neither pools nor stores re-biased: conv (+ relu) into a temporary, then the rest
    I8IE_REQUIRE(L->n % 16 == 0, "i8ie_layer_forward_f32_input_pool: out features % 16 != 0");
    const int oph = pool ? (cg.oh - pool_k) / pool_s + 1 : cg.oh, opw = pool ? (cg.ow - pool_k) / pool_s + 1 : cg.ow;
    uint8_t *tmp = nullptr, *tmp2 = nullptr;
    I8IE_TRY(i8ie_malloc(ctx, (size_t)m * L->n * cg.oh * cg.ow, (void**)&tmp));
    int rc = i8ie_layer_forward_f32_input_pool(L, in, m, h, w, q_scale, q_zp, relu, 0, 0, tmp, I8IE_LAYOUT_NHWC, 0, acc);
    if (rc == I8IE_OK && out_layout == I8IE_LAYOUT_NHWC) {
      rc = i8ie_launch_maxpool_nhwc(ctx, tmp, 0, out, out_border, m, L->n, cg.oh, cg.ow, pool_k, pool_s, 0);
    } else if (rc == I8IE_OK) {
      uint8_t* plain = tmp;
      if (pool) {
        rc = i8ie_malloc(ctx, (size_t)m * L->n * oph * opw, (void**)&tmp2);
        if (rc == I8IE_OK) rc = i8ie_launch_maxpool_nhwc(ctx, tmp, 0, tmp2, 0, m, L->n, cg.oh, cg.ow, pool_k, pool_s, 0);
        plain = tmp2;
      }
      if (rc == I8IE_OK) rc = i8ie_rebias_u8(ctx, plain, plain, (int64_t)m * L->n * oph * opw);
      if (rc == I8IE_OK) rc = i8ie_launch_reborder(ctx, plain, out, m, L->n, oph, opw, 0, out_border, L->zp_out ^ 0x80);
    }
    i8ie_free(ctx, tmp);
    if (tmp2) i8ie_free(ctx, tmp2);
    return rc;
  }
  I8IE_TRY(i8ie_ws_reserve(ctx, i8ie_first_scratch_bytes(m, cg.kh, L->kwg, cg.stride, cg.oh, cg.ow) + 256));
  I8ieFirstCall c{};
  c.x = in; c.grouped = nullptr; c.scratch = (uint8_t*)ctx->ws;
  c.n = m; c.c = cg.c; c.h = h; c.w = w; c.q_scale = q_scale; c.q_zp = q_zp;
  c.KH = cg.kh; c.KW = cg.kw; c.KWG = L->kwg; c.stride = cg.stride; c.pad = cg.pad; c.OH = cg.oh; c.OW = cg.ow;
  c.B = L->Bpack2; c.Kpad = L->Kpad2; c.K2 = L->K2; c.N = L->n; c.ocp = L->ocp;
  c.s_in = q_scale; c.s_w = sw_arg(L); c.s_out = L->s_out; c.zp_out = L->zp_out; c.relu = relu;
  c.out = out; c.ob = out_border; c.acc = acc; c.msv = msv_arg(L); c.sbv = sbv_arg(L);
  return i8ie_first_launch(ctx, c);
}

int i8ie_layer_forward_f32_input(i8ie_layer* L, const float* in, int m, int h, int w, float q_scale, uint8_t q_zp,
                                 int relu, uint8_t* out, int out_border, int32_t* acc) {
  return i8ie_layer_forward_f32_input_pool(L, in, m, h, w, q_scale, q_zp, relu, 0, 0, out, I8IE_LAYOUT_NHWC, out_border, acc);
}

int i8ie_layer_forward(i8ie_layer* L, const uint8_t* in, int m, int h, int w, float s_in, uint8_t zp_in, uint8_t* out,
                       int32_t* acc) {
  return i8ie_layer_forward_fused(L, in, I8IE_LAYOUT_NCHW, 0, m, h, w, s_in, zp_in, 0, out, I8IE_LAYOUT_NCHW, 0, acc);
}

int i8ie_layer_destroy(i8ie_layer* L) {
  if (!L) return I8IE_OK;
  i8ie_ctx* ctx = L->ctx;
  i8ie_free(ctx, L->qw);
  i8ie_free(ctx, L->qb);
  i8ie_free(ctx, L->Bpack);
  i8ie_free(ctx, L->Bpack2);
  if (L->Bstem) i8ie_free(ctx, L->Bstem);
  for (const I8ieWCache::Ent& e : L->wc.ents) i8ie_free(ctx, e.buf);
  i8ie_free(ctx, L->wsum);
  i8ie_free(ctx, L->oc);
  i8ie_free(ctx, L->ocp);
  if (L->Bperm) i8ie_free(ctx, L->Bperm);
  i8ie_free(ctx, L->biasf);
  if (L->swv) i8ie_free(ctx, L->swv);
  if (L->msv) i8ie_free(ctx, L->msv);
  delete L;
  return I8IE_OK;
}

// quantize_weight, src/layer.cc:6-26 (host side, one-shot at convert())
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
