// i8ie_layer.hip -- the forward of a layer handle (Linear / Conv2d / ConvTranspose2d, INT8): validate -> geometry -> plan -> peel ->
// route, the layout / pool queries that read the same plan, and the v1 runners.  How a handle is made,
// which route it takes and the stateless calls: i8ie_layer_create.hip (section 4b).
//   reference: src/fully_connected.cc:22-52, src/conv2d.cc:100-142
//
// Conv2d has five execution paths, all producing the reference's bytes:
//   A  channels % 16 == 0: implicit GEMM over NHWC activations (i8ie_igemm.hip)
//   B  channels <= 4 and stride % 4 == 0 (AlexNet conv1): the NCHW input is repacked
//      once into a physically padded, 4-pixel-grouped NHWC image; then path A's kernel
//   F  anything else: materialised im2col + v1 GEMM (i8ie_gemm.hip)
//   G  groups > 1 (not in the reference): one reference convolution per group, in the grouped kernels of i8ie_gconv.hip over
//      NHWC activations; and every layer with a dilation > 1 (not in the reference), dense ones as groups = 1
//   D  inside G: a dense dilated layer at stride 1 with channels % 16 == 0 runs in dconv_mfma (i8ie_dconv.hip), its input
//      patches phase-subsampled into LDS; what that kernel declines stays in the grouped kernels
//   L  inside G: a dense 1 x k / k x 1 layer at stride 1, dilation 1 with channels % 16 == 0 (i8ie_conv2d_create_rect) runs in
//      lconv_mfma (i8ie_lconv.hip), whole lines of pixels resident in LDS; what that kernel declines, and every other rectangular
//      or anisotropic layer, stays in the grouped kernels with the per-axis geometry in their tap offsets
//   T  ConvTranspose2d (not in the reference): the reference convolution of the equivalent zero-inserted problem, computed
//      phase by phase in the kernels of i8ie_deconv.hip over NHWC activations
// Activations cross the ABI as NCHW (the reference's layout) or, on request, as
// NHWC so that consecutive layers skip the layout conversion.
#include <cstring>
#include <vector>

#include "i8ie_layer.h"
#include "i8ie_first.h"
#include "i8ie_stem.h"
#include "i8ie_requant.h"
#include "i8ie_gconv.h"
#include "i8ie_deconv.h"
#include "i8ie_dconv.h"
#include "i8ie_lconv.h"

// ---- v1 (fallback) runners ------------------------------------------------------------------
int conv_run_v1(i8ie_ctx* ctx, const uint8_t* in, int n, const ConvGeom& cg, const int8_t* Bpack, const int32_t* oc,
                const int32_t* wsum, uint8_t zp_in, float s_in, float s_w, float s_out, uint8_t zp_out, uint8_t* out,
                int32_t* acc, uint8_t* col, int imgs_per_chunk, const float* sbv) {
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
                  uint8_t* out, int32_t* acc, uint8_t* scratch, const float* sbv) {
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

// ---- the layer forward: validate -> geometry -> plan -> peel -> route -----------------------------------
// One forward as an exported entry point hands it over.  `x`: the FP32 NCHW input of the f32-input entry (path B layers; `in` is
// then unused and in_layout NCHW).  `out_f32`: i8ie_layer_forward_dequant (Linear).
struct ConvRequest {
  const uint8_t* in = nullptr;
  const float* x = nullptr;
  int in_layout = I8IE_LAYOUT_NCHW, in_border = 0, m = 0, h = 0, w = 0;
  float s_in = 0.0f;
  uint8_t zp_in = 0;
  int relu = 0, pool_k = 0, pool_s = 0;  // (the pool as the caller gave it)
  uint8_t* out = nullptr;
  int out_layout = I8IE_LAYOUT_NCHW, out_border = 0;
  int32_t* acc = nullptr;
  float* out_f32 = nullptr;
  bool pool() const { return i8ie_is_pool(pool_k, pool_s); }
  int fold_k() const { return pool() ? pool_k : 0; }  // the window as a kernel that folds the pool gets it
  int pooled(int o) const { return pool() ? (o - pool_k) / pool_s + 1 : o; }
  bool in_s8() const { return in_layout == I8IE_LAYOUT_NHWC_S8; }
  bool out_s8() const { return out_layout == I8IE_LAYOUT_NHWC_S8; }
  bool in_nchw() const { return in_layout == I8IE_LAYOUT_NCHW; }
  bool out_nchw() const { return out_layout == I8IE_LAYOUT_NCHW; }
};

static ConvRequest make_request(const uint8_t* in, int in_layout, int in_border, int m, int h, int w, float s_in, uint8_t zp_in,
                                int relu, uint8_t* out, int out_layout, int out_border, int32_t* acc) {
  ConvRequest q;
  q.in = in; q.in_layout = in_layout; q.in_border = in_border; q.m = m; q.h = h; q.w = w; q.s_in = s_in; q.zp_in = zp_in; q.relu = relu;
  q.out = out; q.out_layout = out_layout; q.out_border = out_border; q.acc = acc;
  return q;
}
// the epilogue block of a contraction launch of this layer (`biasf`: the Linear routes)
static I8ieEpilogue layer_epilogue(const i8ie_layer* L, const ConvRequest& q, const float* biasf = nullptr) {
  I8ieEpilogue e{};
  e.ocp = L->ocp; e.biasf = biasf; e.msv = msv_arg(L); e.sbv = sbv_arg(L);
  e.s_in = q.s_in; e.s_w = sw_arg(L); e.s_out = L->s_out; e.zp_out = L->zp_out; e.relu = q.relu; e.acc = q.acc;
  return e;
}
// route A's launch over an NHWC image with `border` pixels around it, as far as the geometry goes: what conv_plan asks the
// patch-stationary kernel about and what forward_implicit launches
static I8ieIgemmCall implicit_call(i8ie_layer* L, const ConvGeom& cg, int m, int border) {
  I8ieIgemmCall c{};
  c.amode = 1; c.M = m * cg.oh * cg.ow; c.B = L->Bpack2; c.Kpad = L->Kpad2; c.Npad = L->Npad;
  c.Kchunks = L->K2 / 16; c.N = L->n; c.wcache = &L->wc; c.OH = cg.oh; c.OW = cg.ow;
  c.Hp = cg.h + 2 * border; c.Wp = cg.w + 2 * border; c.C = cg.c; c.KH = cg.kh; c.KW = cg.kw; c.sh = c.sw = cg.stride;
  c.a_bytes = (size_t)m * c.Hp * c.Wp * cg.c;
  return c;
}
// ... and the rest of a launch of the contraction kernel (routes A and B)
static void implicit_epilogue(I8ieIgemmCall& c, const i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  c.ep = layer_epilogue(L, q); c.Ktrue = cg.K;
}

// Which kernel takes this conv launch whole, with what the request asks folded in: the first-stage kernel (i8ie_stem.hip, path
// B) pools and can store re-biased; the patch-stationary kernel (i8ie_pconv.hip, path A) pools, reads and stores re-biased --
// when it takes the launch at all (kernel choice, geometry, batch, LDS; nothing is launched).  Neither: the plain call, the pool /
// the re-bias as launches of their own around it (the peel passes).  The ONLY place that asks the two kernels: the dispatcher and
// the layout queries read the same plan (the queries ask with output border 0; the kernel's size limits depend on the real one).
struct ConvPlan { bool stem = false, pconv = false; };
static ConvPlan conv_plan(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  ConvPlan p;
  i8ie_ctx* ctx = L->ctx;
  if (!L->conv || force_fallback(ctx) || !(q.acc == nullptr || aligned16(q.acc))) return p;
  if (L->path == PATH_B)
    p.stem = L->Bstem != nullptr && !ctx->pick.no_stem &&
             i8ie_stem_supported(cg.c, cg.stride, L->n, cg.kh, cg.kw, cg.oh, cg.ow, q.fold_k(), q.pool_s) != 0;
  if (L->path != PATH_A || !i8ie_conv_tries(ctx, I8IE_CONV_PCONV)) return p;
  if (!(q.pool_k > 0 || q.in_s8() || q.out_s8()) || q.out_nchw() || !aligned16(q.in) || !aligned16(q.out)) return p;
  I8ieIgemmCall c = implicit_call(L, cg, q.m, q.in_border > cg.pad ? q.in_border : cg.pad);
  c.pool_k = q.fold_k(); c.pool_s = q.pool_s; c.a_s8 = q.in_s8() ? 1 : 0; c.out_s8 = q.out_s8() ? 1 : 0; c.ob = q.out_border;
  p.pconv = c.a_bytes < i8ie_igemm_chunk_limit() && i8ie_pconv_takes(ctx, c) == 1;
  return p;
}

// The kernels of routes A, B, G and T write NHWC.  Their workspace: [front: what the route puts before the kernel][the NHWC
// result, when the caller wants NCHW]; unstage() converts that result back.
struct Staged {
  uint8_t *front, *out;  // the workspace; where the kernel writes, with border `ob`
  const uint8_t* in;     // stage_io: where the kernel reads, with border `ib`
  int ob, ib;
};
static int stage_out(i8ie_ctx* ctx, const ConvRequest& q, size_t front_bytes, size_t out_bytes, Staged* s) {
  const size_t o_bytes = q.out_nchw() ? i8ie_align_up(out_bytes, 256) : 0;
  I8IE_TRY(i8ie_ws_reserve(ctx, front_bytes + o_bytes + 256));
  s->front = (uint8_t*)ctx->ws;
  s->out = o_bytes ? s->front + front_bytes : q.out;
  s->ob = o_bytes ? 0 : q.out_border;
  return I8IE_OK;
}
// routes G and T read NHWC with any border (or none: bounds checks against zp_in): an NCHW input is converted into the front
static int stage_io(i8ie_ctx* ctx, const ConvGeom& cg, const ConvRequest& q, Staged* s) {
  const size_t a_bytes = q.in_nchw() ? i8ie_align_up((size_t)q.m * cg.c * cg.h * cg.w, 256) : 0;
  I8IE_TRY(stage_out(ctx, q, a_bytes, (size_t)q.m * cg.kc * cg.oh * cg.ow, s));
  s->in = q.in_nchw() ? s->front : q.in;
  s->ib = q.in_nchw() ? 0 : q.in_border;
  if (q.in_nchw()) I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, q.in, s->front, q.m, cg.c, cg.h, cg.w, 0));
  return I8IE_OK;
}
static int unstage(i8ie_ctx* ctx, const Staged& s, const ConvRequest& q, int kc, int oh, int ow) {
  if (s.out != q.out) I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, s.out, q.out, q.m, kc, oh, ow, 0));
  return I8IE_OK;
}
// ---- routes: the request as the plan and the peel passes left it (plain bytes and no pool unless the plan's kernel folds them) ----
// route T: one launch (no zero-insert, scatter or fill pass).  The force-fallback option picks deconv_direct inside the launcher.
static int forward_transposed(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  Staged s;
  I8IE_TRY(stage_io(L->ctx, cg, q, &s));
  I8ieDeconvCall d{};
  d.A = s.in; d.m = q.m; d.H = cg.h; d.W = cg.w; d.C = cg.c; d.ib = s.ib;
  d.OH = cg.oh; d.OW = cg.ow; d.k = cg.kh; d.s = cg.stride; d.p = cg.pad;
  d.N = L->n; d.Ngp = L->Ngp; d.Kpp = L->Kpp; d.Bp = L->Bt; d.ktab = L->ttab; d.tph = L->tph;
  d.ep = layer_epilogue(L, q); d.zp_in = q.zp_in;
  d.out = s.out; d.ob = s.ob;
  I8IE_TRY(i8ie_deconv_launch(L->ctx, d));
  return unstage(L->ctx, s, q, cg.kc, cg.oh, cg.ow);
}
// route G: the grouped kernels; the force-fallback option picks gconv_direct inside the launcher
static int forward_grouped(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  Staged s;
  I8IE_TRY(stage_io(L->ctx, cg, q, &s));
  I8ieGconvCall g{};
  g.A = s.in; g.m = q.m; g.H = cg.h; g.W = cg.w; g.C = cg.c; g.ib = s.ib;
  g.OH = cg.oh; g.OW = cg.ow; g.KH = cg.kh; g.KW = cg.kw;
  g.stride_h = cg.stride; g.stride_w = cg.stride_w; g.pad_h = cg.pad; g.pad_w = cg.pad_w; g.dil_h = cg.dil_h; g.dil_w = cg.dil_w;
  g.groups = L->groups; g.Cg = cg.c / L->groups; g.Ng = L->n / L->groups; g.Ngp = L->Ngp; g.Kgp = L->Kgp;
  g.Bp = L->Bg; g.ktab = L->gtab; g.ep = layer_epilogue(L, q); g.zp_in = q.zp_in;
  g.out = s.out; g.ob = s.ob;
  // route D: a dense dilated layer at stride 1 goes to the kernel of i8ie_dconv.hip (input patches resident in LDS) when that
  // takes it -- C % 16 == 0, K >= 32, aligned buffers, an LDS plan that fits, the force-fallback option off; it reads route G's
  // panel (groups = 1: [Ngp][Kgp], K ordered (kh, kw, c)) as it is.  Everything it declines stays in the grouped kernels.
  if (!L->rect && L->dil > 1 && L->groups == 1 && cg.stride == 1 && cg.kh == cg.kw) {
    I8ieDconvCall d{};
    d.A = s.in; d.m = q.m; d.H = cg.h; d.W = cg.w; d.C = cg.c; d.ib = s.ib;
    d.OH = cg.oh; d.OW = cg.ow; d.pad = cg.pad; d.k = cg.kh; d.dil = L->dil;
    d.N = L->n; d.Ngp = L->Ngp; d.Kgp = L->Kgp; d.Bp = L->Bg; d.ep = g.ep; d.zp_in = q.zp_in;
    d.out = s.out; d.ob = s.ob;
    if (i8ie_dconv_takes(L->ctx, d)) {
      I8IE_TRY(i8ie_dconv_launch(L->ctx, d));
      return unstage(L->ctx, s, q, cg.kc, cg.oh, cg.ow);
    }
  }
  // route L: a dense 1 x k / k x 1 layer at stride (1, 1), dilation (1, 1) goes to the kernel of i8ie_lconv.hip (whole lines
  // resident in LDS) when that takes it; it reads the same panel.  Everything it declines stays in the grouped kernels.
  if (L->rect && L->groups == 1 && cg.stride == 1 && cg.stride_w == 1 && cg.dil_h == 1 && cg.dil_w == 1 && (cg.kh == 1 || cg.kw == 1)) {
    I8ieLconvCall d{};
    d.A = s.in; d.m = q.m; d.H = cg.h; d.W = cg.w; d.C = cg.c; d.ib = s.ib;
    d.OH = cg.oh; d.OW = cg.ow; d.KH = cg.kh; d.KW = cg.kw; d.pad_h = cg.pad; d.pad_w = cg.pad_w;
    d.N = L->n; d.Ngp = L->Ngp; d.Kgp = L->Kgp; d.Bp = L->Bg; d.ep = g.ep; d.zp_in = q.zp_in;
    d.out = s.out; d.ob = s.ob;
    if (i8ie_lconv_takes(L->ctx, d)) {
      I8IE_TRY(i8ie_lconv_launch(L->ctx, d));
      return unstage(L->ctx, s, q, cg.kc, cg.oh, cg.ow);
    }
  }
  I8IE_TRY(i8ie_gconv_launch(L->ctx, g));
  return unstage(L->ctx, s, q, cg.kc, cg.oh, cg.ow);
}

// route F: materialised im2col + the v1 GEMM, NCHW in and out of the kernels, relu as its own launch
static int forward_fallback(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  i8ie_ctx* ctx = L->ctx;
  const size_t in_bytes = (size_t)q.m * cg.c * cg.h * cg.w, out_bytes = (size_t)q.m * cg.kc * cg.oh * cg.ow;
  const int ipc = chunk_images(cg, q.m);
  const size_t col_bytes = i8ie_align_up((size_t)ipc * cg.oh * cg.ow * cg.Kpad, 256);
  const size_t a_bytes = q.in_layout == I8IE_LAYOUT_NHWC ? i8ie_align_up(in_bytes, 256) : 0;
  const size_t o_bytes = q.out_layout == I8IE_LAYOUT_NHWC ? i8ie_align_up(out_bytes, 256) : 0;
  I8IE_TRY(i8ie_ws_reserve(ctx, col_bytes + a_bytes + o_bytes));
  uint8_t* ws = (uint8_t*)ctx->ws;
  const uint8_t* src = q.in;
  if (a_bytes) {
    I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, q.in, ws + col_bytes, q.m, cg.c, cg.h, cg.w, q.in_border));
    src = ws + col_bytes;
  }
  uint8_t* dst = o_bytes ? ws + col_bytes + a_bytes : q.out;
  I8IE_TRY(conv_run_v1(ctx, src, q.m, cg, L->Bpack, L->oc, L->wsum, q.zp_in, q.s_in, L->s_w, L->s_out, L->zp_out, dst, q.acc,
                       ws, ipc, sbv_arg(L)));
  if (q.relu) I8IE_TRY(i8ie_relu_u8(ctx, dst, dst, (int64_t)out_bytes, L->zp_out));
  if (o_bytes) I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, dst, q.out, q.m, cg.kc, cg.oh, cg.ow, q.out_border));
  return I8IE_OK;
}

// route A: implicit GEMM over the NHWC image with the layer's padding as a physical border.  `pconv`: the patch-stationary
// kernel said it takes this launch as it is (conv_plan), pool and re-biased layouts included.
static int forward_implicit(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q, bool pconv) {
  i8ie_ctx* ctx = L->ctx;
  const int oh = q.pooled(cg.oh), ow = q.pooled(cg.ow);  // (a pool is still on the request only when `pconv` folds it)
  const bool direct = !q.in_nchw() && q.in_border >= cg.pad && aligned16(q.in);  // the input's own border serves
  I8ieIgemmCall c = implicit_call(L, cg, q.m, direct ? q.in_border : cg.pad);
  Staged s;
  I8IE_TRY(stage_out(ctx, q, direct ? 0 : i8ie_align_up(c.a_bytes, 256), (size_t)q.m * cg.kc * oh * ow, &s));
  if (direct) {
    const int d = q.in_border - cg.pad;
    const size_t shift = ((size_t)d * c.Wp + d) * cg.c;
    c.A = q.in + shift;
    c.a_bytes -= shift;
  } else {
    if (!q.in_nchw()) {  // (re-biased bytes are copied as they are; their border value is zp ^ 0x80)
      I8IE_TRY(i8ie_launch_reborder(ctx, q.in, s.front, q.m, cg.c, cg.h, cg.w, q.in_border, cg.pad, q.in_s8() ? (q.zp_in ^ 0x80) : q.zp_in));
    } else {
      if (cg.pad > 0) I8IE_HIP_TRY(hipMemsetAsync(s.front, q.zp_in, c.a_bytes, ctx->stream));
      I8IE_TRY(i8ie_launch_nchw_to_nhwc(ctx, q.in, s.front, q.m, cg.c, cg.h, cg.w, cg.pad));
    }
    c.A = s.front;
  }
  implicit_epilogue(c, L, cg, q);
  if (pconv) {
    c.pool_k = q.fold_k(); c.pool_s = q.pool_s; c.a_s8 = q.in_s8() ? 1 : 0; c.out_s8 = q.out_s8() ? 1 : 0;
  }
  c.out = s.out; c.ob = s.ob;
  I8IE_TRY(i8ie_igemm_launch(ctx, c));
  return unstage(ctx, s, q, cg.kc, oh, ow);
}
// the calls of the two small-C kernels, all but the source and the destination (shared by the u8 and the f32-input forward)
static I8ieStemCall fill_stem_call(const i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  I8ieStemCall f{};
  f.n = q.m; f.c = cg.c; f.h = cg.h; f.w = cg.w; f.q_scale = q.s_in; f.q_zp = q.zp_in;
  f.KH = cg.kh; f.KW = cg.kw; f.stride = cg.stride; f.pad = cg.pad; f.OH = cg.oh; f.OW = cg.ow;
  f.B = L->Bstem; f.Kpad = L->KpadStem; f.N = L->n; f.ep = layer_epilogue(L, q);
  f.pool_k = q.fold_k(); f.pool_s = q.pool_s; f.out_s8 = q.out_s8() ? 1 : 0;
  return f;
}
static I8ieFirstCall fill_first_call(const i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  I8ieFirstCall f{};
  f.n = q.m; f.c = cg.c; f.h = cg.h; f.w = cg.w; f.q_scale = q.s_in; f.q_zp = q.zp_in;
  f.KH = cg.kh; f.KW = cg.kw; f.KWG = L->kwg; f.stride = cg.stride; f.pad = cg.pad; f.OH = cg.oh; f.OW = cg.ow;
  f.B = L->Bpack2; f.Kpad = L->Kpad2; f.K2 = L->K2; f.N = L->n; f.ep = layer_epilogue(L, q);
  return f;
}

// route B (small-C, stride % 4 == 0): the kernels read NCHW (u8, or FP32 that they quantize on the way: q.x) through an image
// they repack into the workspace.  `stem`: the first-stage kernel (i8ie_stem.hip) takes the launch, conv (+ relu) (+ max-pool) in
// one contraction; else the weights-stationary kernel (i8ie_first.hip) where it supports the layer (an f32-input forward always:
// i8ie_layer_accepts_f32_input), else the 4-pixel-grouped image through the tiled kernel of route A.
static int forward_small_c(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q, bool stem) {
  i8ie_ctx* ctx = L->ctx;
  const int oh = q.pooled(cg.oh), ow = q.pooled(cg.ow);  // (a pool is still on the request only when `stem` folds it)
  const int Hp = (cg.oh - 1) * cg.stride + cg.kh, Wg = (cg.ow - 1) * (cg.stride / 4) + L->kwg;  // the grouped image
  const bool wstat = !stem && (q.acc == nullptr || (L->n % 4 == 0 && aligned16(q.acc))) &&
                     i8ie_first_supported(cg.c, cg.stride, L->n, L->K2, cg.kh, L->kwg, cg.ow);
  const size_t t_bytes = q.x == nullptr && !q.in_nchw() ? i8ie_align_up((size_t)q.m * cg.c * cg.h * cg.w, 256) : 0;
  const size_t r_bytes = i8ie_align_up(stem ? i8ie_stem_scratch_bytes(q.m, cg.kh, cg.kw, cg.stride, cg.oh, cg.ow)
                                            : i8ie_first_scratch_bytes(q.m, cg.kh, L->kwg, cg.stride, cg.oh, cg.ow), 256);
  Staged s;
  I8IE_TRY(stage_out(ctx, q, t_bytes + r_bytes, (size_t)q.m * cg.kc * oh * ow, &s));
  const uint8_t* src = q.in;
  if (t_bytes) {
    I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, q.in, s.front, q.m, cg.c, cg.h, cg.w, q.in_border));
    src = s.front;
  }
  uint8_t* rep = s.front + t_bytes;
  if (stem) {
    I8ieStemCall f = fill_stem_call(L, cg, q);
    f.x = q.x; f.xu8 = q.x ? nullptr : src; f.scratch = rep; f.out = s.out; f.ob = s.ob;
    I8IE_TRY(i8ie_stem_launch(ctx, f));
    return unstage(ctx, s, q, cg.kc, oh, ow);
  }
  if (q.x == nullptr) I8IE_TRY(i8ie_launch_repack_smallc(ctx, src, rep, q.m, cg.c, cg.h, cg.w, Hp, Wg, cg.pad, cg.pad, q.zp_in, wstat));
  if (wstat) {
    I8ieFirstCall f = fill_first_call(L, cg, q);
    f.x = q.x; f.grouped = q.x ? nullptr : rep; f.scratch = q.x ? rep : nullptr; f.out = s.out; f.ob = s.ob;
    I8IE_TRY(i8ie_first_launch(ctx, f));
    return unstage(ctx, s, q, cg.kc, oh, ow);
  }
  I8ieIgemmCall c = implicit_call(L, cg, q.m, 0);
  c.A = rep; c.a_bytes = (size_t)q.m * Hp * Wg * 16;
  c.Hp = Hp; c.Wp = Wg; c.C = 16; c.KW = L->kwg; c.sw = cg.stride / 4;
  implicit_epilogue(c, L, cg, q);
  c.out = s.out; c.ob = s.ob;
  I8IE_TRY(i8ie_igemm_launch(ctx, c));
  return unstage(ctx, s, q, cg.kc, oh, ow);
}

// ---- plan -> peel -> route.  Each peel pass takes one thing off the request that no kernel folds, runs forward_conv on the
// changed request -- which plans AGAIN: the inner layout, border and pool differ, so a peeled re-biased output can still fold
// its pool and a plain-copied input can still get a folded pool or store -- and does that thing as launches of its own.
static int forward_conv(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q);
// re-biased input nobody reads as it is: plain copy first
static int peel_rebiased_input(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  i8ie_ctx* ctx = L->ctx;
  const size_t bytes = (size_t)q.m * (cg.h + 2 * q.in_border) * (cg.w + 2 * q.in_border) * cg.c;
  uint8_t* tmp = nullptr;
  I8IE_TRY(i8ie_malloc(ctx, bytes, (void**)&tmp));
  ConvRequest r = q;
  r.in = tmp; r.in_layout = I8IE_LAYOUT_NHWC;
  int rc = i8ie_rebias_u8(ctx, q.in, tmp, (int64_t)bytes);
  if (rc == I8IE_OK) rc = forward_conv(L, cg, r);
  i8ie_free(ctx, tmp);
  return rc;
}

// re-biased output nobody stores: the plain result into a temporary, re-biased, then laid into `out` with its border
static int peel_rebiased_output(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  i8ie_ctx* ctx = L->ctx;
  const int oph = q.pooled(cg.oh), opw = q.pooled(cg.ow);
  const size_t bytes = (size_t)q.m * L->n * oph * opw;
  I8IE_REQUIRE(L->n % 16 == 0, "re-biased NHWC output needs out features % 16 == 0");
  uint8_t* tmp = nullptr;
  I8IE_TRY(i8ie_malloc(ctx, bytes, (void**)&tmp));
  ConvRequest r = q;
  r.out = tmp; r.out_layout = I8IE_LAYOUT_NHWC; r.out_border = 0;
  int rc = forward_conv(L, cg, r);
  if (rc == I8IE_OK) rc = i8ie_rebias_u8(ctx, tmp, tmp, (int64_t)bytes);
  if (rc == I8IE_OK) rc = i8ie_launch_reborder(ctx, tmp, q.out, q.m, L->n, oph, opw, 0, q.out_border, L->zp_out ^ 0x80);
  i8ie_free(ctx, tmp);
  return rc;
}

// a pool no kernel folds: max_pool2d<u8> (src/functional.cc:36-64) as its own launch behind the convolution
static int peel_pool(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  i8ie_ctx* ctx = L->ctx;
  const int oph = q.pooled(cg.oh), opw = q.pooled(cg.ow);
  const bool nhwc = q.out_layout == I8IE_LAYOUT_NHWC && L->n % 16 == 0;
  uint8_t* tmp = nullptr;
  I8IE_TRY(i8ie_malloc(ctx, (size_t)q.m * L->n * cg.oh * cg.ow, (void**)&tmp));
  ConvRequest r = q;
  r.pool_k = r.pool_s = 0;
  r.out = tmp; r.out_layout = nhwc ? I8IE_LAYOUT_NHWC : I8IE_LAYOUT_NCHW; r.out_border = 0;
  int rc = forward_conv(L, cg, r);
  if (rc == I8IE_OK) {
    if (nhwc) {
      rc = i8ie_launch_maxpool_nhwc(ctx, tmp, 0, q.out, q.out_border, q.m, L->n, cg.oh, cg.ow, q.pool_k, q.pool_s, 0);
    } else if (q.out_nchw()) {
      rc = i8ie_maxpool2d_u8(ctx, tmp, q.out, q.m, L->n, cg.oh, cg.ow, q.pool_k, q.pool_s);
    } else {  // NHWC result with channels % 16 != 0: pool in NCHW, then lay out
      uint8_t* tmp2 = nullptr;
      rc = i8ie_malloc(ctx, (size_t)q.m * L->n * oph * opw, (void**)&tmp2);
      if (rc == I8IE_OK) rc = i8ie_maxpool2d_u8(ctx, tmp, tmp2, q.m, L->n, cg.oh, cg.ow, q.pool_k, q.pool_s);
      if (rc == I8IE_OK) rc = i8ie_launch_nchw_to_nhwc(ctx, tmp2, q.out, q.m, L->n, oph, opw, q.out_border);
      i8ie_free(ctx, tmp2);
    }
  }
  i8ie_free(ctx, tmp);
  return rc;
}

static int forward_conv(i8ie_layer* L, const ConvGeom& cg, const ConvRequest& q) {
  const ConvPlan plan = conv_plan(L, cg, q);
  if (q.in_s8() && !plan.pconv) return peel_rebiased_input(L, cg, q);
  if (q.out_s8() && !plan.pconv && !plan.stem) return peel_rebiased_output(L, cg, q);
  if (q.pool() && !plan.pconv && !plan.stem) return peel_pool(L, cg, q);
  if (L->path == PATH_T) return forward_transposed(L, cg, q);
  if (L->path == PATH_G) return forward_grouped(L, cg, q);
  if (L->path == PATH_F || force_fallback(L->ctx)) return forward_fallback(L, cg, q);
  return L->path == PATH_A ? forward_implicit(L, cg, q, plan.pconv) : forward_small_c(L, cg, q, plan.stem);
}

// ---- Linear: row-major in / out ------------------------------------------------------------------------------------------------
static int forward_linear(i8ie_layer* L, const ConvRequest& q) {
  i8ie_ctx* ctx = L->ctx;
  const int m = q.m;
  I8IE_REQUIRE(q.in_border == 0 && q.out_border == 0, "Linear tensors carry no border");
  // Rows that are a flattened NHWC activation [m][h][w][c] (the engine's layout between layers) instead of
  // the reference's flattened NCHW: same contraction with K walked in (h, w, c) order, so the weight panel
  // is permuted once per (c, h*w) and the input is used as it lies -- no transpose back to NCHW.  oc[] and
  // wsum[] are sums over all of K and keep the reference's accumulation order (they come from qw).
  const int hw = (q.in_layout == I8IE_LAYOUT_NHWC && q.h > 0 && q.w > 0) ? q.h * q.w : 1;
  const int8_t* panel = L->Bpack;
  if (hw > 1) {
    I8IE_REQUIRE(L->K % hw == 0, "Linear: in_features is not c * h * w for the given h, w");
    if (force_fallback(ctx) || L->K % 16 != 0 || !aligned16(q.in)) {
      // the any-geometry route wants reference order: transpose the input instead of the weights, into the workspace BEYOND
      // what the inner forward reserves and uses (its padded rows and split-K partials)
      I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)m * L->K + (size_t)m * L->Kpad + (size_t)8 * m * L->n * 4 + 4096));
      uint8_t* t = (uint8_t*)ctx->ws + i8ie_align_up((size_t)m * L->Kpad + (size_t)8 * m * L->n * 4, 256) + 512;
      I8IE_TRY(i8ie_launch_nhwc_to_nchw(ctx, q.in, t, m, L->K / hw, q.h, q.w, 0));
      ConvRequest r = q;
      r.in = t; r.in_layout = I8IE_LAYOUT_NCHW; r.h = r.w = 0;
      return forward_linear(L, r);
    }
    if (L->Bperm == nullptr || L->perm_c != L->K / hw || L->perm_hw != hw) {
      if (L->Bperm == nullptr) I8IE_TRY(i8ie_layer_buffer(L, (void**)&L->Bperm, (size_t)L->Npad * L->Kpad));
      I8IE_TRY(i8ie_launch_permute_k(ctx, L->Bpack, L->Bperm, L->Npad, L->Kpad, L->K, L->K / hw, hw));
      L->perm_c = L->K / hw;
      L->perm_hw = hw;
    }
    panel = L->Bperm;
  }
  const bool need_pad = (L->K % 16 != 0) || !aligned16(q.in);
  if (!force_fallback(ctx) && !need_pad && L->n <= i8ie_smalln_max_features()) {
    // classifier head: one wave per row, dot4 + wavefront reduction, epilogue (and dequantize) fused
    I8ieSmallNCall sc{};
    sc.A = q.in; sc.lda = (size_t)L->K; sc.M = m; sc.K = L->K; sc.B = panel; sc.Kpad = L->Kpad; sc.N = L->n;
    sc.ep = layer_epilogue(L, q, L->biasf); sc.out = q.out; sc.out_f32 = q.out_f32;
    return i8ie_launch_linear_smalln(ctx, sc);
  }
  I8IE_REQUIRE(q.out != nullptr, "i8ie_layer_forward_dequant: this layer needs the u8 output buffer as well");
  if (q.out_f32 != nullptr) {  // general shape: the ordinary forward, then the dequantize kernel
    ConvRequest r = q;
    r.out_f32 = nullptr; r.out_layout = I8IE_LAYOUT_NCHW;
    I8IE_TRY(forward_linear(L, r));
    return i8ie_dequantize_u8_f32(ctx, q.out, q.out_f32, (int64_t)m * L->n, L->s_out, L->zp_out);
  }
  if (force_fallback(ctx)) {
    if (need_pad) I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)m * L->Kpad));
    I8IE_TRY(linear_run_v1(ctx, q.in, m, L->K, L->Bpack, L->Kpad, L->qb, L->n, L->oc, L->wsum, q.s_in, L->s_w, L->s_out,
                           L->zp_out, q.out, q.acc, (uint8_t*)ctx->ws, sbv_arg(L)));
    if (q.relu) I8IE_TRY(i8ie_relu_u8(ctx, q.out, q.out, (int64_t)m * L->n, L->zp_out));
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
                    aligned16(q.out) && L->Npad % 128 == 0 &&
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
  if (need_pad) I8IE_TRY(i8ie_launch_pad_rows(ctx, q.in, m, L->K, ctx->ws, m, L->Kpad, 0));
  c.A = need_pad ? (const uint8_t*)ctx->ws : q.in;
  c.lda = need_pad ? L->Kpad : L->K;
  c.Kchunks = (int)c.lda / 16;
  c.a_bytes = (size_t)m * c.lda;
  c.amode = 0; c.M = m;
  c.B = panel; c.Kpad = L->Kpad; c.Npad = L->Npad; c.N = L->n; c.ep = layer_epilogue(L, q, L->biasf);
  c.out = q.out; c.ob = 0; c.Ktrue = L->K;
  if (flin) return i8ie_flin_launch(ctx, c);
  if (mlin) return i8ie_mlin_launch(ctx, c);
  return i8ie_igemm_launch(ctx, c);
}

// ---- validate -> geometry, then forward_linear or forward_conv -----------------------------------------------------------------
static int layer_forward(i8ie_layer* L, const ConvRequest& q) {
  I8IE_REQUIRE(L && q.in, "null argument");
  I8IE_REQUIRE(q.out != nullptr || (q.out_f32 != nullptr && !L->conv), "null output");
  I8IE_REQUIRE(q.m > 0, "non-positive batch");
  I8IE_REQUIRE(q.in_layout >= I8IE_LAYOUT_NCHW && q.in_layout <= I8IE_LAYOUT_NHWC_S8 && q.out_layout >= I8IE_LAYOUT_NCHW &&
                   q.out_layout <= I8IE_LAYOUT_NHWC_S8,
               "bad layout tag");
  I8IE_REQUIRE(L->conv || (!q.in_s8() && !q.out_s8()), "the re-biased layout applies to conv layers only");
  I8IE_REQUIRE(q.in_border >= 0 && q.out_border >= 0, "negative border");
  I8IE_REQUIRE(!q.in_nchw() || q.in_border == 0, "only NHWC tensors carry a border");
  I8IE_REQUIRE(!q.out_nchw() || q.out_border == 0, "only NHWC tensors carry a border");
  I8IE_HIP_TRY(hipSetDevice(L->ctx->device));
  I8IE_TRY(ensure_offsets(L, q.s_in, q.zp_in));
  I8IE_TRY(ensure_multipliers(L, q.s_in));
  if (!L->conv) return forward_linear(L, q);
  ConvGeom cg;
  if (L->path == PATH_T)
    I8IE_TRY(deconv_geom(L->c, q.h, q.w, L->n, L->kh, L->stride, L->pad, L->opad, &cg));
  else
    I8IE_TRY(conv_geom(L->c, q.h, q.w, L->n, layer_geom(L), &cg));
  if (q.pool()) I8IE_REQUIRE(q.pool_k <= cg.oh && q.pool_k <= cg.ow, "max-pool window larger than the convolution's output");
  return forward_conv(L, cg, q);
}

int i8ie_layer_forward_fused(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                             float s_in, uint8_t zp_in, int relu, uint8_t* out, int out_layout, int out_border,
                             int32_t* acc) {
  I8IE_REQUIRE(out != nullptr, "null argument");
  return layer_forward(L, make_request(in, in_layout, in_border, m, h, w, s_in, zp_in, relu, out, out_layout, out_border, acc));
}

int i8ie_layer_forward_pool(i8ie_layer* L, const uint8_t* in, int in_layout, int in_border, int m, int h, int w,
                            float s_in, uint8_t zp_in, int relu, int pool_k, int pool_s, uint8_t* out, int out_layout,
                            int out_border, int32_t* acc) {
  I8IE_REQUIRE(L != nullptr && out != nullptr, "null argument");
  I8IE_REQUIRE(L->conv, "i8ie_layer_forward_pool: Conv2d layers only");
  I8IE_REQUIRE(pool_k > 0 && pool_s > 0, "kernel_size and stride must be positive");
  ConvRequest q = make_request(in, in_layout, in_border, m, h, w, s_in, zp_in, relu, out, out_layout, out_border, acc);
  q.pool_k = pool_k; q.pool_s = pool_s;
  return layer_forward(L, q);
}

// dequantize(layer(x)) for a Linear layer: src/quantize_utils.cc:54-58 applied to the result of
// src/fully_connected.cc:22-52.  out_u8 may be null when the layer has at most 16 output features (the fused
// small-N kernel writes the FP32 values directly); otherwise it receives the u8 result as usual.
int i8ie_layer_forward_dequant(i8ie_layer* L, const uint8_t* in, int in_layout, int m, int h, int w, float s_in,
                               uint8_t zp_in, int relu, uint8_t* out_u8, float* out_f32) {
  I8IE_REQUIRE(L && out_f32, "null argument");
  I8IE_REQUIRE(!L->conv, "i8ie_layer_forward_dequant: Linear layers only");
  ConvRequest q = make_request(in, in_layout, 0, m, h, w, s_in, zp_in, relu, out_u8, I8IE_LAYOUT_NCHW, 0, nullptr);
  q.out_f32 = out_f32;
  return layer_forward(L, q);
}

// ---- the layout / pool negotiation: each query builds the request it means and reads the plan -----------------------------
// (NHWC in with the layer's padding as its border, NHWC out without one, no buffers yet: null pointers count as aligned)
static bool query_plan(const i8ie_layer* L, int m, int h, int w, int pool_k, int pool_s, int in_layout, int out_layout, ConvPlan* p,
                       ConvGeom* cg) {
  if (conv_geom(L->c, h, w, L->n, layer_geom(L), cg) != I8IE_OK) return false;
  ConvRequest q = make_request(nullptr, in_layout, cg->pad, m, h, w, 0.0f, 0, 0, nullptr, out_layout, 0, nullptr);
  q.pool_k = pool_k; q.pool_s = pool_s;
  if (q.pool() && (pool_s < 1 || pool_k > cg->oh || pool_k > cg->ow)) return false;
  *p = conv_plan(const_cast<i8ie_layer*>(L), *cg, q);
  return true;
}

int i8ie_layer_accepts_f32_input(const i8ie_layer* L, int h, int w, int* yes) {
  I8IE_REQUIRE(L && yes, "null argument");
  *yes = 0;
  ConvPlan p;
  ConvGeom cg;
  if (!L->conv || L->path != PATH_B || force_fallback(L->ctx)) return I8IE_OK;
  if (!query_plan(L, 1, h, w, 0, 0, I8IE_LAYOUT_NCHW, I8IE_LAYOUT_NHWC, &p, &cg)) return I8IE_OK;
  *yes = (p.stem || i8ie_first_supported(L->c, L->stride, L->n, L->K2, L->kh, L->kwg, cg.ow)) ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_fuses_pool(const i8ie_layer* L, int m, int h, int w, int pool_k, int pool_s, int* yes) {
  I8IE_REQUIRE(L && yes, "null argument");
  *yes = 0;
  ConvPlan p;
  ConvGeom cg;
  if (!L->conv || L->path == PATH_T || pool_k < 1 || pool_s < 1 || m < 1) return I8IE_OK;
  if (query_plan(L, m, h, w, pool_k, pool_s, I8IE_LAYOUT_NHWC, I8IE_LAYOUT_NHWC, &p, &cg)) *yes = (p.stem || p.pconv) ? 1 : 0;
  return I8IE_OK;
}

int i8ie_layer_rebiased_io(const i8ie_layer* L, int m, int h, int w, int pool_k, int pool_s, int* reads, int* stores) {
  I8IE_REQUIRE(L && reads && stores, "null argument");
  *reads = *stores = 0;
  ConvPlan in, out;
  ConvGeom cg;
  if (!L->conv || L->path == PATH_T || m < 1) return I8IE_OK;
  if (!query_plan(L, m, h, w, pool_k, pool_s, I8IE_LAYOUT_NHWC_S8, I8IE_LAYOUT_NHWC, &in, &cg) ||
      !query_plan(L, m, h, w, pool_k, pool_s, I8IE_LAYOUT_NHWC, I8IE_LAYOUT_NHWC_S8, &out, &cg))
    return I8IE_OK;
  *reads = in.pconv ? 1 : 0;
  *stores = (out.stem || out.pconv) ? 1 : 0;
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
  I8IE_HIP_TRY(hipSetDevice(L->ctx->device));
  I8IE_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0, "output must be 16-byte aligned");
  I8IE_REQUIRE(acc == nullptr || aligned16(acc), "accumulator buffer must be 16-byte aligned");
  I8IE_TRY(ensure_offsets(L, q_scale, q_zp));
  I8IE_TRY(ensure_multipliers(L, q_scale));
  ConvGeom cg;
  I8IE_TRY(conv_geom(L->c, h, w, L->n, layer_geom(L), &cg));
  ConvRequest q = make_request(nullptr, I8IE_LAYOUT_NCHW, 0, m, h, w, q_scale, q_zp, relu, out, out_layout, out_border, acc);
  q.x = in; q.pool_k = pool_k; q.pool_s = pool_s;
  if (q.pool()) I8IE_REQUIRE(pool_s > 0 && pool_k <= cg.oh && pool_k <= cg.ow, "max-pool window larger than the convolution's output");
  // plan, peel and route as for a u8 forward: what the kernel that takes the launch does not fold (the older first-layer kernel
  // neither pools nor stores re-biased) runs as launches of its own behind the plain result
  return forward_conv(L, cg, q);
}

int i8ie_layer_forward_f32_input(i8ie_layer* L, const float* in, int m, int h, int w, float q_scale, uint8_t q_zp,
                                 int relu, uint8_t* out, int out_border, int32_t* acc) {
  return i8ie_layer_forward_f32_input_pool(L, in, m, h, w, q_scale, q_zp, relu, 0, 0, out, I8IE_LAYOUT_NHWC, out_border, acc);
}


int i8ie_layer_forward(i8ie_layer* L, const uint8_t* in, int m, int h, int w, float s_in, uint8_t zp_in, uint8_t* out,
                       int32_t* acc) {
  return i8ie_layer_forward_fused(L, in, I8IE_LAYOUT_NCHW, 0, m, h, w, s_in, zp_in, 0, out, I8IE_LAYOUT_NCHW, 0, acc);
}

}  // extern "C"
