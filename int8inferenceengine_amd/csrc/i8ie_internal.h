// i8ie_internal.h -- shared by the translation units of libi8ie_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>

#include "i8ie_hip.h"

typedef int v4i __attribute__((ext_vector_type(4)));  // an MFMA operand / accumulator fragment, a 16-byte access

// I8IE_OPT_KERNEL_VARIANT decoded once (i8ie_decode_variant, i8ie_ctx.hip) into the choices the dispatch sites read.  A value
// changes the one thing it names; a value this build does not know decodes to all-automatic.
enum { I8IE_CONV_AUTO, I8IE_CONV_TILED, I8IE_CONV_PCONV, I8IE_CONV_TCONV };
// the tiled contraction kernel's form: default, or one LDS stage filled through registers / by LDS-DMA (the VAR of
// i8ie_igemm.hip)
enum { I8IE_TILE_DEFAULT = 0, I8IE_TILE_REG = 3, I8IE_TILE_DMA = 5 };
enum {
  I8IE_LIN_AUTO,
  I8IE_LIN_TILED,         // the tiled split-K kernel at every row count
  I8IE_LIN_TILED_MANY,    // the tiled kernel where the many-row kernel would run (> 256 rows); the few-row kernel automatic
  I8IE_LIN_FLIN,          // few-row kernel below its feature threshold
  I8IE_LIN_FLIN128,       // the same, its 128-row form up to 128 rows
  I8IE_LIN_MLIN,          // many-row kernel below its feature threshold
  I8IE_LIN_MLIN64,        // the same, 64-row block tiles
  I8IE_LIN_MLIN128,       // the same, 128-row block tiles
};
struct I8ieKernelChoice {
  int conv = I8IE_CONV_AUTO;  // which kernels a conv launch tries (i8ie_conv_tries)
  int conv_tile = I8IE_TILE_DEFAULT;    // the tiled kernel's form for conv
  int linear_tile = I8IE_TILE_DEFAULT;  // ... and for Linear
  int linear = I8IE_LIN_AUTO;
  bool pconv_2pass = false;  // patch-stationary kernel: N = 384 as two passes of 192, no 128-wide pass split
  bool stem_whole = false;   // first-stage kernel: whole images per block
  bool stem_simd_roles = false;  // first-stage kernel: its two wave roles on separate SIMDs
  bool no_stem = false;      // no first-stage kernel (conv_smallc + separate pools)
  bool no_dot4_head = false;  // the classifier head without its MFMA form
};
I8ieKernelChoice i8ie_decode_variant(int v);

struct i8ie_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  void* ws = nullptr;  // scratch for one op at a time (stream-ordered reuse)
  size_t ws_bytes = 0;
  void* pool = nullptr;  // I8iePool* (i8ie_ctx.hip): stream-ordered caching allocator
  void* prof = nullptr;  // I8ieProf* (i8ie_ctx.hip): HIP-event timing of every launch, when enabled
  unsigned options = 0;  // bit 0: I8IE_OPT_FORCE_FALLBACK
  int cu_limit = 0;  // I8IE_OPT_CU_LIMIT: compute units of the stream's CU mask (0 = the whole device)
  I8ieKernelChoice pick;  // i8ie_decode_variant(I8IE_OPT_KERNEL_VARIANT)
  int prof_mfma_only = 0;  // time only the contraction kernels (fewer event packets in a timed region)
  int prof_stride = 1;     // I8IE_OPT_PROFILE_STRIDE: bracket every prof_stride-th eligible launch
  unsigned prof_seen = 0;  // eligible launches since i8ie_profile_start
  hipStream_t copy_stream = nullptr;  // transfer stream for the *_async copies (created on first use)
  void* pinned = nullptr;  // std::unordered_map<void*, size_t>* of i8ie_host_malloc blocks
  void* capture = nullptr;  // std::vector<void*>* while a graph is being captured: blocks freed meanwhile (i8ie_graph_*)
  int live_graphs = 0;      // graphs captured on this ctx and not yet destroyed: their kernels have ctx->ws baked in
  void* retired_ws = nullptr;  // std::vector<void*>*: workspaces outgrown while graphs were alive (freed with the last graph)
};

// Per-launch HIP-event timing on the ctx's stream (off unless i8ie_profile_start was
// called).  `ops` = algorithmic integer ops (2 * MACs), `bytes` = algorithmic bytes.
void i8ie_prof_begin(i8ie_ctx* ctx, const char* name, double ops, double bytes);
void i8ie_prof_end(i8ie_ctx* ctx);
struct I8ieProfScope {
  i8ie_ctx* c;
  I8ieProfScope(i8ie_ctx* ctx, const char* name, double ops, double bytes) : c(ctx) {
    on = c->prof != nullptr && (!c->prof_mfma_only || ops > 0.0);
    if (on && c->prof_stride > 1) on = (c->prof_seen++ % (unsigned)c->prof_stride) == 0;
    if (on) i8ie_prof_begin(c, name, ops, bytes);
  }
  ~I8ieProfScope() {
    if (on) i8ie_prof_end(c);
  }
  bool on;
};

void i8ie_set_error(const char* fmt, ...);

// compute units a one-block-per-CU kernel may count on: the device's, or the ctx's CU-mask share
inline int i8ie_cus(const i8ie_ctx* ctx, int device_cus) { return ctx->cu_limit > 0 && ctx->cu_limit < device_cus ? ctx->cu_limit : device_cus; }
// does a conv launch try this kernel (I8IE_CONV_PCONV / _TCONV) before the tiled one?  Automatic selection tries the two
// patch-stationary kernels (each declines what it is not measured faster on); a forced choice tries only the kernel it names.
// The layout / pool negotiation (pconv_probe, i8ie_layer.hip) asks the same question as the dispatcher (i8ie_igemm.hip).
inline bool i8ie_conv_tries(const i8ie_ctx* ctx, int kernel) {
  return ctx->pick.conv == kernel || (ctx->pick.conv == I8IE_CONV_AUTO && (kernel == I8IE_CONV_PCONV || kernel == I8IE_CONV_TCONV));
}

#define I8IE_HIP_TRY(expr)                                                                  \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) {                                                                \
      i8ie_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return I8IE_ERR_HIP;                                                                  \
    }                                                                                       \
  } while (0)

#define I8IE_REQUIRE(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) {                                                \
      i8ie_set_error("%s: %s (%s)", __func__, msg, #cond);        \
      return I8IE_ERR_ARG;                                        \
    }                                                             \
  } while (0)

#define I8IE_TRY(expr)            \
  do {                            \
    int rc__ = (expr);            \
    if (rc__ != I8IE_OK) return rc__; \
  } while (0)

#define I8IE_LAUNCH_CHECK()  I8IE_HIP_TRY(hipGetLastError())

// Make sure ctx->ws holds at least `bytes`; grows by sync + realloc (rare).
int i8ie_ws_reserve(i8ie_ctx* ctx, size_t bytes);

static inline size_t i8ie_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- GEMM core (i8ie_gemm.hip) ---------------------------------------------
enum { I8IE_OUT_ROWMAJOR = 0, I8IE_OUT_NCHW = 1 };

struct I8ieGemmArgs {
  const uint8_t* A;  // u8 [M][lda], rows 16-B aligned, K-contiguous
  long lda;
  int M;
  int Ka;            // readable bytes per A row (multiple of 16)
  const int8_t* B;   // s8 packed [Npad][Kpad], zero padded, Npad % 128 == 0, Kpad % 64 == 0
  int Kpad;
  int N;
  const int32_t* oc;    // [N] reference offset vector
  const int32_t* wsum;  // [N] sum_k q_w[j,k] (exact): the u8 -> s8 re-biasing term
  const int8_t* qb;     // [N] or nullptr: Linear's float bias step
  float s_in, s_w, s_out;
  int zp_out;
  uint8_t* out;
  int out_mode;  // I8IE_OUT_ROWMAJOR: out[M][N]; I8IE_OUT_NCHW: out[(img*N + j)*P + p], row = img*P + p
  int P;
  int32_t* acc;  // nullptr or [M][N]
  int Ktrue;     // unpadded reduction length (profiling: algorithmic ops = 2*M*N*Ktrue)
  const float* sbv;  // per-channel layers: [N] weight scales s_w[j] (s_w unused); nullptr otherwise
};
int i8ie_gemm_launch(i8ie_ctx* ctx, const I8ieGemmArgs& a);
