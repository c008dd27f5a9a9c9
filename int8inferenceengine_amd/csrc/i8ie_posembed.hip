// i8ie_posembed.hip -- position embedding with an optional class token: i8ie_posembed_table,
// i8ie_posembed_u8_nhwc, i8ie_posembed_f32.  The arithmetic is defined in include/i8ie_hip.h:
//     fa = (float)((int)a - (int)zp_in) * s_in   (the class column: fa = +0)
//     t  = (fa + E[tok][ch]) / s_out + (float)zp_out;  q = clamp(trunc(t));  relu: q = max(q, zp_out)
// which is the residual Add's sequence (i8ie_binary.hip) with the second operand a float that needs no dequantisation.
//
// Evaluation, bit-identical to that sequence for every input byte and every finite E.  Write J = fa + E, x = J / s_out.
//   exact    the sequence itself ((float)a - (float)zp_in is the exact integer difference).
//   guarded  J as above (the same product, the same one sum), then e = fma(J, r, zp_out - 0.5) with r = fl(1 / s_out) from the
//            host, packed by i8ie_requant.h's guarded pack: a dword holding a value closer than 2^-13 to a rounding boundary
//            replays the exact sequence.  The bound is the Add's, word for word: while |x| < 257 the reference rounds twice
//            behind J (the quotient, the sum: each <= 2^-16) and the estimate twice (r: 257 * 2^-24 < 2^-16, the fma:
//            <= 2^-16), so |t - (e + 0.5)| < 6.2e-5 < 2^-13.  Beyond that range both sides saturate, both being monotone in
//            J: t >= 255 or t < 0 on the one side, e >= 256.4 or e <= -2.4 on the other (with the relu both give zp_out
//            there); a J or a product J * r that overflows is an infinity of the right sign on both sides, and no NaN can
//            arise (J, r and zp_out - 0.5 are never NaN, r is never 0 or infinite).  Taken only for ordinary scales
//            (i8ie_requant.h's rule), so that r is a normal number; E is not pre-multiplied by r: the sum J stays the
//            definition's own, and nothing has to be proven about a cancellation between two scaled terms.
//
// Two u8 kernels, identical bytes:
//   nhwc    An item is VEC bytes of one output token's channels, VEC = 16 / 4 / 1 by c % 16 and c % 4.  A block holds `rows`
//           whole tokens of `lanes_c` items each (rows * lanes_c <= 256; consecutive lanes take consecutive channel items of
//           one token, then the next token, so a wave's accesses are contiguous), and every lane walks up to kWalk images with
//           its VEC values of E in registers: the table is read once per walk * VEC output bytes (from L2: every group of
//           images reads the same table).  The walk is kWalk, halved while the launch has fewer than kFullGrid units: a small
//           batch would otherwise be a few blocks, each a chain of dependent steps.  The class column has no input byte: its
//           lanes evaluate the same line with fa = +0.  Blocks stride over (image group, channel chunk, token tile) units up
//           to a grid cap.  64-bit offsets.  Reads the interior of a bordered, plain or re-biased buffer as it lies and writes
//           the interior of another, of another geometry in the class form (h x w in, 1 x (T + 1) out).
//   direct  the definition verbatim, one lane per output byte, grid-stride: in, out or E not 16-byte aligned, and everything
//           under I8IE_OPT_FORCE_FALLBACK.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_requant.h"

namespace {

constexpr int kMaxC = 16384;
constexpr int kWalk = I8IE_POSEMBED_WALK;  // images a lane of the nhwc kernel walks with its E values in registers, at most
constexpr int kFullGrid = 512;             // units below which the walk is halved: two blocks per compute unit of the 256

struct PeParams {
  float si, zpi, sc, zpc;  // dequantize; the output's scale and zero point
  float rc, zph, lof;      // estimate: fl(1 / s_out), zp_out - 0.5, its lower clamp (relu: zp_out; else -1 = none)
  int lo;                  // relu ? zp_out : 0
  int fast;                // the estimate may be used (ordinary scales)
  uint32_t xi, xo;         // 0x80808080 where that buffer holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
};

// the walk of the nhwc kernel: tokens where i8ie_pointwise.h's PixelWalk has pixels, images where it has a run of pixels
struct TokenWalk {
  int64_t units;      // groups * chunks * tiles
  int cpv;            // items per token: c / VEC
  int lanes_c, rows;  // a block's shape: lanes_c = min(cpv, 256) items by rows = 256 / lanes_c tokens
  int chunks, tiles;  // channel chunks of lanes_c items per token; tiles of `rows` tokens
  int n, c, w, cls;   // images; channels; the input's width; 1 in the class form
  int walk;           // images a lane walks: kWalk, halved while the launch has fewer than kFullGrid units
  int tokens;         // T' = h * w + cls
};

// the exact sequence behind fa
__device__ __forceinline__ uint32_t pe_exact_f(float fa, float e, const PeParams& p) {
  const float t = (fa + e) / p.sc + p.zpc;
  const int u = (t >= 255.0f) ? 255 : ((t < 0.0f) ? 0 : (int)t);
  return (uint32_t)(u > p.lo ? u : p.lo);
}
__device__ __forceinline__ float pe_deq(uint32_t a, const PeParams& p) { return ((float)a - p.zpi) * p.si; }

// four elements as they lie in memory against the four channels' E; has_in = false: the class column (fa = +0, a4 unused)
template <bool HAS_IN>
__device__ __forceinline__ uint32_t pe4(uint32_t a4, const float* e, const PeParams& p) {
  a4 ^= p.xi;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = HAS_IN ? pe_deq((a4 >> (8 * r)) & 0xFFu, p) : 0.0f;
      packed = i8ie_requant_est_step(__builtin_fmaf(fa + e[r], p.rc, p.zph), p.lof, r, packed, worst);
    }
    if (i8ie_requant_est_ok(worst)) return packed ^ p.xo;
  }
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= pe_exact_f(HAS_IN ? pe_deq((a4 >> (8 * r)) & 0xFFu, p) : 0.0f, e[r], p) << (8 * r);
  return packed ^ p.xo;
}

// one item: VEC bytes at `in` (not read when !HAS_IN) against ev -> VEC bytes at `out`
template <int VEC, bool HAS_IN>
__device__ __forceinline__ void pe_item(const uint8_t* in, uint8_t* out, const float* ev, const PeParams& p) {
  if constexpr (VEC == 16) {
    uint4 v = {0u, 0u, 0u, 0u};
    if constexpr (HAS_IN) v = *reinterpret_cast<const uint4*>(in);
    v.x = pe4<HAS_IN>(v.x, ev, p);
    v.y = pe4<HAS_IN>(v.y, ev + 4, p);
    v.z = pe4<HAS_IN>(v.z, ev + 8, p);
    v.w = pe4<HAS_IN>(v.w, ev + 12, p);
    *reinterpret_cast<uint4*>(out) = v;
  } else if constexpr (VEC == 4) {
    uint32_t v = 0u;
    if constexpr (HAS_IN) v = *reinterpret_cast<const uint32_t*>(in);
    *reinterpret_cast<uint32_t*>(out) = pe4<HAS_IN>(v, ev, p);
  } else {  // (one byte per lane takes the exact sequence)
    const float fa = HAS_IN ? pe_deq(((uint32_t)*in ^ p.xi) & 0xFFu, p) : 0.0f;
    *out = (uint8_t)(pe_exact_f(fa, ev[0], p) ^ (p.xo & 0xFFu));
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void posembed_u8_nhwc_kernel(const uint8_t* __restrict__ in, NhwcGeom gi, uint8_t* __restrict__ out,
                                                                     NhwcGeom go, const float* __restrict__ E, TokenWalk t, PeParams p) {
  const int pc = (int)threadIdx.x / t.lanes_c, ci = (int)threadIdx.x - pc * t.lanes_c;
  if (pc >= t.rows) return;  // (the lanes behind the block's last whole token)
  for (int64_t u = blockIdx.x; u < t.units; u += gridDim.x) {
    const int tile = (int)(u % t.tiles);
    const int64_t rest = u / t.tiles;
    const int chan = (int)(rest % t.chunks) * t.lanes_c + ci;
    const int img0 = (int)(rest / t.chunks) * t.walk;
    const int tok = tile * t.rows + pc;
    if (chan >= t.cpv || tok >= t.tokens) continue;
    float ev[VEC];
    const float* pe = E + (int64_t)tok * t.c + (int64_t)chan * VEC;
    if constexpr (VEC >= 4) {
#pragma unroll
      for (int j = 0; j < VEC; j += 4) {
        const float4 e4 = *reinterpret_cast<const float4*>(pe + j);
        ev[j] = e4.x; ev[j + 1] = e4.y; ev[j + 2] = e4.z; ev[j + 3] = e4.w;
      }
    } else {
      ev[0] = pe[0];
    }
    const int images = (t.n - img0) < t.walk ? (t.n - img0) : t.walk;
    const int j = tok - t.cls;  // the input token; -1: the class column
    // the output token's pixel: (0, tok) of the 1 x T' map in the class form, the input's own pixel otherwise
    const int y = j >= 0 ? j / t.w : 0, x = j >= 0 ? j - y * t.w : 0;
    int64_t oo = (int64_t)img0 * go.img + go.org + (t.cls ? (int64_t)tok * t.c : (int64_t)y * go.row + (int64_t)x * t.c) + (int64_t)chan * VEC;
    if (j < 0) {  // no input byte (one token in T': its few lanes recompute the same VEC bytes per image)
      for (int k = 0; k < images; ++k) pe_item<VEC, false>(nullptr, out + oo + k * go.img, ev, p);
      continue;
    }
    int64_t oi = (int64_t)img0 * gi.img + gi.org + (int64_t)y * gi.row + (int64_t)x * t.c + (int64_t)chan * VEC;
#pragma unroll 2
    for (int k = 0; k < images; ++k) {
      pe_item<VEC, true>(in + oi, out + oo, ev, p);
      oi += gi.img;
      oo += go.img;
    }
  }
}

// the definition verbatim, one lane per output byte: element e = (image, output token, channel)
__global__ __launch_bounds__(kThreads) void posembed_u8_direct_kernel(const uint8_t* in, NhwcGeom gi, uint8_t* out, NhwcGeom go, int64_t total,
                                                                       int c, int w, int cls, int tokens, const float* E, PeParams p) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t tk = e / c, img = tk / tokens;
    const int ch = (int)(e - tk * c), tok = (int)(tk - img * tokens);
    const int j = tok - cls;
    const int y = j >= 0 ? j / w : 0, x = j >= 0 ? j - y * w : 0;
    const int64_t oo = img * go.img + go.org + (cls ? (int64_t)tok * c : (int64_t)y * go.row + (int64_t)x * c) + ch;
    float fa = 0.0f;
    if (j >= 0) {
      const int64_t oi = img * gi.img + gi.org + (int64_t)y * gi.row + (int64_t)x * c + ch;
      fa = (float)((int)((in[oi] ^ p.xi) & 0xFFu) - (int)p.zpi) * p.si;
    }
    const float t = (fa + E[(int64_t)tok * c + ch]) / p.sc + p.zpc;
    int q = t >= 255.0f ? 255 : (t < 0.0f ? 0 : (int)t);
    q = q > p.lo ? q : p.lo;
    out[oo] = (uint8_t)((uint32_t)q ^ (p.xo & 0xFFu));
  }
}

// FP32, off the timed path: one lane per output element of NCHW [n, c, T']
__global__ __launch_bounds__(kThreads) void posembed_f32_kernel(const float* in, float* out, int64_t total, int c, int hw, int cls,
                                                                 const float* E) {
  const int tokens = hw + cls;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / tokens;  // image * c + channel
    const int tok = (int)(e - row * tokens), ch = (int)(row % c);
    const float ev = E[(int64_t)tok * c + ch];
    out[e] = tok < cls ? ev : in[row * hw + (tok - cls)] + ev;
  }
}

template <int VEC>
void pe_launch(i8ie_ctx* ctx, const uint8_t* in, const NhwcGeom& gi, uint8_t* out, const NhwcGeom& go, int n, int c, int h, int w, int cls,
               const float* E, const PeParams& p) {
  TokenWalk t;
  t.cpv = c / VEC;
  t.lanes_c = t.cpv < kThreads ? t.cpv : kThreads;
  t.rows = kThreads / t.lanes_c;
  t.chunks = (t.cpv + t.lanes_c - 1) / t.lanes_c;
  t.n = n; t.c = c; t.w = w; t.cls = cls;
  t.tokens = h * w + cls;
  t.tiles = (t.tokens + t.rows - 1) / t.rows;
  // a long walk reads the table once per kWalk images but leaves a small batch with too few blocks, each a chain of dependent
  // steps: the walk is halved until the grid is full (or the walk is one image)
  const auto units = [&](int walk) { return (int64_t)((n + walk - 1) / walk) * t.chunks * t.tiles; };
  t.walk = kWalk;
  while (t.walk > 1 && units(t.walk) < kFullGrid) t.walk >>= 1;
  t.units = units(t.walk);
  const int blocks = (int)(t.units > kMaxBlocks ? kMaxBlocks : t.units);
  posembed_u8_nhwc_kernel<VEC><<<blocks, kThreads, 0, ctx->stream>>>(in, gi, out, go, E, t, p);
}

}  // namespace

extern "C" {

int i8ie_posembed_table(const float* P, const float* cls, int tokens, int c, float* E_host) {
  I8IE_REQUIRE(P && E_host, "null argument");
  I8IE_REQUIRE(c >= 1 && c <= kMaxC, "bad dimension (1 <= c <= 16384)");
  I8IE_REQUIRE(tokens >= 1 && tokens <= 0x40000000, "bad dimension (1 <= tokens <= 2^30)");
  // (two passes: an error is reported before anything is written)
  for (int pass = 0; pass < 2; ++pass)
    for (int64_t i = 0; i < (int64_t)tokens * c; ++i) {
      const bool row0 = cls && i < c;
      const volatile float sum = row0 ? cls[i] + P[i] : P[i];  // (one rounding, whatever the host compiler's flags)
      const float e = sum;
      I8IE_REQUIRE(std::isfinite(P[i]) && (!row0 || std::isfinite(cls[i])) && std::isfinite(e),
                   "the position table, the class token and their sum must be finite");
      if (pass) E_host[i] = e;
    }
  return I8IE_OK;
}

int i8ie_posembed_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n, int c,
                          int h, int w, int class_token, const float* E, float s_in, uint8_t zp_in, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && in && out && E, "null argument");
  I8IE_REQUIRE(c >= 1 && c <= kMaxC, "bad dimension (1 <= c <= 16384)");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0 && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE((int64_t)h * w < 0x40000000, "bad dimension: more than 2^30 tokens per image");
  I8IE_REQUIRE(std::isfinite(s_in) && std::isfinite(255.0f * s_in) && std::isfinite(s_out) && s_out > 0.0f,
               "scales must be finite (255 * s_in too) and the output scale positive");
  I8IE_REQUIRE(aligned_to(E, 4), "the table must be 4-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int cls = class_token ? 1 : 0, tokens = h * w + cls;
  PeParams p;
  p.si = s_in; p.zpi = (float)zp_in; p.sc = s_out; p.zpc = (float)zp_out;
  p.rc = 1.0f / s_out;
  p.zph = (float)zp_out - 0.5f;
  p.lof = relu ? (float)zp_out : -1.0f;
  p.lo = relu ? zp_out : 0;
  p.fast = ordinary(s_in) && ordinary(s_out) ? 1 : 0;
  p.xi = in_s8 ? 0x80808080u : 0u;
  p.xo = out_s8 ? 0x80808080u : 0u;
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = cls ? buf_geom(c, 1, tokens, out_border) : buf_geom(c, h, w, out_border);
  const int64_t total = (int64_t)n * tokens * c;
  const double bytes = (double)total + (double)n * h * w * c + 4.0 * tokens * c;
  if ((ctx->options & 1u) || !aligned_to(in, 16) || !aligned_to(out, 16) || !aligned_to(E, 16)) {
    I8ieProfScope prof(ctx, "posembed_u8_direct", 0.0, bytes);
    posembed_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, gi, out, go, total, c, w, cls, tokens, E, p);
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  I8ieProfScope prof(ctx, "posembed_u8_nhwc", 0.0, bytes);
  if (c % 16 == 0) pe_launch<16>(ctx, in, gi, out, go, n, c, h, w, cls, E, p);
  else if (c % 4 == 0) pe_launch<4>(ctx, in, gi, out, go, n, c, h, w, cls, E, p);
  else pe_launch<1>(ctx, in, gi, out, go, n, c, h, w, cls, E, p);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_posembed_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int class_token, const float* E) {
  I8IE_REQUIRE(ctx && in && out && E, "null argument");
  I8IE_REQUIRE(c >= 1 && c <= kMaxC, "bad dimension (1 <= c <= 16384)");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0, "bad dimension");
  I8IE_REQUIRE((int64_t)h * w < 0x40000000, "bad dimension: more than 2^30 tokens per image");
  I8IE_REQUIRE(aligned_to(in, 4) && aligned_to(out, 4) && aligned_to(E, 4), "buffers must be 4-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int cls = class_token ? 1 : 0;
  const int64_t total = (int64_t)n * c * (h * w + cls);
  I8ieProfScope prof(ctx, "posembed_f32", 0.0, 8.0 * (double)total);
  posembed_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, c, h * w, cls, E);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
