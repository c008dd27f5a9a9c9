// i8ie_layernorm.hip -- quantized LayerNorm over the last axis: i8ie_layernorm_affine,
// i8ie_layernorm_u8, i8ie_layernorm_u8_nhwc, i8ie_layernorm_f32.  The arithmetic is defined in include/i8ie_hip.h:
//     S1 = sum a, S2 = sum a^2, V = C S2 - S1^2 (integers), r = (float)(1 / sqrt((double)V + E)),
//     d = C a - S1, t = (float)d * r, u = t * g[c], v = u + b[c], q = clamp(trunc(v)), relu: q = max(q, zp_out)
// Every kernel here evaluates the last line as it is written (three fp32 operations; the library is built with
// -ffp-contract=off), so there is no estimate, no guard and nothing to replay: the op is bound by its 2 C bytes per row, and
// three multiply / add, two compares and a convert per byte stay below that.
//
// Three forms, identical bytes:
//   group   C <= 4096: a row belongs to a group of G lanes, G a power of two, 64 / G rows per wave.  A lane keeps ITEMS <= 4
//           items of 16 bytes in registers, item i of lane l at byte 16 (l + G i) of the row, so that one load instruction of a
//           group covers 16 G contiguous bytes.  G = the smallest power of two with 4 G >= ceil(C / 16):
//               C <=  64: 1     <= 128: 2     <= 256: 4     <= 512: 8     <= 1024: 16     <= 2048: 32     <= 4096: 64
//           (a row of 96 bytes: 2 lanes x 3 items, 32 rows per wave; 256 bytes: 4 lanes x 4 items, 16 rows per wave).  S1 and
//           S2 come from the packed dwords by the unsigned dot-4 instruction (x . 0x01010101 and x . x) and are reduced over
//           the group with __shfl_xor at distances G / 2 .. 1.  The row is read once.
//   block   longer rows: one block of 256 lanes per row, the same items (256 x 4 x 16 = 16384 bytes), the two sums reduced
//           per wave and then through LDS.
//   direct  one lane per row, plain loops over bytes, the row walked twice: for in, out, g or b not 16-byte aligned and for
//           everything under I8IE_OPT_FORCE_FALLBACK.  Grid-strides (grid_for).
// ALIGN is the widest access every row start allows: 16 (C % 16 == 0), 4 (C % 4 == 0) or 1; bytes of an item past the row's
// end are neither read nor written and count as 0 in both sums.  r is computed once per row (every lane of the group holds
// it); g and b are read as fp32, four at a time where ALIGN >= 4.  Stores are vector stores (16, 4 or 1 bytes).  out may
// alias in: a lane writes only the bytes it read itself, after the reductions.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxC = 16384;
constexpr int kGroupMaxC = 4096;  // 64 lanes x 4 items x 16 bytes

// where row p of a launch lies: flat rows (border 0 on this side: p * C) or pixels of a bordered NHWC buffer
struct LnSide {
  int64_t img, row, org;  // NhwcGeom
  int flat;
  uint32_t x4;  // 0x80808080 where this side is stored re-biased
};
struct LnArgs {
  const uint8_t* in;
  uint8_t* out;
  LnSide si, so;
  int64_t rows;
  int C, h, w;
  const float* g;
  const float* b;
  double E;
  int lo;  // relu: zp_out, else 0
};

__device__ __forceinline__ int64_t ln_at(const LnSide& s, int64_t p, int C, int h, int w) {
  if (s.flat) return p * C;
  const int64_t pr = p / w, x = p - pr * w, img = pr / h, y = pr - img * h;
  return img * s.img + s.org + y * s.row + x * C;
}

__device__ __forceinline__ float ln_rstd(uint32_t S1, uint32_t S2, int C, double E) {
  const int64_t V = (int64_t)C * (int64_t)S2 - (int64_t)S1 * (int64_t)S1;
  return (float)__ddiv_rn(1.0, __dsqrt_rn(__dadd_rn((double)V, E)));
}
__device__ __forceinline__ uint32_t ln_byte(uint32_t a, int C, uint32_t S1, float r, float g, float b, int lo) {
  const int d = C * (int)a - (int)S1;
  const float t = (float)d * r;
  const float u = t * g;
  const float v = u + b;
  const int q = v >= 255.0f ? 255 : (v < 0.0f ? 0 : (int)v);
  return (uint32_t)(q > lo ? q : lo);
}

// the 16 bytes at src + j of a row of C bytes as four plain dwords; bytes past the row's end are 0
template <int ALIGN>
__device__ __forceinline__ void ln_load(const uint8_t* src, int j, int C, uint32_t x4, uint32_t (&w)[4]) {
  if (ALIGN == 16) {
    const uint4 x = *reinterpret_cast<const uint4*>(src + j);
    w[0] = x.x ^ x4; w[1] = x.y ^ x4; w[2] = x.z ^ x4; w[3] = x.w ^ x4;
  } else if (ALIGN == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = j + 4 * k < C ? *reinterpret_cast<const uint32_t*>(src + j + 4 * k) ^ x4 : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + 4 * k + e < C) v |= ((uint32_t)src[j + 4 * k + e] ^ (x4 & 0xFFu)) << (8 * e);
      w[k] = v;
    }
  }
}

// normalise and store the item at byte j of the row
template <int ALIGN>
__device__ __forceinline__ void ln_store(uint8_t* dst, int j, int C, uint32_t x4, const uint32_t (&w)[4], uint32_t S1, float r,
                                         const float* g, const float* b, int lo) {
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = j + 4 * k;
    float gg[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ALIGN >= 4) {
      if (c < C) {
        const float4 g4 = *reinterpret_cast<const float4*>(g + c), b4 = *reinterpret_cast<const float4*>(b + c);
        gg[0] = g4.x; gg[1] = g4.y; gg[2] = g4.z; gg[3] = g4.w;
        bb[0] = b4.x; bb[1] = b4.y; bb[2] = b4.z; bb[3] = b4.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < C) {
          gg[e] = g[c + e];
          bb[e] = b[c + e];
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) v |= ln_byte((w[k] >> (8 * e)) & 0xFFu, C, S1, r, gg[e], bb[e], lo) << (8 * e);
    o[k] = v ^ x4;
  }
  if (ALIGN == 16) {
    *reinterpret_cast<uint4*>(dst + j) = make_uint4(o[0], o[1], o[2], o[3]);
  } else if (ALIGN == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j + 4 * k < C) *reinterpret_cast<uint32_t*>(dst + j + 4 * k) = o[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + 4 * k + e < C) dst[j + 4 * k + e] = (uint8_t)(o[k] >> (8 * e));
  }
}

// BLOCK = false: G lanes per row (G a power of two <= 64), kThreads / G rows per block.  BLOCK = true: G == kThreads, one
// row per block.  ITEMS * G * 16 >= C.
template <int ITEMS, int ALIGN, bool BLOCK>
__global__ __launch_bounds__(kThreads) void layernorm_u8_kernel(const LnArgs a, int G) {
  __shared__ uint32_t red[2][kThreads / 64];
  const int l = BLOCK ? (int)threadIdx.x : (int)threadIdx.x & (G - 1);
  const int64_t row = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (kThreads / G) + (int)threadIdx.x / G;
  if (row >= a.rows) return;  // (a whole group leaves together; BLOCK: never taken)
  const int C = a.C;
  const uint8_t* src = a.in + ln_at(a.si, row, C, a.h, a.w);
  uint8_t* dst = a.out + ln_at(a.so, row, C, a.h, a.w);
  uint32_t w[ITEMS][4];
  uint32_t S1 = 0, S2 = 0;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int j = 16 * (l + G * i);
    if (j < C) {
      ln_load<ALIGN>(src, j, C, a.si.x4, w[i]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        S1 = __builtin_amdgcn_udot4(w[i][k], 0x01010101u, S1, false);
        S2 = __builtin_amdgcn_udot4(w[i][k], w[i][k], S2, false);
      }
    }
  }
  if (BLOCK) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      S1 += (uint32_t)__shfl_xor((int)S1, o, 64);
      S2 += (uint32_t)__shfl_xor((int)S2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = S1;
      red[1][threadIdx.x >> 6] = S2;
    }
    __syncthreads();
    S1 = S2 = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
      S1 += red[0][k];
      S2 += red[1][k];
    }
  } else {
    for (int o = G >> 1; o > 0; o >>= 1) {
      S1 += (uint32_t)__shfl_xor((int)S1, o, 64);
      S2 += (uint32_t)__shfl_xor((int)S2, o, 64);
    }
  }
  const float r = ln_rstd(S1, S2, C, a.E);
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int j = 16 * (l + G * i);
    if (j < C) ln_store<ALIGN>(dst, j, C, a.so.x4, w[i], S1, r, a.g, a.b, a.lo);
  }
}

// the definition verbatim: one lane per row, bytes in ascending c, the row walked twice
__global__ __launch_bounds__(kThreads) void layernorm_u8_direct_kernel(const LnArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int C = a.C;
  const uint32_t xi = a.si.x4 & 0xFFu, xo = a.so.x4 & 0xFFu;
  for (int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x; row < a.rows; row += stride) {
    const uint8_t* src = a.in + ln_at(a.si, row, C, a.h, a.w);
    uint8_t* dst = a.out + ln_at(a.so, row, C, a.h, a.w);
    uint32_t S1 = 0, S2 = 0;
    for (int c = 0; c < C; ++c) {
      const uint32_t v = (uint32_t)src[c] ^ xi;
      S1 += v;
      S2 += v * v;
    }
    const float r = ln_rstd(S1, S2, C, a.E);
    for (int c = 0; c < C; ++c) dst[c] = (uint8_t)(ln_byte((uint32_t)src[c] ^ xi, C, S1, r, a.g[c], a.b[c], a.lo) ^ xo);
  }
}

// FP32, off the timed path: one lane per row, plain loops in ascending c
// (element c of row r = (o, i) lies at (o * C + c) * inner + i)
__global__ __launch_bounds__(kThreads) void layernorm_f32_kernel(const float* in, float* out, int64_t rows, int C, const float* gamma,
                                                                 const float* beta, float eps, int64_t inner) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += stride) {
    const int64_t o = r / inner;
    const float* src = in + o * C * inner + (r - o * inner);
    float* dst = out + o * C * inner + (r - o * inner);
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum = sum + src[c * inner];
    const float mean = sum / (float)C;
    float sq = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float dx = src[c * inner] - mean;
      const float p = dx * dx;
      sq = sq + p;
    }
    const float var = sq / (float)C;
    const float sd = sqrtf(var + eps);
    for (int c = 0; c < C; ++c) {
      const float dx = src[c * inner] - mean;
      const float nrm = dx / sd;
      const float sc = nrm * gamma[c];
      dst[c * inner] = sc + beta[c];
    }
  }
}

// E of the definition, or a negative value where the arguments do not allow it
double ln_E(int C, float s_in, float eps) {
  if (!(std::isfinite(eps) && eps > 0.0f && std::isfinite(s_in) && s_in > 0.0f)) return -1.0;
  const double E = (double)C * (double)C * (double)eps / ((double)s_in * (double)s_in);
  if (!(std::isfinite(E) && E > 0.0 && std::isfinite((float)(1.0 / std::sqrt(E))))) return -1.0;
  return E;
}

LnSide ln_side(int C, int h, int w, int border, int s8) {
  const NhwcGeom g = buf_geom(C, h, w, border);
  return {g.img, g.row, g.org, border == 0 ? 1 : 0, s8 ? 0x80808080u : 0u};
}

template <int ALIGN, bool BLOCK>
void ln_launch_items(i8ie_ctx* ctx, const LnArgs& a, int items, int G, unsigned grid) {
  switch (items) {
    case 1: layernorm_u8_kernel<1, ALIGN, BLOCK><<<grid, kThreads, 0, ctx->stream>>>(a, G); break;
    case 2: layernorm_u8_kernel<2, ALIGN, BLOCK><<<grid, kThreads, 0, ctx->stream>>>(a, G); break;
    case 3: layernorm_u8_kernel<3, ALIGN, BLOCK><<<grid, kThreads, 0, ctx->stream>>>(a, G); break;
    default: layernorm_u8_kernel<4, ALIGN, BLOCK><<<grid, kThreads, 0, ctx->stream>>>(a, G); break;
  }
}
template <bool BLOCK>
void ln_launch_align(i8ie_ctx* ctx, const LnArgs& a, int items, int G, unsigned grid) {
  if (a.C % 16 == 0) ln_launch_items<16, BLOCK>(ctx, a, items, G, grid);
  else if (a.C % 4 == 0) ln_launch_items<4, BLOCK>(ctx, a, items, G, grid);
  else ln_launch_items<1, BLOCK>(ctx, a, items, G, grid);
}

int ln_run(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n, int C, int h,
           int w, const float* g, const float* b, double E, int relu, uint8_t zp_out) {
  LnArgs a;
  a.in = in;
  a.out = out;
  a.si = ln_side(C, h, w, in_border, in_s8);
  a.so = ln_side(C, h, w, out_border, out_s8);
  a.rows = (int64_t)n * h * w;
  a.C = C;
  a.h = h;
  a.w = w;
  a.g = g;
  a.b = b;
  a.E = E;
  a.lo = relu ? (int)zp_out : 0;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const bool direct = (ctx->options & 1u) || !aligned_to(in, 16) || !aligned_to(out, 16) || !aligned_to(g, 16) || !aligned_to(b, 16);
  const int n16 = (C + 15) / 16;
  const double bytes = 2.0 * (double)a.rows * C;
  if (direct) {
    I8ieProfScope prof(ctx, "layernorm_u8_direct", 0.0, bytes);
    layernorm_u8_direct_kernel<<<grid_for(a.rows), kThreads, 0, ctx->stream>>>(a);
  } else if (C <= kGroupMaxC) {
    int G = 1;
    while (4 * G < n16) G <<= 1;
    const int rpb = kThreads / G;
    I8ieProfScope prof(ctx, "layernorm_u8_group", 0.0, bytes);
    ln_launch_align<false>(ctx, a, (n16 + G - 1) / G, G, (unsigned)((a.rows + rpb - 1) / rpb));
  } else {
    I8ieProfScope prof(ctx, "layernorm_u8_block", 0.0, bytes);
    ln_launch_align<true>(ctx, a, (n16 + kThreads - 1) / kThreads, kThreads, (unsigned)a.rows);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // namespace

extern "C" {

int i8ie_layernorm_affine(const float* gamma, const float* beta, int C, float s_out, uint8_t zp_out, float* g_host, float* b_host) {
  I8IE_REQUIRE(gamma && beta && g_host && b_host, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(std::isfinite(s_out) && s_out > 0.0f, "the output scale must be finite and positive");
  for (int c = 0; c < C; ++c) {
    const float g = gamma[c] / s_out;
    const float q = beta[c] / s_out;
    const float b = q + (float)zp_out;
    I8IE_REQUIRE(std::isfinite(g) && std::isfinite(b), "gamma / s_out and beta / s_out must be finite");
    g_host[c] = g;
    b_host[c] = b;
  }
  return I8IE_OK;
}

int i8ie_layernorm_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t rows, int C, const float* g, const float* b, float s_in,
                      float eps, int relu, uint8_t zp_out) {
  I8IE_REQUIRE(ctx && in && out && g && b, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(rows > 0 && rows <= 0x7FFFFFFF, "bad row count (1 <= rows <= 2^31 - 1)");
  const double E = ln_E(C, s_in, eps);
  I8IE_REQUIRE(E > 0.0, "eps and the input scale must be finite and positive (and C^2 eps / s_in^2 an ordinary number)");
  I8IE_REQUIRE(aligned_to(g, 4) && aligned_to(b, 4), "g and b must be 4-byte aligned");
  return ln_run(ctx, in, 0, 0, out, 0, 0, 1, C, 1, (int)rows, g, b, E, relu, zp_out);
}

int i8ie_layernorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
                           int C, int h, int w, const float* g, const float* b, float s_in, float eps, int relu, uint8_t zp_out) {
  I8IE_REQUIRE(ctx && in && out && g && b, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0 && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE((int64_t)n * h * w <= 0x7FFFFFFF, "too many pixels for one launch");
  const double E = ln_E(C, s_in, eps);
  I8IE_REQUIRE(E > 0.0, "eps and the input scale must be finite and positive (and C^2 eps / s_in^2 an ordinary number)");
  I8IE_REQUIRE(aligned_to(g, 4) && aligned_to(b, 4), "g and b must be 4-byte aligned");
  return ln_run(ctx, in, in_border, in_s8, out, out_border, out_s8, n, C, h, w, g, b, E, relu, zp_out);
}

int i8ie_layernorm_f32(i8ie_ctx* ctx, const float* in, float* out, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                       int64_t inner) {
  I8IE_REQUIRE(ctx && in && out && gamma && beta, "null argument");
  I8IE_REQUIRE(inner >= 1 && rows % inner == 0, "inner must be positive and divide rows");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(rows > 0, "bad row count");
  I8IE_REQUIRE(std::isfinite(eps) && eps > 0.0f, "eps must be finite and positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "layernorm_f32", 0.0, 8.0 * (double)rows * C);
  layernorm_f32_kernel<<<grid_for(rows), kThreads, 0, ctx->stream>>>(in, out, rows, C, gamma, beta, eps, inner);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
