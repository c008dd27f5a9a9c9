// i8ie_batchnorm.hip -- quantized inference BatchNorm: i8ie_batchnorm_affine, i8ie_batchnorm_u8,
// i8ie_batchnorm_u8_nhwc, i8ie_batchnorm_f32.  The arithmetic is defined in include/i8ie_hip.h:
//     x = (float)((int)a - (int)zp_in) * s_in;  t = x * g[c];  v = t + b[c];  q = clamp(trunc(v));  relu: q = max(q, zp_out)
// with g[c], b[c] from i8ie_batchnorm_affine (the running statistics, gamma, beta and the output's scale and zero point folded
// on the host, in double).  Every kernel here evaluates that line as it is written (three fp32 operations; the library is
// built with -ffp-contract=off), so there is no estimate, no guard and nothing to replay, as in i8ie_layernorm.hip: the op
// moves two bytes per element, and a subtract, three multiply / add, a clamp and a convert per byte stay below that.
//   clamp + truncation + relu in one step: q = (int)min(max(v, lo), 255), lo = relu ? zp_out : 0.  For v >= 255 both give 255;
//   for v < lo the definition gives max(trunc(max(v, 0)), lo) = lo; in between trunc(v) = floor(v) >= lo, lo being an integer.
//   v is never a NaN (the entries refuse a g, b or 255 * s_in that is not finite).
//
// Two u8 kernels, identical bytes:
//   nhwc    The structure of Mul's gate form (i8ie_binary.hip).  An item is VEC bytes of one pixel's channels, VEC = 16 / 4 /
//           1 by C % 16 and C % 4.  A block holds `rows` whole pixels of `lanes_c` items each (rows * lanes_c <= 256;
//           consecutive lanes take consecutive channel items of one pixel, then the next pixel, so a wave's loads are
//           contiguous), and every lane walks kWalk pixels of one image, `rows` pixels apart: its channel item never changes,
//           so its VEC values of g and of b are loaded once per kWalk * VEC output bytes and stay in registers.  Blocks stride
//           over (image, channel chunk, pixel tile) units up to a grid cap.  64-bit offsets.  Reads the interior of a bordered,
//           plain or re-biased buffer as it lies and writes the interior of another.
//   direct  the definition verbatim, one lane per byte, grid-stride: the flat entry (reference-order tensors: the channel of
//           physical byte p is (p / inner) % C), in, out, g or b not 16-byte aligned, and everything under
//           I8IE_OPT_FORCE_FALLBACK.
// out may be in itself where both geometries agree: a lane reads its bytes before it stores them and no other lane reads them.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxC = 16384;
constexpr int kWalk = 8;  // pixels a lane of the nhwc kernel walks with its g and b in registers

struct BnParams {
  float s_in, zp_in;  // dequantize
  float lo;           // relu ? zp_out : 0
  uint32_t xi, xo;    // 0x80808080 where that buffer holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
};

__device__ __forceinline__ uint32_t bn_byte(uint32_t a, float g, float b, const BnParams& p) {
  const float x = ((float)a - p.zp_in) * p.s_in;  // ((float)a - (float)zp_in is the exact integer difference)
  const float t = x * g;
  const float v = t + b;
  return (uint32_t)(int)__builtin_fminf(__builtin_fmaxf(v, p.lo), 255.0f);
}
// four elements as they lie in memory against the four channels' g and b
__device__ __forceinline__ uint32_t bn4(uint32_t a4, const float* g, const float* b, const BnParams& p) {
  a4 ^= p.xi;
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= bn_byte((a4 >> (8 * r)) & 0xFFu, g[r], b[r], p) << (8 * r);
  return packed ^ p.xo;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void batchnorm_u8_nhwc_kernel(const uint8_t* in, NhwcGeom gi, uint8_t* out, NhwcGeom go,
                                                                      const float* __restrict__ g, const float* __restrict__ b, PixelWalk t,
                                                                      BnParams p) {
  const int pc = (int)threadIdx.x / t.lanes_c, ci = (int)threadIdx.x - pc * t.lanes_c;
  if (pc >= t.rows) return;  // (the lanes behind the block's last whole pixel)
  for (int64_t u = blockIdx.x; u < t.units; u += gridDim.x) {
    const int tile = (int)(u % t.tiles);
    const int64_t rest = u / t.tiles;
    const int chan = (int)(rest % t.chunks) * t.lanes_c + ci;
    const int64_t img = rest / t.chunks;
    int pix = tile * (t.rows * kWalk) + pc;
    if (chan >= t.cpv || pix >= t.hw) continue;
    float gv[VEC], bv[VEC];
    if constexpr (VEC >= 4) {
#pragma unroll
      for (int j = 0; j < VEC; j += 4) {
        const float4 g4 = *reinterpret_cast<const float4*>(g + chan * VEC + j), b4 = *reinterpret_cast<const float4*>(b + chan * VEC + j);
        gv[j] = g4.x; gv[j + 1] = g4.y; gv[j + 2] = g4.z; gv[j + 3] = g4.w;
        bv[j] = b4.x; bv[j + 1] = b4.y; bv[j + 2] = b4.z; bv[j + 3] = b4.w;
      }
    } else {
      gv[0] = g[chan];
      bv[0] = b[chan];
    }
    const int y = pix / t.w;
    int x = pix - y * t.w;
    int64_t oi = img * gi.img + gi.org + (int64_t)y * gi.row + (int64_t)x * t.c + (int64_t)chan * VEC;
    int64_t oo = img * go.img + go.org + (int64_t)y * go.row + (int64_t)x * t.c + (int64_t)chan * VEC;
#pragma unroll 2
    for (int k = 0; k < kWalk; ++k) {
      if constexpr (VEC == 16) {
        uint4 v = *reinterpret_cast<const uint4*>(in + oi);
        v.x = bn4(v.x, gv, bv, p);
        v.y = bn4(v.y, gv + 4, bv + 4, p);
        v.z = bn4(v.z, gv + 8, bv + 8, p);
        v.w = bn4(v.w, gv + 12, bv + 12, p);
        *reinterpret_cast<uint4*>(out + oo) = v;
      } else if constexpr (VEC == 4) {
        *reinterpret_cast<uint32_t*>(out + oo) = bn4(*reinterpret_cast<const uint32_t*>(in + oi), gv, bv, p);
      } else {
        out[oo] = (uint8_t)(bn_byte(((uint32_t)in[oi] ^ p.xi) & 0xFFu, gv[0], bv[0], p) ^ (p.xo & 0xFFu));
      }
      pix += t.rows;
      if (pix >= t.hw) break;
      x += t.step_x;
      oi += t.a_step;
      oo += t.o_step;
      if (x >= t.w) {
        x -= t.w;
        oi += t.a_wrap;
        oo += t.o_wrap;
      }
    }
  }
}

// the definition verbatim, one lane per byte.  flat: physical byte e of both buffers, channel (e / inner) % C.  Otherwise
// element e = (pixel, channel) of [n, h, w, C], each side at its own bordered address.
__global__ __launch_bounds__(kThreads) void batchnorm_u8_direct_kernel(const uint8_t* in, NhwcGeom gi, uint8_t* out, NhwcGeom go, int64_t total,
                                                                        int C, int h, int w, int64_t inner, int flat, const float* g,
                                                                        const float* b, BnParams p) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    int c;
    int64_t oi, oo;
    if (flat) {
      c = (int)((e / inner) % C);
      oi = oo = e;
    } else {
      const int64_t px = e / C, pr = px / w, img = pr / h;
      c = (int)(e - px * C);
      const int64_t x = px - pr * w, y = pr - img * h;
      oi = img * gi.img + gi.org + y * gi.row + x * C + c;
      oo = img * go.img + go.org + y * go.row + x * C + c;
    }
    const float xf = (float)((int)((in[oi] ^ p.xi) & 0xFFu) - (int)p.zp_in) * p.s_in;
    const float t = xf * g[c];
    const float v = t + b[c];
    int q = v >= 255.0f ? 255 : (v < 0.0f ? 0 : (int)v);
    q = q > (int)p.lo ? q : (int)p.lo;
    out[oo] = (uint8_t)((uint32_t)q ^ (p.xo & 0xFFu));
  }
}

// FP32, off the timed path: one lane per element, channel (e / inner) % C
__global__ __launch_bounds__(kThreads) void batchnorm_f32_kernel(const float* in, float* out, int64_t total, int C, int64_t inner,
                                                                  const float* gamma, const float* beta, const float* mean, const float* var,
                                                                  float eps) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int c = (int)((e / inner) % C);
    const float dx = in[e] - mean[c];
    const float sd = sqrtf(var[c] + eps);
    const float nrm = dx / sd;
    const float sc = nrm * gamma[c];
    out[e] = sc + beta[c];
  }
}

BnParams bn_params(float s_in, uint8_t zp_in, int relu, uint8_t zp_out, int in_s8, int out_s8) {
  BnParams p;
  p.s_in = s_in;
  p.zp_in = (float)zp_in;
  p.lo = relu ? (float)zp_out : 0.0f;
  p.xi = in_s8 ? 0x80808080u : 0u;
  p.xo = out_s8 ? 0x80808080u : 0u;
  return p;
}

// |x| <= 255 |s_in| must be finite: x * g is then never 0 * inf
bool bn_scale_ok(float s_in) { return std::isfinite(s_in) && std::isfinite(255.0f * s_in); }

template <int VEC>
void bn_launch(i8ie_ctx* ctx, const uint8_t* in, const NhwcGeom& gi, uint8_t* out, const NhwcGeom& go, int n, int C, int h, int w,
               const float* g, const float* b, const BnParams& p) {
  PixelWalk t;  // (i8ie_pointwise.h: the walk Mul's gate form takes)
  pixel_walk_init(t, VEC, kWalk, n, C, h, w, gi, go);
  const int blocks = pixel_walk_blocks(t);
  batchnorm_u8_nhwc_kernel<VEC><<<blocks, kThreads, 0, ctx->stream>>>(in, gi, out, go, g, b, t, p);
}

int bn_direct(i8ie_ctx* ctx, const uint8_t* in, const NhwcGeom& gi, uint8_t* out, const NhwcGeom& go, int64_t total, int C, int h, int w,
              int64_t inner, int flat, const float* g, const float* b, const BnParams& p) {
  I8ieProfScope prof(ctx, "batchnorm_u8_direct", 0.0, 2.0 * (double)total);
  batchnorm_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, gi, out, go, total, C, h, w, inner, flat, g, b, p);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // namespace

extern "C" {

int i8ie_batchnorm_affine(const float* gamma, const float* beta, const float* mean, const float* var, int C, float eps, float s_out,
                          uint8_t zp_out, float* g_host, float* b_host) {
  I8IE_REQUIRE(gamma && beta && mean && var && g_host && b_host, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(std::isfinite(eps) && eps > 0.0f, "eps must be finite and positive");
  I8IE_REQUIRE(std::isfinite(s_out) && s_out > 0.0f, "the output scale must be finite and positive");
  for (int c = 0; c < C; ++c) {
    I8IE_REQUIRE(std::isfinite(gamma[c]) && std::isfinite(beta[c]) && std::isfinite(mean[c]) && std::isfinite(var[c]),
                 "gamma, beta, mean and var must be finite");
    I8IE_REQUIRE(var[c] >= 0.0f, "var must not be negative");
  }
  // (two passes: an error is reported before anything is written)
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < C; ++c) {
      const double sd = std::sqrt((double)var[c] + (double)eps);
      const double k = (double)gamma[c] / sd;
      const float g = (float)(k / (double)s_out);
      const double mk = (double)mean[c] * k;
      const double num = (double)beta[c] - mk;
      const double q = num / (double)s_out;
      const float b = (float)(q + (double)zp_out);
      I8IE_REQUIRE(std::isfinite(g) && std::isfinite(b), "g = gamma / sqrt(var + eps) / s_out and b = (beta - mean k) / s_out + zp_out must be finite");
      if (pass) {
        g_host[c] = g;
        b_host[c] = b;
      }
    }
  return I8IE_OK;
}

int i8ie_batchnorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
                           int C, int h, int w, const float* g, const float* b, float s_in, uint8_t zp_in, int relu, uint8_t zp_out) {
  I8IE_REQUIRE(ctx && in && out && g && b, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0 && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE((int64_t)h * w <= 0x3FFFFFFF, "bad dimension: more than 2^30 pixels per image");
  I8IE_REQUIRE(bn_scale_ok(s_in), "the input scale must be finite (and 255 * s_in too)");
  I8IE_REQUIRE(aligned_to(g, 4) && aligned_to(b, 4), "g and b must be 4-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const BnParams p = bn_params(s_in, zp_in, relu, zp_out, in_s8, out_s8);
  const NhwcGeom gi = buf_geom(C, h, w, in_border), go = buf_geom(C, h, w, out_border);
  const int64_t total = (int64_t)n * h * w * C;
  if ((ctx->options & 1u) || !aligned_to(in, 16) || !aligned_to(out, 16) || !aligned_to(g, 16) || !aligned_to(b, 16))
    return bn_direct(ctx, in, gi, out, go, total, C, h, w, 1, 0, g, b, p);
  I8ieProfScope prof(ctx, "batchnorm_u8_nhwc", 0.0, 2.0 * (double)total);
  if (C % 16 == 0) bn_launch<16>(ctx, in, gi, out, go, n, C, h, w, g, b, p);
  else if (C % 4 == 0) bn_launch<4>(ctx, in, gi, out, go, n, C, h, w, g, b, p);
  else bn_launch<1>(ctx, in, gi, out, go, n, C, h, w, g, b, p);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_batchnorm_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t rows, int C, int64_t inner, const float* g, const float* b,
                      float s_in, uint8_t zp_in, int relu, uint8_t zp_out) {
  I8IE_REQUIRE(ctx && in && out && g && b, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(rows > 0 && rows <= 0x7FFFFFFF, "bad row count (1 <= rows <= 2^31 - 1)");
  I8IE_REQUIRE(inner >= 1 && rows % inner == 0, "inner must be positive and divide rows");
  I8IE_REQUIRE(bn_scale_ok(s_in), "the input scale must be finite (and 255 * s_in too)");
  I8IE_REQUIRE(aligned_to(g, 4) && aligned_to(b, 4), "g and b must be 4-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const NhwcGeom none = {0, 0, 0};
  return bn_direct(ctx, in, none, out, none, rows * C, C, 1, 1, inner, 1, g, b, bn_params(s_in, zp_in, relu, zp_out, 0, 0));
}

int i8ie_batchnorm_f32(i8ie_ctx* ctx, const float* in, float* out, int64_t rows, int C, int64_t inner, const float* gamma, const float* beta,
                       const float* mean, const float* var, float eps) {
  I8IE_REQUIRE(ctx && in && out && gamma && beta && mean && var, "null argument");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(rows > 0, "bad row count");
  I8IE_REQUIRE(inner >= 1 && rows % inner == 0, "inner must be positive and divide rows");
  I8IE_REQUIRE(std::isfinite(eps) && eps > 0.0f, "eps must be finite and positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "batchnorm_f32", 0.0, 8.0 * (double)rows * C);
  batchnorm_f32_kernel<<<grid_for(rows * C), kThreads, 0, ctx->stream>>>(in, out, rows * C, C, inner, gamma, beta, mean, var, eps);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
