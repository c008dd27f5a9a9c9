// i8ie_avgpool.hip -- quantized average pooling: i8ie_avgpool2d_u8, i8ie_avgpool2d_u8_nhwc,
// i8ie_avgpool2d_f32.
//
// The reference has no average pool.  Everything but the reduction follows its max_pool2d<u8_t> (src/functional.cc:36-64):
// NCHW logical shape, window kh x kw, stride s, floor output size (h - kh) / s + 1 by (w - kw) / s + 1, no padding, and the
// result carries the input's (scale, zero_point) unchanged.
//
// INT8: with n = kh * kw and S = the exact integer sum of the window's bytes,
//     q = (S + n / 2) / n          integer floor division: round to nearest, ties up
//     q = relu ? max(q, zp) : q    relu<u8> (src/functional.cc:15-26) on the result
// No fp32 step of the reference applies here, because the value never leaves the integers: input and output share one scale
// and one zero point, so the mean of the bytes is the mean of the values, and the only rounding is the one above.  Truncation
// (S / n) would put a bias of -1/2 LSB on every pooled tensor; round-to-nearest has none, and ties-up keeps it a pure integer
// rule.  The result does not depend on summation order.  n <= 65536 (I8IE_ERR_ARG beyond), so S <= 255 * 65536 < 2^24.
//
// FP32 (before convert(), and while calibrating): sum / n, the sum taken in fp32 in window order (rows outer, columns
// inner), then one IEEE division.  NaN and inf propagate as IEEE gives them.
//
// The division by the uniform n, without an integer-divide sequence (div_round below; tests/test_gpu_avgpool.py runs every
// reachable S through it):
//   multiplier  x = S + n / 2 <= 255 n + n / 2;  M = ceil(2^24 / n), e = M n - 2^24 in [0, n).  x M / 2^24 = x / n + x e / (n 2^24),
//               and floor() of it equals floor(x / n) when x e / (n 2^24) < 1 / n, i.e. x e < 2^24 (the fraction of x / n is at
//               most (n - 1) / n).  The host checks (255 n + n / 2) e < 2^24 with the actual e; it holds for every n <= 257
//               (for n <= 256 already by e < n: 255.5 n^2 < 2^24; n = 257 has e = 1).  x M < 2^32 there.
//   estimate    otherwise: y = fl(float(x) * fl(1 / n)), q' = trunc(y).  x < 2^25 converts with relative error <= 2^-24, as do
//               the reciprocal and the product, and x / n < 256, so |y - x / n| < 256 * 3.1 * 2^-24 < 2^-15: q' is
//               floor(x / n) or, where x / n lies that close to an integer, one off.  r = x - q' n is computed exactly in
//               integers and q' corrected by one where r < 0 or r >= n.
//
// NHWC kernels (the hot path), two regimes:
//   windowed   a lane owns one output pixel x one channel item (16 / 4 / 1 channels by c % 16, c % 4, as the add kernel),
//              reads dwordx4 / dword / byte per window pixel, sums the bytes of a dword in packed 16-bit halves (windows
//              with 255 n < 65536), divides with the multiplier, packs and stores once.  32-bit index arithmetic.
//   reduce     few outputs per image (the global pool: [N, 512, 4, 4] is 512 output bytes per image): one lane per output
//              would leave the machine idle at batch 125 and serialise its loads.  A block owns one output pixel x CI
//              channel items; its 256 lanes are CI items x SL slices of the window's pixels (SL = min(32, n rounded up
//              to a power of two), CI = 256 / SL), each lane sums its pixels in 32-bit sums, the slices are added through
//              LDS, and slice 0 divides, packs and stores.  [125, 512, 4, 4] is 250 blocks, [125, 512, 7, 7] 500.
//   The rule:  reduce when n >= 16 and there are fewer than 65536 windowed items (a quarter of the 256 CUs' 2048 lanes
//              each: below that the windowed form cannot fill the machine while each of its lanes walks n >= 16 pixels),
//              and always when 255 n >= 65536 (the windowed form has no 32-bit sums: such a window has more pixels than
//              a block has lanes, and is best split).  Everything else is windowed.
// Neither uses scratch or a per-call device allocation.  The NCHW and FP32 forms are off the timed path: one lane per
// output, plain loops.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxWindow = 65536;
constexpr int kPackedMax = 257;            // 255 * n < 65536
constexpr int kReduceMinWindow = 16;       // the regime rule (header)
constexpr int64_t kReduceMaxItems = 65536;

struct DivParams {
  uint32_t n, rnd;   // window size, n / 2
  uint32_t mul;      // ceil(2^24 / n) where the multiplier is proven exact (header), else 0: the estimate
  float rinv;        // fl(1 / n)
  uint32_t lo;       // relu ? zp : 0
};

DivParams make_div(int n, int relu, int zp) {
  DivParams d;
  d.n = (uint32_t)n;
  d.rnd = (uint32_t)n / 2;
  d.rinv = 1.0f / (float)n;
  d.lo = relu ? (uint32_t)zp : 0u;
  d.mul = 0;
  if (n <= kPackedMax) {
    const uint64_t M = ((1ull << 24) + (uint64_t)n - 1) / (uint64_t)n, e = M * (uint64_t)n - (1ull << 24);
    const uint64_t xmax = 255ull * (uint64_t)n + (uint64_t)n / 2;
    if (xmax * e < (1ull << 24) && xmax * M < (1ull << 32)) d.mul = (uint32_t)M;
  }
  return d;
}

// (S + n / 2) / n, then the relu floor
__device__ __forceinline__ uint32_t div_round(uint32_t S, const DivParams& d) {
  const uint32_t x = S + d.rnd;
  uint32_t q;
  if (d.mul) {
    q = (x * d.mul) >> 24;
  } else {
    q = (uint32_t)((float)x * d.rinv);
    const int r = (int)x - (int)(q * d.n);
    q += (r >= (int)d.n) ? 1u : 0u;
    q -= (r < 0) ? 1u : 0u;
  }
  return q > d.lo ? q : d.lo;
}

// ---- NCHW: one lane per output
__global__ __launch_bounds__(kThreads) void avgpool_u8_nchw_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                   int64_t total, int h, int w, int oh, int ow, int kh, int kw,
                                                                   int s, DivParams d) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    const int64_t plane = t / oh;  // img * c + channel
    const uint8_t* p = in + plane * h * w + (int64_t)(y * s) * w + x * s;
    uint32_t sum = 0;
    for (int m = 0; m < kh; ++m)
      for (int l = 0; l < kw; ++l) sum += p[(int64_t)m * w + l];
    out[e] = (uint8_t)div_round(sum, d);
  }
}

__global__ __launch_bounds__(kThreads) void avgpool_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total,
                                                               int h, int w, int oh, int ow, int kh, int kw, int s, float nf) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    const int64_t plane = t / oh;
    const float* p = in + plane * h * w + (int64_t)(y * s) * w + x * s;
    float sum = 0.0f;
    for (int m = 0; m < kh; ++m)
      for (int l = 0; l < kw; ++l) sum += p[(int64_t)m * w + l];
    out[e] = sum / nf;
  }
}

// ---- bordered NHWC buffers [n][h + 2b][w + 2b][c]
struct PoolGeom {
  // in bytes; 32-bit in the windowed kernel (its launcher checks the buffer sizes), added to 64-bit bases in the reduce kernel
  uint32_t in_img, in_row, in_org;     // per image, per physical row, offset of interior pixel (0, 0)
  uint32_t out_img, out_row, out_org;
  uint32_t c, oh, ow, kh, kw, s;
  uint32_t xin, xout;                  // 0x80808080 where that buffer holds re-biased bytes, else 0
};

// two packed 16-bit sums per dword: bytes 0 and 2 of x go to `even`, bytes 1 and 3 to `odd`
__device__ __forceinline__ void acc4(uint32_t x, uint32_t& even, uint32_t& odd) {
  even += x & 0x00FF00FFu;
  odd += (x >> 8) & 0x00FF00FFu;
}
__device__ __forceinline__ uint32_t fin4(uint32_t even, uint32_t odd, const DivParams& d) {
  return div_round(even & 0xFFFFu, d) | (div_round(odd & 0xFFFFu, d) << 8) | (div_round(even >> 16, d) << 16) |
         (div_round(odd >> 16, d) << 24);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void avgpool_u8_nhwc_win_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                       uint32_t items, PoolGeom g, DivParams d) {
  const uint32_t per_pix = g.c / VEC;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint32_t v = blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const uint32_t pix = v / per_pix, ci = v - pix * per_pix;
    const uint32_t row = pix / g.ow, ox = pix - row * g.ow;
    const uint32_t img = row / g.oh, oy = row - img * g.oh;
    const uint8_t* p = in + (img * g.in_img + g.in_org + oy * g.s * g.in_row + (ox * g.s) * g.c + ci * VEC);
    uint8_t* po = out + (img * g.out_img + g.out_org + oy * g.out_row + ox * g.c + ci * VEC);
    if (VEC == 16) {
      uint32_t e0 = 0, o0 = 0, e1 = 0, o1 = 0, e2 = 0, o2 = 0, e3 = 0, o3 = 0;
      for (uint32_t m = 0; m < g.kh; ++m) {
        const uint8_t* pr = p + m * g.in_row;
        for (uint32_t l = 0; l < g.kw; ++l) {
          const uint4 x = *reinterpret_cast<const uint4*>(pr + l * g.c);
          acc4(x.x ^ g.xin, e0, o0);
          acc4(x.y ^ g.xin, e1, o1);
          acc4(x.z ^ g.xin, e2, o2);
          acc4(x.w ^ g.xin, e3, o3);
        }
      }
      uint4 r;
      r.x = fin4(e0, o0, d) ^ g.xout;
      r.y = fin4(e1, o1, d) ^ g.xout;
      r.z = fin4(e2, o2, d) ^ g.xout;
      r.w = fin4(e3, o3, d) ^ g.xout;
      *reinterpret_cast<uint4*>(po) = r;
    } else if (VEC == 4) {
      uint32_t e0 = 0, o0 = 0;
      for (uint32_t m = 0; m < g.kh; ++m) {
        const uint8_t* pr = p + m * g.in_row;
        for (uint32_t l = 0; l < g.kw; ++l) acc4(*reinterpret_cast<const uint32_t*>(pr + l * g.c) ^ g.xin, e0, o0);
      }
      *reinterpret_cast<uint32_t*>(po) = fin4(e0, o0, d) ^ g.xout;
    } else {
      uint32_t sum = 0;
      for (uint32_t m = 0; m < g.kh; ++m) {
        const uint8_t* pr = p + m * g.in_row;
        for (uint32_t l = 0; l < g.kw; ++l) sum += (uint32_t)(pr[l * g.c] ^ (uint8_t)g.xin);
      }
      *po = (uint8_t)(div_round(sum, d) ^ (g.xout & 0xFFu));
    }
  }
}

// reduce regime: block = one output pixel x CI channel items; lane = (slice, item), slice-major so that the CI lanes of
// one slice read CI * VEC contiguous bytes.  blockIdx.x = pixel * chunks + chunk.
template <int VEC>
__global__ __launch_bounds__(kThreads) void avgpool_u8_nhwc_red_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                       PoolGeom g, DivParams d, uint32_t ci_per_block, uint32_t chunks,
                                                                       uint32_t window) {
  __shared__ uint32_t part[VEC * kThreads];  // [byte of the item][lane]
  const uint32_t tid = threadIdx.x;
  const uint32_t slices = kThreads / ci_per_block;
  const uint32_t slice = tid / ci_per_block, item = tid - slice * ci_per_block;
  const uint32_t pix = blockIdx.x / chunks, chunk = blockIdx.x - pix * chunks;
  const uint32_t ci = chunk * ci_per_block + item;
  const bool live = ci * VEC < g.c;
  const uint32_t row = pix / g.ow, ox = pix - row * g.ow;
  const uint32_t img = row / g.oh, oy = row - img * g.oh;
  const uint8_t* p = in + ((int64_t)img * g.in_img + g.in_org + (int64_t)(oy * g.s) * g.in_row + (int64_t)(ox * g.s) * g.c + ci * VEC);
  uint32_t sum[VEC];
#pragma unroll
  for (int b = 0; b < VEC; ++b) sum[b] = 0;
  if (live) {
    uint32_t ky = slice / g.kw, kx = slice - ky * g.kw;
    for (uint32_t q = slice; q < window; q += slices) {
      const uint8_t* px = p + (int64_t)ky * g.in_row + (int64_t)kx * g.c;
      if (VEC == 16) {
        const uint4 x = *reinterpret_cast<const uint4*>(px);
        const uint32_t w4[4] = {x.x ^ g.xin, x.y ^ g.xin, x.z ^ g.xin, x.w ^ g.xin};
#pragma unroll
        for (int b = 0; b < 16; ++b) sum[b] += (w4[b >> 2] >> (8 * (b & 3))) & 0xFFu;
      } else if (VEC == 4) {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(px) ^ g.xin;
#pragma unroll
        for (int b = 0; b < 4; ++b) sum[b] += (x >> (8 * b)) & 0xFFu;
      } else {
        sum[0] += (uint32_t)(*px ^ (uint8_t)g.xin);
      }
      kx += slices;
      while (kx >= g.kw) {
        kx -= g.kw;
        ++ky;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < VEC; ++b) part[b * kThreads + tid] = sum[b];
  __syncthreads();
  for (uint32_t hs = slices >> 1; hs > 0; hs >>= 1) {
    if (slice < hs) {
#pragma unroll
      for (int b = 0; b < VEC; ++b) part[b * kThreads + tid] += part[b * kThreads + tid + hs * ci_per_block];
    }
    __syncthreads();
  }
  if (slice == 0 && live) {
    uint8_t* po = out + ((int64_t)img * g.out_img + g.out_org + (int64_t)oy * g.out_row + (int64_t)ox * g.c + ci * VEC);
    if (VEC == 16) {
      uint32_t r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) r[j] |= div_round(part[(4 * j + b) * kThreads + tid], d) << (8 * b);
        r[j] ^= g.xout;
      }
      *reinterpret_cast<uint4*>(po) = make_uint4(r[0], r[1], r[2], r[3]);
    } else if (VEC == 4) {
      uint32_t r = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) r |= div_round(part[b * kThreads + tid], d) << (8 * b);
      *reinterpret_cast<uint32_t*>(po) = r ^ g.xout;
    } else {
      *po = (uint8_t)(div_round(part[tid], d) ^ (g.xout & 0xFFu));
    }
  }
}

template <int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, const PoolGeom& g, const DivParams& d, int n, bool reduce) {
  const int64_t per_pix = g.c / VEC, pixels = (int64_t)n * g.oh * g.ow;
  if (reduce) {
    const uint32_t window = g.kh * g.kw;
    uint32_t slices = 1;
    while (slices < 32 && slices < window) slices <<= 1;
    const uint32_t ci_per_block = kThreads / slices;
    const uint32_t chunks = (uint32_t)((per_pix + ci_per_block - 1) / ci_per_block);
    avgpool_u8_nhwc_red_kernel<VEC><<<(unsigned)(pixels * chunks), kThreads, 0, ctx->stream>>>(in, out, g, d, ci_per_block, chunks, window);
  } else {
    const int64_t items = pixels * per_pix;
    avgpool_u8_nhwc_win_kernel<VEC><<<grid_for(items), kThreads, 0, ctx->stream>>>(in, out, (uint32_t)items, g, d);
  }
}

bool pool_args_ok(int n, int c, int h, int w, int kh, int kw, int s) {
  return n > 0 && c > 0 && h > 0 && w > 0 && kh > 0 && kw > 0 && s > 0;
}

}  // namespace

extern "C" {

int i8ie_avgpool2d_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int kernel_h, int kernel_w,
                      int stride) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(pool_args_ok(n, c, h, w, kernel_h, kernel_w, stride), "bad dimension");
  I8IE_REQUIRE(kernel_h <= h && kernel_w <= w, "window larger than input");
  I8IE_REQUIRE((int64_t)kernel_h * kernel_w <= kMaxWindow, "window of more than 65536 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int oh = (h - kernel_h) / stride + 1, ow = (w - kernel_w) / stride + 1;
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "avgpool_u8_nchw", 0.0, (double)n * c * h * w + (double)total);
  avgpool_u8_nchw_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, oh, ow, kernel_h, kernel_w, stride,
                                                                       make_div(kernel_h * kernel_w, 0, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_avgpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8,
                           int n, int c, int h, int w, int kernel_h, int kernel_w, int stride, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(pool_args_ok(n, c, h, w, kernel_h, kernel_w, stride) && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(kernel_h <= h && kernel_w <= w, "window larger than input");
  I8IE_REQUIRE((int64_t)kernel_h * kernel_w <= kMaxWindow, "window of more than 65536 elements");
  const int oh = (h - kernel_h) / stride + 1, ow = (w - kernel_w) / stride + 1;
  const int64_t in_row = (int64_t)(w + 2 * in_border) * c, in_img = (int64_t)(h + 2 * in_border) * in_row;
  const int64_t out_row = (int64_t)(ow + 2 * out_border) * c, out_img = (int64_t)(oh + 2 * out_border) * out_row;
  I8IE_REQUIRE(in_img <= 0x7FFFFFFF && out_img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const int window = kernel_h * kernel_w;
  const int vec = (c % 16 == 0 && aligned_to(in, 16) && aligned_to(out, 16)) ? 16 : ((c % 4 == 0 && aligned_to(in, 4) && aligned_to(out, 4)) ? 4 : 1);
  const int64_t pixels = (int64_t)n * oh * ow, items = pixels * (c / vec);
  // the regime rule (header): the windowed kernel indexes whole buffers in 32 bits, so buffers beyond that are split too
  const bool fits32 = in_img * n <= 0xFFFFFFFFll && out_img * n <= 0xFFFFFFFFll && items <= 0x7FFFFFFF;
  const bool reduce = window > kPackedMax || !fits32 || (window >= kReduceMinWindow && items < kReduceMaxItems);
  if (reduce) {
    uint32_t slices = 1;
    while (slices < 32 && slices < (uint32_t)window) slices <<= 1;
    const int64_t ci_per_block = kThreads / slices, chunks = (c / vec + ci_per_block - 1) / ci_per_block;
    I8IE_REQUIRE(pixels * chunks <= 0x7FFFFFFF, "too many outputs for one launch");
  }
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  PoolGeom g;
  g.in_img = (uint32_t)in_img; g.in_row = (uint32_t)in_row; g.in_org = (uint32_t)(in_border * in_row + (int64_t)in_border * c);
  g.out_img = (uint32_t)out_img; g.out_row = (uint32_t)out_row; g.out_org = (uint32_t)(out_border * out_row + (int64_t)out_border * c);
  g.c = (uint32_t)c; g.oh = (uint32_t)oh; g.ow = (uint32_t)ow; g.kh = (uint32_t)kernel_h; g.kw = (uint32_t)kernel_w; g.s = (uint32_t)stride;
  g.xin = in_s8 ? 0x80808080u : 0u;
  g.xout = out_s8 ? 0x80808080u : 0u;
  const DivParams d = make_div(window, relu, zero_point);
  I8ieProfScope prof(ctx, reduce ? "avgpool_u8_nhwc_reduce" : "avgpool_u8_nhwc", 0.0, (double)n * c * h * w + (double)pixels * c);
  if (vec == 16) launch_nhwc<16>(ctx, in, out, g, d, n, reduce);
  else if (vec == 4) launch_nhwc<4>(ctx, in, out, g, d, n, reduce);
  else launch_nhwc<1>(ctx, in, out, g, d, n, reduce);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_avgpool2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int kernel_h, int kernel_w, int stride) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(pool_args_ok(n, c, h, w, kernel_h, kernel_w, stride), "bad dimension");
  I8IE_REQUIRE(kernel_h <= h && kernel_w <= w, "window larger than input");
  I8IE_REQUIRE((int64_t)kernel_h * kernel_w <= kMaxWindow, "window of more than 65536 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int oh = (h - kernel_h) / stride + 1, ow = (w - kernel_w) / stride + 1;
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "avgpool_f32", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  avgpool_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, oh, ow, kernel_h, kernel_w, stride,
                                                                   (float)(kernel_h * kernel_w));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
