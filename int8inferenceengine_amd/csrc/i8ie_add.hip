// i8ie_add.hip -- the quantized residual Add: i8ie_add_u8, i8ie_add_u8_nhwc, i8ie_add_f32.
//
// The reference has no add.  It is defined as a composition of the reference's own expressions, dequantize
// (src/quantize_utils.cc:38-42) of both operands and down_scale's clamp and truncation (src/quantize_utils.cc:27-36),
// IEEE fp32, one rounding per operation, no contraction:
//     fa = (float)((int)a - (int)zp_a) * s_a;   fb = (float)((int)b - (int)zp_b) * s_b
//     t  = (fa + fb) / s_out + (float)zp_out
//     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t);   q = relu ? max(q, zp_out) : q        (relu<u8>, src/functional.cc:15-26)
//
// Evaluation, bit-identical to that sequence for every byte pair (tests/test_gpu_add.py runs all 65 536 of them):
//   exact    the sequence itself ((float)a - (float)zp_a is the exact integer difference).
//   guarded  S = fa + fb as above (the same two products and one sum), then e = fma(S, r, zp_out - 0.5) with
//            r = fl(1 / s_out) from the host, packed with v_cvt_pk_u8_f32 (round to nearest even, saturate).  A dword holding
//            a value closer than 2^-13 to a rounding boundary replays the exact sequence: the rule of i8ie_requant.h.
//            Bound: while |S / s_out| < 257 (which covers every t in (-1, 256), zp_out being in [0, 255]) the reference rounds
//            twice (the quotient, the sum: each <= 2^-16) and the estimate twice (r: 257 * 2^-24 < 2^-16, the fma: <= 2^-16),
//            so |t - (e + 0.5)| < 6.2e-5 < 2^-13.  Beyond that range both sides saturate: both are monotone in S.
//            Taken only for ordinary scales (i8ie_requant.h's rule): zero, denormal or huge scales run the exact sequence.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

struct AddParams {
  float sa, zpa, sb, zpb, sc, zpc;
  float rc, zph, lof;    // estimate: fl(1 / s_out), zp_out - 0.5, its lower clamp (relu: zp_out; else -1 = none, the pack saturates at 0)
  int lo;                // relu ? zp_out : 0
  int fast;              // the estimate may be used (ordinary scales)
  uint32_t xa, xb, xo;   // 0x80808080 where that buffer holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
};

__device__ __forceinline__ uint32_t add_exact1(uint32_t a, uint32_t b, const AddParams& p) {
  const float fa = ((float)a - p.zpa) * p.sa;
  const float fb = ((float)b - p.zpb) * p.sb;
  const float t = (fa + fb) / p.sc + p.zpc;
  const int u = (t >= 255.0f) ? 255 : ((t < 0.0f) ? 0 : (int)t);
  return (uint32_t)(u > p.lo ? u : p.lo);
}

// four elements: a4 / b4 / the result as they lie in memory (re-biased or not)
__device__ __forceinline__ uint32_t add4(uint32_t a4, uint32_t b4, const AddParams& p) {
  a4 ^= p.xa;
  b4 ^= p.xb;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = ((float)((a4 >> (8 * r)) & 0xFFu) - p.zpa) * p.sa;
      const float fb = ((float)((b4 >> (8 * r)) & 0xFFu) - p.zpb) * p.sb;
      const float e = __builtin_fmaf(fa + fb, p.rc, p.zph);
      packed = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaxf(e, p.lof), r, packed);
      worst = __builtin_fminf(worst, __builtin_fabsf(__builtin_amdgcn_fractf(e) - 0.5f));
    }
    if (worst >= 1.220703125e-4f) return packed ^ p.xo;  // 2^-13 > 6.2e-5, the proven bound
  }
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= add_exact1((a4 >> (8 * r)) & 0xFFu, (b4 >> (8 * r)) & 0xFFu, p) << (8 * r);
  return packed ^ p.xo;
}
__device__ __forceinline__ uint8_t add1(uint8_t a, uint8_t b, const AddParams& p) {
  return (uint8_t)(add_exact1((a ^ p.xa) & 0xFFu, (b ^ p.xb) & 0xFFu, p) ^ (p.xo & 0xFFu));
}
__device__ __forceinline__ uint4 add16(uint4 x, const uint4& y, const AddParams& p) {
  x.x = add4(x.x, y.x, p);
  x.y = add4(x.y, y.y, p);
  x.z = add4(x.z, y.z, p);
  x.w = add4(x.w, y.w, p);
  return x;
}

// ---- flat form: one physical order, no border.  out may alias a or b: a lane reads its 16 bytes before it stores them.
__global__ __launch_bounds__(kThreads) void add_u8_flat_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n,
                                                               AddParams p) {
  const int64_t nvec = n >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    const uint4 x = reinterpret_cast<const uint4*>(a)[v];
    const uint4 y = reinterpret_cast<const uint4*>(b)[v];
    reinterpret_cast<uint4*>(out)[v] = add16(x, y, p);
  }
  const int64_t t0 = nvec << 4;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = add1(a[t0 + threadIdx.x], b[t0 + threadIdx.x], p);
}

// ---- bordered NHWC form: [n][h + 2b][w + 2b][c] per buffer, each with its own b.  The w * c interior bytes of an image row
// are the contiguous unit; an item is VEC bytes of one row (VEC = 16 / 4 / 1 by c's divisibility: every row start is then
// VEC-aligned in all three buffers).  Only the interior of `out` is written.
template <int VEC, typename Idx>
__global__ __launch_bounds__(kThreads) void add_u8_nhwc_kernel(const uint8_t* __restrict__ a, NhwcGeom ga, const uint8_t* __restrict__ b,
                                                               NhwcGeom gb, uint8_t* __restrict__ out, NhwcGeom go, Idx items, Idx per_row,
                                                               Idx h, AddParams p) {
  const Idx stride = (Idx)gridDim.x * kThreads;
  for (Idx v = (Idx)blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const Idx r = v / per_row;
    const int64_t col = (int64_t)(v - r * per_row) * VEC;
    const Idx img = r / h;
    const int64_t y = (int64_t)(r - img * h);
    const uint8_t* pa = a + (int64_t)img * ga.img + ga.org + y * ga.row + col;
    const uint8_t* pb = b + (int64_t)img * gb.img + gb.org + y * gb.row + col;
    uint8_t* po = out + (int64_t)img * go.img + go.org + y * go.row + col;
    if (VEC == 16)
      *reinterpret_cast<uint4*>(po) = add16(*reinterpret_cast<const uint4*>(pa), *reinterpret_cast<const uint4*>(pb), p);
    else if (VEC == 4)
      *reinterpret_cast<uint32_t*>(po) = add4(*reinterpret_cast<const uint32_t*>(pa), *reinterpret_cast<const uint32_t*>(pb), p);
    else
      *po = add1(*pa, *pb, p);
  }
}

__global__ __launch_bounds__(kThreads) void add_f32_kernel(const float* a, const float* b, float* out, int64_t n) {
  const int64_t nvec = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    float4 x = reinterpret_cast<const float4*>(a)[v];
    const float4 y = reinterpret_cast<const float4*>(b)[v];
    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
    reinterpret_cast<float4*>(out)[v] = x;
  }
  const int64_t t0 = nvec << 2;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = a[t0 + threadIdx.x] + b[t0 + threadIdx.x];
}

AddParams make_params(float s_a, int zp_a, float s_b, int zp_b, float s_out, int zp_out, int relu, int a_s8, int b_s8, int out_s8) {
  AddParams p;
  p.sa = s_a; p.zpa = (float)zp_a; p.sb = s_b; p.zpb = (float)zp_b; p.sc = s_out; p.zpc = (float)zp_out;
  p.rc = 1.0f / s_out;
  p.zph = (float)zp_out - 0.5f;
  p.lof = relu ? (float)zp_out : -1.0f;
  p.lo = relu ? zp_out : 0;
  // the estimate only where nothing can overflow or go denormal on the way: ordinary scales and an ordinary largest |S / s_out|
  const double top = 255.0 * ((double)s_a + (double)s_b) / (double)s_out;
  p.fast = (ordinary(s_a) && ordinary(s_b) && ordinary(s_out) && top < 1e30) ? 1 : 0;
  p.xa = a_s8 ? 0x80808080u : 0u;
  p.xb = b_s8 ? 0x80808080u : 0u;
  p.xo = out_s8 ? 0x80808080u : 0u;
  return p;
}

template <int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* a, const NhwcGeom& ga, const uint8_t* b, const NhwcGeom& gb, uint8_t* out,
                 const NhwcGeom& go, int n, int c, int h, int w, const AddParams& p) {
  const int64_t per_row = (int64_t)w * c / VEC, items = (int64_t)n * h * per_row;
  if (items <= 0x7FFFFFFF)
    add_u8_nhwc_kernel<VEC, uint32_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, (uint32_t)items,
                                                                                     (uint32_t)per_row, (uint32_t)h, p);
  else
    add_u8_nhwc_kernel<VEC, int64_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, items, per_row,
                                                                                    (int64_t)h, p);
}

}  // namespace

extern "C" {

int i8ie_add_u8(i8ie_ctx* ctx, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, float s_a, uint8_t zp_a, float s_b,
                uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "add_u8", 0.0, 3.0 * n);
  add_u8_flat_kernel<<<grid_for((n >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n,
                                                                         make_params(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, 0, 0, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_add_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8,
                     uint8_t* out, int out_border, int out_s8, int n, int c, int h, int w, float s_a, uint8_t zp_a, float s_b,
                     uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && a_border >= 0 && b_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const AddParams p = make_params(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, a_s8, b_s8, out_s8);
  const int64_t total = (int64_t)n * c * h * w;
  I8ieProfScope prof(ctx, "add_u8_nhwc", 0.0, 3.0 * total);
  const bool al16 = aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16);
  const bool al4 = aligned_to(a, 4) && aligned_to(b, 4) && aligned_to(out, 4);
  if (a_border == 0 && b_border == 0 && out_border == 0 && al16) {  // one physical order, no border: the flat form
    add_u8_flat_kernel<<<grid_for((total >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, total, p);
  } else {
    const NhwcGeom ga = buf_geom(c, h, w, a_border), gb = buf_geom(c, h, w, b_border), go = buf_geom(c, h, w, out_border);
    if (c % 16 == 0 && al16) launch_nhwc<16>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else if (c % 4 == 0 && al4) launch_nhwc<4>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else launch_nhwc<1>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_add_f32(i8ie_ctx* ctx, const float* a, const float* b, float* out, int64_t n) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "add_f32", 0.0, 12.0 * n);
  add_f32_kernel<<<grid_for((n >> 2) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
