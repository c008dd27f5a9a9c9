// i8ie_softmax.hip -- quantized softmax over the last axis: i8ie_softmax_table, i8ie_softmax_u8,
// i8ie_softmax_f32.  The arithmetic is defined in include/i8ie_hip.h; everything between the two u8 tensors is integer:
//     mx = max_j x_j;  d_j = mx - x_j;  S = sum_j E[d_j];  q_j = min(255, (E[d_j] * 256 + S / 2) / S)
// with the host-built table E[d] = floor(65536 exp(-s d) + 0.5).  E[0] = 65536 and E <= 65536, so 65536 <= S <= 65535 * 65536
// < 2^32 and x = E * 256 + S / 2 < 2^24 + 2^31: nothing wraps in unsigned 32-bit arithmetic.
//
// The division by the row's S, without an integer-divide sequence (div_by below, the scheme of i8ie_avgpool.hip's estimate):
//     y = fl(float(x) * fl(1 / float(S))), q' = trunc(y).  float(x), float(S), the reciprocal and the product each carry a
//     relative error <= 2^-24 (the reciprocal 2^-23 with S's conversion), x / S <= 256.5, so |y - x / S| < 2^-13: q' is
//     floor(x / S) or one off.  r = x - q' S is taken exactly in 64-bit integers (q' S can pass 2^32) and q' corrected by one
//     where r < 0 or r >= S.
//
// Two forms:
//   wave   L <= 1024: one wave per row, four rows per block.  A lane keeps 16 values of the row in registers (items of 4 bytes
//          where rows start 4-byte aligned, else single bytes, interleaved over the lanes so that loads coalesce); the max and
//          the sum go through wave reductions (__shfl_xor), and the row is never read twice.
//   block  longer rows: one block per row, three walks (max, sum, quotient) of which the second and third find the row in the
//          cache; the two reductions go through LDS.
// The table arrives by value in the kernel arguments and is copied to LDS once per block.  All stores are vector stores
// (dword or byte).  `out` may alias `in`: a lane writes only the bytes it read itself, after the reductions.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_softmax_dev.h"

namespace {

constexpr int kWaveMaxL = 1024;  // 64 lanes x 16 values
constexpr int kMaxL = 65535;

// (SoftmaxTable, div_by, wave_max and wave_sum live in i8ie_softmax_dev.h: the fused attention kernel uses them too)

// VEC = 4: item i of lane l is bytes 4 (l + 64 i) .. + 3 of the row, i < 4 (rows start 4-byte aligned: L % 4 == 0 and aligned
// buffers).  VEC = 1: item i is byte l + 64 i, i < 16.
template <int VEC>
__global__ __launch_bounds__(kThreads) void softmax_u8_wave_kernel(const uint8_t* in, uint8_t* out, int64_t rows, int L,
                                                                  SoftmaxTable tab) {
  __shared__ uint32_t E[256];
  E[threadIdx.x] = tab.e[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint8_t* src = in + row * L;
  uint8_t* dst = out + row * L;
  constexpr int ITEMS = 16 / VEC;
  uint32_t v[16];
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int j = VEC * (lane + 64 * i);
    if (VEC == 4) {
      uint32_t w = 0;
      if (j < L) w = *reinterpret_cast<const uint32_t*>(src + j);
#pragma unroll
      for (int b = 0; b < 4; ++b) v[4 * i + b] = (w >> (8 * b)) & 0xFFu;
    } else {
      v[i] = j < L ? (uint32_t)src[j] : 0u;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) mx = v[i] > mx ? v[i] : mx;   // (values past the row's end are 0: they never raise the max)
  mx = wave_max(mx);
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = VEC == 4 ? 4 * (lane + 64 * (i >> 2)) + (i & 3) : lane + 64 * i;
    v[i] = E[mx - v[i]];
    sum += j < L ? v[i] : 0u;
  }
  const uint32_t S = wave_sum(sum);
  const float rinv = 1.0f / (float)S;
  const uint32_t half = S >> 1;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int j = VEC * (lane + 64 * i);
    if (j >= L) continue;
    if (VEC == 4) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) w |= div_by(v[4 * i + b] * 256u + half, S, rinv) << (8 * b);
      *reinterpret_cast<uint32_t*>(dst + j) = w;
    } else {
      dst[j] = (uint8_t)div_by(v[i] * 256u + half, S, rinv);
    }
  }
}

__global__ __launch_bounds__(kThreads) void softmax_u8_block_kernel(const uint8_t* in, uint8_t* out, int L, SoftmaxTable tab) {
  __shared__ uint32_t E[256];
  __shared__ uint32_t red[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  E[tid] = tab.e[tid];
  const uint8_t* src = in + (int64_t)blockIdx.x * L;
  uint8_t* dst = out + (int64_t)blockIdx.x * L;
  uint32_t mx = 0;
  for (int j = tid; j < L; j += kThreads) {
    const uint32_t x = src[j];
    mx = x > mx ? x : mx;
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();  // (also: E is complete)
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) mx = red[w] > mx ? red[w] : mx;
  __syncthreads();
  uint32_t sum = 0;
  for (int j = tid; j < L; j += kThreads) sum += E[mx - (uint32_t)src[j]];
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  uint32_t S = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) S += red[w];
  const float rinv = 1.0f / (float)S;
  const uint32_t half = S >> 1;
  for (int j = tid; j < L; j += kThreads) dst[j] = (uint8_t)div_by(E[mx - (uint32_t)src[j]] * 256u + half, S, rinv);
}

// FP32, off the timed path: one lane per row, plain loops in ascending j
__global__ __launch_bounds__(kThreads) void softmax_f32_kernel(const float* in, float* out, int64_t rows, int L) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += stride) {
    const float* src = in + r * L;
    float* dst = out + r * L;
    float mx = src[0];
    for (int j = 1; j < L; ++j) mx = src[j] > mx ? src[j] : mx;
    float sum = 0.0f;
    for (int j = 0; j < L; ++j) sum += expf(src[j] - mx);
    for (int j = 0; j < L; ++j) dst[j] = expf(src[j] - mx) / sum;
  }
}

}  // namespace

extern "C" {

int i8ie_softmax_table(float s_in, uint32_t table_host[256]) {
  I8IE_REQUIRE(table_host != nullptr, "null argument");
  I8IE_REQUIRE(std::isfinite(s_in) && s_in >= 0.0f, "the input scale must be finite and not negative");
  for (int d = 0; d < 256; ++d) table_host[d] = (uint32_t)std::floor(65536.0 * std::exp(-(double)s_in * (double)d) + 0.5);
  return I8IE_OK;
}

int i8ie_softmax_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t rows, int L, float s_in) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(rows > 0 && L >= 1 && L <= kMaxL, "bad dimension (1 <= L <= 65535)");
  I8IE_REQUIRE(rows <= 0x7FFFFFFF, "too many rows for one launch");
  SoftmaxTable tab;
  I8IE_TRY(i8ie_softmax_table(s_in, tab.e));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const bool wave = L <= kWaveMaxL;
  I8ieProfScope prof(ctx, wave ? "softmax_u8_wave" : "softmax_u8_block", 0.0, 2.0 * (double)rows * L);
  if (wave) {
    const unsigned grid = (unsigned)((rows + kThreads / 64 - 1) / (kThreads / 64));
    if (L % 4 == 0 && aligned_to(in, 4) && aligned_to(out, 4))
      softmax_u8_wave_kernel<4><<<grid, kThreads, 0, ctx->stream>>>(in, out, rows, L, tab);
    else
      softmax_u8_wave_kernel<1><<<grid, kThreads, 0, ctx->stream>>>(in, out, rows, L, tab);
  } else {
    softmax_u8_block_kernel<<<(unsigned)rows, kThreads, 0, ctx->stream>>>(in, out, L, tab);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_softmax_f32(i8ie_ctx* ctx, const float* in, float* out, int64_t rows, int L) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(rows > 0 && L >= 1 && L <= kMaxL, "bad dimension (1 <= L <= 65535)");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "softmax_f32", 0.0, 8.0 * (double)rows * L);
  softmax_f32_kernel<<<grid_for(rows), kThreads, 0, ctx->stream>>>(in, out, rows, L);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
