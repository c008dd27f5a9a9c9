// i8ie_lut.hip -- table-driven quantized activations: i8ie_activation_table, i8ie_lut_u8,
// i8ie_lut_u8_nhwc, i8ie_activation_f32.
//
// The reference's one non-linearity is relu<u8> (src/functional.cc:15-26).  Any other activation between two quantised
// tensors is a function from one byte to one byte, so one kernel covers them all: out = table[in].  The table is built on the
// host from the reference's own dequantize (src/quantize_utils.cc:38-42) and down_scale's clamp and truncation (:27-36) around
// f (include/i8ie_hip.h has the sequence), and absorbs the change of (scale, zero_point), a following relu and the ^0x80
// re-bias of either side.  It travels by value in the kernel arguments (64 dwords): no device allocation, no copy.
//
// The lookup.  A lane holds 16 input bytes and needs 16 table bytes.  A sub-dword LDS read is served per half-wave of 32 lanes
// and conflicts on the bank (a / 4) % 32 of its byte address: a plain 256-byte table (64 dwords, two per bank) serialises on
// unequal bytes.  The table is therefore stored once PER BANK: LDS row k (128 bytes) holds table dword k in each of its 32
// dwords, and lane l only ever reads bank l % 32:
//     address(a, l) = (a >> 2) * 128 + (l % 32) * 4 + (a & 3)
// 64 rows x 128 bytes = 8 KiB per block, conflict-free for any data (the 32 lanes of a group sit on 32 different banks, whatever
// their rows).  The block fills it with 8 ds_write_b32 per thread, rotated so that the 32 lanes of a group hit 32 banks.
#include <cmath>
#include <cstring>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kKinds = 6;

struct LutTable {
  uint32_t w[64];  // table[4k .. 4k+3] in dword k, as the bytes lie in memory
};

// all kThreads threads of the block: the per-bank copies of the table, then the barrier
__device__ __forceinline__ void lut_fill(uint32_t* lds, const LutTable& t) {
  const uint32_t tid = threadIdx.x, row = tid >> 2, q = tid & 3u, rot = (tid >> 2) & 7u;
  const uint32_t v = t.w[row];
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) lds[row * 32 + q * 8 + ((j + rot) & 7u)] = v;
  __syncthreads();
}
// `mine`: the lane's own bank column, (const uint8_t*)lds + (lane % 32) * 4
__device__ __forceinline__ uint32_t lut1(const uint8_t* mine, uint32_t a) { return mine[((a & 0xFCu) << 5) | (a & 3u)]; }
__device__ __forceinline__ uint32_t lut4(const uint8_t* mine, uint32_t x) {
  return lut1(mine, x & 0xFFu) | (lut1(mine, (x >> 8) & 0xFFu) << 8) | (lut1(mine, (x >> 16) & 0xFFu) << 16) | (lut1(mine, x >> 24) << 24);
}
template <int VEC>
__device__ __forceinline__ void lut_item(const uint8_t* mine, const uint8_t* src, uint8_t* dst) {
  if (VEC == 16) {
    uint4 x = *reinterpret_cast<const uint4*>(src);
    x.x = lut4(mine, x.x);
    x.y = lut4(mine, x.y);
    x.z = lut4(mine, x.z);
    x.w = lut4(mine, x.w);
    *reinterpret_cast<uint4*>(dst) = x;
  } else if (VEC == 4) {
    *reinterpret_cast<uint32_t*>(dst) = lut4(mine, *reinterpret_cast<const uint32_t*>(src));
  } else {
    *dst = (uint8_t)lut1(mine, *src);
  }
}

// ---- flat form: one physical order.  out may be in itself: a lane reads its item before it stores it.
template <int VEC>
__global__ __launch_bounds__(kThreads) void lut_u8_flat_kernel(const uint8_t* in, uint8_t* out, int64_t n, const LutTable t) {
  __shared__ uint32_t lds[64 * 32];
  lut_fill(lds, t);
  const uint8_t* mine = reinterpret_cast<const uint8_t*>(lds) + (threadIdx.x & 31u) * 4;
  const int64_t items = n / VEC;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) lut_item<VEC>(mine, in + v * VEC, out + v * VEC);
  const int64_t t0 = items * VEC;  // tail: fewer than VEC bytes
  if (VEC > 1 && blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = (uint8_t)lut1(mine, in[t0 + threadIdx.x]);
}

// ---- bordered NHWC form: [n][h + 2b][w + 2b][c] per buffer, each with its own b, walked by row items (i8ie_pointwise.h)
template <int VEC, typename Idx>
__global__ __launch_bounds__(kThreads) void lut_u8_nhwc_kernel(const uint8_t* __restrict__ in, NhwcGeom gi, uint8_t* __restrict__ out, NhwcGeom go,
                                                               Idx items, Idx per_row, Idx h, const LutTable t) {
  __shared__ uint32_t lds[64 * 32];
  lut_fill(lds, t);
  const uint8_t* mine = reinterpret_cast<const uint8_t*>(lds) + (threadIdx.x & 31u) * 4;
  const Idx stride = (Idx)gridDim.x * kThreads;
  for (Idx v = (Idx)blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const RowItem<Idx> it = row_item<VEC>(v, per_row, h);
    lut_item<VEC>(mine, in + nhwc_at(gi, it), out + nhwc_at(go, it));
  }
}

// ---- f(x), fp32 (include/i8ie_hip.h): the same text compiled for the host (the table) and the device (the FP32 entry)
__host__ __device__ inline float act_f32(int kind, float param, float x) {
  switch (kind) {
    case I8IE_ACT_RELU6: {
      const float v = x > 0.0f ? x : 0.0f;
      return v < 6.0f ? v : 6.0f;
    }
    case I8IE_ACT_LEAKY_RELU:
      return x >= 0.0f ? x : x * param;
    case I8IE_ACT_HARDSIGMOID:
    case I8IE_ACT_HARDSWISH: {
      float v = x + 3.0f;
      v = v > 0.0f ? v : 0.0f;
      const float h = v < 6.0f ? v : 6.0f;
      return kind == I8IE_ACT_HARDSIGMOID ? h / 6.0f : (x * h) / 6.0f;
    }
    case I8IE_ACT_SIGMOID:
      return (float)(1.0 / (1.0 + exp(-(double)x)));
    default:
      return (float)tanh((double)x);
  }
}

__global__ __launch_bounds__(kThreads) void activation_f32_kernel(const float* in, float* out, int64_t n, int kind, float param) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = act_f32(kind, param, in[i]);
}

bool kind_ok(int kind, float param) {
  return kind >= 0 && kind < kKinds && (kind != I8IE_ACT_LEAKY_RELU || std::isfinite(param));
}

// the table as the kernel takes it, with the re-bias of either side folded in: t'[a ^ xi] = table[a] ^ xo
LutTable pack_table(const uint8_t* table, int in_s8, int out_s8) {
  uint8_t b[256];
  const unsigned xi = in_s8 ? 0x80u : 0u, xo = out_s8 ? 0x80u : 0u;
  for (unsigned a = 0; a < 256; ++a) b[a ^ xi] = (uint8_t)(table[a] ^ xo);
  LutTable t;
  std::memcpy(t.w, b, 256);
  return t;
}

void launch_flat(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t n, const LutTable& t) {
  const int vec = item_width({}, {in, out});  // (a ragged end goes byte by byte: n need not be a multiple)
  if (vec == 16) lut_u8_flat_kernel<16><<<grid_for((n >> 4) + 1), kThreads, 0, ctx->stream>>>(in, out, n, t);
  else if (vec == 4) lut_u8_flat_kernel<4><<<grid_for((n >> 2) + 1), kThreads, 0, ctx->stream>>>(in, out, n, t);
  else lut_u8_flat_kernel<1><<<grid_for(n), kThreads, 0, ctx->stream>>>(in, out, n, t);
}

template <int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* in, const NhwcGeom& gi, uint8_t* out, const NhwcGeom& go, int n, int c, int h, int w,
                 const LutTable& t) {
  const int64_t per_row = (int64_t)w * c / VEC, items = (int64_t)n * h * per_row;
  if (items <= 0x7FFFFFFF)
    lut_u8_nhwc_kernel<VEC, uint32_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(in, gi, out, go, (uint32_t)items, (uint32_t)per_row,
                                                                                     (uint32_t)h, t);
  else
    lut_u8_nhwc_kernel<VEC, int64_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(in, gi, out, go, items, per_row, (int64_t)h, t);
}

}  // namespace

extern "C" {

int i8ie_activation_table(int kind, float param, float s_in, uint8_t zp_in, float s_out, uint8_t zp_out, uint8_t* table) {
  I8IE_REQUIRE(table, "null argument");
  I8IE_REQUIRE(kind_ok(kind, param), "unknown activation kind, or a slope that is not finite");
  I8IE_REQUIRE(std::isfinite(s_in) && std::isfinite(s_out) && s_out > 0.0f, "scales must be finite and the output scale positive");
  const float top = 255.0f * s_in;
  I8IE_REQUIRE(std::isfinite(top), "255 * s_in overflows fp32");
  for (int a = 0; a < 256; ++a) {
    const float x = (float)(a - (int)zp_in) * s_in;
    const float t = act_f32(kind, param, x) / s_out + (float)zp_out;
    table[a] = t >= 255.0f ? (uint8_t)255 : (t < 0.0f ? (uint8_t)0 : (uint8_t)(int)t);
  }
  return I8IE_OK;
}

int i8ie_lut_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t n, const uint8_t* table) {
  I8IE_REQUIRE(ctx && in && out && table, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  if (n == 0) return I8IE_OK;
  const LutTable t = pack_table(table, 0, 0);
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "lut_u8", 0.0, 2.0 * n);
  launch_flat(ctx, in, out, n, t);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_lut_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n, int c,
                     int h, int w, const uint8_t* table) {
  I8IE_REQUIRE(ctx && in && out && table, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && in_border >= 0 && out_border >= 0, "bad dimension");
  const LutTable t = pack_table(table, in_s8, out_s8);
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * h * w;
  I8ieProfScope prof(ctx, "lut_u8_nhwc", 0.0, 2.0 * total);
  if (in_border == 0 && out_border == 0) {  // one physical order, no border: the flat form
    launch_flat(ctx, in, out, total, t);
  } else {
    const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, h, w, out_border);
    const int vec = item_width({c}, {in, out});
    if (vec == 16) launch_nhwc<16>(ctx, in, gi, out, go, n, c, h, w, t);
    else if (vec == 4) launch_nhwc<4>(ctx, in, gi, out, go, n, c, h, w, t);
    else launch_nhwc<1>(ctx, in, gi, out, go, n, c, h, w, t);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_activation_f32(i8ie_ctx* ctx, int kind, float param, const float* in, float* out, int64_t n) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(kind_ok(kind, param), "unknown activation kind, or a slope that is not finite");
  I8IE_REQUIRE(aligned_to(in, 4) && aligned_to(out, 4), "buffers must be 4-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "activation_f32", 0.0, 8.0 * n);
  activation_f32_kernel<<<grid_for(n), kThreads, 0, ctx->stream>>>(in, out, n, kind, param);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
