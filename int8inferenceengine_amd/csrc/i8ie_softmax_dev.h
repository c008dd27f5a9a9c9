// i8ie_softmax_dev.h -- the device pieces of the integer softmax that i8ie_softmax.hip and i8ie_attention.hip share: the table
// as it travels in the kernel arguments, the division by a row's S and the two wave reductions.  The arithmetic is defined in
// include/i8ie_hip.h (i8ie_softmax_u8); the derivation of div_by stands at the top of i8ie_softmax.hip.  Internal linkage (an
// unnamed namespace per including unit), like i8ie_pointwise.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

struct SoftmaxTable {
  uint32_t e[256];
};

__device__ __forceinline__ uint32_t div_by(uint32_t x, uint32_t S, float rinv) {
  uint32_t q = (uint32_t)((float)x * rinv);
  const int64_t r = (int64_t)x - (int64_t)((uint64_t)q * (uint64_t)S);
  q += (r >= (int64_t)S) ? 1u : 0u;
  q -= (r < 0) ? 1u : 0u;
  return q > 255u ? 255u : q;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

}  // namespace
