// i8ie_bytemax.h -- the byte-wise unsigned maximum the NHWC max-pool kernels share (i8ie_igemm.hip's maxpool_u8_nhwc_kernel,
// i8ie_padpool.hip).  Device only; internal linkage (an unnamed namespace per including unit).
#pragma once

#include <cstdint>

namespace {

// Byte-wise unsigned max without SWAR arithmetic: a dword's even and odd bytes are spread into two pairs of
// 16-bit lanes (v_perm_b32, zero fill), the running maxima live in that form (v_pk_max_u16: two bytes per
// instruction) and are packed back once per output (one more v_perm_b32).  The SWAR form (bmax4 of i8ie_igemm.hip) cost
// ~10 VALU operations per input dword and made the max-pool kernel VALU-bound (rocprofv3: 43 M VALU wave-instructions
// per launch); this form needs 4.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
struct BytesEO {
  us2 e, o;
};
__device__ __forceinline__ BytesEO spread_eo(uint32_t x) {
  BytesEO r;
  r.e = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, x, 0x0c020c00u));  // [x0, 0, x2, 0]
  r.o = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, x, 0x0c030c01u));  // [x1, 0, x3, 0]
  return r;
}
__device__ __forceinline__ void max_eo(BytesEO& m, uint32_t x) {
  const BytesEO v = spread_eo(x);
  m.e = __builtin_elementwise_max(m.e, v.e);
  m.o = __builtin_elementwise_max(m.o, v.o);
}
__device__ __forceinline__ uint32_t pack_eo(const BytesEO& m) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, m.o), __builtin_bit_cast(uint32_t, m.e), 0x06020400u);
}

}  // namespace
