// i8ie_bmm_tile.h -- the operand tile of the MFMA matmul kernels that i8ie_matmul.hip (bmm_mfma) and i8ie_attention.hip
// (attn_mfma) share: an operand as "rows x k" and its 64 x 64 tile staged into LDS, re-biased, K-contiguous per row (DESIGN.md
// section 8k).  Internal linkage (an unnamed namespace per including unit), like i8ie_pointwise.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "i8ie_internal.h"

namespace {


constexpr int TM = 64, TN = 64, TK = 64;  // block tile
constexpr int LROW = TK + 16;             // LDS bytes per staged row

struct BmmOp {          // an operand as rows x k
  const uint8_t* p;
  int64_t batch, rs, ks;  // strides in bytes; rs == 1 or ks == 1
  uint32_t x;           // 0x80808080 for plain bytes (re-biased while staging), 0 for bytes stored re-biased
  int vec;              // bytes per load the strides allow along the contiguous axis: 16, 4 or 1
  int zp;               // plain zero point
};

// The byte offset of index i along the strided axis (a row of a K-contiguous operand, a k of a K-strided one).  LinearRows is
// the operand as BmmOp describes it; attn_mfma's windowed form passes a map of its own (WindowRows, i8ie_attention.hip).
struct LinearRows {
  __device__ __forceinline__ int64_t operator()(int i, int64_t stride) const { return (int64_t)i * stride; }
};

// one 64 x 64 tile of `op` (rows row0.., k k0..) into lds[64][LROW], re-biased, zero-filled outside the operand
template <class RowMap = LinearRows>
__device__ __forceinline__ void stage_tile(const BmmOp& op, const uint8_t* base, int rows, int K, int row0, int k0, uint8_t* lds,
                                           const RowMap& at = RowMap()) {
  const int t = threadIdx.x;
  const uint32_t x8 = op.x & 0xFFu;
  if (op.ks == 1) {  // K-contiguous: a lane moves 16 consecutive k of one row
    const int r = t >> 2, kc = (t & 3) * 16;
    const int gr = row0 + r, gk = k0 + kc;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (gr < rows && gk < K) {
      const uint8_t* src = base + at(gr, op.rs) + gk;
      if (gk + 16 <= K && op.vec == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        w[0] = v.x ^ op.x; w[1] = v.y ^ op.x; w[2] = v.z ^ op.x; w[3] = v.w ^ op.x;
      } else if (gk + 16 <= K && op.vec == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = *reinterpret_cast<const uint32_t*>(src + 4 * i) ^ op.x;
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (gk + i < K) w[i >> 2] |= ((uint32_t)src[i] ^ x8) << (8 * (i & 3));
      }
    }
    *reinterpret_cast<uint4*>(lds + r * LROW + kc) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {  // K-strided (rows contiguous): a lane moves 4 rows x 4 k and transposes them in registers
    const int rb = (t & 15) * 4, kb = (t >> 4) * 4;
    const int gr = row0 + rb;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gk = k0 + kb + i;
      w[i] = 0u;
      if (gk < K && gr < rows) {
        const uint8_t* src = base + at(gk, op.ks) + gr;
        if (gr + 4 <= rows && op.vec >= 4) {
          w[i] = *reinterpret_cast<const uint32_t*>(src) ^ op.x;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (gr + j < rows) w[i] |= ((uint32_t)src[j] ^ x8) << (8 * j);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t o = ((w[0] >> (8 * j)) & 0xFFu) | (((w[1] >> (8 * j)) & 0xFFu) << 8) | (((w[2] >> (8 * j)) & 0xFFu) << 16) |
                         (((w[3] >> (8 * j)) & 0xFFu) << 24);
      *reinterpret_cast<uint32_t*>(lds + (rb + j) * LROW + kb) = o;
    }
  }
}

}  // namespace
