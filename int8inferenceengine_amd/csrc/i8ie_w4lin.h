// i8ie_w4lin.h -- the 4-bit weight panel of i8ie_w4lin.hip and that file's launchers, as i8ie_layer.hip and
// i8ie_layer_create.hip see them.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"

// The panel: [feature tiles of 16, an even number][chunks of 256 K values][2 pairs] fragments of 1 KiB (the order is derived at
// the top of i8ie_w4lin.hip); zero nibbles past n and past K.
inline int i8ie_w4_chunks(int K) { return (K + 255) / 256; }
inline int i8ie_w4_ftiles(int n) { return ((n + 15) / 16 + 1) / 2 * 2; }
size_t i8ie_w4_panel_bytes(int n, int K);

// where weight (j, k) lies: the byte, and *hi = 1 for its high nibble
__host__ __device__ inline size_t i8ie_w4_at(int j, int k, int nch, int* hi) {
  const int ft = j >> 4, r = j & 15, ch = k >> 8, slot = (k & 255) >> 4, i = k & 15;
  const int pr = slot >> 3, q = slot & 3;
  *hi = (slot >> 2) & 1;
  return ((((size_t)ft * nch + ch) * 2 + pr) * 64 + q * 16 + r) * 16 + i;
}
// ... and its value, sign extended
__host__ __device__ inline int i8ie_w4_get(const uint8_t* panel, int j, int k, int nch) {
  int hi;
  const unsigned b = panel[i8ie_w4_at(j, k, nch, &hi)];
  return (int)(((b >> (4 * hi)) & 15u) ^ 8u) - 8;
}

// host: the C-ABI's packed rows (element 2 i in the low nibble of byte i) into a zeroed panel
void i8ie_w4_pack_panel(const uint8_t* packed, int n, int K, uint8_t* panel);

struct I8ieW4Call {
  const uint8_t* A;  // [M][K] u8
  int M, N, K;
  const uint8_t* B;  // the panel; for the MFMA kernel in the K order of A's rows
  int hw;            // w4lin_direct: rows are a flattened NHWC activation of hw pixels (1: reference order); B is in reference order
  I8ieEpilogue ep;   // per-feature (msv, sbv, biasf set); ocp: oc + 128 * wsum for the MFMA kernel, the plain oc for w4lin_direct
  uint8_t* out;
};
bool i8ie_w4lin_mfma_takes(const I8ieW4Call& c);  // K % 32 == 0 and 16-byte aligned operands
int i8ie_w4lin_mfma_launch(i8ie_ctx* ctx, const I8ieW4Call& c);
int i8ie_w4lin_direct_launch(i8ie_ctx* ctx, const I8ieW4Call& c);

// one-off kernels of a handle: oc / wsum / oc' / the float bias for (s_in, zp_in) in the reference's accumulation order, and the
// panel re-packed for rows in (h, w, c) order.  conv: the bias goes into oc as src/conv2d.cc:123 folds it, and biasf stays zero.
// cpad > 0: the panel of a k x k conv in the K order of i8ie_w4conv.h (taps = k * k, cpad channels per tap), walked in the
// reference's order (c, ky, kx) -- the fp32 sum is order-free only while 255 * 8 * K < 2^24
int i8ie_w4_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in, int32_t* oc,
                           int32_t* wsum, int32_t* ocp, float* biasf, bool conv = false, int taps = 1, int cpad = 0);
int i8ie_w4_launch_permute(i8ie_ctx* ctx, const uint8_t* panel, uint8_t* out, int n, int K, int c, int hw);
