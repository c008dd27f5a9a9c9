// i8ie_sp24lin.h -- the 2:4 structured-sparse weight panel of i8ie_sp24lin.hip and that file's launchers, as i8ie_layer.hip and
// i8ie_layer_create.hip see them.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"

// The panel: [feature tiles of 16][chunks of 512 dense K][4 value fragments, 1 position fragment] of 1 KiB each (the order is
// derived at the top of i8ie_sp24lin.hip); zero past n and past K.  The tiles are padded to whole blocks of the widest kernel
// instance (128 features), so no block reads past the panel.
inline int i8ie_sp24_chunks(int K) { return (K + 511) / 512; }
inline int i8ie_sp24_ftiles(int n) { return (n + 127) / 128 * 8; }
inline size_t i8ie_sp24_panel_bytes(int n, int K) { return (size_t)i8ie_sp24_ftiles(n) * i8ie_sp24_chunks(K) * 5120; }

// where kept value e (0 or 1) of group g (dense k = 4 g .. 4 g + 3) of feature j lies ...
__host__ __device__ inline size_t i8ie_sp24_value_at(int j, int g, int e, int nch) {
  const int ft = j >> 4, r = j & 15, ch = g >> 7, v = (g >> 5) & 3, q = (g >> 3) & 3, gi = g & 7;
  return (((size_t)ft * nch + ch) * 5 + v) * 1024 + (q * 16 + r) * 16 + 2 * gi + e;
}
// ... and the byte whose nibble (g & 1) holds the group's two positions
__host__ __device__ inline size_t i8ie_sp24_index_at(int j, int g, int nch) {
  const int ft = j >> 4, r = j & 15, ch = g >> 7, v = (g >> 5) & 3, q = (g >> 3) & 3, gi = g & 7;
  return (((size_t)ft * nch + ch) * 5 + 4) * 1024 + (q * 16 + r) * 16 + 4 * v + (gi >> 1);
}
// the dense weight (j, k) read back from the panel: the kept value whose position is k & 3, or 0
__host__ __device__ inline int i8ie_sp24_get(const uint8_t* panel, int j, int k, int nch) {
  const int g = k >> 2, pos = k & 3;
  const unsigned nib = (panel[i8ie_sp24_index_at(j, g, nch)] >> (4 * (g & 1))) & 15u;
  if ((int)(nib & 3u) == pos) return (int)(int8_t)panel[i8ie_sp24_value_at(j, g, 0, nch)];
  if ((int)(nib >> 2) == pos) return (int)(int8_t)panel[i8ie_sp24_value_at(j, g, 1, nch)];
  return 0;
}

// host: the C-ABI's compressed rows (values [n][K4 / 2], positions [n][K4 / 8], K4 = 4 ceil(K / 4)) into a zeroed panel
void i8ie_sp24_pack_panel(const int8_t* values, const uint8_t* index, int n, int K, uint8_t* panel);

struct I8ieSp24Call {
  const uint8_t* A;  // [M][K] u8
  int M, N, K;
  const uint8_t* B;  // the panel, in the reference's K order
  int hw;            // sp24lin_direct: rows are a flattened NHWC activation of hw pixels (1: reference order)
  I8ieEpilogue ep;   // ocp: oc + 128 * wsum for the MFMA kernel, the plain oc for sp24lin_direct; biasf set; per-feature or per-tensor
  uint8_t* out;
};
bool i8ie_sp24lin_mfma_takes(const I8ieSp24Call& c);  // K % 32 == 0, reference K order and 16-byte aligned operands
int i8ie_sp24lin_mfma_launch(i8ie_ctx* ctx, const I8ieSp24Call& c);
int i8ie_sp24lin_direct_launch(i8ie_ctx* ctx, const I8ieSp24Call& c);

// the one-off kernel of a handle: oc / wsum / oc' / the float bias for (s_in, zp_in) in the reference's accumulation order
int i8ie_sp24_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in, int32_t* oc,
                             int32_t* wsum, int32_t* ocp, float* biasf);
