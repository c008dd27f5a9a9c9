// i8ie_w4glin.h -- the group multipliers of a 4-bit Linear with group-wise scales along K (i8ie_w4glin.hip) and that file's
// launchers, as i8ie_layer.hip and i8ie_layer_create.hip see them.  The nibbles lie in the panel of i8ie_w4lin.h, unchanged.
// Internal: nothing here is part of the C-ABI.
#pragma once
#include "i8ie_w4lin.h"

// The multipliers on the device: u8 [feature tiles of the panel][Gp groups][16 features of the tile], Gp = chunks * (256 / gs)
// -- every group the panel's chunks cover, so a kernel never asks for one past the array; groups past ceil(K / gs) and features
// past n hold 1 (their nibbles are zero).  The sixteen bytes of (tile, group) are one LDS bank row: lane (q, r) of an accumulator
// tile holds features 4 q .. 4 q + 3 and reads its four multipliers as the dword at 4 q.
inline bool i8ie_w4g_size_ok(int gs) { return gs == 64 || gs == 128 || gs == 256; }
inline int i8ie_w4g_groups(int K, int gs) { return (K + gs - 1) / gs; }
inline int i8ie_w4g_padded_groups(int K, int gs) { return i8ie_w4_chunks(K) * (256 / gs); }
inline size_t i8ie_w4g_mult_bytes(int n, int K, int gs) { return (size_t)i8ie_w4_ftiles(n) * i8ie_w4g_padded_groups(K, gs) * 16; }
__host__ __device__ inline size_t i8ie_w4g_mult_at(int j, int g, int Gp) { return ((size_t)(j >> 4) * Gp + g) * 16 + (j & 15); }

// host: the C-ABI's m [n][ceil(K / gs)] into the device layout (every byte of `out` is written)
void i8ie_w4g_pack_mult(const uint8_t* m_host, int n, int K, int gs, uint8_t* out);

struct I8ieW4gCall {
  const uint8_t* A;   // [M][K] u8
  int M, N, K, gs;
  const uint8_t* B;   // the nibble panel, in the reference's K order
  const uint8_t* Mg;  // the multipliers, laid out as above
  int hw;             // w4glin_direct: rows are a flattened NHWC activation of hw pixels (1: reference order)
  I8ieEpilogue ep;    // per-feature; ocp: oc + 128 * wsum_eff for the MFMA kernel, the plain oc for w4glin_direct
  uint8_t* out;
};
bool i8ie_w4glin_mfma_takes(const I8ieW4gCall& c);  // K % 32 == 0, 16-byte aligned operands, rows in reference order
int i8ie_w4glin_mfma_launch(i8ie_ctx* ctx, const I8ieW4gCall& c);
int i8ie_w4glin_direct_launch(i8ie_ctx* ctx, const I8ieW4gCall& c);

// the handle's one-off kernel: oc / wsum_eff / oc' / the float bias (32 q_b / s_in) for (s_in, zp_in), from panel and multipliers
// in the reference's accumulation order
int i8ie_w4g_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const uint8_t* mg, const int8_t* qb, int n, int K, int gs,
                            float s_in, int zp_in, int32_t* oc, int32_t* wsum, int32_t* ocp, float* biasf);
