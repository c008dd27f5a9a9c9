// i8ie_w4pw.h -- the launchers of i8ie_w4pw.hip (pointwise Conv2d with 4-bit weights), as i8ie_layer.hip
// sees them, and the device helpers that file shares with i8ie_w4conv.hip (k x k; section 8zc).  The weights are the nibble panel
// of i8ie_w4lin.h.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"
#include "i8ie_epilogue.h"

// one pointwise launch: m images of H x W pixels, C channels in, N features out
struct I8ieW4pwCall {
  const uint8_t* A;    // NHWC with `ib` border pixels around every image, or NCHW (in_nchw; ib = 0)
  int m, H, W, C, ib;
  int in_nchw, in_s8;  // in_s8: the input bytes are stored re-biased (^0x80); their border is never read
  int N;
  const uint8_t* B;    // the panel [ftiles][chunks][2] of i8ie_w4lin.h
  I8ieEpilogue ep;     // per-feature (msv, sbv set), biasf null; ocp: oc + 128 * wsum for the MFMA kernel, the plain oc for w4pw_direct
  uint8_t* out;        // NHWC with `ob` border pixels (written by the caller), or NCHW (out_nchw; ob = 0)
  int ob, out_nchw, out_s8;
};
// C % 32 == 0, NHWC at both ends, 16-byte aligned input and panel, offsets inside 32 bits
bool i8ie_w4pw_mfma_takes(const I8ieW4pwCall& c);
// the row count above which the many-row instance (64 pixels x 128 features per block) replaces the few-row one (16 x 64)
constexpr int kW4pwFewRows = 256;
int i8ie_w4pw_mfma_launch(i8ie_ctx* ctx, const I8ieW4pwCall& c);
int i8ie_w4pw_direct_launch(i8ie_ctx* ctx, const I8ieW4pwCall& c);

// ---- shared by the kernels of i8ie_w4pw.hip and i8ie_w4conv.hip ------------------------------------------------------------------
constexpr int kChunk = 256;  // K values per chunk: 256 activation bytes per pixel, 128 weight bytes per feature

// how the pixels of one side lie (NHWC): pixels per image and per line, the physical line and image, the border
struct PwSide {
  int HW, W, Wp, HpWp, b;
};
inline PwSide pw_side(int H, int W, int b) { return PwSide{H * W, W, W + 2 * b, (H + 2 * b) * (W + 2 * b), b}; }

__device__ __forceinline__ long long pw_pixel(const PwSide& s, long long g) {
  if (s.b == 0) return g;
  const long long img = g / s.HW;
  const int rem = (int)(g - img * s.HW), y = rem / s.W;
  return img * s.HpWp + (long long)(y + s.b) * s.Wp + (rem - y * s.W) + s.b;
}

// c with oc' -> the accumulators' copy -> requantise -> (re-bias) -> store: the quad epilogue's steps (a conv has no float bias)
__device__ __forceinline__ void pw_finish(const I8ieEpiArgs& ep, int (&c)[4], const I8ieQuadCols<true>& q, int nf, long long acc0,
                                          uint8_t* o, bool whole, uint32_t o_xor) {
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] += q.oc[r];
  i8ie_epi_copy_acc(ep, c, acc0, nf);
  i8ie_epi_store(o, i8ie_epi_pack<true>(ep, c, q) ^ o_xor, whole, nf);
}

// a block of 16 RT rows x 16 WAVES FPW features, its chunks in a ring of STAGES stages
template <int RT, int WAVES, int FPW, int STAGES>
struct PwShape {
  static constexpr int kThreads = 64 * WAVES, kFT = WAVES * FPW;
  static constexpr int kRows = RT * 16, kFeats = kFT * 16;
  static constexpr int kPA = RT * 4, kPB = kFT * 2;               // 1-KiB DMA pieces of a chunk: 4 pixels' rows / one fragment
  static constexpr int kPPW = (kPA + kPB + WAVES - 1) / WAVES;    // pieces per wave and chunk (every wave issues the same number)
  static constexpr int kStageA = kPA * 1024;
  static constexpr int kStage = kPPW * WAVES * 1024;              // (pieces past kPA + kPB land in the stage's padding)
  static constexpr int kLds = STAGES * kStage;
  static_assert(STAGES >= 2 && (STAGES - 2) * kPPW < 64, "the vmcnt immediate");
};
