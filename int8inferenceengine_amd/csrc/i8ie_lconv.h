// i8ie_lconv.h -- dense 1 x k / k x 1 Conv2d at stride 1 (i8ie_lconv.hip): the call block and the decision
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"
#include "i8ie_requant.h"

struct i8ie_ctx;

// The LDS budget of one block's line plan.  The compiler gives both instances of the kernel 58 VGPRs + 32 AGPRs per lane, an
// occupancy of 5 waves per SIMD: registers cap residency at 5 blocks of 256 lanes per CU.  160 KiB of LDS per CU hold 5 plans of
// 32 KiB, so this budget is the largest that never lets LDS cut residency below what the registers allow.  The intent of
// keeping several blocks resident is that one block's staging (two barriers per channel chunk, no double buffer) overlaps the
// MFMA loops of the others; that overlap has not been measured.  Inception's lines (17 and 8 pixels) plan 9 to 14 KiB.  A longer line is staged whole by every block that holds
// a piece of it, so beyond a few hundred pixels the grouped kernels' direct gather reads less: the plan declines there anyway.
constexpr size_t I8IE_LCONV_LDS_BUDGET = (size_t)32 << 10;

struct I8ieLconvCall {
  const uint8_t* A;  // NHWC [m][H + 2 ib][W + 2 ib][C], border bytes = zp_in; positions beyond the border read as zp_in
  int m, H, W, C, ib;
  int OH, OW, KH, KW, pad_h, pad_w;  // KH == 1 or KW == 1, the other >= 2; stride 1, dilation 1
  int N, Ngp, Kgp;                   // out features; the panel's rows (N rounded up to 16) and pitch (C k rounded up to 64)
  const int8_t* Bp;                  // [Ngp][Kgp], K ordered (tap, c), zero padded: route G's panel of a layer with groups = 1
  I8ieEpilogue ep;                   // ocp [N]; acc nullptr or [m * OH * OW][N]
  int zp_in;
  uint8_t* out;                      // NHWC [m][OH + 2 ob][OW + 2 ob][N], interior written
  int ob;
};
// the LDS plan of a line: lines per block x (Lo + k - 1) pixels x (channel chunk + 16) bytes; Lo = the output pixels of a line
size_t i8ie_lconv_lds_bytes(int C, int k, int Lo);
// takes: 1 x k or k x 1 with k >= 2, C % 16 == 0, the force-fallback option off, A and Bp 16-byte aligned, and the LDS plan
// inside I8IE_LCONV_LDS_BUDGET.  Otherwise the caller runs the grouped kernels.
bool i8ie_lconv_takes(const i8ie_ctx* ctx, const I8ieLconvCall& c);
int i8ie_lconv_launch(i8ie_ctx* ctx, const I8ieLconvCall& c);
