// i8ie_dconv.h -- dense dilated Conv2d at stride 1 (i8ie_dconv.hip): the call block and the decision
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"
#include "i8ie_requant.h"

struct i8ie_ctx;

struct I8ieDconvCall {
  const uint8_t* A;  // NHWC [m][H + 2 ib][W + 2 ib][C], border bytes = zp_in; positions beyond the border read as zp_in
  int m, H, W, C, ib;
  int OH, OW, pad, k, dil;  // square kernel, stride 1; OH = H + 2 pad - dil (k - 1)
  int N, Ngp, Kgp;          // out features; the panel's rows (N rounded up to 16) and pitch (C k k rounded up to 64)
  const int8_t* Bp;         // [Ngp][Kgp], K ordered (kh, kw, c), zero padded: route G's panel of a layer with groups = 1
  I8ieEpilogue ep;          // ocp [N]; acc nullptr or [m * OH * OW][N]
  int zp_in;
  uint8_t* out;             // NHWC [m][OH + 2 ob][OW + 2 ob][N], interior written
  int ob;
};
// takes: dil >= 2, k >= 2, C % 16 == 0, C k k >= 32, the force-fallback option off, A and Bp 16-byte aligned, and the LDS
// plan (8 patches of (k + 3)^2 pixels by the channel chunk) inside 64 KiB.  Otherwise the caller runs the grouped kernels.
bool i8ie_dconv_takes(const i8ie_ctx* ctx, const I8ieDconvCall& c);
int i8ie_dconv_launch(i8ie_ctx* ctx, const I8ieDconvCall& c);
