// i8ie_gconv.h -- grouped / depthwise Conv2d (i8ie_gconv.hip): the call block and the weight-side helpers the layer
// handle uses at create time
#pragma once
#include <cstddef>
#include <cstdint>

#include <vector>

#include "i8ie_calls.h"
#include "i8ie_requant.h"

struct i8ie_ctx;

struct I8ieGconvCall {
  const uint8_t* A;  // NHWC [m][H + 2 ib][W + 2 ib][C], border bytes = zp_in; taps beyond the border read as zp_in
  int m, H, W, C, ib;
  int OH, OW, KH, KW;
  // per axis (DESIGN.md sections 8j, 8p): tap (ky, kx) reads input pixel (oy * stride_h - pad_h + ky * dil_h, ox * stride_w -
  // pad_w + kx * dil_w); dil >= 1.  A square layer passes equal pairs.
  int stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int groups, Cg, Ng, Ngp, Kgp;  // Ngp = Ng rounded up to 16, Kgp = Cg * KH * KW rounded up to 64
  const int8_t* Bp;   // [groups][Ngp][Kgp], K ordered (kh, kw, cg), zero padded
  const int* ktab;    // device, from i8ie_gconv_ktab
  I8ieEpilogue ep;    // ocp [groups * Ng]; acc nullptr or [m * OH * OW][groups * Ng]
  int zp_in;
  uint8_t* out;       // NHWC [m][OH + 2 ob][OW + 2 ob][groups * Ng], interior written
  int ob;
};
// gconv_mfma when Cg * KH * KW >= 32, the force-fallback option is off and the buffers are aligned for its gather;
// gconv_direct otherwise
bool i8ie_gconv_mfma_takes(const i8ie_ctx* ctx, const I8ieGconvCall& c);
int i8ie_gconv_launch(i8ie_ctx* ctx, const I8ieGconvCall& c);
int i8ie_gconv_granularity(int Cg);
// host: the gather table of a layer, pairs {(kh << 16) | kw, cg} per K position in units of the granularity
void i8ie_gconv_ktab(int Cg, int kh, int kw, int Kgp, std::vector<int>& tab);
