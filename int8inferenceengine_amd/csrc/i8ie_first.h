// i8ie_first.h -- the weights-stationary small-C kernel of i8ie_first.hip as seen by i8ie_layer.hip
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"

struct i8ie_ctx;

struct I8ieFirstCall {
  const float* x;        // FP32 NCHW input, or nullptr when `grouped` is given
  const uint8_t* grouped;  // grouped u8 image produced elsewhere (repack_smallc), or nullptr
  uint8_t* scratch;      // room for the grouped image when x is given: n * Hp * WG * 16 bytes
  int n, c, h, w;
  float q_scale;
  int q_zp;
  int KH, KW, KWG, stride, pad, OH, OW;
  const int8_t* B;
  int Kpad, K2, N;
  I8ieEpilogue ep;  // acc null, or [n * OH * OW][N]
  uint8_t* out;
  int ob;
};
int i8ie_first_supported(int c, int stride, int n_out, int K2, int KH, int KWG, int OW);
size_t i8ie_first_scratch_bytes(int n, int KH, int KWG, int stride, int OH, int OW);
int i8ie_first_launch(i8ie_ctx* ctx, const I8ieFirstCall& c);
