// i8ie_w4pw.h -- the launchers of i8ie_w4pw.hip (pointwise Conv2d with 4-bit weights), as i8ie_layer.hip
// sees them.  The weights are the nibble panel of i8ie_w4lin.h.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"

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
