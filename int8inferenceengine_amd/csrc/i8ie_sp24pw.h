// i8ie_sp24pw.h -- the launchers of i8ie_sp24pw.hip (pointwise Conv2d with 2:4 structured-sparse 8-bit weights; DESIGN.md section
// 8zd), as i8ie_layer.hip sees them.  The weights are the compressed panel of i8ie_sp24lin.h, the map at both ends is the one of
// i8ie_w4pw.h (PwSide / pw_pixel).  Internal: nothing here is part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"
#include "i8ie_epilogue.h"

// one pointwise launch: m images of H x W pixels, C channels in, N features out
struct I8ieSp24pwCall {
  const uint8_t* A;    // NHWC with `ib` border pixels around every image, or NCHW (in_nchw; ib = 0)
  int m, H, W, C, ib;
  int in_nchw, in_s8;  // in_s8: the input bytes are stored re-biased (^0x80); their border is never read
  int N;
  const uint8_t* B;    // the panel [ftiles][chunks][5] of i8ie_sp24lin.h
  I8ieEpilogue ep;     // per-feature (msv, sbv set) or per-tensor, biasf null; ocp: oc + 128 * wsum for the MFMA kernel, the plain oc
                       // for sp24pw_direct
  uint8_t* out;        // NHWC with `ob` border pixels (written by the caller), or NCHW (out_nchw; ob = 0)
  int ob, out_nchw, out_s8;
};
// C % 32 == 0, NHWC at both ends, 16-byte aligned input and panel, offsets inside 32 bits
bool i8ie_sp24pw_mfma_takes(const I8ieSp24pwCall& c);
// the pixel count above which the many-pixel instance (64 pixels x 128 features per block) replaces the few-pixel one (16 x 32)
constexpr int kSp24pwFewRows = 256;
int i8ie_sp24pw_mfma_launch(i8ie_ctx* ctx, const I8ieSp24pwCall& c);
int i8ie_sp24pw_direct_launch(i8ie_ctx* ctx, const I8ieSp24pwCall& c);

// the one-off kernel of a conv handle: oc (the bias folded in, src/conv2d.cc:117-124) / wsum / oc' for (s_in, zp_in) from the panel
int i8ie_sp24pw_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in, int32_t* oc,
                               int32_t* wsum, int32_t* ocp);
