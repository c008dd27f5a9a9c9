// i8ie_w4conv.h -- the launchers of i8ie_w4conv.hip (k x k Conv2d with 4-bit weights), as i8ie_layer.hip and
// i8ie_layer_create.hip see them.  The weights are the nibble panel of i8ie_w4lin.h in the kernel's own K order.  Internal:
// nothing here is part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "i8ie_calls.h"

// The kernel's K order: tap (ky, kx) major, channels minor, every tap's channels padded to the MFMA's 64 with zero nibbles.
// Reference weight k = (c, ky, kx) lies at panel position (ky * k + kx) * cpad + c.
inline int i8ie_w4conv_cpad(int c) { return (c + 63) / 64 * 64; }
inline int i8ie_w4conv_kpanel(int c, int k) { return k * k * i8ie_w4conv_cpad(c); }
// host: the C-ABI's packed rows [n][ceil(c * k * k / 2)] in reference order into a zeroed panel of i8ie_w4_panel_bytes(n, kpanel)
void i8ie_w4conv_pack_panel(const uint8_t* packed, int n, int c, int k, uint8_t* panel);

// one launch: m images of H x W pixels, C channels in; a k x k window with one stride, padding and dilation; N features out
struct I8ieW4convCall {
  const uint8_t* A;    // NHWC with `ib` border pixels around every image, or NCHW (in_nchw; ib = 0)
  int m, H, W, C, ib;
  int in_nchw, in_s8;  // in_s8: the bytes are stored re-biased (^0x80), their border too
  int k, stride, pad, dil, OH, OW;
  int zp_in;           // w4conv_direct: what a tap outside the image reads
  int N;
  const uint8_t* B;    // the panel in the kernel's K order
  I8ieEpilogue ep;     // per-feature (msv, sbv set), biasf null; ocp: oc + 128 * wsum for the MFMA kernel, the plain oc for w4conv_direct
  uint8_t* out;        // NHWC with `ob` border pixels (written by the caller), or NCHW (out_nchw; ob = 0)
  int ob, out_nchw, out_s8;
};
// C % 32 == 0, NHWC at both ends, ib >= pad (the border holds zp_in), 16-byte aligned input and panel, offsets inside 32 bits
bool i8ie_w4conv_mfma_takes(const I8ieW4convCall& c);
int i8ie_w4conv_mfma_launch(i8ie_ctx* ctx, const I8ieW4convCall& c);
int i8ie_w4conv_direct_launch(i8ie_ctx* ctx, const I8ieW4convCall& c);
