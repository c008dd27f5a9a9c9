// i8ie_deconv.h -- ConvTranspose2d (i8ie_deconv.hip): the call block and the weight-side helpers the layer handle uses at
// create time
//
// Dispatch (i8ie_deconv_mfma_takes): deconv_mfma when the longest phase reduction, C * ceil(k / s)^2, is at least 32 bytes
// (half a K step of the matrix instruction: below that more than half of every step is padding), the force-fallback option is
// off and the buffers are aligned for its gather; deconv_direct otherwise.
#pragma once
#include <cstddef>
#include <cstdint>

#include <vector>

#include "i8ie_calls.h"
#include "i8ie_requant.h"

struct i8ie_ctx;

struct I8ieDeconvCall {
  const uint8_t* A;  // NHWC [m][H + 2 ib][W + 2 ib][C]; taps outside the H x W image read as zp_in (the border is not read)
  int m, H, W, C, ib;
  int OH, OW, k, s, p;  // square kernel, stride, padding; OH = (H - 1) s - 2 p + k + output_padding
  int N, Ngp, Kpp;      // out features, N rounded up to 16, the phase panels' K pitch (i8ie_deconv_kpitch)
  const int8_t* Bp;     // [s * s][Ngp][Kpp]: phase (ry, rx)'s taps, K ordered (ty, tx, c), zero padded (i8ie_deconv_pack)
  const int* ktab;      // device, from i8ie_deconv_ktab
  const int32_t* tph;   // [s * s][Ngp]: the sum of feature j's weights at the taps phase ph does NOT see
  I8ieEpilogue ep;      // ocp [N], over the whole equivalent matrix; acc nullptr or [m * OH * OW][N]
  int zp_in;
  uint8_t* out;         // NHWC [m][OH + 2 ob][OW + 2 ob][N], interior written
  int ob;
};
bool i8ie_deconv_mfma_takes(const i8ie_ctx* ctx, const I8ieDeconvCall& c);
int i8ie_deconv_launch(i8ie_ctx* ctx, const I8ieDeconvCall& c);
// taps of residue r along one axis: ky = r + s * t, t < i8ie_deconv_taps(k, s, r)
__host__ __device__ inline int i8ie_deconv_taps(int k, int s, int r) { return r < k ? (k - r + s - 1) / s : 0; }
int i8ie_deconv_kpitch(int C, int k, int s);
// the argument rules of every transposed entry (I8IE_ERR_ARG; no device call): sizes positive, k and stride below 65536,
// stride >= 1, 0 <= pad <= k - 1, 0 <= output_pad < stride, c * k * k below 2^30
int i8ie_deconv_check_args(int kc, int c, int k, int stride, int pad, int output_pad);
// host: the phase panels and the per-(phase, feature) sums of the unseen taps from the equivalent matrix qw [N][C * k * k]
// (K ordered (c, ky', kx'), the kernel already flipped: the transposed layer's tap (ky, kx) is its (k - 1 - ky, k - 1 - kx))
void i8ie_deconv_pack(const int8_t* qw, int N, int C, int k, int s, std::vector<int8_t>& panels, std::vector<int32_t>& tph);
// host: the MFMA kernel's gather table, per phase pairs {(ty << 16) | tx, c} per K position in units of the granularity
void i8ie_deconv_ktab(int C, int k, int s, std::vector<int>& tab);
// FP32 form (i8ie_fp32-style plain kernel, off the timed path): NCHW in / out, weight [c][kc][k][k], bias [kc]
int i8ie_deconv_f32_launch(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b, int kc,
                           int k, int s, int p, int oh, int ow, float* out);
