// i8ie_fp32.hip -- FP32 forward ops used before convert() and during
// calibration (prepare() -> one FP32 batch -> convert()).  They are off the
// timed INT8 path.  Conv2d and Linear run on the f32
// matrix instruction (round 4); relu / max-pool are plain streaming kernels.
// The reference computes these with cblas_sgemm
// (src/conv2d.cc:63-98, src/fully_connected.cc:5-21) and pins them only to
// atol 0.1 against torch (unittest/test_layers.py:10-11), so summation order
// is free here.
#include "i8ie_internal.h"
#include "i8ie_deconv.h"


namespace {

// ---- one implicit-GEMM kernel for Conv2d and Linear in FP32 on the f32 matrix instruction -------------------------------
//   out[r][j] = sum_k X[r][k] * W[j][k] + b[j],   X = im2col(in) (zero padding; src/conv2d.cc:63-98) or in itself (Linear,
//   src/fully_connected.cc:5-21)
// v_mfma_f32_32x32x2_f32 is an exact fp32 fma chain (64 FLOP per clock and SIMD = the vector rate, 157 TFLOP/s on the chip) and
// leaves the vector unit to the gathers.  Round 3's kernels were one-thread-per-output VALU loops: 43 ms per launch on AlexNet's
// convolutions, 1.7 k images/s through the FP32 network (what prepare() / calibration / the FP32 teacher run).
//   * block = 256 threads, tile = 128 rows (output pixels / input rows) x 128 features, K walked 16 at a time through ONE LDS
//     stage per operand, k-major ([16][132] floats: a fragment read is 64 consecutive floats, conflict-free); the next K block's
//     16 + 16 values per thread are in registers before this block's MFMAs start.
//   * the im2col gather: a row's (image, oy, ox) is worked out once per thread (its row never changes); a K position's
//     (input offset, kernel row, kernel column) comes from a table of K entries built per launch (k_table_kernel) -- no
//     division in the loop.
//   * each wave owns 64 x 64 outputs (2 x 2 MFMA tiles, 64 accumulator registers).  Which operand is srcA decides what a lane
//     holds: for Conv2d a lane = an output pixel (NCHW stores: 32 consecutive pixels of one feature per instruction), for Linear
//     a lane = a feature (row-major stores).
constexpr int FB = 128, FK = 16, FP = 132;  // tile edge, K block, LDS row pitch (floats)
typedef float v16f __attribute__((ext_vector_type(16)));

struct F32Args {
  const float* in;
  const float* w;
  const float* b;
  float* out;
  const int2* ktab;  // [K]: {input offset of K position k relative to the window origin, (kernel row << 16) | kernel column}
  int M, N, K;
  int c, h, wd, oh, ow, stride, pad, P;  // P = oh * ow output pixels per image (1 for Linear); stride / pad: the h axis'
  int stride_w, pad_w;                   // ... and the w axis' (equal unless i8ie_conv2d_f32_rect says otherwise)
  // grouped Conv2d (blockIdx.z = group): N, K, c above are one group's; these the whole tensors' channel counts
  int ctot, Ntot;
};

// dil_h, dil_w: the dilation of a Conv2d (1 otherwise): kernel row l / column m read the window's pixel (l * dil_h, m * dil_w)
__global__ __launch_bounds__(256) void k_table_kernel(int2* tab, int K, int h, int w, int kh, int kw, int dil_h, int dil_w) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
    const int ch = k / (kh * kw), rem = k - ch * (kh * kw), l = rem / kw * dil_h, m = (rem % kw) * dil_w;
    tab[k] = make_int2((ch * h + l) * w + m, (l << 16) | m);
  }
}

template <bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(F32Args p) {
  __shared__ float Xs[FK][FP], Ws[FK][FP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bm0 = blockIdx.y * FB, bn0 = blockIdx.x * FB;
  const int grp = blockIdx.z;  // (0 unless a grouped Conv2d)
  const float* wg = p.w + (size_t)grp * p.N * p.K;
  const float* bg = p.b + (size_t)grp * p.N;

  // ---- this thread's gather row (activations): row bm0 + tid % 128, K positions (tid / 128) + 2 e
  const int xr = bm0 + (tid & 127), xk0 = tid >> 7;
  const bool xrow_ok = xr < p.M;
  const int ximg = xr / p.P, xpix = xr - ximg * p.P;
  const int xoy = xpix / p.ow, xox = xpix - xoy * p.ow;
  const int y0 = xoy * p.stride - p.pad, x0 = xox * p.stride_w - p.pad_w;
  const float* xbase = p.in + (((size_t)ximg * p.ctot + (size_t)grp * p.c) * p.h + y0) * (size_t)p.wd + x0;  // (may point before the image: only used with valid taps)
  // ---- this thread's weight elements: K position tid % 16, features tid / 16 + 16 e
  const int wk = tid & 15, wj0 = tid >> 4;

  float xv[8], wv[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + xk0 + 2 * e;
      float v = 0.0f;
      if (xrow_ok && k < p.K) {
        const int2 t = p.ktab[k];
        const int yy = y0 + (t.y >> 16), xx = x0 + (t.y & 0xffff);
        if (!CONV || ((unsigned)yy < (unsigned)p.h && (unsigned)xx < (unsigned)p.wd)) v = xbase[t.x];
      }
      xv[e] = v;
      const int j = bn0 + wj0 + 16 * e, kw_ = k0 + wk;
      wv[e] = (j < p.N && kw_ < p.K) ? wg[(size_t)j * p.K + kw_] : 0.0f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      Xs[xk0 + 2 * e][tid & 127] = xv[e];
      Ws[wk][wj0 + 16 * e] = wv[e];
    }
  };

  v16f acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
  // srcA's rows become the accumulator's registers, srcB's columns its lanes: Conv2d multiplies (features x K) by (K x pixels),
  // Linear (rows x K) by (K x features)
  const int wa = wave >> 1, wb = wave & 1;  // this wave's 64-wide slices of the srcA / srcB tiles
  const float(*As)[FP] = CONV ? Ws : Xs;
  const float(*Bs)[FP] = CONV ? Xs : Ws;
  const int hh = lane >> 5, l31 = lane & 31;

  fetch(0);
  for (int k0 = 0; k0 < p.K; k0 += FK) {
    __syncthreads();  // everyone is done with the previous K block
    stage();
    __syncthreads();
    if (k0 + FK < p.K) fetch(k0 + FK);
#pragma unroll
    for (int kk = 0; kk < FK; kk += 2) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = As[kk + hh][64 * wa + 32 * i + l31];
        b[i] = Bs[kk + hh][64 * wb + 32 * i + l31];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---- + bias, store.  Register 4 g + r of tile (i, j) = srcA row 64 wa + 32 i + 8 g + 4 hh + r, srcB column 64 wb + 32 j + l31
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = 64 * wb + 32 * j + l31;
    if (CONV) {
      const int r = bm0 + col;  // output pixel (global row)
      if (r >= p.M) continue;
      const int img = r / p.P, pix = r - img * p.P;
      float* obase = p.out + ((size_t)img * p.Ntot + (size_t)grp * p.N) * p.P + pix;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int f = bn0 + 64 * wa + 32 * i + 8 * (e >> 2) + 4 * hh + (e & 3);
          if (f < p.N) obase[(size_t)f * p.P] = acc[i][j][e] + bg[f];
        }
    } else {
      const int f = bn0 + col;
      if (f >= p.N) continue;
      const float bias = bg[f];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = bm0 + 64 * wa + 32 * i + 8 * (e >> 2) + 4 * hh + (e & 3);
          if (r < p.M) p.out[(size_t)r * p.N + f] = acc[i][j][e] + bias;
        }
    }
  }
}

template <bool CONV>
int launch_gemm_f32(i8ie_ctx* ctx, F32Args a, int kh, int kw, const char* name, int groups = 1, int dil_h = 1, int dil_w = 1) {
  I8IE_REQUIRE((size_t)a.M * a.K < ((size_t)1 << 62) && a.K < (1 << 30), "f32 gemm: dimensions");
  I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)a.K * sizeof(int2) + 256));
  int2* tab = reinterpret_cast<int2*>(ctx->ws);
  k_table_kernel<<<(a.K + 255) / 256 < 64 ? (a.K + 255) / 256 : 64, 256, 0, ctx->stream>>>(tab, a.K, a.h, a.wd, kh, kw, dil_h, dil_w);
  I8IE_LAUNCH_CHECK();
  a.ktab = tab;
  const dim3 grid((unsigned)((a.N + FB - 1) / FB), (unsigned)((a.M + FB - 1) / FB), (unsigned)groups);
  // (blockIdx.y carries the row tiles: 65 535 x 128 = 8.4 M rows per launch; AlexNet's largest, 1000 x 55 x 55, is 3.0 M)
  I8IE_REQUIRE(grid.y <= 65535u, "f32 gemm: more than 8.4 M output rows in one call");
  I8ieProfScope prof(ctx, name, 0.0, ((double)a.M * a.K * 4 + (double)a.N * a.K * 4 + (double)a.M * a.N * 4) * groups);
  gemm_f32_kernel<CONV><<<grid, 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

__global__ __launch_bounds__(256) void relu_f32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       int64_t n) {
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride)
    out[i] = in[i] > 0.0f ? in[i] : 0.0f;  // src/functional.cc:5-13
}

// src/functional.cc:36-64 with T = float: running max starts at -FLT_MAX
__global__ __launch_bounds__(256) void maxpool_f32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          int64_t total, int h, int w, int oh, int ow, int k,
                                                          int s) {
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gstride) {
    const int x = (int)(e % ow);
    int64_t t = e / ow;
    const int y = (int)(t % oh);
    const int64_t plane = t / oh;
    const float* p = in + plane * h * w + (int64_t)(y * s) * w + x * s;
    float mx = -3.402823466e+38f;
    for (int m = 0; m < k; ++m)
      for (int l = 0; l < k; ++l) {
        const float v = p[m * w + l];
        mx = mx >= v ? mx : v;
      }
    out[e] = mx;
  }
}

inline int cap_grid(int64_t items) {
  int64_t b = (items + 255) / 256;
  if (b < 1) b = 1;
  return (int)(b > 256 * 32 ? 256 * 32 : b);
}

// the launch of a checked Conv2d: what i8ie_conv2d_f32_dilated and i8ie_conv2d_f32_rect share behind their argument rules
int conv2d_f32_run(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b, int kc, int groups,
                   const i8ie_conv_geom& g, int oh, int ow, float* out) {
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  F32Args a{};
  a.in = in; a.w = wt; a.b = b; a.out = out;
  a.M = n * oh * ow; a.N = kc / groups; a.K = (c / groups) * g.kh * g.kw;
  a.c = c / groups; a.h = h; a.wd = w; a.oh = oh; a.ow = ow; a.P = oh * ow;
  a.stride = g.stride_h; a.stride_w = g.stride_w; a.pad = g.pad_h; a.pad_w = g.pad_w;
  a.ctot = c; a.Ntot = kc;
  return launch_gemm_f32<true>(ctx, a, g.kh, g.kw, "conv2d_f32_mfma", groups, g.dilation_h, g.dilation_w);
}

}  // namespace

extern "C" {

int i8ie_linear_f32(i8ie_ctx* ctx, const float* in, int m, int k, const float* w, const float* b, int n,
                    float* out) {
  I8IE_REQUIRE(ctx && in && w && b && out, "null argument");
  I8IE_REQUIRE(m > 0 && k > 0 && n > 0, "non-positive dimension");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  F32Args a{};
  a.in = in; a.w = w; a.b = b; a.out = out;
  a.M = m; a.N = n; a.K = k;
  a.c = k; a.h = 1; a.wd = 1; a.oh = 1; a.ow = 1; a.stride = a.stride_w = 1; a.pad = a.pad_w = 0; a.P = 1;
  a.ctot = k; a.Ntot = n;
  return launch_gemm_f32<false>(ctx, a, 1, 1, "linear_f32_mfma");
}

int i8ie_conv2d_f32(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt,
                    const float* b, int kc, int kh, int kw, int stride, int pad, float* out) {
  return i8ie_conv2d_f32_grouped(ctx, in, n, c, h, w, wt, b, kc, kh, kw, stride, pad, 1, out);
}

// src/conv2d.cc:63-98 per group; groups: not in the reference.  One launch: the group is the grid's z dimension.
int i8ie_conv2d_f32_grouped(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt,
                            const float* b, int kc, int kh, int kw, int stride, int pad, int groups, float* out) {
  return i8ie_conv2d_f32_dilated(ctx, in, n, c, h, w, wt, b, kc, kh, kw, stride, pad, groups, 1, out);
}

// ... and with a dilation (not in the reference): the gather table carries it, the kernel is the same
int i8ie_conv2d_f32_dilated(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b, int kc,
                            int kh, int kw, int stride, int pad, int groups, int dilation, float* out) {
  // (this entry's own rules, in its order and under its name: the texts are what its callers have always seen)
  I8IE_REQUIRE(dilation >= 1, "dilation must be >= 1");
  I8IE_REQUIRE(groups >= 1 && groups <= 65535, "groups must be in [1, 65535]");
  I8IE_REQUIRE(c > 0 && kc > 0 && c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && kc > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(stride > 0 && pad >= 0, "bad stride/padding");
  const int64_t eh = (int64_t)dilation * (kh - 1) + 1, ew = (int64_t)dilation * (kw - 1) + 1;  // the kernel's extent
  I8IE_REQUIRE(h - eh + 2 * pad >= 0 && w - ew + 2 * pad >= 0,
               dilation > 1 ? "dilated kernel larger than padded input" : "kernel larger than padded input");
  const int oh = (int)((h - eh + 2 * pad) / stride) + 1, ow = (int)((w - ew + 2 * pad) / stride) + 1;
  I8IE_REQUIRE((int64_t)n * oh * ow < ((int64_t)1 << 31) && eh < 65536 && ew < 65536, "conv2d_f32: too many output pixels");
  I8IE_REQUIRE(ctx && in && wt && b && out, "null argument");  // (behind the argument rules: they need no device)
  return conv2d_f32_run(ctx, in, n, c, h, w, wt, b, kc, groups, i8ie_conv_geom{kh, kw, stride, stride, pad, pad, dilation, dilation}, oh, ow, out);
}

// ... and with every geometry number per axis: still the gather table and the window origin alone
int i8ie_conv2d_f32_rect(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b, int kc,
                         int groups, const i8ie_conv_geom* geom, float* out) {
  I8IE_REQUIRE(geom != nullptr, "null geometry");
  const int kh = geom->kh, kw = geom->kw, dilation_h = geom->dilation_h, dilation_w = geom->dilation_w;
  I8IE_REQUIRE(dilation_h >= 1 && dilation_w >= 1, "dilation must be >= 1");
  I8IE_REQUIRE(groups >= 1 && groups <= 65535, "groups must be in [1, 65535]");
  I8IE_REQUIRE(c > 0 && kc > 0 && c % groups == 0 && kc % groups == 0, "groups must divide the input and the output channels");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && kc > 0 && kh > 0 && kw > 0, "non-positive dimension");
  I8IE_REQUIRE(geom->stride_h > 0 && geom->stride_w > 0 && geom->pad_h >= 0 && geom->pad_w >= 0, "bad stride/padding");
  const int64_t eh = (int64_t)dilation_h * (kh - 1) + 1, ew = (int64_t)dilation_w * (kw - 1) + 1;  // the kernel's extent
  I8IE_REQUIRE(h - eh + 2 * (int64_t)geom->pad_h >= 0 && w - ew + 2 * (int64_t)geom->pad_w >= 0,
               (dilation_h > 1 || dilation_w > 1) ? "dilated kernel larger than padded input" : "kernel larger than padded input");
  const int oh = (int)((h - eh + 2 * (int64_t)geom->pad_h) / geom->stride_h) + 1;
  const int ow = (int)((w - ew + 2 * (int64_t)geom->pad_w) / geom->stride_w) + 1;
  I8IE_REQUIRE((int64_t)n * oh * ow < ((int64_t)1 << 31) && eh < 65536 && ew < 65536, "conv2d_f32: too many output pixels");
  I8IE_REQUIRE(ctx && in && wt && b && out, "null argument");  // (behind the argument rules: they need no device)
  return conv2d_f32_run(ctx, in, n, c, h, w, wt, b, kc, groups, *geom, oh, ow, out);
}

// ConvTranspose2d in FP32 (not in the reference; torch.nn.functional.conv_transpose2d's definition): wt is [c][kc][k][k]
int i8ie_conv_transpose2d_f32(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b,
                              int kc, int k, int stride, int pad, int output_pad, float* out) {
  I8IE_TRY(i8ie_deconv_check_args(kc, c, k, stride, pad, output_pad));
  I8IE_REQUIRE(ctx && in && wt && b && out, "null argument");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0, "non-positive dimension");
  const int64_t oh = (int64_t)(h - 1) * stride - 2 * pad + k + output_pad, ow = (int64_t)(w - 1) * stride - 2 * pad + k + output_pad;
  I8IE_REQUIRE(oh > 0 && ow > 0 && oh < (1 << 30) && ow < (1 << 30), "transposed conv: empty or oversized output");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return i8ie_deconv_f32_launch(ctx, in, n, c, h, w, wt, b, kc, k, stride, pad, (int)oh, (int)ow, out);
}

int i8ie_relu_f32(i8ie_ctx* ctx, const float* in, float* out, int64_t n) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  if (n <= 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  relu_f32_kernel<<<cap_grid(n), 256, 0, ctx->stream>>>(in, out, n);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_maxpool2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int k, int s) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && k > 0 && s > 0, "non-positive dimension");
  I8IE_REQUIRE(k <= h && k <= w, "window larger than the input");
  const int oh = (h - k) / s + 1, ow = (w - k) / s + 1;
  const int64_t total = (int64_t)n * c * oh * ow;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  maxpool_f32_kernel<<<cap_grid(total), 256, 0, ctx->stream>>>(in, out, total, h, w, oh, ow, k, s);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
