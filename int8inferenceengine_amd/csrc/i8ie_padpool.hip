// i8ie_padpool.hip -- max and average pooling with torch's padding and ceil_mode:
// i8ie_pool_output_size, i8ie_maxpool2d_u8_pad, i8ie_maxpool2d_u8_nhwc_pad, i8ie_maxpool2d_f32_pad, i8ie_avgpool2d_u8_pad,
// i8ie_avgpool2d_u8_nhwc_pad, i8ie_avgpool2d_f32_pad.  The definition is in include/i8ie_hip.h; the unpadded floor pools
// (i8ie_igemm.hip's maxpool_u8_nhwc_kernel, i8ie_avgpool.hip) stay what they were and keep their callers.
//
// Geometry.  Output (y, x) sees rows [ys, ye) = [y s - p, min(y s - p + k, h + p)) cut to [0, h), columns likewise.  The
// host checks 0 <= p <= k / 2 and k <= in + 2 p and computes the output size with the ceil-mode drop rule, after which
// 0 <= max(ys, 0) < min(ye, h): every window has a valid tap (ys >= -p > -k; ys < h: in floor mode ys <= h + p - k <= h - 1
// because k >= 2 p and k >= 1, in ceil mode by the drop rule).  Neither kernel reads outside the interior [0, h) x [0, w) of
// its input: a bordered buffer's border bytes hold zp, which is not padding for a max, and the padded mean needs no byte
// of it either -- a padded zero is the byte zp, so the D - n_valid padded taps add (D - n_valid) zp to the sum, a product.
//
// The NHWC kernels (the hot path).  A lane owns one output pixel x one channel item (16 / 4 / 1 channels by c % 16, c % 4
// and pointer alignment, as i8ie_avgpool.hip); an item is handled as 4 / 1 / 1 dwords (a byte item is a dword with one byte
// in it).  Output pixels with y in [iy0, iy1) and x in [ix0, ix1) -- iy0 = ceil(p / s), iy1 = (h + p - k) / s + 1 -- have their
// whole window inside the image.  They are almost all of them (the ResNet stem's 3/2/1 pool on 112 x 112: all but one row
// and one column), and for k = 2 and 3 (max) and 3 (avg) they take a path with no bounds test, the k k loads issued
// together, as maxpool_u8_nhwc_kernel<KT> does.  Every other pixel, and every other k, walks the cut window.  The grid is
// that kernel's too: eight slabs of the output, one per XCD (blockIdx % 8), so that window rows shared by neighbouring
// output rows meet in one L2.  32-bit index arithmetic: the launcher splits a batch whose buffers pass 2^32 bytes or whose
// items pass 2^31 into several launches.  No scratch, no per-call allocation, no atomics.
//   max   byte-wise maximum in spread 16-bit lanes (i8ie_bytemax.h), starting from 0 (every window has a valid tap and no
//         byte is below 0), or from zp when a relu folds in.  Re-biased input is un-biased by one XOR per dword (a template
//         flag: plain input pays nothing).
//   avg   packed 16-bit sums per dword (k k <= 257: 255 n < 65536), 32-bit sums per byte beyond.  Then S' = S + (D - n_valid) zp
//         and q = (S' + D / 2) / D.
//
// The division (S' + D / 2) / D with a per-output D <= k k <= 65536 (div_round below), x = S' + D / 2 <= 255 D + D / 2 < 2^25:
//   multiplier  the full window D = k k, which every inner pixel has, through M = ceil(2^24 / D): e = M D - 2^24 in [0, D),
//               x M / 2^24 = x / D + x e / (D 2^24), and floor() of it equals floor(x / D) when x e / (D 2^24) < 1 / D, i.e.
//               x e < 2^24 (the fraction of x / D is at most (D - 1) / D).  The host checks (255 D + D / 2) e < 2^24 and
//               x M < 2^32 with the actual e and M, and passes M = 0 where either fails.
//   estimate    every other D (the edge pixels' cut windows: at most two values per axis with count_include_pad, more
//               without), and the full window where M = 0: y = fl(float(x) * fl(1.0f / float(D))), q' = trunc(y).  float(x)
//               and the product round once each (relative error <= 2^-24 each); the reciprocal is at most a few ulp off
//               (IEEE division: half an ulp); x / D < 256.  So |y - x / D| < 256 * 8 * 2^-24 = 2^-13 < 1, and q' lies in
//               [floor(x / D) - 1, floor(x / D) + 1].  r = x - q' D is exact in 32-bit integers (q' D <= x + D < 2^26); q' is
//               lowered by one where r < 0 and raised by one where r >= D, which leaves floor(x / D) in all three cases.
//   tests/test_gpu_padpool.py runs every residue of x mod D for every D its cases produce through both.
//
// The NCHW u8 and the FP32 forms are off the timed path: one lane per output, plain loops over the cut window.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_bytemax.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxWindow = 65536;
constexpr int kPackedMax = 257;  // 255 * n < 65536: packed 16-bit sums
constexpr int kPadMaxBlocks = 256 * 32;

// the output size of include/i8ie_hip.h; -1 for arguments the entries refuse
int pool_out(int in, int k, int s, int p, int ceil_mode) {
  if (in <= 0 || k <= 0 || s <= 0 || p < 0 || p > k / 2 || (int64_t)k > (int64_t)in + 2 * (int64_t)p) return -1;
  int64_t o = ((int64_t)in + 2 * (int64_t)p - k + (ceil_mode ? s - 1 : 0)) / s + 1;
  if (ceil_mode && (o - 1) * s >= (int64_t)in + p) --o;
  return (int)o;
}

struct DivParams {
  uint32_t n, rnd;  // divisor D, D / 2
  uint32_t mul;     // ceil(2^24 / D) where the multiplier is proven exact (header), else 0: the estimate
  float rinv;       // fl(1 / D)
};
DivParams make_div(int n) {
  DivParams d;
  d.n = (uint32_t)n;
  d.rnd = (uint32_t)n / 2;
  d.rinv = 1.0f / (float)n;
  d.mul = 0;
  if (n <= kPackedMax) {
    const uint64_t M = ((1ull << 24) + (uint64_t)n - 1) / (uint64_t)n, e = M * (uint64_t)n - (1ull << 24);
    const uint64_t xmax = 255ull * (uint64_t)n + (uint64_t)n / 2;
    if (xmax * e < (1ull << 24) && xmax * M < (1ull << 32)) d.mul = (uint32_t)M;
  }
  return d;
}
// (S + D / 2) / D, then the relu floor `lo`
__device__ __forceinline__ uint32_t div_round(uint32_t S, const DivParams& d, uint32_t lo) {
  const uint32_t x = S + d.rnd;
  uint32_t q;
  if (d.mul) {
    q = (x * d.mul) >> 24;
  } else {
    q = (uint32_t)((float)x * d.rinv);
    const int r = (int)x - (int)(q * d.n);
    q += (r >= (int)d.n) ? 1u : 0u;
    q -= (r < 0) ? 1u : 0u;
  }
  return q > lo ? q : lo;
}

// ---- NCHW and FP32: one lane per output, the cut window in window order
struct PlainGeom {
  int h, w, oh, ow, k, s, p;
};
struct Cut {
  int ys, ye, xs, xe;  // the valid taps
  int D;               // the divisor with count_include_pad
};
__device__ __forceinline__ Cut cut_window(int y, int x, int h, int w, int k, int s, int p) {
  const int y0 = y * s - p, x0 = x * s - p;
  const int y1 = min(y0 + k, h + p), x1 = min(x0 + k, w + p);
  Cut c;
  c.D = (y1 - y0) * (x1 - x0);
  c.ys = max(y0, 0);
  c.xs = max(x0, 0);
  c.ye = min(y1, h);
  c.xe = min(x1, w);
  return c;
}

// T = uint8_t: running max from 0 (src/functional.cc:36-64); T = float: from -FLT_MAX, mx >= v ? mx : v (i8ie_fp32.hip)
template <typename T>
__global__ __launch_bounds__(kThreads) void maxpool_plain_pad_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t total,
                                                                      PlainGeom g, T start) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % g.ow);
    const int64_t t = e / g.ow;
    const int y = (int)(t % g.oh);
    const T* p = in + (t / g.oh) * g.h * g.w;  // plane = img * c + channel
    const Cut c = cut_window(y, x, g.h, g.w, g.k, g.s, g.p);
    T mx = start;
    for (int m = c.ys; m < c.ye; ++m)
      for (int l = c.xs; l < c.xe; ++l) {
        const T v = p[(int64_t)m * g.w + l];
        mx = mx >= v ? mx : v;
      }
    out[e] = mx;
  }
}

__global__ __launch_bounds__(kThreads) void avgpool_u8_nchw_pad_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                       int64_t total, PlainGeom g, int include_pad, uint32_t zp) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % g.ow);
    const int64_t t = e / g.ow;
    const int y = (int)(t % g.oh);
    const uint8_t* p = in + (t / g.oh) * g.h * g.w;
    const Cut c = cut_window(y, x, g.h, g.w, g.k, g.s, g.p);
    uint32_t sum = 0;
    for (int m = c.ys; m < c.ye; ++m)
      for (int l = c.xs; l < c.xe; ++l) sum += p[(int64_t)m * g.w + l];
    const uint32_t nv = (uint32_t)((c.ye - c.ys) * (c.xe - c.xs));
    const uint32_t D = include_pad ? (uint32_t)c.D : nv;
    const DivParams d = {D, D / 2, 0u, 1.0f / (float)D};
    out[e] = (uint8_t)div_round(sum + (D - nv) * zp, d, 0u);
  }
}

__global__ __launch_bounds__(kThreads) void avgpool_f32_pad_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                   int64_t total, PlainGeom g, int include_pad) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % g.ow);
    const int64_t t = e / g.ow;
    const int y = (int)(t % g.oh);
    const float* p = in + (t / g.oh) * g.h * g.w;
    const Cut c = cut_window(y, x, g.h, g.w, g.k, g.s, g.p);
    float sum = 0.0f;
    for (int m = c.ys; m < c.ye; ++m)
      for (int l = c.xs; l < c.xe; ++l) sum += p[(int64_t)m * g.w + l];
    out[e] = sum / (float)(include_pad ? c.D : (c.ye - c.ys) * (c.xe - c.xs));
  }
}

// ---- bordered NHWC buffers [n][h + 2b][w + 2b][c]
struct PadGeom {
  uint32_t in_img, in_row, in_org;  // bytes per image, per physical row, offset of interior pixel (0, 0)
  uint32_t out_img, out_row, out_org;
  uint32_t c, oh, ow;
  int h, w, k, s, p;
  uint32_t iy0, iy1, ix0, ix1;  // the inner output pixels: the whole window inside the image
  uint32_t xout;                // 0x80808080 where the result is stored re-biased, else 0
  uint32_t lo;                  // relu ? zp : 0
  uint32_t zp;
  int include_pad;
};

template <int VEC>
struct Words {
  static constexpr int W = VEC == 16 ? 4 : 1;
};
// an item as dwords of plain bytes
template <int VEC, bool XIN>
__device__ __forceinline__ void load_item(const uint8_t* p, uint32_t (&w)[Words<VEC>::W]) {
  if constexpr (VEC == 16) {
    const uint4 x = *reinterpret_cast<const uint4*>(p);
    w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
  } else if constexpr (VEC == 4) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else {
    w[0] = (uint32_t)*p;
  }
  if constexpr (XIN) {
#pragma unroll
    for (int j = 0; j < Words<VEC>::W; ++j) w[j] ^= (VEC == 1 ? 0x80u : 0x80808080u);
  }
}
template <int VEC>
__device__ __forceinline__ void store_item(uint8_t* p, const uint32_t (&w)[Words<VEC>::W], uint32_t xout) {
  if constexpr (VEC == 16) *reinterpret_cast<uint4*>(p) = make_uint4(w[0] ^ xout, w[1] ^ xout, w[2] ^ xout, w[3] ^ xout);
  else if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(p) = w[0] ^ xout;
  else *p = (uint8_t)((w[0] ^ xout) & 0xFFu);
}

// one lane's place: item v of `items` is (image, output row, output column, channel item)
struct Place {
  uint32_t img, oy, ox, cb;  // cb: the item's first channel, a byte offset
  bool inner;
};
template <int VEC>
__device__ __forceinline__ Place place_of(uint32_t v, const PadGeom& g) {
  const uint32_t per_pix = g.c / VEC;
  const uint32_t pix = v / per_pix, ci = v - pix * per_pix;
  const uint32_t row = pix / g.ow, ox = pix - row * g.ow;
  const uint32_t img = row / g.oh, oy = row - img * g.oh;
  return {img, oy, ox, ci * VEC, oy >= g.iy0 && oy < g.iy1 && ox >= g.ix0 && ox < g.ix1};
}
// the XCD-aware grid walk of maxpool_u8_nhwc_kernel (gridDim.x % 8 == 0): blocks with equal blockIdx % 8 share an L2 and
// sweep one contiguous eighth of the items
struct Sweep {
  uint32_t first, end, step;
};
__device__ __forceinline__ Sweep sweep_of(uint32_t items) {
  const uint32_t slab = ((items + 7) / 8 + 255) / 256 * 256;
  const uint32_t lo = (blockIdx.x & 7) * slab;
  return {lo + (blockIdx.x >> 3) * 256u + threadIdx.x, lo + slab < items ? lo + slab : items, (gridDim.x >> 3) * 256u};
}

// KT: compile-time window size whose inner pixels load their KT * KT taps together (0: none)
template <int VEC, int KT, bool XIN>
__global__ __launch_bounds__(kThreads) void maxpool_u8_nhwc_pad_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                       uint32_t items, PadGeom g) {
  constexpr int W = Words<VEC>::W;
  const BytesEO m0 = spread_eo(g.lo * 0x01010101u);
  const Sweep sw = sweep_of(items);
  for (uint32_t v = sw.first; v < sw.end; v += sw.step) {
    const Place at = place_of<VEC>(v, g);
    const uint8_t* pi = in + (at.img * g.in_img + g.in_org + at.cb);
    const int y0 = (int)at.oy * g.s - g.p, x0 = (int)at.ox * g.s - g.p;
    BytesEO m[W];
#pragma unroll
    for (int j = 0; j < W; ++j) m[j] = m0;
    if (KT > 0 && at.inner) {
      const uint8_t* p = pi + ((uint32_t)y0 * g.in_row + (uint32_t)x0 * g.c);
      uint32_t t[KT > 0 ? KT * KT : 1][W];
#pragma unroll
      for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b) load_item<VEC, XIN>(p + ((uint32_t)a * g.in_row + (uint32_t)b * g.c), t[a * KT + b]);
#pragma unroll
      for (int i = 0; i < KT * KT; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j) max_eo(m[j], t[i][j]);
    } else {
      const int ys = max(y0, 0), ye = min(y0 + g.k, g.h), xs = max(x0, 0), xe = min(x0 + g.k, g.w);
      for (int a = ys; a < ye; ++a) {
        const uint8_t* pr = pi + (uint32_t)a * g.in_row;
        for (int b = xs; b < xe; ++b) {
          uint32_t t[W];
          load_item<VEC, XIN>(pr + (uint32_t)b * g.c, t);
#pragma unroll
          for (int j = 0; j < W; ++j) max_eo(m[j], t[j]);
        }
      }
    }
    uint32_t r[W];
#pragma unroll
    for (int j = 0; j < W; ++j) r[j] = pack_eo(m[j]);
    store_item<VEC>(out + (at.img * g.out_img + g.out_org + at.oy * g.out_row + at.ox * g.c + at.cb), r, g.xout);
  }
}

// the sums of one item: packed 16-bit halves per dword (bytes 0 and 2 in `even`, 1 and 3 in `odd`), or 32 bits per byte
template <int W, bool WIDE>
struct Sums {
  uint32_t a[WIDE ? 4 * W : 2 * W];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < (WIDE ? 4 * W : 2 * W); ++i) a[i] = 0;
  }
  __device__ __forceinline__ void add(const uint32_t (&w)[W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if constexpr (WIDE) {
#pragma unroll
        for (int b = 0; b < 4; ++b) a[4 * j + b] += (w[j] >> (8 * b)) & 0xFFu;
      } else {
        a[2 * j] += w[j] & 0x00FF00FFu;
        a[2 * j + 1] += (w[j] >> 8) & 0x00FF00FFu;
      }
    }
  }
  __device__ __forceinline__ uint32_t byte_sum(int j, int b) const {
    if constexpr (WIDE) return a[4 * j + b];
    const uint32_t half = a[2 * j + (b & 1)];
    return (b & 2) ? half >> 16 : half & 0xFFFFu;
  }
};

template <int VEC, int KT, bool WIDE, bool XIN>
__global__ __launch_bounds__(kThreads) void avgpool_u8_nhwc_pad_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                       uint32_t items, PadGeom g, DivParams full) {
  constexpr int W = Words<VEC>::W;
  const Sweep sw = sweep_of(items);
  for (uint32_t v = sw.first; v < sw.end; v += sw.step) {
    const Place at = place_of<VEC>(v, g);
    const uint8_t* pi = in + (at.img * g.in_img + g.in_org + at.cb);
    const int y0 = (int)at.oy * g.s - g.p, x0 = (int)at.ox * g.s - g.p;
    Sums<W, WIDE> sum;
    sum.clear();
    DivParams d = full;
    uint32_t extra = 0;  // (D - n_valid) * zp: the padded taps
    if (KT > 0 && at.inner) {
      const uint8_t* p = pi + ((uint32_t)y0 * g.in_row + (uint32_t)x0 * g.c);
      uint32_t t[KT > 0 ? KT * KT : 1][W];
#pragma unroll
      for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b) load_item<VEC, XIN>(p + ((uint32_t)a * g.in_row + (uint32_t)b * g.c), t[a * KT + b]);
#pragma unroll
      for (int i = 0; i < KT * KT; ++i) sum.add(t[i]);
    } else {
      const int y1 = min(y0 + g.k, g.h + g.p), x1 = min(x0 + g.k, g.w + g.p);
      const int ys = max(y0, 0), ye = min(y1, g.h), xs = max(x0, 0), xe = min(x1, g.w);
      for (int a = ys; a < ye; ++a) {
        const uint8_t* pr = pi + (uint32_t)a * g.in_row;
        for (int b = xs; b < xe; ++b) {
          uint32_t t[W];
          load_item<VEC, XIN>(pr + (uint32_t)b * g.c, t);
          sum.add(t);
        }
      }
      if (!at.inner) {  // a cut window: its own divisor, through the estimate
        const uint32_t nv = (uint32_t)((ye - ys) * (xe - xs));
        const uint32_t D = g.include_pad ? (uint32_t)((y1 - y0) * (x1 - x0)) : nv;
        extra = (D - nv) * g.zp;
        d.n = D;
        d.rnd = D / 2;
        d.mul = 0;
        d.rinv = 1.0f / (float)D;
      }
    }
    uint32_t r[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      r[j] = 0;
#pragma unroll
      for (int b = 0; b < (VEC == 1 ? 1 : 4); ++b) r[j] |= div_round(sum.byte_sum(j, b) + extra, d, g.lo) << (8 * b);
    }
    store_item<VEC>(out + (at.img * g.out_img + g.out_org + at.oy * g.out_row + at.ox * g.c + at.cb), r, g.xout);
  }
}

inline int pad_grid(int64_t items) {
  int64_t b = (items + kThreads - 1) / kThreads;
  if (b < 1) b = 1;
  if (b > kPadMaxBlocks) b = kPadMaxBlocks;
  return (int)((b + 7) / 8 * 8);
}

template <int VEC, bool XIN>
void launch_max(hipStream_t st, int k, const uint8_t* in, uint8_t* out, uint32_t items, const PadGeom& g) {
  const int grid = pad_grid(items);
  if (k == 3) maxpool_u8_nhwc_pad_kernel<VEC, 3, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g);
  else if (k == 2) maxpool_u8_nhwc_pad_kernel<VEC, 2, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g);
  else maxpool_u8_nhwc_pad_kernel<VEC, 0, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g);
}
template <int VEC, bool XIN>
void launch_avg(hipStream_t st, int k, const uint8_t* in, uint8_t* out, uint32_t items, const PadGeom& g, const DivParams& d) {
  const int grid = pad_grid(items);
  if (k * k > kPackedMax) avgpool_u8_nhwc_pad_kernel<VEC, 0, true, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g, d);
  else if (k == 3) avgpool_u8_nhwc_pad_kernel<VEC, 3, false, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g, d);
  else avgpool_u8_nhwc_pad_kernel<VEC, 0, false, XIN><<<grid, kThreads, 0, st>>>(in, out, items, g, d);
}

// what every entry checks before any device call; on success *oh, *ow hold the output size
int check_geometry(const char* who, int n, int c, int h, int w, int k, int s, int p, int ceil_mode, int* oh, int* ow) {
  if (!(n > 0 && c > 0 && h > 0 && w > 0 && k > 0 && s > 0 && p >= 0)) {
    i8ie_set_error("%s: bad dimension", who);
    return I8IE_ERR_ARG;
  }
  if (p > k / 2) {
    i8ie_set_error("%s: padding larger than half the window", who);
    return I8IE_ERR_ARG;
  }
  if ((int64_t)k > (int64_t)h + 2 * (int64_t)p || (int64_t)k > (int64_t)w + 2 * (int64_t)p) {
    i8ie_set_error("%s: window larger than the padded input", who);
    return I8IE_ERR_ARG;
  }
  if ((int64_t)k * k > kMaxWindow) {
    i8ie_set_error("%s: window of more than 65536 elements", who);
    return I8IE_ERR_ARG;
  }
  *oh = pool_out(h, k, s, p, ceil_mode);
  *ow = pool_out(w, k, s, p, ceil_mode);
  return I8IE_OK;
}

// both NHWC entries: geometry, item width, the split into launches of 32-bit extent
int run_nhwc(i8ie_ctx* ctx, bool avg, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
             int c, int h, int w, int k, int s, int p, int oh, int ow, int include_pad, int relu, uint8_t zp) {
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const int vec = item_width({(int64_t)c}, {in, out});
  const int64_t per_img = (int64_t)oh * ow * (c / vec);
  int64_t imgs_per = 0x7FFFFFFFll / per_img;
  if (0xFFFFFFFFll / gi.img < imgs_per) imgs_per = 0xFFFFFFFFll / gi.img;
  if (0xFFFFFFFFll / go.img < imgs_per) imgs_per = 0xFFFFFFFFll / go.img;
  I8IE_REQUIRE(imgs_per >= 1, "an image with more than 2^31 items");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  PadGeom g;
  g.in_img = (uint32_t)gi.img; g.in_row = (uint32_t)gi.row; g.in_org = (uint32_t)gi.org;
  g.out_img = (uint32_t)go.img; g.out_row = (uint32_t)go.row; g.out_org = (uint32_t)go.org;
  g.c = (uint32_t)c; g.oh = (uint32_t)oh; g.ow = (uint32_t)ow;
  g.h = h; g.w = w; g.k = k; g.s = s; g.p = p;
  // inner pixels: o * s - p >= 0 and o * s - p + k <= in
  g.iy0 = (uint32_t)((p + s - 1) / s); g.ix0 = g.iy0;
  const int fy = h + p - k >= 0 ? (h + p - k) / s + 1 : 0, fx = w + p - k >= 0 ? (w + p - k) / s + 1 : 0;
  g.iy1 = (uint32_t)(fy < oh ? fy : oh);
  g.ix1 = (uint32_t)(fx < ow ? fx : ow);
  g.xout = out_s8 ? 0x80808080u : 0u;
  g.lo = relu ? (uint32_t)zp : 0u;
  g.zp = zp;
  g.include_pad = include_pad;
  const DivParams d = make_div(k * k);
  for (int64_t i0 = 0; i0 < n; i0 += imgs_per) {
    const int64_t nb = n - i0 < imgs_per ? n - i0 : imgs_per;
    const uint32_t items = (uint32_t)(nb * per_img);
    const uint8_t* src = in + i0 * gi.img;
    uint8_t* dst = out + i0 * go.img;
    I8ieProfScope prof(ctx, avg ? "avgpool_u8_nhwc_pad" : "maxpool_u8_nhwc_pad", 0.0, (double)nb * c * h * w + (double)nb * c * oh * ow);
#define I8IE_PADPOOL_LAUNCH(VEC)                                                          \
  do {                                                                                    \
    if (avg) {                                                                            \
      if (in_s8) launch_avg<VEC, true>(ctx->stream, k, src, dst, items, g, d);            \
      else launch_avg<VEC, false>(ctx->stream, k, src, dst, items, g, d);                 \
    } else {                                                                              \
      if (in_s8) launch_max<VEC, true>(ctx->stream, k, src, dst, items, g);               \
      else launch_max<VEC, false>(ctx->stream, k, src, dst, items, g);                    \
    }                                                                                     \
  } while (0)
    if (vec == 16) I8IE_PADPOOL_LAUNCH(16);
    else if (vec == 4) I8IE_PADPOOL_LAUNCH(4);
    else I8IE_PADPOOL_LAUNCH(1);
#undef I8IE_PADPOOL_LAUNCH
    I8IE_LAUNCH_CHECK();
  }
  return I8IE_OK;
}

}  // namespace

extern "C" {

int i8ie_pool_output_size(int in, int kernel_size, int stride, int padding, int ceil_mode) {
  const int o = pool_out(in, kernel_size, stride, padding, ceil_mode);
  if (o < 0) {
    i8ie_set_error("i8ie_pool_output_size: bad geometry (in %d, kernel_size %d, stride %d, padding %d)", in, kernel_size, stride, padding);
    return I8IE_ERR_ARG;
  }
  return o;
}

int i8ie_maxpool2d_u8_pad(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int k, int s, int p,
                          int ceil_mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "maxpool_u8_nchw_pad", 0.0, (double)n * c * h * w + (double)total);
  maxpool_plain_pad_kernel<uint8_t><<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, PlainGeom{h, w, oh, ow, k, s, p},
                                                                                  (uint8_t)0);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_maxpool2d_f32_pad(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int k, int s, int p,
                           int ceil_mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "maxpool_f32_pad", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  maxpool_plain_pad_kernel<float><<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, PlainGeom{h, w, oh, ow, k, s, p},
                                                                                -3.402823466e+38f);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_avgpool2d_u8_pad(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int k, int s, int p,
                          int ceil_mode, int count_include_pad, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "avgpool_u8_nchw_pad", 0.0, (double)n * c * h * w + (double)total);
  avgpool_u8_nchw_pad_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, PlainGeom{h, w, oh, ow, k, s, p},
                                                                           count_include_pad ? 1 : 0, (uint32_t)zero_point);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_avgpool2d_f32_pad(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int k, int s, int p,
                           int ceil_mode, int count_include_pad) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "avgpool_f32_pad", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  avgpool_f32_pad_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, PlainGeom{h, w, oh, ow, k, s, p},
                                                                       count_include_pad ? 1 : 0);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_maxpool2d_u8_nhwc_pad(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8,
                               int n, int c, int h, int w, int k, int s, int p, int ceil_mode, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "bad dimension");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  return run_nhwc(ctx, false, in, in_border, in_s8, out, out_border, out_s8, n, c, h, w, k, s, p, oh, ow, 0, relu, zero_point);
}

int i8ie_avgpool2d_u8_nhwc_pad(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8,
                               int n, int c, int h, int w, int k, int s, int p, int ceil_mode, int count_include_pad, int relu,
                               uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "bad dimension");
  int oh, ow;
  I8IE_TRY(check_geometry(__func__, n, c, h, w, k, s, p, ceil_mode, &oh, &ow));
  return run_nhwc(ctx, true, in, in_border, in_s8, out, out_border, out_s8, n, c, h, w, k, s, p, oh, ow, count_include_pad ? 1 : 0,
                  relu, zero_point);
}

}  // extern "C"
