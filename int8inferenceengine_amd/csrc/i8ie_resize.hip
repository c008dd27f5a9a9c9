// i8ie_resize.hip -- resize to any size and adaptive average pooling: i8ie_resize_axis,
// i8ie_resize2d_u8, i8ie_resize2d_u8_nhwc, i8ie_resize2d_f32, i8ie_adaptive_avgpool2d_u8, i8ie_adaptive_avgpool2d_u8_nhwc,
// i8ie_adaptive_avgpool2d_f32.  The definitions are in include/i8ie_hip.h; i8ie_upsample.hip and i8ie_avgpool.hip stay what
// they were and keep their callers.
//
// Resize.  Per axis (input length L, output length O) an output index o has taps (i0, i1) and weights (w0, w1) of `den`
// (axis_of below, the rule of the header in 64-bit integers).  Bilinear on bytes: D = den_y den_x,
//     S = wx0 (wy0 q[y0, x0] + wy1 q[y1, x0]) + wx1 (wy0 q[y0, x1] + wy1 q[y1, x1]),  out = (S + D / 2) / D.
// The two weights of an axis sum to den and a byte is at most 255, so a column blend is at most 255 den_y, S at most 255 D
// and S + D / 2 <= 255.5 D < 2^30 + 2^21 < 2^31 for D <= 2^22 (the entries refuse a larger D): unsigned 32-bit lanes.
//
// The division by D in the NHWC kernel (never an integer-divide sequence; make_div below).  D a power of two: a shift.
// Otherwise l = ceil(log2 D) (so 2^(l-1) < D < 2^l), M = ceil(2^(31+l) / D) and q = (x M) >> (31 + l), computed as
// mulhi(x, M) >> (l - 1).  M < 2^32 because 2^(31+l) / D < 2^(31+l) / 2^(l-1) = 2^32 and D >= 2^(l-1) + 1 keeps the quotient
// at least 2^(32-l) below 2^32.  With e = M D - 2^(31+l) in [0, D):  x M / 2^(31+l) = x / D + x e / (D 2^(31+l)); the fraction of
// x / D is at most (D - 1) / D, so floor() of the left side is floor(x / D) whenever x e / (D 2^(31+l)) < 1 / D, i.e.
// x e < 2^(31+l): true for every x < 2^31 because e < D < 2^l.  The host checks M < 2^32 and xmax e < 2^(31+l) with the
// actual e and xmax = 255 D + D / 2 all the same, and the test at D = 2^22 - and at the non-powers of two of its cases -
// compares every byte with the direct kernel's rule.  The adaptive pool divides by its window's own n the same way.
//
// resize_u8_nhwc (the hot path): a lane owns one output pixel x one channel item (16 / 4 / 1 channels by c % 16, c % 4;
// buffers off that alignment take the direct kernel).  A block is lanes_c = min(c / VEC, 256) channel items by
// 256 / lanes_c pixels; those pixels are a run of RX = min(256 / lanes_c, ow) pixels of RY = 256 / lanes_c / RX consecutive output rows (RY = 1 unless the
// output is narrower than the block: an 8 x 8 map would otherwise leave most lanes idle).  Per unit the block builds the
// RX x-axis entries (byte offsets of x0 and x1, wx1) and the RY y-axis entries in LDS, one lane per entry: the 64-bit
// multiply and divide of axis_of run once per entry, and no lane computes a coordinate.  A lane's position in the block
// (pixel, channel item) is fixed for the whole kernel and computed once.  The four taps are read with full-width loads at
// the clamped indices of the rule, so an input border byte is never read; each dword is blended byte by byte in 32-bit
// lanes, divided, floored at zp for a folded relu, re-biased for the consumer and stored once.  Nearest is the same kernel
// without the blend (one tap).  Blocks stride over units (grid-stride: correct when units exceed the grid).  32-bit offsets
// inside an image, 64-bit image bases.  LDS: 5 tables of 256 dwords, 5 KiB; no scratch, no device allocation.
//
// adaptive_avgpool_u8_nhwc: the same block shape and LDS tables, holding each output column's first input column (as a
// byte offset) and window width, each row's first input row and window height.  A lane walks its own window and adds the
// bytes of a dword in packed 16-bit halves (as i8ie_avgpool.hip's windowed kernel); that needs 255 n + n / 2 < 2^16, so
// this kernel takes the shapes whose largest window has at most 256 elements, and the direct kernel -- 32-bit sums -- the
// rest.  An axis has at most two distinct window lengths (L = q O + r: q when r == 0, else q + 1 and q + 2), so the
// multipliers of the at most four distinct n are a 2 x 2 table in LDS indexed by (window_h - min_h, window_w - min_w).
//
// resize_u8_direct / adaptive_avgpool_u8_direct: the definitions verbatim, one lane per output byte, plain integer
// division, any strides: the flat NCHW entries; the NHWC entries where a buffer is not aligned to the item width c allows
// (the engine's own buffers always are) and under I8IE_OPT_FORCE_FALLBACK; the pool for windows of more than 256 elements.
// Same bytes.  The FP32 kernels: NCHW, one lane per output value.
#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr uint32_t kMaxD = 1u << 22;
constexpr int kMaxWindow = 65536;  // as i8ie_avgpool2d_u8
constexpr int kPackedWindow = 256;  // 255 n + n / 2 < 2^16

// ---- the axis rule (header), host and device
struct Ax {
  int32_t i0, i1;
  uint32_t w1, den;  // w0 = den - w1
};
__host__ __device__ __forceinline__ Ax axis_of(int64_t L, int64_t O, int mode, int64_t o) {
  Ax a;
  int64_t num, den;
  if (mode == I8IE_RESIZE_NEAREST) {
    a.i0 = a.i1 = (int32_t)((o * L) / O);
    a.w1 = 0;
    a.den = 1;
    return a;
  }
  if (mode == I8IE_RESIZE_BILINEAR) {
    den = 2 * O;
    num = (2 * o + 1) * L - O;
    if (num < 0) num = 0;
  } else {
    den = O > 1 ? O - 1 : 1;
    num = O > 1 ? o * (L - 1) : 0;
  }
  const int64_t i0 = num / den;
  a.i0 = (int32_t)i0;
  a.w1 = (uint32_t)(num - i0 * den);
  a.den = (uint32_t)den;
  a.i1 = (int32_t)(i0 + 1 < L ? i0 + 1 : L - 1);
  return a;
}
__host__ __device__ __forceinline__ uint32_t axis_den(int64_t O, int mode) {
  return mode == I8IE_RESIZE_NEAREST ? 1u : (mode == I8IE_RESIZE_BILINEAR ? (uint32_t)(2 * O) : (uint32_t)(O > 1 ? O - 1 : 1));
}
// the window of output i of an adaptive pool axis: [floor(i L / O), ceil((i + 1) L / O))
__host__ __device__ __forceinline__ void window_of(int64_t L, int64_t O, int64_t i, int32_t* start, int32_t* len) {
  const int64_t s = (i * L) / O, e = ((i + 1) * L + O - 1) / O;
  *start = (int32_t)s;
  *len = (int32_t)(e - s);
}

// ---- the division (header)
struct Div {
  uint32_t rnd;    // D / 2
  uint32_t mul;    // 0: D is a power of two
  uint32_t shift;  // log2 D, or l - 1 behind the multiply
};
bool make_div(uint32_t D, Div* d) {
  d->rnd = D / 2;
  d->mul = 0;
  d->shift = 0;
  if ((D & (D - 1)) == 0) {
    while ((1u << d->shift) < D) ++d->shift;
    return true;
  }
  uint32_t l = 0;
  while ((1ull << l) < D) ++l;
  const uint64_t two = 1ull << (31 + l), M = (two + D - 1) / D, e = M * D - two, xmax = 255ull * D + D / 2;
  if (M >= (1ull << 32) || xmax >= (1ull << 31) || xmax * e >= two) return false;
  d->mul = (uint32_t)M;
  d->shift = l - 1;
  return true;
}
__device__ __forceinline__ uint32_t div_round(uint32_t S, uint32_t rnd, uint32_t mul, uint32_t shift) {
  const uint32_t x = S + rnd;
  return (mul ? __umulhi(x, mul) : x) >> shift;
}

// ---- the direct kernels: one lane per output byte, any strides
struct DirGeom {
  int64_t in_img, in_c, in_row, in_px, in_org;  // bytes (elements): per image, channel, row, pixel; interior origin
  int64_t out_img, out_c, out_row, out_px, out_org;
  int c, h, w, oh, ow;
  int c_fastest;  // the order in which lanes walk the outputs: NHWC (1) or NCHW (0)
  int mode;
  uint32_t xin, xout, lo;  // 0x80 where that buffer holds re-biased bytes; relu ? zp : 0
};
struct DirAt {
  int64_t in_base, out_at;
  int y, x;
};
__device__ __forceinline__ DirAt dir_at(int64_t e, const DirGeom& g) {
  int ch, x, y;
  int64_t img;
  if (g.c_fastest) {
    ch = (int)(e % g.c);
    int64_t t = e / g.c;
    x = (int)(t % g.ow);
    t /= g.ow;
    y = (int)(t % g.oh);
    img = t / g.oh;
  } else {
    x = (int)(e % g.ow);
    int64_t t = e / g.ow;
    y = (int)(t % g.oh);
    t /= g.oh;
    ch = (int)(t % g.c);
    img = t / g.c;
  }
  return {img * g.in_img + g.in_org + ch * g.in_c, img * g.out_img + g.out_org + ch * g.out_c + y * g.out_row + x * g.out_px, y, x};
}

__global__ __launch_bounds__(kThreads) void resize_u8_direct_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t total,
                                                                    DirGeom g) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const DirAt at = dir_at(e, g);
    const uint8_t* p = in + at.in_base;
    const Ax ty = axis_of(g.h, g.oh, g.mode, at.y), tx = axis_of(g.w, g.ow, g.mode, at.x);
    const uint32_t q00 = p[ty.i0 * g.in_row + tx.i0 * g.in_px] ^ g.xin;
    uint32_t q = q00;
    if (g.mode != I8IE_RESIZE_NEAREST) {
      const uint32_t q10 = p[ty.i1 * g.in_row + tx.i0 * g.in_px] ^ g.xin, q01 = p[ty.i0 * g.in_row + tx.i1 * g.in_px] ^ g.xin;
      const uint32_t q11 = p[ty.i1 * g.in_row + tx.i1 * g.in_px] ^ g.xin;
      const uint32_t wy1 = ty.w1, wy0 = ty.den - wy1, wx1 = tx.w1, wx0 = tx.den - wx1, D = ty.den * tx.den;
      const uint32_t S = wx0 * (wy0 * q00 + wy1 * q10) + wx1 * (wy0 * q01 + wy1 * q11);
      q = (S + D / 2) / D;
    }
    q = q > g.lo ? q : g.lo;
    out[at.out_at] = (uint8_t)(q ^ g.xout);
  }
}

__global__ __launch_bounds__(kThreads) void adaptive_avgpool_u8_direct_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                              int64_t total, DirGeom g) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const DirAt at = dir_at(e, g);
    int32_t ys, yl, xs, xl;
    window_of(g.h, g.oh, at.y, &ys, &yl);
    window_of(g.w, g.ow, at.x, &xs, &xl);
    const uint8_t* p = in + at.in_base + ys * g.in_row + xs * g.in_px;
    uint32_t S = 0;
    for (int m = 0; m < yl; ++m)
      for (int l = 0; l < xl; ++l) S += p[m * g.in_row + l * g.in_px] ^ g.xin;
    const uint32_t n = (uint32_t)(yl * xl);
    uint32_t q = (S + n / 2) / n;
    q = q > g.lo ? q : g.lo;
    out[at.out_at] = (uint8_t)(q ^ g.xout);
  }
}

// ---- FP32, NCHW: one lane per output value
__global__ __launch_bounds__(kThreads) void resize_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total, int h, int w,
                                                              int oh, int ow, int mode) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    const float* p = in + (t / oh) * h * w;
    const Ax ty = axis_of(h, oh, mode, y), tx = axis_of(w, ow, mode, x);
    if (mode == I8IE_RESIZE_NEAREST) {
      out[e] = p[(int64_t)ty.i0 * w + tx.i0];
      continue;
    }
    const float ly = (float)ty.w1 / (float)ty.den, lx = (float)tx.w1 / (float)tx.den;
    const float my = 1.0f - ly, mx = 1.0f - lx;
    const float top = p[(int64_t)ty.i0 * w + tx.i0] * mx + p[(int64_t)ty.i0 * w + tx.i1] * lx;
    const float bot = p[(int64_t)ty.i1 * w + tx.i0] * mx + p[(int64_t)ty.i1 * w + tx.i1] * lx;
    out[e] = top * my + bot * ly;
  }
}

__global__ __launch_bounds__(kThreads) void adaptive_avgpool_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total,
                                                                        int h, int w, int oh, int ow) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    int32_t ys, yl, xs, xl;
    window_of(h, oh, y, &ys, &yl);
    window_of(w, ow, x, &xs, &xl);
    const float* p = in + (t / oh) * h * w + (int64_t)ys * w + xs;
    float sum = 0.0f;
    for (int m = 0; m < yl; ++m)
      for (int l = 0; l < xl; ++l) sum += p[(int64_t)m * w + l];
    out[e] = sum / (float)(yl * xl);
  }
}

// ---- bordered NHWC buffers [n][h + 2b][w + 2b][c] -> [n][oh + 2b'][ow + 2b'][c]: the block shape both hot kernels share
struct TileGeom {
  int64_t in_img, out_img;              // bytes per image
  uint32_t in_row, in_org;              // bytes per physical row, offset of interior pixel (0, 0)
  uint32_t out_row, out_org;
  uint32_t c, h, w, oh, ow;
  uint32_t per_pix, lanes_c;            // channel items per pixel; of them side by side in a block
  uint32_t rx, ry;                      // a block's pixels: rx of one row by ry rows (header)
  uint32_t runs, groups;                // ceil(ow / rx), ceil(oh / ry)
  uint32_t xin, xout, lo;               // 0x80808080 where that buffer holds re-biased bytes; relu ? zp : 0
  int mode;
};
int64_t tile_init(TileGeom& g, int vec, int n, int c, int h, int w, int oh, int ow, int in_border, int out_border, int in_s8, int out_s8,
                  int relu, int zp) {
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  g.in_img = gi.img; g.in_row = (uint32_t)gi.row; g.in_org = (uint32_t)gi.org;
  g.out_img = go.img; g.out_row = (uint32_t)go.row; g.out_org = (uint32_t)go.org;
  g.c = (uint32_t)c; g.h = (uint32_t)h; g.w = (uint32_t)w; g.oh = (uint32_t)oh; g.ow = (uint32_t)ow;
  g.per_pix = (uint32_t)(c / vec);
  g.lanes_c = g.per_pix < (uint32_t)kThreads ? g.per_pix : (uint32_t)kThreads;
  const uint32_t pixels = (uint32_t)kThreads / g.lanes_c;
  g.rx = pixels < g.ow ? pixels : g.ow;
  g.ry = pixels / g.rx < g.oh ? pixels / g.rx : g.oh;
  g.runs = (g.ow + g.rx - 1) / g.rx;
  g.groups = (g.oh + g.ry - 1) / g.ry;
  g.xin = in_s8 ? 0x80808080u : 0u;
  g.xout = out_s8 ? 0x80808080u : 0u;
  g.lo = relu ? (uint32_t)zp : 0u;
  g.mode = 0;
  return (int64_t)n * g.groups * g.runs;  // units
}
// a lane's place in its block, fixed for the whole kernel
struct LanePlace {
  uint32_t lx, ly, cl;
  bool on;
};
__device__ __forceinline__ LanePlace lane_place(const TileGeom& g) {
  const uint32_t p = threadIdx.x / g.lanes_c, cl = threadIdx.x - p * g.lanes_c;
  const uint32_t ly = p / g.rx, lx = p - ly * g.rx;
  return {lx, ly, cl, ly < g.ry};
}
// a unit of the grid-stride walk: image, first output row, first output column (block-uniform)
struct UnitAt {
  uint32_t img, y0, x0;
};
__device__ __forceinline__ UnitAt unit_at(uint32_t u, const TileGeom& g) {
  const uint32_t t = u / g.runs, run = u - t * g.runs;
  const uint32_t img = t / g.groups, grp = t - img * g.groups;
  return {img, grp * g.ry, run * g.rx};
}

template <int VEC>
__device__ __forceinline__ void load_dwords(const uint8_t* p, uint32_t xin, uint32_t (&x)[VEC == 16 ? 4 : 1]) {
  if constexpr (VEC == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    x[0] = v.x ^ xin;
    x[1] = v.y ^ xin;
    x[2] = v.z ^ xin;
    x[3] = v.w ^ xin;
  } else if constexpr (VEC == 4) {
    x[0] = *reinterpret_cast<const uint32_t*>(p) ^ xin;
  } else {
    x[0] = (uint32_t)*p ^ (xin & 0xFFu);  // (the upper three bytes are zero lanes: what they become is not stored)
  }
}
template <int VEC>
__device__ __forceinline__ void store_dwords(uint8_t* p, const uint32_t (&x)[VEC == 16 ? 4 : 1]) {
  if constexpr (VEC == 16) *reinterpret_cast<uint4*>(p) = make_uint4(x[0], x[1], x[2], x[3]);
  else if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(p) = x[0];
  else *p = (uint8_t)x[0];
}

template <int VEC, bool BLEND>
__global__ __launch_bounds__(kThreads) void resize_u8_nhwc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t units,
                                                                  TileGeom g, Div d) {
  constexpr int NDW = VEC == 16 ? 4 : 1;
  __shared__ uint32_t sx0[kThreads], sx1[kThreads], sxw[kThreads];  // per column of the run: byte offsets of x0, x1; wx1
  __shared__ uint32_t sy0[kThreads], sy1[kThreads], syw[kThreads];  // per row of the group: byte offsets of y0, y1; wy1
  const LanePlace me = lane_place(g);
  const uint32_t tid = threadIdx.x;
  const uint32_t den_y = axis_den(g.oh, g.mode), den_x = axis_den(g.ow, g.mode);
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
    const UnitAt at = unit_at(u, g);
    __syncthreads();  // the tables of the unit before are no longer read
    if (tid < g.rx && at.x0 + tid < g.ow) {
      const Ax a = axis_of(g.w, g.ow, g.mode, at.x0 + tid);
      sx0[tid] = (uint32_t)a.i0 * g.c;
      sx1[tid] = (uint32_t)a.i1 * g.c;
      sxw[tid] = a.w1;
    }
    if (tid < g.ry && at.y0 + tid < g.oh) {
      const Ax a = axis_of(g.h, g.oh, g.mode, at.y0 + tid);
      sy0[tid] = (uint32_t)a.i0 * g.in_row;
      sy1[tid] = (uint32_t)a.i1 * g.in_row;
      syw[tid] = a.w1;
    }
    __syncthreads();
    const uint32_t oy = at.y0 + me.ly, ox = at.x0 + me.lx;
    if (!me.on || oy >= g.oh || ox >= g.ow) continue;  // (the barriers above are reached by every lane: the loop is block-uniform)
    const uint8_t* const pi = in + ((int64_t)at.img * g.in_img + g.in_org);
    uint8_t* const po = out + ((int64_t)at.img * g.out_img + g.out_org + oy * g.out_row + ox * g.c);
    const uint32_t y0 = sy0[me.ly], y1 = sy1[me.ly], x0 = sx0[me.lx], x1 = sx1[me.lx];
    const uint32_t wy1 = syw[me.ly], wy0 = den_y - wy1, wx1 = sxw[me.lx], wx0 = den_x - wx1;
    for (uint32_t ci = me.cl; ci < g.per_pix; ci += g.lanes_c) {
      const uint32_t co = ci * VEC;
      uint32_t r[NDW];
      if constexpr (BLEND) {
        uint32_t a[NDW], b[NDW], e[NDW], f[NDW];
        load_dwords<VEC>(pi + y0 + x0 + co, g.xin, a);
        load_dwords<VEC>(pi + y1 + x0 + co, g.xin, b);
        load_dwords<VEC>(pi + y0 + x1 + co, g.xin, e);
        load_dwords<VEC>(pi + y1 + x1 + co, g.xin, f);
#pragma unroll
        for (int j = 0; j < NDW; ++j) {
          uint32_t word = 0;
#pragma unroll
          for (int k = 0; k < 32; k += 8) {
            const uint32_t c0 = wy0 * ((a[j] >> k) & 0xFFu) + wy1 * ((b[j] >> k) & 0xFFu);
            const uint32_t c1 = wy0 * ((e[j] >> k) & 0xFFu) + wy1 * ((f[j] >> k) & 0xFFu);
            uint32_t q = div_round(wx0 * c0 + wx1 * c1, d.rnd, d.mul, d.shift);
            q = q > g.lo ? q : g.lo;
            word |= q << k;
          }
          r[j] = word ^ g.xout;
        }
      } else {
        uint32_t a[NDW];
        load_dwords<VEC>(pi + y0 + x0 + co, g.xin, a);
#pragma unroll
        for (int j = 0; j < NDW; ++j) {
          uint32_t word = 0;
#pragma unroll
          for (int k = 0; k < 32; k += 8) {
            const uint32_t q = (a[j] >> k) & 0xFFu;
            word |= (q > g.lo ? q : g.lo) << k;
          }
          r[j] = word ^ g.xout;
        }
      }
      store_dwords<VEC>(po + co, r);
    }
  }
}

// the divisors of the at most four distinct window sizes (header): [window_h - min_h][window_w - min_w]
struct PoolDivs {
  uint32_t min_h, min_w;
  Div d[4];
};

template <int VEC>
__global__ __launch_bounds__(kThreads) void adaptive_avgpool_u8_nhwc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                            uint32_t units, TileGeom g, PoolDivs pd) {
  constexpr int NDW = VEC == 16 ? 4 : 1;
  __shared__ uint32_t sxs[kThreads], sxl[kThreads];  // per column of the run: byte offset of the window's first column; its width
  __shared__ uint32_t sys[kThreads], syl[kThreads];  // per row of the group: byte offset of the window's first row; its height
  __shared__ uint32_t srnd[4], smul[4], sshift[4];
  const LanePlace me = lane_place(g);
  const uint32_t tid = threadIdx.x;
  if (tid < 4) {
    srnd[tid] = pd.d[tid].rnd;
    smul[tid] = pd.d[tid].mul;
    sshift[tid] = pd.d[tid].shift;
  }
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
    const UnitAt at = unit_at(u, g);
    __syncthreads();  // the tables of the unit before are no longer read (and, the first time, the divisors are in place)
    if (tid < g.rx && at.x0 + tid < g.ow) {
      int32_t s, l;
      window_of(g.w, g.ow, at.x0 + tid, &s, &l);
      sxs[tid] = (uint32_t)s * g.c;
      sxl[tid] = (uint32_t)l;
    }
    if (tid < g.ry && at.y0 + tid < g.oh) {
      int32_t s, l;
      window_of(g.h, g.oh, at.y0 + tid, &s, &l);
      sys[tid] = (uint32_t)s * g.in_row;
      syl[tid] = (uint32_t)l;
    }
    __syncthreads();
    const uint32_t oy = at.y0 + me.ly, ox = at.x0 + me.lx;
    if (!me.on || oy >= g.oh || ox >= g.ow) continue;
    const uint32_t wh = syl[me.ly], ww = sxl[me.lx];
    const uint32_t which = (wh - pd.min_h) * 2 + (ww - pd.min_w);
    const uint32_t rnd = srnd[which], mul = smul[which], shift = sshift[which];
    const uint8_t* const pw = in + ((int64_t)at.img * g.in_img + g.in_org + sys[me.ly] + sxs[me.lx]);
    uint8_t* const po = out + ((int64_t)at.img * g.out_img + g.out_org + oy * g.out_row + ox * g.c);
    for (uint32_t ci = me.cl; ci < g.per_pix; ci += g.lanes_c) {
      const uint32_t co = ci * VEC;
      uint32_t ev[NDW], od[NDW];  // two packed 16-bit sums each: bytes 0 and 2 of a dword, bytes 1 and 3
#pragma unroll
      for (int j = 0; j < NDW; ++j) ev[j] = od[j] = 0;
      for (uint32_t m = 0; m < wh; ++m) {
        const uint8_t* pr = pw + m * g.in_row + co;
        for (uint32_t l = 0; l < ww; ++l) {
          uint32_t x[NDW];
          load_dwords<VEC>(pr + l * g.c, g.xin, x);
#pragma unroll
          for (int j = 0; j < NDW; ++j) {
            ev[j] += x[j] & 0x00FF00FFu;
            od[j] += (x[j] >> 8) & 0x00FF00FFu;
          }
        }
      }
      uint32_t r[NDW];
#pragma unroll
      for (int j = 0; j < NDW; ++j) {
        const uint32_t s4[4] = {ev[j] & 0xFFFFu, od[j] & 0xFFFFu, ev[j] >> 16, od[j] >> 16};
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t q = div_round(s4[k], rnd, mul, shift);
          word |= (q > g.lo ? q : g.lo) << (8 * k);
        }
        r[j] = word ^ g.xout;
      }
      store_dwords<VEC>(po + co, r);
    }
  }
}

int units_grid(int64_t units) { return (int)(units > kMaxBlocks ? kMaxBlocks : units); }

bool dims_ok(int n, int c, int h, int w, int oh, int ow) { return n > 0 && c > 0 && h > 0 && w > 0 && oh > 0 && ow > 0; }
bool mode_ok(int mode) { return mode == I8IE_RESIZE_NEAREST || mode == I8IE_RESIZE_BILINEAR || mode == I8IE_RESIZE_BILINEAR_ALIGNED; }
// den_y * den_x <= 2^22 (header); the nearest copy has no D
bool d_ok(int oh, int ow, int mode) {
  if (mode == I8IE_RESIZE_NEAREST) return true;
  const int64_t dy = mode == I8IE_RESIZE_BILINEAR ? 2 * (int64_t)oh : (oh > 1 ? oh - 1 : 1);
  const int64_t dx = mode == I8IE_RESIZE_BILINEAR ? 2 * (int64_t)ow : (ow > 1 ? ow - 1 : 1);
  return dy * dx <= (int64_t)kMaxD;
}
// the smallest and the largest window length of an adaptive pool axis (header: at most two lengths, one apart)
void window_range(int L, int O, int* lo, int* hi) {
  const int q = L / O, r = L % O;
  *lo = r == 0 ? q : q + 1;
  *hi = *lo;
  for (int i = 0; i < O && *hi == *lo; ++i) {
    int32_t s, l;
    window_of(L, O, i, &s, &l);
    if (l > *hi) *hi = l;
  }
}

DirGeom dir_nchw(int c, int h, int w, int oh, int ow, int mode) {
  DirGeom g;
  g.in_img = (int64_t)c * h * w; g.in_c = (int64_t)h * w; g.in_row = w; g.in_px = 1; g.in_org = 0;
  g.out_img = (int64_t)c * oh * ow; g.out_c = (int64_t)oh * ow; g.out_row = ow; g.out_px = 1; g.out_org = 0;
  g.c = c; g.h = h; g.w = w; g.oh = oh; g.ow = ow;
  g.c_fastest = 0;
  g.mode = mode;
  g.xin = g.xout = g.lo = 0;
  return g;
}
DirGeom dir_nhwc(int c, int h, int w, int oh, int ow, int in_border, int out_border, int in_s8, int out_s8, int relu, int zp, int mode) {
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  DirGeom g;
  g.in_img = gi.img; g.in_c = 1; g.in_row = gi.row; g.in_px = c; g.in_org = gi.org;
  g.out_img = go.img; g.out_c = 1; g.out_row = go.row; g.out_px = c; g.out_org = go.org;
  g.c = c; g.h = h; g.w = w; g.oh = oh; g.ow = ow;
  g.c_fastest = 1;
  g.mode = mode;
  g.xin = in_s8 ? 0x80u : 0u;
  g.xout = out_s8 ? 0x80u : 0u;
  g.lo = relu ? (uint32_t)zp : 0u;
  return g;
}

}  // namespace

extern "C" {

int i8ie_resize_axis(int in_len, int out_len, int mode, int out_index, int* i0, int* i1, int* w0, int* w1, int* den) {
  I8IE_REQUIRE(i0 && i1 && w0 && w1 && den, "null argument");
  I8IE_REQUIRE(in_len > 0 && out_len > 0 && out_len <= (1 << 30), "bad length");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE(out_index >= 0 && out_index < out_len, "output index outside the axis");
  const Ax a = axis_of(in_len, out_len, mode, out_index);
  *i0 = a.i0;
  *i1 = a.i1;
  *w1 = (int)a.w1;
  *w0 = (int)(a.den - a.w1);
  *den = (int)a.den;
  return I8IE_OK;
}

int i8ie_resize2d_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int oh, int ow, int mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow), "bad dimension");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE(d_ok(oh, ow, mode), "den_y * den_x above 2^22");
  I8IE_REQUIRE((int64_t)h * w <= 0x7FFFFFFF && (int64_t)oh * ow <= 0x7FFFFFFF, "a plane of more than 2^31 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "resize_u8_direct", 0.0, (double)n * c * h * w + (double)total);
  resize_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, dir_nchw(c, h, w, oh, ow, mode));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_resize2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n, int c,
                          int h, int w, int oh, int ow, int mode, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow) && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE(d_ok(oh, ow, mode), "den_y * den_x above 2^22");
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const int vec = item_width({c}, {});
  const bool direct = (ctx->options & 1u) != 0 || item_width({c}, {in, out}) != vec;  // forced, or a buffer off the item's alignment
  TileGeom g;
  const int64_t units = tile_init(g, vec, n, c, h, w, oh, ow, in_border, out_border, in_s8, out_s8, relu, zero_point);
  g.mode = mode;
  I8IE_REQUIRE(units <= 0x7FFFFFFF, "too many outputs for one launch");
  Div d;
  I8IE_REQUIRE(make_div(axis_den(oh, mode) * axis_den(ow, mode), &d), "no exact division for this size");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const double bytes = (double)n * c * ((double)h * w + (double)oh * ow);
  if (direct) {
    const int64_t total = (int64_t)n * c * oh * ow;
    I8ieProfScope prof(ctx, "resize_u8_direct", 0.0, bytes);
    resize_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(
        in, out, total, dir_nhwc(c, h, w, oh, ow, in_border, out_border, in_s8, out_s8, relu, zero_point, mode));
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  I8ieProfScope prof(ctx, "resize_u8_nhwc", 0.0, bytes);
  const int grid = units_grid(units);
  const bool blend = mode != I8IE_RESIZE_NEAREST;
#define I8IE_RESIZE_LAUNCH(V)                                                                                              \
  do {                                                                                                                     \
    if (blend) resize_u8_nhwc_kernel<V, true><<<grid, kThreads, 0, ctx->stream>>>(in, out, (uint32_t)units, g, d);         \
    else resize_u8_nhwc_kernel<V, false><<<grid, kThreads, 0, ctx->stream>>>(in, out, (uint32_t)units, g, d);              \
  } while (0)
  if (vec == 16) I8IE_RESIZE_LAUNCH(16);
  else if (vec == 4) I8IE_RESIZE_LAUNCH(4);
  else I8IE_RESIZE_LAUNCH(1);
#undef I8IE_RESIZE_LAUNCH
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_resize2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int oh, int ow, int mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow), "bad dimension");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE(d_ok(oh, ow, mode), "den_y * den_x above 2^22");
  I8IE_REQUIRE((int64_t)h * w <= 0x7FFFFFFF && (int64_t)oh * ow <= 0x7FFFFFFF, "a plane of more than 2^31 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "resize_f32", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  resize_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, oh, ow, mode);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_adaptive_avgpool2d_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int oh, int ow) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow), "bad dimension");
  int lo_h, hi_h, lo_w, hi_w;
  window_range(h, oh, &lo_h, &hi_h);
  window_range(w, ow, &lo_w, &hi_w);
  I8IE_REQUIRE((int64_t)hi_h * hi_w <= kMaxWindow, "window of more than 65536 elements");
  I8IE_REQUIRE((int64_t)h * w <= 0x7FFFFFFF && (int64_t)oh * ow <= 0x7FFFFFFF, "a plane of more than 2^31 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "adaptive_avgpool_u8_direct", 0.0, (double)n * c * h * w + (double)total);
  adaptive_avgpool_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, dir_nchw(c, h, w, oh, ow, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_adaptive_avgpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8,
                                    int n, int c, int h, int w, int oh, int ow, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow) && in_border >= 0 && out_border >= 0, "bad dimension");
  int lo_h, hi_h, lo_w, hi_w;
  window_range(h, oh, &lo_h, &hi_h);
  window_range(w, ow, &lo_w, &hi_w);
  I8IE_REQUIRE((int64_t)hi_h * hi_w <= kMaxWindow, "window of more than 65536 elements");
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const int vec = item_width({c}, {});
  const bool direct = (ctx->options & 1u) != 0 || item_width({c}, {in, out}) != vec || hi_h * hi_w > kPackedWindow;
  TileGeom g;
  const int64_t units = tile_init(g, vec, n, c, h, w, oh, ow, in_border, out_border, in_s8, out_s8, relu, zero_point);
  I8IE_REQUIRE(units <= 0x7FFFFFFF, "too many outputs for one launch");
  PoolDivs pd;
  pd.min_h = (uint32_t)lo_h;
  pd.min_w = (uint32_t)lo_w;
  bool exact = true;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) exact = make_div((uint32_t)((lo_h + a) * (lo_w + b)), &pd.d[a * 2 + b]) && exact;
  I8IE_REQUIRE(exact, "no exact division for this window");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const double bytes = (double)n * c * ((double)h * w + (double)oh * ow);
  if (direct) {
    const int64_t total = (int64_t)n * c * oh * ow;
    I8ieProfScope prof(ctx, "adaptive_avgpool_u8_direct", 0.0, bytes);
    adaptive_avgpool_u8_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(
        in, out, total, dir_nhwc(c, h, w, oh, ow, in_border, out_border, in_s8, out_s8, relu, zero_point, 0));
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  I8ieProfScope prof(ctx, "adaptive_avgpool_u8_nhwc", 0.0, bytes);
  const int grid = units_grid(units);
  if (vec == 16) adaptive_avgpool_u8_nhwc_kernel<16><<<grid, kThreads, 0, ctx->stream>>>(in, out, (uint32_t)units, g, pd);
  else if (vec == 4) adaptive_avgpool_u8_nhwc_kernel<4><<<grid, kThreads, 0, ctx->stream>>>(in, out, (uint32_t)units, g, pd);
  else adaptive_avgpool_u8_nhwc_kernel<1><<<grid, kThreads, 0, ctx->stream>>>(in, out, (uint32_t)units, g, pd);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_adaptive_avgpool2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int oh, int ow) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(dims_ok(n, c, h, w, oh, ow), "bad dimension");
  int lo_h, hi_h, lo_w, hi_w;
  window_range(h, oh, &lo_h, &hi_h);
  window_range(w, ow, &lo_w, &hi_w);
  I8IE_REQUIRE((int64_t)hi_h * hi_w <= kMaxWindow, "window of more than 65536 elements");
  I8IE_REQUIRE((int64_t)h * w <= 0x7FFFFFFF && (int64_t)oh * ow <= 0x7FFFFFFF, "a plane of more than 2^31 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * oh * ow;
  I8ieProfScope prof(ctx, "adaptive_avgpool_f32", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  adaptive_avgpool_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, oh, ow);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
