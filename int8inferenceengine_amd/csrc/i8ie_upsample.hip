// i8ie_upsample.hip -- quantized upsampling by integer factors: i8ie_upsample2d_u8,
// i8ie_upsample2d_u8_nhwc, i8ie_upsample2d_f32.
//
// The reference has no resize op.  Like its max_pool2d<u8_t> (src/functional.cc:36-64) the op works on the NCHW logical
// shape and the result carries the input's (scale, zero_point) unchanged.  [n, c, h, w] -> [n, c, h fh, w fw], fh and fw
// integers in 1..8.
//
// Nearest: out[y, x] = in[y / fh, x / fw], a byte copy.
//
// Bilinear (torch's align_corners=False), along one axis of length L with factor f: output index o = f i + r, t = 2 r + 1 - f;
//     t >= 0:  i0 = i,      w1 = t
//     t <  0:  i0 = i - 1,  w1 = 2 f + t
//     i0 < 0:  i0 = 0,      w1 = 0
//     i1 = min(i0 + 1, L - 1),  w0 = 2 f - w1
// and with (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) from that rule, D = 4 fh fw and
//     S = wx0 (wy0 q[y0, x0] + wy1 q[y1, x0]) + wx1 (wy0 q[y0, x1] + wy1 q[y1, x1])
//     out = (S + D / 2) / D          integer floor division: round to nearest, ties up (the rule of i8ie_avgpool2d_u8)
//     out = relu ? max(out, zp) : out
// The value never leaves the integers.  Both rules of the edge (i0 < 0 and the min) say "the neighbour that does not exist
// is the edge pixel itself", because the two weights always sum to 2 f: the kernels clamp the neighbour's index and keep
// the interior weights.  A column blend wy0 a + wy1 b is at most 2 fh 255 = 4080, S + D / 2 at most 256 * 255 + 128 =
// 65408 < 2^16 at fh = fw = 8: everything fits 16-bit lanes, which is the reason for the bound of 8.
//
// The division by D (never an integer-divide sequence): a shift where D is a power of two; otherwise the multiplier of
// i8ie_avgpool.hip, x M >> 24 with M = ceil(2^24 / D), exact while x e < 2^24 for e = M D - 2^24 (the host checks it with
// the actual e and x = 255 D + D / 2; it holds for every D <= 256) and x M < 2^32; both factors are below 2^24 (D >= 12
// where it is no power of two), so the product is one 24-bit multiply.
//
// FP32 (before convert(), and while calibrating): nearest copies bits.  Bilinear: l = (float)w1 / (float)(2 f) per axis, the
// two row blends a (1 - lx) + b lx first, then the column blend of their results with ly; one rounding per operation, no
// contraction.
//
// The NHWC kernels (the hot path): a lane owns one input pixel x one channel item (16 / 4 / 1 channels by c % 16, c % 4 and
// the pointers' alignment) and writes that pixel's fh x fw output items.  It loads the 3 x 3 neighbourhood with clamped
// indices -- a bordered input's border holds zp, not the edge pixel, and is never read -- undoes the input's re-bias and
// splits every dword into its even and its odd bytes, two 16-bit lanes each.  Per output row one column blend of the three
// columns, per output pixel one row blend, the division, the relu floor and the re-bias of the result, all on packed
// 16-bit pairs; one full-width store per output item.  Output rows with t < 0 blend (row above, own row), the others (own
// row, row below), and the same along x: two loops each, no register array is indexed at run time.  Every input byte is
// fetched from memory once (its eight other readers are neighbouring lanes: L2 / L1 hits).  Nearest is the same loop without
// the neighbours and the blend.  32-bit offsets inside an image, 64-bit image bases.  No scratch, no device allocation.
// The NCHW and FP32 forms are off the timed path: one lane per output, plain arithmetic.
#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxFactor = 8;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

struct UpDiv {
  uint32_t rnd;    // D / 2
  uint32_t shift;  // log2 D where D is a power of two (mul == 0)
  uint32_t mul;    // ceil(2^24 / D) otherwise
  uint32_t lo;     // relu ? zp : 0
};

// false: no exact division for this D (cannot happen for a factor pair within 1..8; the entries check it all the same)
bool make_div(int fh, int fw, int relu, int zp, UpDiv* d) {
  const uint32_t D = 4u * (uint32_t)fh * (uint32_t)fw;
  d->rnd = D / 2;
  d->lo = relu ? (uint32_t)zp : 0u;
  d->shift = 0;
  d->mul = 0;
  if ((D & (D - 1)) == 0) {
    while ((1u << d->shift) < D) ++d->shift;
    return true;
  }
  const uint64_t M = ((1ull << 24) + D - 1) / D, e = M * D - (1ull << 24), xmax = 255ull * D + D / 2;
  if (M >= (1ull << 24) || xmax >= (1ull << 16) || xmax * e >= (1ull << 24) || xmax * M >= (1ull << 32)) return false;
  d->mul = (uint32_t)M;
  return true;
}

// one axis of the bilinear rule (header): output index o of an axis of length L with factor f
struct Tap {
  int i0, i1;
  int w1;  // of 2 f; w0 = 2 f - w1
};
__host__ __device__ __forceinline__ Tap tap_of(int o, int f, int L) {
  const int i = o / f, r = o - i * f, t = 2 * r + 1 - f;
  Tap p;
  p.i0 = t >= 0 ? i : i - 1;
  p.w1 = t >= 0 ? t : 2 * f + t;
  if (p.i0 < 0) {
    p.i0 = 0;
    p.w1 = 0;
  }
  p.i1 = p.i0 + 1 < L ? p.i0 + 1 : L - 1;
  return p;
}

// the low 32 bits of the product of two factors below 2^24 (the masks tell the compiler so: one 24-bit multiply), unsigned
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }

// (x + D / 2) / D for x = S, then the relu floor
__device__ __forceinline__ uint32_t div_round(uint32_t S, const UpDiv& d) {
  const uint32_t x = S + d.rnd;
  const uint32_t q = d.mul ? (mul24(x, d.mul) >> 24) : (x >> d.shift);
  return q > d.lo ? q : d.lo;
}

// ---- NCHW and FP32: one lane per output
__global__ __launch_bounds__(kThreads) void upsample_u8_nchw_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                    int64_t total, int h, int w, int fh, int fw, int bilinear,
                                                                    UpDiv d) {
  const int oh = h * fh, ow = w * fw;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    const uint8_t* p = in + (t / oh) * h * w;  // plane: img * c + channel
    if (!bilinear) {
      out[e] = p[(y / fh) * w + x / fw];
      continue;
    }
    const Tap ty = tap_of(y, fh, h), tx = tap_of(x, fw, w);
    const uint32_t wy1 = (uint32_t)ty.w1, wy0 = 2u * fh - wy1, wx1 = (uint32_t)tx.w1, wx0 = 2u * fw - wx1;
    const uint32_t c0 = wy0 * p[ty.i0 * w + tx.i0] + wy1 * p[ty.i1 * w + tx.i0];
    const uint32_t c1 = wy0 * p[ty.i0 * w + tx.i1] + wy1 * p[ty.i1 * w + tx.i1];
    out[e] = (uint8_t)div_round(wx0 * c0 + wx1 * c1, d);
  }
}

__global__ __launch_bounds__(kThreads) void upsample_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total,
                                                                int h, int w, int fh, int fw, int bilinear) {
  const int oh = h * fh, ow = w * fw;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int x = (int)(e % ow);
    const int64_t t = e / ow;
    const int y = (int)(t % oh);
    const float* p = in + (t / oh) * h * w;
    if (!bilinear) {
      out[e] = p[(y / fh) * w + x / fw];
      continue;
    }
    const Tap ty = tap_of(y, fh, h), tx = tap_of(x, fw, w);
    const float ly = (float)ty.w1 / (float)(2 * fh), lx = (float)tx.w1 / (float)(2 * fw);
    const float my = 1.0f - ly, mx = 1.0f - lx;
    const float top = p[ty.i0 * w + tx.i0] * mx + p[ty.i0 * w + tx.i1] * lx;
    const float bot = p[ty.i1 * w + tx.i0] * mx + p[ty.i1 * w + tx.i1] * lx;
    out[e] = top * my + bot * ly;
  }
}

// ---- bordered NHWC buffers [n][h + 2b][w + 2b][c] -> [n][h fh + 2b'][w fw + 2b'][c]
struct UpGeom {
  int64_t in_img, out_img;             // bytes per image
  uint32_t in_row, in_org;             // bytes per physical row, offset of interior pixel (0, 0)
  uint32_t out_row, out_org;
  uint32_t c, h, w, fh, fw;
  uint32_t xin, xout;                  // 0x80808080 where that buffer holds re-biased bytes, else 0
};

// an item of VEC channels as NDW dwords, each split into its even bytes (0 and 2) and its odd bytes (1 and 3): two 16-bit lanes
template <int NDW>
struct Item {
  us2 e[NDW], o[NDW];
};
__device__ __forceinline__ us2 as_us2(uint32_t x) { return __builtin_bit_cast(us2, x); }
__device__ __forceinline__ uint32_t as_u32(us2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ us2 splat(uint32_t x) {
  us2 r;
  r.x = (unsigned short)x;
  r.y = (unsigned short)x;
  return r;
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
    x[0] = (uint32_t)*p ^ (xin & 0xFFu);  // (the upper three bytes are zero lanes: they blend to zero and are not stored)
  }
}
template <int VEC>
__device__ __forceinline__ void store_dwords(uint8_t* p, const uint32_t (&x)[VEC == 16 ? 4 : 1]) {
  if constexpr (VEC == 16) *reinterpret_cast<uint4*>(p) = make_uint4(x[0], x[1], x[2], x[3]);
  else if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(p) = x[0];
  else *p = (uint8_t)x[0];
}
template <int VEC>
__device__ __forceinline__ Item<(VEC == 16 ? 4 : 1)> load_item(const uint8_t* p, uint32_t xin) {
  constexpr int NDW = VEC == 16 ? 4 : 1;
  uint32_t x[NDW];
  load_dwords<VEC>(p, xin, x);
  Item<NDW> it;
#pragma unroll
  for (int j = 0; j < NDW; ++j) {
    it.e[j] = as_us2(x[j] & 0x00FF00FFu);
    it.o[j] = as_us2((x[j] >> 8) & 0x00FF00FFu);
  }
  return it;
}

// (s + D / 2) / D on both 16-bit lanes (s already holds the + D / 2), then the relu floor
__device__ __forceinline__ us2 div_pair(us2 s, const UpDiv& d, us2 lo) {
  us2 q;
  if (d.mul) {
    const uint32_t x = as_u32(s);
    q = as_us2((mul24(x & 0xFFFFu, d.mul) >> 24) | ((mul24(x >> 16, d.mul) >> 24) << 16));
  } else {
    q = s >> splat(d.shift);
  }
  return __builtin_elementwise_max(q, lo);
}

// the decomposition of a lane's item index, shared by the two kernels
struct Where {
  const uint8_t* pi;  // the image's interior origin + the item's channel offset
  uint8_t* po;
  uint32_t y, x;
};
template <int VEC>
__device__ __forceinline__ Where where_of(uint32_t v, const uint8_t* in, uint8_t* out, const UpGeom& g) {
  const uint32_t per_pix = g.c / VEC;
  const uint32_t pix = v / per_pix, ci = v - pix * per_pix;
  const uint32_t row = pix / g.w, x = pix - row * g.w;
  const uint32_t img = row / g.h, y = row - img * g.h;
  return {in + ((int64_t)img * g.in_img + g.in_org + ci * VEC), out + ((int64_t)img * g.out_img + g.out_org + ci * VEC), y, x};
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void upsample_bilinear_u8_nhwc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                             uint32_t items, UpGeom g, UpDiv d) {
  constexpr int NDW = VEC == 16 ? 4 : 1;
  const uint32_t stride = gridDim.x * kThreads;
  const us2 rnd = splat(d.rnd), lo = splat(d.lo);
  const uint32_t neg_y = g.fh / 2, neg_x = g.fw / 2;  // the output rows / columns with t < 0: r < f / 2
  for (uint32_t v = blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const Where at = where_of<VEC>(v, in, out, g);
    // clamped neighbours: the edge pixel stands in for the one that does not exist
    const uint32_t yo[3] = {(at.y ? at.y - 1 : 0u) * g.in_row, at.y * g.in_row, (at.y + 1 < g.h ? at.y + 1 : at.y) * g.in_row};
    const uint32_t xo[3] = {(at.x ? at.x - 1 : 0u) * g.c, at.x * g.c, (at.x + 1 < g.w ? at.x + 1 : at.x) * g.c};
    Item<NDW> q[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) q[a][b] = load_item<VEC>(at.pi + yo[a] + xo[b], g.xin);
    uint8_t* const pix0 = at.po + (at.y * g.fh) * g.out_row + (at.x * g.fw) * g.c;

    // one output row: rows A and B of the neighbourhood with weights 2 fh - wy1 and wy1
    auto emit_row = [&](const Item<NDW>(&A)[3], const Item<NDW>(&B)[3], uint32_t ry, uint32_t wy1) {
      const us2 vy0 = splat(2 * g.fh - wy1), vy1 = splat(wy1);
      Item<NDW> V[3];
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int j = 0; j < NDW; ++j) {
          V[b].e[j] = A[b].e[j] * vy0 + B[b].e[j] * vy1;
          V[b].o[j] = A[b].o[j] * vy0 + B[b].o[j] * vy1;
        }
      uint8_t* const prow = pix0 + ry * g.out_row;
      // one output pixel: columns L and R with weights 2 fw - wx1 and wx1
      auto emit_px = [&](const Item<NDW>& L, const Item<NDW>& R, uint32_t rx, uint32_t wx1) {
        const us2 vx0 = splat(2 * g.fw - wx1), vx1 = splat(wx1);
        uint32_t r[NDW];
#pragma unroll
        for (int j = 0; j < NDW; ++j) {
          const us2 re = div_pair(L.e[j] * vx0 + R.e[j] * vx1 + rnd, d, lo);
          const us2 ro = div_pair(L.o[j] * vx0 + R.o[j] * vx1 + rnd, d, lo);
          r[j] = (as_u32(re) | (as_u32(ro) << 8)) ^ g.xout;
        }
        store_dwords<VEC>(prow + rx * g.c, r);
      };
      for (uint32_t rx = 0; rx < neg_x; ++rx) emit_px(V[0], V[1], rx, g.fw + 2 * rx + 1);   // 2 fw + t
      for (uint32_t rx = neg_x; rx < g.fw; ++rx) emit_px(V[1], V[2], rx, 2 * rx + 1 - g.fw);  // t
    };
    for (uint32_t ry = 0; ry < neg_y; ++ry) emit_row(q[0], q[1], ry, g.fh + 2 * ry + 1);
    for (uint32_t ry = neg_y; ry < g.fh; ++ry) emit_row(q[1], q[2], ry, 2 * ry + 1 - g.fh);
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void upsample_nearest_u8_nhwc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                            uint32_t items, UpGeom g, UpDiv d) {
  constexpr int NDW = VEC == 16 ? 4 : 1;
  const uint32_t stride = gridDim.x * kThreads;
  const us2 lo = splat(d.lo);
  for (uint32_t v = blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const Where at = where_of<VEC>(v, in, out, g);
    const Item<NDW> it = load_item<VEC>(at.pi + at.y * g.in_row + at.x * g.c, g.xin);
    uint32_t r[NDW];
#pragma unroll
    for (int j = 0; j < NDW; ++j)
      r[j] = (as_u32(__builtin_elementwise_max(it.e[j], lo)) | (as_u32(__builtin_elementwise_max(it.o[j], lo)) << 8)) ^ g.xout;
    uint8_t* const pix0 = at.po + (at.y * g.fh) * g.out_row + (at.x * g.fw) * g.c;
    for (uint32_t ry = 0; ry < g.fh; ++ry)
      for (uint32_t rx = 0; rx < g.fw; ++rx) store_dwords<VEC>(pix0 + ry * g.out_row + rx * g.c, r);
  }
}

template <int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int64_t items, const UpGeom& g, const UpDiv& d, bool bilinear) {
  if (bilinear) upsample_bilinear_u8_nhwc_kernel<VEC><<<grid_for(items), kThreads, 0, ctx->stream>>>(in, out, (uint32_t)items, g, d);
  else upsample_nearest_u8_nhwc_kernel<VEC><<<grid_for(items), kThreads, 0, ctx->stream>>>(in, out, (uint32_t)items, g, d);
}

bool up_args_ok(int n, int c, int h, int w) { return n > 0 && c > 0 && h > 0 && w > 0; }
bool factor_ok(int f) { return f >= 1 && f <= kMaxFactor; }
bool mode_ok(int mode) { return mode == I8IE_UPSAMPLE_NEAREST || mode == I8IE_UPSAMPLE_BILINEAR; }

}  // namespace

extern "C" {

int i8ie_upsample2d_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int fh, int fw, int mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(up_args_ok(n, c, h, w), "bad dimension");
  I8IE_REQUIRE(factor_ok(fh) && factor_ok(fw), "factor outside 1..8");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE((int64_t)h * fh * w * fw <= 0x7FFFFFFF, "an output plane of more than 2^31 elements");
  UpDiv d;
  I8IE_REQUIRE(make_div(fh, fw, 0, 0, &d), "no exact division for this factor pair");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * h * fh * w * fw;
  I8ieProfScope prof(ctx, "upsample_u8_nchw", 0.0, (double)n * c * h * w + (double)total);
  upsample_u8_nchw_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, fh, fw, mode == I8IE_UPSAMPLE_BILINEAR, d);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_upsample2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
                            int c, int h, int w, int fh, int fw, int mode, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(up_args_ok(n, c, h, w) && in_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(factor_ok(fh) && factor_ok(fw), "factor outside 1..8");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, h * fh, w * fw, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const int vec = item_width({c}, {in, out});
  const int64_t items = (int64_t)n * h * w * (c / vec);
  I8IE_REQUIRE(items <= 0x7FFFFFFF, "too many items for one launch");
  UpDiv d;
  I8IE_REQUIRE(make_div(fh, fw, relu, zero_point, &d), "no exact division for this factor pair");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  UpGeom g;
  g.in_img = gi.img; g.in_row = (uint32_t)gi.row; g.in_org = (uint32_t)gi.org;
  g.out_img = go.img; g.out_row = (uint32_t)go.row; g.out_org = (uint32_t)go.org;
  g.c = (uint32_t)c; g.h = (uint32_t)h; g.w = (uint32_t)w; g.fh = (uint32_t)fh; g.fw = (uint32_t)fw;
  g.xin = in_s8 ? 0x80808080u : 0u;
  g.xout = out_s8 ? 0x80808080u : 0u;
  const bool bilinear = mode == I8IE_UPSAMPLE_BILINEAR;
  const double bytes = (double)n * c * h * w * (1.0 + (double)fh * fw);
  I8ieProfScope prof(ctx, bilinear ? "upsample_bilinear_u8_nhwc" : "upsample_nearest_u8_nhwc", 0.0, bytes);
  if (vec == 16) launch_nhwc<16>(ctx, in, out, items, g, d, bilinear);
  else if (vec == 4) launch_nhwc<4>(ctx, in, out, items, g, d, bilinear);
  else launch_nhwc<1>(ctx, in, out, items, g, d, bilinear);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_upsample2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int fh, int fw, int mode) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(up_args_ok(n, c, h, w), "bad dimension");
  I8IE_REQUIRE(factor_ok(fh) && factor_ok(fw), "factor outside 1..8");
  I8IE_REQUIRE(mode_ok(mode), "unknown mode");
  I8IE_REQUIRE((int64_t)h * fh * w * fw <= 0x7FFFFFFF, "an output plane of more than 2^31 elements");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t total = (int64_t)n * c * h * fh * w * fw;
  I8ieProfScope prof(ctx, "upsample_f32", 0.0, 4.0 * ((double)n * c * h * w + (double)total));
  upsample_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(in, out, total, h, w, fh, fw, mode == I8IE_UPSAMPLE_BILINEAR);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
