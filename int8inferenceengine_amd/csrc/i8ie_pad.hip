// i8ie_pad.hip -- spatial padding (constant, reflect, replicate, circular) and cropping:
// i8ie_pad_output_shape, i8ie_pad2d_u8_nhwc, i8ie_pad2d_u8, i8ie_pad2d_f32.
//
// The reference has no such op.  On [n, c, h, w] (NCHW logical shape), per spatial axis of input length L with amounts
// (before, after): O = L + before + after >= 1, output index o reads input index i = o - before, and for i outside [0, L)
//     constant    the fill value                     (negative amounts cut pixels off; this mode only)
//     reflect     -i, respectively 2 (L - 1) - i     amounts <= L - 1
//     replicate   0, respectively L - 1              any amount >= 0
//     circular    i + L, respectively i - L          amounts <= L
//     q = relu ? max(q, zp) : q                      (relu<u8>, src/functional.cc:15-26; fill bytes included)
// |amount| <= 65535.  The result carries the input's (scale, zero_point); bytes (FP32: bits) are copied.
//
// Three kernels give identical bytes.
//
// pad_u8_nhwc (the hot path).  A lane owns one output pixel x one channel item of 16 / 4 / 1 bytes, the widest that c and both
// base pointers allow; consecutive lanes take consecutive items of a pixel, then the next pixel of the output row, so a wave's
// stores are one contiguous run and so are its loads wherever the run stays inside the copied interior.  A lane decomposes its
// first index (< 2^19) into (image, oy, ox, item) once by host-made multipliers (Div40, as i8ie_rearrange.hip) and then steps
// the digits by the grid stride, which the host decomposed the same way, with a carry chain: no division anywhere.  Per item
// two subtracts and two unsigned compares say whether (oy, ox) lies in the interior (before <= o < before + L on both axes).
// A wave whose lanes are all inside -- one ballot, a wave-uniform branch -- copies with the offsets it already has; any other
// wave evaluates the mode's rule per axis (compares, subtracts; circular is one conditional add or subtract because amounts
// are <= L) and stores the fill item, which the host made once (byte splat, relu'd, re-biased) and which lives in registers.
// The source offset is built from the mapped (row, column) and the interior origin of the input: a bordered input's border
// holds zp, not what reflect / replicate / circular want, and is never read.  Only the interior of the result is written: its
// border is the caller's (i8ie_fill_border_u8), as for every other NHWC producer.  32-bit offsets inside an image, 64-bit
// image bases.  No LDS, no scratch, no device allocation: the geometry travels in the kernel arguments.
//
// pad_u8_direct: the definition verbatim, one lane per output byte, strides for any layout: the flat NCHW entry and every NHWC
// call under the force-fallback option.  pad_f32: the same kernel on 4-byte elements, bits copied.  Both are off the timed
// path and divide plainly.
#include <algorithm>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_bytemax.h"

namespace {

constexpr int kMaxAmount = 65535;
constexpr int kDigits = 3;  // (oy, ox, item) below the image

// the result's spatial dims, or false with the error set (the op's name first)
bool shape_of(int mode, int left, int right, int top, int bottom, int n, int c, int h, int w, int* oh, int* ow) {
  if (mode < I8IE_PAD_CONSTANT || mode > I8IE_PAD_CIRCULAR) {
    i8ie_set_error("pad: unknown mode %d", mode);
    return false;
  }
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) {
    i8ie_set_error("pad: empty tensor");
    return false;
  }
  static const char* const kMode[] = {"constant", "reflect", "replicate", "circular"};
  const int amount[4] = {left, right, top, bottom};
  static const char* const kSide[] = {"left", "right", "top", "bottom"};
  for (int k = 0; k < 4; ++k) {
    const int a = amount[k], L = k < 2 ? w : h;
    if (a > kMaxAmount || a < -kMaxAmount) {
      i8ie_set_error("pad: %s = %d is beyond +-65535", kSide[k], a);
      return false;
    }
    if (a < 0 && mode != I8IE_PAD_CONSTANT) {
      i8ie_set_error("pad: %s = %d: negative amounts (cropping) go with the constant mode only, not %s", kSide[k], a, kMode[mode]);
      return false;
    }
    const int64_t limit = mode == I8IE_PAD_REFLECT ? (int64_t)L - 1 : (mode == I8IE_PAD_CIRCULAR ? (int64_t)L : kMaxAmount);
    if (a > limit) {
      i8ie_set_error("pad: %s = %d is more than %s padding allows on an axis of %d (at most %lld)", kSide[k], a, kMode[mode], L,
                     (long long)limit);
      return false;
    }
  }
  const int64_t O_w = (int64_t)w + left + right, O_h = (int64_t)h + top + bottom;
  if (O_w < 1 || O_h < 1) {
    i8ie_set_error("pad: the result would be %lld x %lld (at least 1 x 1)", (long long)O_h, (long long)O_w);
    return false;
  }
  if (O_w > 0x7FFFFFFF || O_h > 0x7FFFFFFF) {
    i8ie_set_error("pad: the result is too large");
    return false;
  }
  *oh = (int)O_h;
  *ow = (int)O_w;
  return true;
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// the rule of one axis: the input index that output index o reads, or -1 for the fill value
__device__ __forceinline__ int src_of(int o, int before, int L, int mode) {
  const int i = o - before;
  if ((uint32_t)i < (uint32_t)L) return i;
  switch (mode) {
    case I8IE_PAD_REFLECT: return i < 0 ? -i : 2 * (L - 1) - i;
    case I8IE_PAD_REPLICATE: return i < 0 ? 0 : L - 1;
    case I8IE_PAD_CIRCULAR: return i < 0 ? i + L : i - L;
  }
  return -1;
}

struct ByteOps {
  uint32_t xin, xout;  // 0x80808080 where that buffer holds re-biased bytes, else 0
  uint32_t lo2;        // relu ? zp in both 16-bit halves : 0
  uint32_t relu;
};
ByteOps make_ops(int in_s8, int out_s8, int relu, int zp) {
  return {in_s8 ? 0x80808080u : 0u, out_s8 ? 0x80808080u : 0u, relu ? (uint32_t)zp * 0x00010001u : 0u, relu ? 1u : 0u};
}
// the fill byte as it lies in the result: relu'd and re-biased once, on the host
uint8_t fill_as_stored(uint8_t fill, int out_s8, int relu, uint8_t zp) {
  const uint8_t f = relu && fill < zp ? zp : fill;
  return out_s8 ? (uint8_t)(f ^ 0x80u) : f;
}
// four bytes as they lie in the input -> as they lie in the result
__device__ __forceinline__ uint32_t fix4(uint32_t x, const ByteOps& o) {
  x ^= o.xin;
  if (o.relu) {
    const us2 lo = __builtin_bit_cast(us2, o.lo2);
    BytesEO m = spread_eo(x);
    m.e = __builtin_elementwise_max(m.e, lo);
    m.o = __builtin_elementwise_max(m.o, lo);
    x = pack_eo(m);
  }
  return x ^ o.xout;
}

// x / d for x < 2^19 and any d >= 1 by one 64-bit multiply: m = ceil(2^40 / d), q = x m >> 40 (the proof: i8ie_rearrange.hip)
struct Div40 {
  uint64_t m;
  uint32_t d;
};
Div40 make_div40(uint32_t d) { return {((1ull << 40) + d - 1) / d, d}; }
__device__ __forceinline__ uint32_t div40(uint32_t x, const Div40& v) { return (uint32_t)(((uint64_t)x * v.m) >> 40); }

// ---- pad_u8_nhwc ------------------------------------------------------------------------------------------------------------
struct PadWalk {
  Div40 byR[kDigits];                   // the radices as multipliers
  int64_t in_img, out_img;              // bytes per image
  int64_t simg;                         // the grid stride's image digit
  int64_t total;                        // items
  uint32_t R[kDigits], sd[kDigits];     // radices (oh, ow, items per pixel) and the grid stride's digits
  uint32_t in_row, in_org, out_row, out_org;  // bytes per physical row, offset of interior pixel (0, 0)
  uint32_t c;
  int h, w, top, left, mode;
  uint32_t fill4;                       // the fill byte as stored, in all four bytes
  ByteOps ops;
};

template <int VEC>
__device__ __forceinline__ void copy_item(const uint8_t* src, uint8_t* dst, const ByteOps& o) {
  if constexpr (VEC == 16) {
    uint4 q = *reinterpret_cast<const uint4*>(src);
    q.x = fix4(q.x, o); q.y = fix4(q.y, o); q.z = fix4(q.z, o); q.w = fix4(q.w, o);
    *reinterpret_cast<uint4*>(dst) = q;
  } else if constexpr (VEC == 4) {
    *reinterpret_cast<uint32_t*>(dst) = fix4(*reinterpret_cast<const uint32_t*>(src), o);
  } else {  // (the upper lanes of the dword are computed and dropped)
    *dst = (uint8_t)fix4(*src, o);
  }
}
template <int VEC>
__device__ __forceinline__ void fill_item(uint8_t* dst, uint32_t f4) {
  if constexpr (VEC == 16) *reinterpret_cast<uint4*>(dst) = make_uint4(f4, f4, f4, f4);
  else if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(dst) = f4;
  else *dst = (uint8_t)f4;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void pad_u8_nhwc_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const PadWalk g) {
  const uint32_t v0 = blockIdx.x * kThreads + threadIdx.x;  // < kMaxBlocks * kThreads = 2^19
  if ((int64_t)v0 >= g.total) return;
  uint32_t d[kDigits], t = v0;
#pragma unroll
  for (int k = kDigits - 1; k >= 0; --k) {
    const uint32_t q = div40(t, g.byR[k]);
    d[k] = t - q * g.R[k];
    t = q;
  }
  int64_t img = t;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = v0; v < g.total; v += stride) {
    const uint32_t oy = d[0], ox = d[1], ci = d[2] * VEC;
    const int iy = (int)oy - g.top, ix = (int)ox - g.left;
    const bool edge = (uint32_t)iy >= (uint32_t)g.h || (uint32_t)ix >= (uint32_t)g.w;
    const uint8_t* const src = in + (img * g.in_img + g.in_org + ci);  // (inside one image: below 2^31)
    uint8_t* const dst = out + (img * g.out_img + (g.out_org + oy * g.out_row + ox * g.c + ci));
    if (__builtin_amdgcn_ballot_w64(edge) == 0) {  // every lane of the wave copies an interior pixel
      copy_item<VEC>(src + ((uint32_t)iy * g.in_row + (uint32_t)ix * g.c), dst, g.ops);
    } else {
      const int sy = src_of((int)oy, g.top, g.h, g.mode), sx = src_of((int)ox, g.left, g.w, g.mode);
      if (sy < 0 || sx < 0) fill_item<VEC>(dst, g.fill4);
      else copy_item<VEC>(src + ((uint32_t)sy * g.in_row + (uint32_t)sx * g.c), dst, g.ops);
    }
    // step by the grid stride, carrying upwards (each sum stays below twice its radix: one subtraction is enough)
    uint32_t carry = 0;
#pragma unroll
    for (int k = kDigits - 1; k >= 0; --k) {
      d[k] += g.sd[k] + carry;
      carry = d[k] >= g.R[k] ? 1u : 0u;
      d[k] -= carry ? g.R[k] : 0u;
    }
    img += g.simg + carry;
  }
}

int launch_nhwc(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int vec, const NhwcGeom& gi, const NhwcGeom& go, int n, int c, int h, int w,
                int oh, int ow, int mode, int left, int top, uint8_t fill_stored, const ByteOps& ops) {
  PadWalk g;
  g.ops = ops;
  g.in_img = gi.img; g.in_row = (uint32_t)gi.row; g.in_org = (uint32_t)gi.org;
  g.out_img = go.img; g.out_row = (uint32_t)go.row; g.out_org = (uint32_t)go.org;
  g.c = (uint32_t)c; g.h = h; g.w = w; g.top = top; g.left = left; g.mode = mode;
  g.fill4 = (uint32_t)fill_stored * 0x01010101u;
  g.R[0] = (uint32_t)oh; g.R[1] = (uint32_t)ow; g.R[2] = (uint32_t)(c / vec);
  int64_t total = n;
  for (int k = 0; k < kDigits; ++k) {
    total *= g.R[k];
    g.byR[k] = make_div40(g.R[k]);
  }
  g.total = total;
  const int gx = grid_for(total);
  int64_t t = (int64_t)gx * kThreads;
  for (int k = kDigits - 1; k >= 0; --k) {
    g.sd[k] = (uint32_t)(t % g.R[k]);
    t /= g.R[k];
  }
  g.simg = t;
  switch (vec) {
    case 16: pad_u8_nhwc_kernel<16><<<gx, kThreads, 0, ctx->stream>>>(in, out, g); break;
    case 4: pad_u8_nhwc_kernel<4><<<gx, kThreads, 0, ctx->stream>>>(in, out, g); break;
    default: pad_u8_nhwc_kernel<1><<<gx, kThreads, 0, ctx->stream>>>(in, out, g); break;
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

// ---- pad_u8_direct / pad_f32: one lane per output element, any layout ---------------------------------------------------------
struct Plane {  // where element (img, ch, y, x) of a buffer lies: off = org + img * img_s + ch * c_s + y * y_s + x * x_s
  int64_t org, img_s, c_s, y_s, x_s;
};
Plane nhwc_plane(int c, const NhwcGeom& g) { return {g.org, g.img, 1, g.row, c}; }
Plane nchw_plane(int c, int h, int w) { return {0, (int64_t)c * h * w, (int64_t)h * w, w, 1}; }

struct Flat {
  Plane in, out;
  int64_t total;
  int c, oh, ow, h, w, top, left, mode;
  int inner_c;  // the channel is the fastest output axis (NHWC): consecutive lanes write consecutive elements
};

template <typename T, bool BYTES>
__global__ __launch_bounds__(kThreads) void pad_direct_kernel(const T* __restrict__ in, T* __restrict__ out, const Flat g, const T fill,
                                                              const ByteOps ops) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < g.total; e += stride) {
    int ch, oy, ox;
    int64_t t = e;
    if (g.inner_c) {
      ch = (int)(t % g.c); t /= g.c;
      ox = (int)(t % g.ow); t /= g.ow;
      oy = (int)(t % g.oh); t /= g.oh;
    } else {
      ox = (int)(t % g.ow); t /= g.ow;
      oy = (int)(t % g.oh); t /= g.oh;
      ch = (int)(t % g.c); t /= g.c;
    }
    const int sy = src_of(oy, g.top, g.h, g.mode), sx = src_of(ox, g.left, g.w, g.mode);
    T val = fill;
    if (sy >= 0 && sx >= 0) {
      val = in[g.in.org + t * g.in.img_s + ch * g.in.c_s + sy * g.in.y_s + sx * g.in.x_s];
      if (BYTES) val = (T)fix4((uint32_t)val, ops);
    }
    out[g.out.org + t * g.out.img_s + ch * g.out.c_s + oy * g.out.y_s + ox * g.out.x_s] = val;
  }
}

Flat flat_of(const Plane& pi, const Plane& po, int n, int c, int h, int w, int oh, int ow, int mode, int left, int top, bool inner_c) {
  Flat g;
  g.in = pi; g.out = po;
  g.total = (int64_t)n * c * oh * ow;
  g.c = c; g.oh = oh; g.ow = ow; g.h = h; g.w = w; g.top = top; g.left = left; g.mode = mode;
  g.inner_c = inner_c ? 1 : 0;
  return g;
}

}  // namespace

extern "C" {

int i8ie_pad_output_shape(int mode, int left, int right, int top, int bottom, int n, int c, int h, int w, int* out_dims) {
  if (!out_dims) {
    i8ie_set_error("i8ie_pad_output_shape: null argument");
    return I8IE_ERR_ARG;
  }
  int oh = 0, ow = 0;
  if (!shape_of(mode, left, right, top, bottom, n, c, h, w, &oh, &ow)) return I8IE_ERR_ARG;
  out_dims[0] = n; out_dims[1] = c; out_dims[2] = oh; out_dims[3] = ow;
  return I8IE_OK;
}

int i8ie_pad2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n, int c,
                       int h, int w, int mode, int left, int right, int top, int bottom, uint8_t fill, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "bad dimension");
  int oh = 0, ow = 0;
  if (!shape_of(mode, left, right, top, bottom, n, c, h, w, &oh, &ow)) return I8IE_ERR_ARG;
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(c, oh, ow, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  I8IE_REQUIRE(!overlap(in, n * gi.img, out, n * go.img), "out overlaps in");
  const ByteOps ops = make_ops(in_s8, out_s8, relu, zero_point);
  const uint8_t stored = fill_as_stored(fill, out_s8, relu, zero_point);
  const double bytes = 2.0 * (double)n * c * oh * ow;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  if ((ctx->options & 1u) != 0) {
    const Flat g = flat_of(nhwc_plane(c, gi), nhwc_plane(c, go), n, c, h, w, oh, ow, mode, left, top, true);
    I8ieProfScope prof(ctx, "pad_u8_direct", 0.0, bytes);
    pad_direct_kernel<uint8_t, true><<<grid_for(g.total), kThreads, 0, ctx->stream>>>(in, out, g, stored, ops);
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  const int vec = item_width({c}, {in, out});
  I8ieProfScope prof(ctx, "pad_u8_nhwc", 0.0, bytes);
  return launch_nhwc(ctx, in, out, vec, gi, go, n, c, h, w, oh, ow, mode, left, top, stored, ops);
}

int i8ie_pad2d_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int mode, int left, int right, int top,
                  int bottom, uint8_t fill) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oh = 0, ow = 0;
  if (!shape_of(mode, left, right, top, bottom, n, c, h, w, &oh, &ow)) return I8IE_ERR_ARG;
  const Flat g = flat_of(nchw_plane(c, h, w), nchw_plane(c, oh, ow), n, c, h, w, oh, ow, mode, left, top, false);
  I8IE_REQUIRE(!overlap(in, n * g.in.img_s, out, g.total), "out overlaps in");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "pad_u8_direct", 0.0, 2.0 * (double)g.total);
  pad_direct_kernel<uint8_t, false><<<grid_for(g.total), kThreads, 0, ctx->stream>>>(in, out, g, fill, make_ops(0, 0, 0, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_pad2d_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int mode, int left, int right, int top,
                   int bottom, float fill) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(aligned_to(in, 4) && aligned_to(out, 4), "buffers must be 4-byte aligned");
  int oh = 0, ow = 0;
  if (!shape_of(mode, left, right, top, bottom, n, c, h, w, &oh, &ow)) return I8IE_ERR_ARG;
  const Flat g = flat_of(nchw_plane(c, h, w), nchw_plane(c, oh, ow), n, c, h, w, oh, ow, mode, left, top, false);
  I8IE_REQUIRE(!overlap(in, 4 * n * g.in.img_s, out, 4 * g.total), "out overlaps in");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "pad_f32", 0.0, 8.0 * (double)g.total);
  pad_direct_kernel<uint32_t, false><<<grid_for(g.total), kThreads, 0, ctx->stream>>>(
      reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), g, __builtin_bit_cast(uint32_t, fill), make_ops(0, 0, 0, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
