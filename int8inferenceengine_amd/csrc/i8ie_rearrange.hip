// i8ie_rearrange.hip -- channel narrow / channel shuffle / pixel shuffle / pixel unshuffle:
// i8ie_rearrange_output_shape, i8ie_rearrange_u8_nhwc, i8ie_rearrange_u8, i8ie_rearrange_f32.
//
// The reference has none of them.  All four move bytes and compute nothing; on [n, c, h, w] (NCHW logical shape):
//     narrow(start, length)   out[n, k, y, x]            = in[n, start + k, y, x]                       -> [n, length, h, w]
//     channel_shuffle(g)      out[n, j g + i, y, x]      = in[n, i (c / g) + j, y, x]                   -> [n, c, h, w]
//     pixel_shuffle(r)        out[n, co, y r + i, x r + j] = in[n, co r r + i r + j, y, x]              -> [n, c / r^2, h r, w r]
//     pixel_unshuffle(r)      out[n, ci r r + i r + j, y, x] = in[n, ci, y r + i, x r + j]              -> [n, c r^2, h / r, w / r]
//     q = relu ? max(q, zp) : q                                                       (relu<u8>, src/functional.cc:15-26)
// The result carries the input's (scale, zero_point).
//
// Three kernel forms give identical bytes.
//
// mapped copy (narrow_u8_nhwc, rearrange_u8_direct, rearrange_u8_nchw, rearrange_f32).  Each op on each layout is a copy
// out[obase + sum d_k os_k] = in[ibase + sum d_k is_k] over a mixed-radix counter (d_0 .. d_5) whose radices and strides the
// host writes down (map_of): d_0 is the image, the last digit the item inside a run of consecutive bytes.  A lane decomposes
// its first index (< 2^19) once, by host-made multipliers (Div40), and then steps all digits by the grid stride, which the host decomposed the same way, with a
// carry chain: no division in the loop.  narrow takes items of 16 / 8 / 4 / 2 / 1 bytes, the widest that start, length, both
// pixel pitches and both base pointers allow, and reads only its slice of each pixel row; the direct form is one lane per
// output byte and takes every shape, any alignment and the force-fallback option; the FP32 form moves 4-byte items.
//
// chanperm_u8_nhwc, the fast path of the three permuting ops: per unit all three are the byte-matrix transposition
// [A][B] -> [B][A] of T = A B bytes:
//     channel shuffle   A = g,    B = c / g   one pixel in, one pixel out
//     pixel shuffle     A = c_out, B = r r    one pixel in, r r rows of c_out bytes to r r output pixels
//     pixel unshuffle   A = r r,  B = c_in    the rows of r r input pixels in, one pixel out
// Taken where c_in % 16 == 0, c_out % 16 == 0, both bases are 16-byte aligned and T <= 16384.  Global memory is touched with
// 16-byte accesses only.  A block takes U units at a time: (0) one lane per unit writes the unit's two 64-bit buffer offsets
// to LDS (by host-made multipliers and the tile's stepped origin: no integer divide anywhere); (1) consecutive lanes load consecutive 16-byte chunks of the units' pixel rows
// and store them to LDS as they lie, unit u at u * pitch; (2) consecutive lanes assemble consecutive 16-byte chunks of the
// units' output rows from LDS, apply relu and the two re-biases on packed dwords and store them.  Assembly of one output
// dword o = 4 d, (b, a) = divmod(o, A) by a host-made multiplier, then stepped:
//     quad (A % 4 == 0 && B % 4 == 0)   four dword reads lds[(a + k) B + (b & ~3)], byte b & 3 of each: three v_perm_b32
//     pair (A == 2 && B % 4 == 0)       two dword reads lds[2 d & ~3], lds[B + (2 d & ~3)], interleaved: one v_perm_b32
//     byte (anything else)              four byte reads lds[a B + b]
// LDS pitch: a unit lies linearly (so that stage 1 is a plain 16-byte copy), and the pitch between units is T rounded up to
// an odd number of 16-byte slots: units that a wave reads side by side start 4 (mod 8) banks apart instead of on one bank.
// Inside one unit the quad reads of neighbouring lanes are 16 B bytes apart (a conflict of up to 16 lanes at B = 4, none
// for A <= 16); DESIGN.md section 8q has the plan; the conflict counters were not measured.  32 KiB + 4 KiB of LDS per block.
#include <algorithm>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_bytemax.h"

namespace {

constexpr int kMaxFactor = 8;
constexpr int kMaxChannels = 65535;
constexpr int kDigits = 5;            // digits below the image
constexpr int kPermLds = 32768;       // bytes of unit storage per block
constexpr int kPermMaxUnits = 256;    // units per tile
constexpr int kPermMaxT = 16384;
constexpr int kPermTileChunks = 1024; // 16-byte chunks a tile aims at (4 per lane and stage)

const char* kind_name(int kind) {
  switch (kind) {
    case I8IE_REARRANGE_NARROW: return "narrow";
    case I8IE_REARRANGE_CHANNEL_SHUFFLE: return "channel_shuffle";
    case I8IE_REARRANGE_PIXEL_SHUFFLE: return "pixel_shuffle";
    case I8IE_REARRANGE_PIXEL_UNSHUFFLE: return "pixel_unshuffle";
  }
  return "rearrange";
}

// the result's dims, or false with the error set (the op's name first)
bool shape_of(int kind, int p0, int p1, int n, int c, int h, int w, int* oc, int* oh, int* ow) {
  const char* nm = kind_name(kind);
  if (kind < I8IE_REARRANGE_NARROW || kind > I8IE_REARRANGE_PIXEL_UNSHUFFLE) {
    i8ie_set_error("rearrange: unknown kind %d", kind);
    return false;
  }
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) {
    i8ie_set_error("%s: empty tensor", nm);
    return false;
  }
  *oc = c; *oh = h; *ow = w;
  if (kind == I8IE_REARRANGE_NARROW) {
    if (p0 < 0 || p1 <= 0 || (int64_t)p0 + p1 > c) {
      i8ie_set_error("%s: channels %d .. %lld are not inside 0 .. %d", nm, p0, (long long)p0 + p1 - 1, c - 1);
      return false;
    }
    *oc = p1;
    return true;
  }
  if (kind == I8IE_REARRANGE_CHANNEL_SHUFFLE) {
    if (p0 < 1 || c % p0 != 0) {
      i8ie_set_error("%s: %d channels are not a multiple of groups = %d", nm, c, p0);
      return false;
    }
  } else {
    if (p0 < 1 || p0 > kMaxFactor) {
      i8ie_set_error("%s: the factor must be an integer in 1..8", nm);
      return false;
    }
    if (kind == I8IE_REARRANGE_PIXEL_SHUFFLE) {
      if (c % (p0 * p0) != 0) {
        i8ie_set_error("%s: %d channels are not a multiple of r * r = %d", nm, c, p0 * p0);
        return false;
      }
      if ((int64_t)h * p0 > 0x7FFFFFFF || (int64_t)w * p0 > 0x7FFFFFFF) {
        i8ie_set_error("%s: the result is too large", nm);
        return false;
      }
      *oc = c / (p0 * p0); *oh = h * p0; *ow = w * p0;
    } else {
      if (h % p0 != 0 || w % p0 != 0) {
        i8ie_set_error("%s: height %d and width %d must be multiples of r = %d", nm, h, w, p0);
        return false;
      }
      *oc = c * p0 * p0; *oh = h / p0; *ow = w / p0;
    }
  }
  if (c > kMaxChannels || *oc > kMaxChannels) {
    i8ie_set_error("%s: more than 65535 channels", nm);
    return false;
  }
  return true;
}

// ---- the mapped copy ------------------------------------------------------------------------------------------------------
// one op on one layout as a mixed-radix copy; strides in elements, digit 0 (the image) first
struct Map {
  int64_t R[1 + kDigits], is[1 + kDigits], os[1 + kDigits];
  int64_t ibase, obase;
};
struct Plane {  // where element (img, ch, y, x) of a buffer lies: off = org + img * img_s + ch * c_s + y * y_s + x * x_s
  int64_t org, img_s, c_s, y_s, x_s;
};
Plane nhwc_plane(int c, int h, int w, int border) {
  const NhwcGeom g = buf_geom(c, h, w, border);
  return {g.org, g.img, 1, g.row, c};
}
Plane nchw_plane(int c, int h, int w) { return {0, (int64_t)c * h * w, (int64_t)h * w, w, 1}; }

// `inner_c`: the channel is the fastest output axis (NHWC) -- the digit order follows the output's memory order
Map map_of(int kind, int p0, int n, int c, int h, int w, int oc, int oh, int ow, const Plane& pi, const Plane& po, bool inner_c) {
  Map m;
  for (int k = 0; k <= kDigits; ++k) { m.R[k] = 1; m.is[k] = 0; m.os[k] = 0; }
  m.ibase = pi.org; m.obase = po.org;
  m.R[0] = n; m.is[0] = pi.img_s; m.os[0] = po.img_s;
  // the digits an op uses are the least significant ones (the item division acts on the last): count them, then fill
  const int used = kind == I8IE_REARRANGE_NARROW ? 3 : (kind == I8IE_REARRANGE_CHANNEL_SHUFFLE ? 4 : 5);
  int k = 1 + kDigits - used;
  auto digit = [&](int64_t R, int64_t is, int64_t os) { m.R[k] = R; m.is[k] = is; m.os[k] = os; ++k; };
  const int r = p0;
  if (kind == I8IE_REARRANGE_NARROW) {
    m.ibase += (int64_t)p0 * pi.c_s;
    if (!inner_c) digit(oc, pi.c_s, po.c_s);
    digit(h, pi.y_s, po.y_s);
    digit(w, pi.x_s, po.x_s);
    if (inner_c) digit(oc, pi.c_s, po.c_s);
  } else if (kind == I8IE_REARRANGE_CHANNEL_SHUFFLE) {  // out channel j g + i <- in channel i (c / g) + j
    const int g = p0, cg = c / p0;
    if (!inner_c) { digit(cg, pi.c_s, g * po.c_s); digit(g, cg * pi.c_s, po.c_s); }
    digit(h, pi.y_s, po.y_s);
    digit(w, pi.x_s, po.x_s);
    if (inner_c) { digit(cg, pi.c_s, g * po.c_s); digit(g, cg * pi.c_s, po.c_s); }
  } else if (kind == I8IE_REARRANGE_PIXEL_SHUFFLE) {  // out (co, y r + i, x r + j) <- in (co r r + i r + j, y, x)
    if (!inner_c) digit(oc, (int64_t)r * r * pi.c_s, po.c_s);
    digit(h, pi.y_s, r * po.y_s);
    digit(r, r * pi.c_s, po.y_s);
    digit(w, pi.x_s, r * po.x_s);
    digit(r, pi.c_s, po.x_s);
    if (inner_c) digit(oc, (int64_t)r * r * pi.c_s, po.c_s);
  } else {  // out (ci r r + i r + j, y, x) <- in (ci, y r + i, x r + j)
    if (!inner_c) { digit(c, pi.c_s, (int64_t)r * r * po.c_s); digit(r, pi.y_s, r * po.c_s); digit(r, pi.x_s, po.c_s); }
    digit(oh, r * pi.y_s, po.y_s);
    digit(ow, r * pi.x_s, po.x_s);
    if (inner_c) { digit(c, pi.c_s, (int64_t)r * r * po.c_s); digit(r, pi.y_s, r * po.c_s); digit(r, pi.x_s, po.c_s); }
  }
  return m;
}

struct ByteOps {
  uint32_t xin, xout;  // 0x80808080 where that buffer holds re-biased bytes, else 0
  uint32_t lo2;        // relu ? zp in both 16-bit halves : 0
  uint32_t relu;
};
ByteOps make_ops(int in_s8, int out_s8, int relu, int zp) {
  return {in_s8 ? 0x80808080u : 0u, out_s8 ? 0x80808080u : 0u, relu ? (uint32_t)zp * 0x00010001u : 0u, relu ? 1u : 0u};
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

// x / d for x < 2^19 and any d >= 1 by one 64-bit multiply: m = ceil(2^40 / d), q = x m >> 40.  With e = m d - 2^40 < d the
// quotient is exact while x e < 2^40: d < 2^21 gives x e < 2^19 2^21; d >= 2^21 > x gives x m <= x 2^40 / d + x < 2^40, q = 0.
struct Div40 {
  uint64_t m;
  uint32_t d;
};
Div40 make_div40(uint32_t d) { return {((1ull << 40) + d - 1) / d, d}; }
__device__ __forceinline__ uint32_t div40(uint32_t x, const Div40& v) { return (uint32_t)(((uint64_t)x * v.m) >> 40); }

struct Walk {
  Div40 byR[kDigits];       // the radices as multipliers: a lane's first index is decomposed without an integer divide
  int64_t in_img, out_img;  // byte strides of the image digit
  int64_t simg;             // the grid stride's image digit
  int64_t total;            // items
  uint32_t R[kDigits], is[kDigits], os[kDigits], sd[kDigits];  // the digits below the image, least significant last; byte strides
  ByteOps ops;
};

template <int VEC, bool BYTES>
__device__ __forceinline__ void copy_item(const uint8_t* src, uint8_t* dst, const ByteOps& o) {
  if constexpr (VEC == 16) {
    uint4 q = *reinterpret_cast<const uint4*>(src);
    if (BYTES) { q.x = fix4(q.x, o); q.y = fix4(q.y, o); q.z = fix4(q.z, o); q.w = fix4(q.w, o); }
    *reinterpret_cast<uint4*>(dst) = q;
  } else if constexpr (VEC == 8) {
    uint2 q = *reinterpret_cast<const uint2*>(src);
    if (BYTES) { q.x = fix4(q.x, o); q.y = fix4(q.y, o); }
    *reinterpret_cast<uint2*>(dst) = q;
  } else if constexpr (VEC == 4) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(src);
    *reinterpret_cast<uint32_t*>(dst) = BYTES ? fix4(q, o) : q;
  } else if constexpr (VEC == 2) {  // (the upper lanes of the dword are computed and dropped)
    const uint32_t q = *reinterpret_cast<const uint16_t*>(src);
    *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(BYTES ? fix4(q, o) : q);
  } else {
    const uint32_t q = *src;
    *dst = (uint8_t)(BYTES ? fix4(q, o) : q);
  }
}

template <int VEC, bool BYTES>
__global__ __launch_bounds__(kThreads) void mapped_copy_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Walk g) {
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
    uint32_t io = 0, oo = 0;  // (inside one image: below 2^31)
#pragma unroll
    for (int k = 0; k < kDigits; ++k) {
      io += d[k] * g.is[k];
      oo += d[k] * g.os[k];
    }
    copy_item<VEC, BYTES>(in + (img * g.in_img + io), out + (img * g.out_img + oo), g.ops);
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

// Launch `m` (strides in elements of `elem` bytes) with items of `vec` bytes along the last digit.  The caller has checked
// that vec divides the last digit's run and every other stride, and that an image is below 2^31 bytes on both sides.
template <bool BYTES>
int launch_map(i8ie_ctx* ctx, const Map& m, int elem, int vec, const uint8_t* in, uint8_t* out, const ByteOps& ops) {
  Walk g;
  g.ops = ops;
  g.in_img = m.is[0] * elem;
  g.out_img = m.os[0] * elem;
  const int per = vec / elem;  // elements per item
  int64_t total = m.R[0];
  for (int k = 0; k < kDigits; ++k) {
    g.R[k] = (uint32_t)m.R[k + 1];
    g.is[k] = (uint32_t)(m.is[k + 1] * elem);
    g.os[k] = (uint32_t)(m.os[k + 1] * elem);
  }
  g.R[kDigits - 1] /= (uint32_t)per;
  g.is[kDigits - 1] *= (uint32_t)per;
  g.os[kDigits - 1] *= (uint32_t)per;
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
  const uint8_t* pi = in + m.ibase * elem;
  uint8_t* po = out + m.obase * elem;
  switch (vec) {
    case 16: mapped_copy_kernel<16, BYTES><<<gx, kThreads, 0, ctx->stream>>>(pi, po, g); break;
    case 8: mapped_copy_kernel<8, BYTES><<<gx, kThreads, 0, ctx->stream>>>(pi, po, g); break;
    case 4: mapped_copy_kernel<4, BYTES><<<gx, kThreads, 0, ctx->stream>>>(pi, po, g); break;
    case 2: mapped_copy_kernel<2, BYTES><<<gx, kThreads, 0, ctx->stream>>>(pi, po, g); break;
    default: mapped_copy_kernel<1, BYTES><<<gx, kThreads, 0, ctx->stream>>>(pi, po, g); break;
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

// ---- chanperm ---------------------------------------------------------------------------------------------------------------
enum { kPermByte = 0, kPermQuad = 1, kPermPair = 2 };

// x / d for x < 2^16, d < 2^16 by one multiply: m = ceil(2^32 / d) (e = m d - 2^32 < d, x e < 2^32: exact); d == 1: m = 0
struct Div {
  uint32_t d, m;
};
Div make_divisor(uint32_t d) { return {d, d == 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d)}; }
__device__ __forceinline__ uint32_t div_by(uint32_t x, const Div& v) { return v.m ? __umulhi(x, v.m) : x; }

// one side of the transposition: a unit is r x r segments of `seg` bytes, segment (i, j) at i * row + j * seg
struct Side {
  int64_t img;        // bytes per image
  uint32_t row, org;  // bytes per physical row, offset of interior pixel (0, 0)
  uint32_t seg, r;
  Div per_seg;        // 16-byte chunks per segment
  Div by_r;
};
struct Perm {
  Side in, out;
  int64_t units;         // n * uh * uw
  uint32_t uh, uw;       // the unit grid of one image
  Div40 byW, byH;        // ... as multipliers (for indices below 2^19: a block's first unit, a unit inside a tile)
  int64_t simg;          // the tile stride gridDim.x * U in (image, row, column) digits
  uint32_t sy, sx;
  uint32_t A, B;
  Div byA, byQ;          // Q: 16-byte chunks per unit
  uint32_t pitch;        // LDS bytes per unit
  uint32_t U;            // units per tile
  ByteOps ops;
};
__device__ __forceinline__ uint32_t chunk_at(const Side& s, uint32_t q) {
  const uint32_t sg = div_by(q, s.per_seg), wi = q - sg * s.per_seg.d;
  const uint32_t i = div_by(sg, s.by_r), j = sg - i * s.by_r.d;
  return i * s.row + j * s.seg + wi * 16;
}
__device__ __forceinline__ int64_t unit_at(const Side& s, int64_t img, uint32_t uy, uint32_t ux) {
  return img * s.img + s.org + (int64_t)uy * s.r * s.row + (int64_t)ux * s.r * s.seg;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void chanperm_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Perm g) {
  __shared__ uint4 tile[kPermLds / 16];
  __shared__ int64_t ioff[kPermMaxUnits], ooff[kPermMaxUnits];
  const uint8_t* const lds = reinterpret_cast<const uint8_t*>(tile);
  const uint32_t Q = g.byQ.d;
  // the first unit of this block's first tile, blockIdx.x * U < 2^19, in (image, row, column) digits; stepped per tile
  const uint32_t f0 = blockIdx.x * g.U, frw = div40(f0, g.byW);
  uint32_t x0 = f0 - frw * g.uw;
  int64_t img0 = div40(frw, g.byH);
  uint32_t y0 = frw - (uint32_t)img0 * g.uh;
  const int64_t stride = (int64_t)gridDim.x * g.U;
  for (int64_t u0 = f0; u0 < g.units; u0 += stride) {
    const uint32_t Ut = (uint32_t)(g.units - u0 < (int64_t)g.U ? g.units - u0 : (int64_t)g.U);
    for (uint32_t u = threadIdx.x; u < Ut; u += kThreads) {  // once per unit: its digits are the tile's plus u's, with carries
      const uint32_t rw = div40(u, g.byW), dimg = div40(rw, g.byH);
      uint32_t ux = x0 + (u - rw * g.uw), uy = y0 + (rw - dimg * g.uh);
      uint32_t carry = ux >= g.uw ? 1u : 0u;
      ux -= carry ? g.uw : 0u;
      uy += carry;
      carry = uy >= g.uh ? 1u : 0u;
      uy -= carry ? g.uh : 0u;
      const int64_t img = img0 + dimg + carry;
      ioff[u] = unit_at(g.in, img, uy, ux);
      ooff[u] = unit_at(g.out, img, uy, ux);
    }
    __syncthreads();
    const uint32_t chunks = Ut * Q;
    for (uint32_t idx = threadIdx.x; idx < chunks; idx += kThreads) {
      const uint32_t u = div_by(idx, g.byQ), q = idx - u * Q;
      tile[u * (g.pitch / 16) + q] = *reinterpret_cast<const uint4*>(in + (ioff[u] + chunk_at(g.in, q)));
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < chunks; idx += kThreads) {
      const uint32_t u = div_by(idx, g.byQ), q = idx - u * Q;
      const uint8_t* const L = lds + u * g.pitch;
      uint32_t r[4];
      if (MODE == kPermPair) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b2 = 2 * (4 * q + j), col = b2 & ~3u, h = b2 & 2u;
          const uint32_t X = *reinterpret_cast<const uint32_t*>(L + col), Y = *reinterpret_cast<const uint32_t*>(L + g.B + col);
          r[j] = __builtin_amdgcn_perm(Y, X, 0x05010400u + h * 0x01010101u);  // [X[h], Y[h], X[h + 1], Y[h + 1]]
        }
      } else {
        uint32_t b = div_by(16 * q, g.byA), a = 16 * q - b * g.A;
        if (MODE == kPermQuad) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint8_t* p = L + (a * g.B + (b & ~3u));
            const uint32_t bb = b & 3u;
            const uint32_t L0 = *reinterpret_cast<const uint32_t*>(p), L1 = *reinterpret_cast<const uint32_t*>(p + g.B);
            const uint32_t L2 = *reinterpret_cast<const uint32_t*>(p + 2 * g.B), L3 = *reinterpret_cast<const uint32_t*>(p + 3 * g.B);
            const uint32_t sel = 0x0c0c0400u + bb * 0x0101u;  // [lo[bb], hi[bb], 0, 0]
            r[j] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(L3, L2, sel), __builtin_amdgcn_perm(L1, L0, sel), 0x05040100u);
            a += 4;
            if (a == g.A) { a = 0; ++b; }
          }
        } else {
          uint32_t addr = a * g.B + b;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint32_t x = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              x |= (uint32_t)L[addr] << (8 * i);
              ++a;
              addr += g.B;
              if (a == g.A) { a = 0; ++b; addr = b; }
            }
            r[j] = x;
          }
        }
      }
      *reinterpret_cast<uint4*>(out + (ooff[u] + chunk_at(g.out, q))) =
          make_uint4(fix4(r[0], g.ops), fix4(r[1], g.ops), fix4(r[2], g.ops), fix4(r[3], g.ops));
    }
    __syncthreads();  // the next tile overwrites the units and their offsets
    x0 += g.sx;
    uint32_t carry = x0 >= g.uw ? 1u : 0u;
    x0 -= carry ? g.uw : 0u;
    y0 += g.sy + carry;
    carry = y0 >= g.uh ? 1u : 0u;
    y0 -= carry ? g.uh : 0u;
    img0 += g.simg + carry;
  }
}

Side side_of(int c, int h, int w, int border, int r) {
  const NhwcGeom gm = buf_geom(c, h, w, border);
  Side s;
  s.img = gm.img; s.row = (uint32_t)gm.row; s.org = (uint32_t)gm.org;
  s.seg = (uint32_t)c; s.r = (uint32_t)r;
  s.per_seg = make_divisor((uint32_t)c / 16);
  s.by_r = make_divisor((uint32_t)r);
  return s;
}

int launch_perm(i8ie_ctx* ctx, int kind, int p0, const uint8_t* in, int in_border, uint8_t* out, int out_border, int n, int c, int h, int w,
                int oc, int oh, int ow, const ByteOps& ops) {
  Perm g;
  g.ops = ops;
  g.in = side_of(c, h, w, in_border, kind == I8IE_REARRANGE_PIXEL_UNSHUFFLE ? p0 : 1);
  g.out = side_of(oc, oh, ow, out_border, kind == I8IE_REARRANGE_PIXEL_SHUFFLE ? p0 : 1);
  g.uh = (uint32_t)(kind == I8IE_REARRANGE_PIXEL_UNSHUFFLE ? oh : h);
  g.uw = (uint32_t)(kind == I8IE_REARRANGE_PIXEL_UNSHUFFLE ? ow : w);
  g.units = (int64_t)n * g.uh * g.uw;
  if (kind == I8IE_REARRANGE_CHANNEL_SHUFFLE) { g.A = (uint32_t)p0; g.B = (uint32_t)(c / p0); }
  else if (kind == I8IE_REARRANGE_PIXEL_SHUFFLE) { g.A = (uint32_t)oc; g.B = (uint32_t)(p0 * p0); }
  else { g.A = (uint32_t)(p0 * p0); g.B = (uint32_t)c; }
  const uint32_t T = g.A * g.B, Q = T / 16;
  g.byA = make_divisor(g.A);
  g.byQ = make_divisor(Q);
  g.pitch = (Q % 2 ? Q : Q + 1) * 16;  // an odd number of 16-byte slots
  uint32_t U = (uint32_t)kPermLds / g.pitch;
  U = std::min(U, (uint32_t)kPermMaxUnits);
  U = std::min(U, std::max(1u, ((uint32_t)kPermTileChunks + Q - 1) / Q));
  g.U = U;
  const int64_t tiles = (g.units + U - 1) / U;
  const int gx = (int)std::min<int64_t>(tiles, kMaxBlocks);
  g.byW = make_div40(g.uw);
  g.byH = make_div40(g.uh);
  int64_t t = (int64_t)gx * U;  // (gx * U <= 2048 * 256 = 2^19)
  g.sx = (uint32_t)(t % g.uw);
  t /= g.uw;
  g.sy = (uint32_t)(t % g.uh);
  g.simg = t / g.uh;
  const int mode = g.A == 2 && g.B % 4 == 0 ? kPermPair : (g.A % 4 == 0 && g.B % 4 == 0 ? kPermQuad : kPermByte);
  if (mode == kPermPair) chanperm_kernel<kPermPair><<<gx, kThreads, 0, ctx->stream>>>(in, out, g);
  else if (mode == kPermQuad) chanperm_kernel<kPermQuad><<<gx, kThreads, 0, ctx->stream>>>(in, out, g);
  else chanperm_kernel<kPermByte><<<gx, kThreads, 0, ctx->stream>>>(in, out, g);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

// the widest item of 16 / 8 / 4 / 2 / 1 bytes that divides every one of `sizes` and to which both buffers are aligned.  Not
// item_width of i8ie_pointwise.h: that one answers 16 / 4 / 1 only, which is what every other pointwise kernel is instantiated
// for (widening it would hand them widths they have no instance of); the 8- and 2-byte items exist here alone, for the
// 8- and 58-channel slices a split leaves
int narrow_item(std::initializer_list<int64_t> sizes, const void* a, const void* b) {
  for (int v = 16; v > 1; v >>= 1) {
    bool ok = aligned_to(a, (unsigned)v) && aligned_to(b, (unsigned)v);
    for (int64_t s : sizes) ok = ok && s % v == 0;
    if (ok) return v;
  }
  return 1;
}

}  // namespace

extern "C" {

int i8ie_rearrange_output_shape(int kind, int p0, int p1, int n, int c, int h, int w, int* out_dims) {
  if (!out_dims) {
    i8ie_set_error("i8ie_rearrange_output_shape: null argument");
    return I8IE_ERR_ARG;
  }
  int oc = 0, oh = 0, ow = 0;
  if (!shape_of(kind, p0, p1, n, c, h, w, &oc, &oh, &ow)) return I8IE_ERR_ARG;
  out_dims[0] = n; out_dims[1] = oc; out_dims[2] = oh; out_dims[3] = ow;
  return I8IE_OK;
}

int i8ie_rearrange_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
                           int c, int h, int w, int kind, int p0, int p1, int relu, uint8_t zero_point) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "bad dimension");
  int oc = 0, oh = 0, ow = 0;
  if (!shape_of(kind, p0, p1, n, c, h, w, &oc, &oh, &ow)) return I8IE_ERR_ARG;
  const NhwcGeom gi = buf_geom(c, h, w, in_border), go = buf_geom(oc, oh, ow, out_border);
  I8IE_REQUIRE(gi.img <= 0x7FFFFFFF && go.img <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  const ByteOps ops = make_ops(in_s8, out_s8, relu, zero_point);
  const bool fallback = (ctx->options & 1u) != 0;
  const double bytes = 2.0 * (double)n * oc * oh * ow;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const Map m = map_of(kind, p0, n, c, h, w, oc, oh, ow, nhwc_plane(c, h, w, in_border), nhwc_plane(oc, oh, ow, out_border), true);
  if (kind == I8IE_REARRANGE_NARROW && !fallback) {
    const int vec = narrow_item({p0, p1, c}, in, out);
    I8ieProfScope prof(ctx, "narrow_u8_nhwc", 0.0, bytes);
    return launch_map<true>(ctx, m, 1, vec, in, out, ops);
  }
  if (kind != I8IE_REARRANGE_NARROW && !fallback && c % 16 == 0 && oc % 16 == 0 && aligned_to(in, 16) && aligned_to(out, 16) &&
      (int64_t)c * (kind == I8IE_REARRANGE_PIXEL_UNSHUFFLE ? p0 * p0 : 1) <= kPermMaxT) {
    I8ieProfScope prof(ctx, "chanperm_u8_nhwc", 0.0, bytes);
    return launch_perm(ctx, kind, p0, in, in_border, out, out_border, n, c, h, w, oc, oh, ow, ops);
  }
  I8ieProfScope prof(ctx, "rearrange_u8_direct", 0.0, bytes);
  return launch_map<true>(ctx, m, 1, 1, in, out, ops);
}

int i8ie_rearrange_u8(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int kind, int p0, int p1) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  int oc = 0, oh = 0, ow = 0;
  if (!shape_of(kind, p0, p1, n, c, h, w, &oc, &oh, &ow)) return I8IE_ERR_ARG;
  I8IE_REQUIRE((int64_t)c * h * w <= 0x7FFFFFFF && (int64_t)oc * oh * ow <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const Map m = map_of(kind, p0, n, c, h, w, oc, oh, ow, nchw_plane(c, h, w), nchw_plane(oc, oh, ow), false);
  I8ieProfScope prof(ctx, "rearrange_u8_nchw", 0.0, 2.0 * (double)n * oc * oh * ow);
  return launch_map<true>(ctx, m, 1, 1, in, out, make_ops(0, 0, 0, 0));
}

int i8ie_rearrange_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int c, int h, int w, int kind, int p0, int p1) {
  I8IE_REQUIRE(ctx && in && out, "null argument");
  I8IE_REQUIRE(aligned_to(in, 4) && aligned_to(out, 4), "buffers must be 4-byte aligned");
  int oc = 0, oh = 0, ow = 0;
  if (!shape_of(kind, p0, p1, n, c, h, w, &oc, &oh, &ow)) return I8IE_ERR_ARG;
  I8IE_REQUIRE(4 * (int64_t)c * h * w <= 0x7FFFFFFF && 4 * (int64_t)oc * oh * ow <= 0x7FFFFFFF, "an image of more than 2^31 bytes");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const Map m = map_of(kind, p0, n, c, h, w, oc, oh, ow, nchw_plane(c, h, w), nchw_plane(oc, oh, ow), false);
  I8ieProfScope prof(ctx, "rearrange_f32", 0.0, 8.0 * (double)n * oc * oh * ow);
  return launch_map<false>(ctx, m, 4, 4, (const uint8_t*)in, (uint8_t*)out, make_ops(0, 0, 0, 0));
}

}  // extern "C"
