// i8ie_concat.hip -- quantized channel concatenation: i8ie_concat_u8, i8ie_concat_u8_nhwc, i8ie_concat_f32.
//
// The reference has no concat.  Each input byte a, with its tensor's (s_i, zp_i), becomes a byte of the result's (s_out, zp_out)
// by a composition of the reference's own expressions, dequantize (src/quantize_utils.cc:38-42) and down_scale's clamp and
// truncation (src/quantize_utils.cc:27-36), IEEE fp32, one rounding per operation, no contraction:
//     copy rule:  bits(s_i) == bits(s_out) && zp_i == zp_out  ->  q = a
//     otherwise:  f = (float)((int)a - (int)zp_i) * s_i;   t = f / s_out + (float)zp_out
//                 q = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)
//     q = relu ? max(q, zp_out) : q                                                      (relu<u8>, src/functional.cc:15-26)
// The copy rule is part of the definition: the literal sequence is not the identity at equal parameters.
//
// One launch for all k inputs: blockIdx.y names the input, its descriptor comes by value in the kernel arguments.  An input is
// `units` contiguous runs of `c` bytes (NHWC: one pixel's channels; run form: one outer row's len_i bytes), cut into items of
// VEC = 16 / 4 / 1 bytes, the widest that divides c_i, the input's offset in the output unit and the output unit (every item is
// then VEC-aligned on both sides).  A lane decomposes its first item index (< 2^19: 32-bit divisions) once and then steps
// (item, pixel, row, image) by the grid stride, which the host decomposed the same way: no division in the loop, none in 64 bits.
//
// Evaluation, bit-identical to the sequence for every byte (tests/test_gpu_concat.py runs all 256 of them per parameter set):
//   copy     bytes only: ^0x80 where the two sides differ in re-bias, a packed max for the relu.
//   exact    the sequence itself ((float)a - (float)zp_i is the exact integer difference).
//   guarded  f as above (the same one product), then e = fma(f, r, zp_out - 0.5) with r = fl(1 / s_out) from the host, packed
//            with v_cvt_pk_u8_f32 (round to nearest even, saturate).  A dword holding a value closer than 2^-13 to a rounding
//            boundary replays the exact sequence: the guarded pack of i8ie_requant.h.
//            Bound: while |f / s_out| < 257 (which covers every t in (-1, 256), zp_out being in [0, 255]) every value involved
//            is below 512, where half an ulp is 2^-16.  The reference rounds twice (the quotient, the sum: each <= 2^-16); the
//            estimate has the relative error 2^-24 of r on a product below 257 (<= 257 * 2^-24 < 2^-15.99) and the one rounding
//            of the fma (<= 2^-16).  f itself is the same number on both sides.  So |t - (e + 0.5)| < 3 * 2^-16 + 257 * 2^-24
//            < 6.2e-5 < 2^-13.  Beyond that range both sides saturate: both are monotone in f.
//            Taken only for ordinary scales (i8ie_requant.h's rule): zero, denormal or huge scales run the exact sequence.
#include <cmath>
#include <cstring>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_requant.h"

namespace {

enum { kCopy = 0, kGuarded = 1, kExact = 2 };

struct CatIn {
  const uint8_t* p;
  int64_t img, row, org;  // bytes per image and per physical row, offset of interior pixel (0, 0); run form: img = len_i, rest 0
  int64_t items;          // units * per
  int64_t simg;           // the grid stride in items = ((simg * h + sy) * w + sx) * per + sj
  uint32_t sy, sx, sj;
  uint32_t c;     // bytes per unit
  uint32_t off;   // byte offset of this input inside an output unit
  uint32_t per;   // items per unit: c / vec
  uint32_t vec;   // 16 / 4 / 1
  uint32_t mode;  // kCopy / kGuarded / kExact
  uint32_t x;     // 0x80808080 where the input holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
  float s, zp;
};
struct CatOut {
  uint8_t* p;
  int64_t img, row, org;
  uint32_t c;      // bytes per output unit: the sum of the inputs'
  uint32_t h, w;   // NHWC: image rows and pixels per row (run form: 1, 1)
  uint32_t x;      // re-bias of the result
  float sc, zpc;   // s_out, zp_out
  float rc, zph, lof;  // estimate: fl(1 / s_out), zp_out - 0.5, its lower clamp (relu: zp_out; else -1 = none, the pack saturates at 0)
  int lo;          // relu ? zp_out : 0
  uint32_t lo2;    // lo in both 16-bit halves (the packed max of the copy path)
};
struct CatArgs {
  CatOut out;
  CatIn in[I8IE_CONCAT_MAX_INPUTS];
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// max(a, lo) on four bytes: even and odd bytes as two pairs of 16-bit lanes (v_pk_max_u16)
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t lo2) {
  const us2 z = __builtin_bit_cast(us2, lo2);
  const us2 e = __builtin_elementwise_max(__builtin_bit_cast(us2, a & 0x00FF00FFu), z);
  const us2 o = __builtin_elementwise_max(__builtin_bit_cast(us2, (a >> 8) & 0x00FF00FFu), z);
  return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}

__device__ __forceinline__ uint32_t cat_exact1(uint32_t a, const CatIn& d, const CatOut& o) {
  const float f = ((float)a - d.zp) * d.s;
  const float t = f / o.sc + o.zpc;
  const int u = (t >= 255.0f) ? 255 : ((t < 0.0f) ? 0 : (int)t);
  return (uint32_t)(u > o.lo ? u : o.lo);
}

// four elements as they lie in memory (re-biased or not) -> four bytes of the result as they lie
__device__ __forceinline__ uint32_t cat4(uint32_t a4, const CatIn& d, const CatOut& o) {
  a4 ^= d.x;
  if (d.mode == kCopy) return max_u8x4(a4, o.lo2) ^ o.x;
  if (d.mode == kGuarded) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float f = ((float)((a4 >> (8 * r)) & 0xFFu) - d.zp) * d.s;
      packed = i8ie_requant_est_step(__builtin_fmaf(f, o.rc, o.zph), o.lof, r, packed, worst);
    }
    if (i8ie_requant_est_ok(worst)) return packed ^ o.x;
  }
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= cat_exact1((a4 >> (8 * r)) & 0xFFu, d, o) << (8 * r);
  return packed ^ o.x;
}
__device__ __forceinline__ uint8_t cat1(uint8_t a, const CatIn& d, const CatOut& o) {
  const uint32_t v = (a ^ d.x) & 0xFFu;
  const uint32_t q = d.mode == kCopy ? (v > (uint32_t)o.lo ? v : (uint32_t)o.lo) : cat_exact1(v, d, o);
  return (uint8_t)(q ^ (o.x & 0xFFu));
}

template <int VEC, bool NHWC, typename Idx>
__device__ __forceinline__ void cat_items(const CatIn& d, const CatOut& o) {
  const uint32_t v0 = blockIdx.x * kThreads + threadIdx.x;  // < kMaxBlocks * kThreads = 2^19
  if ((int64_t)v0 >= d.items) return;
  uint32_t unit = v0 / d.per;
  uint32_t j = v0 - unit * d.per, x = 0, y = 0;
  if (NHWC) {
    const uint32_t r = unit / o.w;
    x = unit - r * o.w;
    unit = r / o.h;
    y = r - unit * o.h;
  }
  int64_t img = unit;
  const Idx items = (Idx)d.items, stride = (Idx)gridDim.x * kThreads;
  for (Idx v = v0; v < items; v += stride) {
    const uint8_t* src = d.p + img * d.img + j * VEC;
    uint8_t* dst = o.p + img * o.img + (d.off + j * VEC);
    if (NHWC) {
      src += d.org + (int64_t)y * d.row + (int64_t)x * d.c;
      dst += o.org + (int64_t)y * o.row + (int64_t)x * o.c;
    }
    if (VEC == 16) {
      uint4 q = *reinterpret_cast<const uint4*>(src);
      q.x = cat4(q.x, d, o);
      q.y = cat4(q.y, d, o);
      q.z = cat4(q.z, d, o);
      q.w = cat4(q.w, d, o);
      *reinterpret_cast<uint4*>(dst) = q;
    } else if (VEC == 4) {
      *reinterpret_cast<uint32_t*>(dst) = cat4(*reinterpret_cast<const uint32_t*>(src), d, o);
    } else {
      *dst = cat1(*src, d, o);
    }
    // step by the grid stride, carrying upwards (each sum stays below twice its modulus: one subtraction is enough)
    j += d.sj;
    uint32_t carry = j >= d.per ? 1u : 0u;
    j -= carry ? d.per : 0u;
    if (NHWC) {
      x += d.sx + carry;
      carry = x >= o.w ? 1u : 0u;
      x -= carry ? o.w : 0u;
      y += d.sy + carry;
      carry = y >= o.h ? 1u : 0u;
      y -= carry ? o.h : 0u;
    }
    img += d.simg + carry;
  }
}

template <bool NHWC, typename Idx>
__global__ __launch_bounds__(kThreads) void concat_kernel(const CatArgs a) {
  const CatIn& d = a.in[blockIdx.y];
  if (d.vec == 16) cat_items<16, NHWC, Idx>(d, a.out);
  else if (d.vec == 4) cat_items<4, NHWC, Idx>(d, a.out);
  else cat_items<1, NHWC, Idx>(d, a.out);
}

inline uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

void set_out(CatOut& o, uint8_t* out, float s_out, int zp_out, int relu, int out_s8) {
  o.p = out;
  o.x = out_s8 ? 0x80808080u : 0u;
  o.sc = s_out;
  o.zpc = (float)zp_out;
  o.rc = 1.0f / s_out;
  o.zph = (float)zp_out - 0.5f;
  o.lof = relu ? (float)zp_out : -1.0f;
  o.lo = relu ? zp_out : 0;
  o.lo2 = (uint32_t)o.lo * 0x00010001u;
}
int mode_of(float s_i, int zp_i, float s_out, int zp_out) {
  if (bits_of(s_i) == bits_of(s_out) && zp_i == zp_out) return kCopy;
  // the estimate only where nothing can overflow or go denormal on the way: ordinary scales and an ordinary largest |f / s_out|
  const double top = 255.0 * (double)std::fabs(s_i) / (double)s_out;
  return (ordinary(s_i) && ordinary(s_out) && top < 1e30) ? kGuarded : kExact;
}
// items of 16 / 4 / 1 bytes: the widest that divides the input's unit, its offset in the output unit, the output unit, and
// both base addresses
uint32_t vec_of(int64_t c, int64_t off, int64_t total, const void* in, const void* out) {
  return (uint32_t)item_width({c, off, total}, {in, out});
}
// items of input i and the grid stride in its own (image, row, pixel, item) digits
void set_walk(CatIn& d, int64_t units, uint32_t h, uint32_t w, int64_t stride) {
  d.per = d.c / d.vec;
  d.items = units * d.per;
  d.sj = (uint32_t)(stride % d.per);
  int64_t t = stride / d.per;
  d.sx = (uint32_t)(t % w);
  t /= w;
  d.sy = (uint32_t)(t % h);
  d.simg = t / h;
}

template <bool NHWC>
int launch(i8ie_ctx* ctx, CatArgs& a, int k, int64_t units) {
  int64_t most = 0;
  for (int i = 0; i < k; ++i) most = std::max(most, units * (int64_t)(a.in[i].c / a.in[i].vec));
  const int gx = grid_for(most);
  for (int i = 0; i < k; ++i) set_walk(a.in[i], units, a.out.h, a.out.w, (int64_t)gx * kThreads);
  for (int i = k; i < I8IE_CONCAT_MAX_INPUTS; ++i) a.in[i] = a.in[0];
  const dim3 grid(gx, k);
  if (most <= 0x7FFFFFFF) concat_kernel<NHWC, uint32_t><<<grid, kThreads, 0, ctx->stream>>>(a);
  else concat_kernel<NHWC, int64_t><<<grid, kThreads, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

// the run form on `unit`-byte elements (1: u8, 4: fp32 moved as bytes): outer x (k runs of len[i] elements)
int run_form(i8ie_ctx* ctx, const char* name, int k, const void* const* in, const int64_t* len, const float* s_in, const uint8_t* zp_in,
             void* out, int64_t outer, int unit, float s_out, int zp_out, int relu) {
  CatArgs a;
  std::memset(&a, 0, sizeof(a));
  set_out(a.out, (uint8_t*)out, s_out, zp_out, relu, 0);
  int64_t total = 0;
  for (int i = 0; i < k; ++i) total += len[i] * unit;
  I8IE_REQUIRE(total <= 0x7FFFFFFF, "more than 2^31 - 1 bytes in one row of the result");
  a.out.img = total;
  a.out.c = (uint32_t)total;
  a.out.h = a.out.w = 1;
  int64_t off = 0;
  for (int i = 0; i < k; ++i) {
    CatIn& d = a.in[i];
    d.p = (const uint8_t*)in[i];
    d.img = len[i] * unit;
    d.c = (uint32_t)d.img;
    d.off = (uint32_t)off;
    d.vec = vec_of(d.img, off, total, in[i], out);
    d.mode = s_in ? mode_of(s_in[i], zp_in[i], s_out, zp_out) : kCopy;
    d.s = s_in ? s_in[i] : 1.0f;
    d.zp = s_in ? (float)zp_in[i] : 0.0f;
    off += d.img;
  }
  if (outer == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, name, 0.0, 2.0 * (double)outer * (double)total);
  return launch<false>(ctx, a, k, outer);
}

bool scales_ok(int k, const float* s_in, float s_out) {
  for (int i = 0; i < k; ++i)
    if (!std::isfinite(s_in[i])) return false;
  return std::isfinite(s_out) && s_out > 0.0f;
}
template <typename T>
bool none_null(int k, const T* const* in) {
  for (int i = 0; i < k; ++i)
    if (!in[i]) return false;
  return true;
}
bool all_positive(int k, const int64_t* len) {
  for (int i = 0; i < k; ++i)
    if (len[i] <= 0) return false;
  return true;
}

}  // namespace

extern "C" {

int i8ie_concat_u8(i8ie_ctx* ctx, int k, const uint8_t* const* in, const int64_t* len, const float* s_in, const uint8_t* zp_in,
                   uint8_t* out, int64_t outer, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && in && len && s_in && zp_in && out, "null argument");
  I8IE_REQUIRE(k >= 1 && k <= I8IE_CONCAT_MAX_INPUTS, "between 1 and I8IE_CONCAT_MAX_INPUTS inputs");
  I8IE_REQUIRE(none_null(k, in), "null argument");
  I8IE_REQUIRE(outer >= 0 && all_positive(k, len), "bad dimension");
  I8IE_REQUIRE(scales_ok(k, s_in, s_out), "scales must be finite and the output scale positive");
  return run_form(ctx, "concat_u8", k, (const void* const*)in, len, s_in, zp_in, out, outer, 1, s_out, zp_out, relu);
}

int i8ie_concat_u8_nhwc(i8ie_ctx* ctx, int k, const uint8_t* const* in, const int* c_in, const int* border_in, const int* s8_in,
                        const float* s_in, const uint8_t* zp_in, uint8_t* out, int out_border, int out_s8, int n, int h, int w,
                        float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && in && c_in && border_in && s8_in && s_in && zp_in && out, "null argument");
  I8IE_REQUIRE(k >= 1 && k <= I8IE_CONCAT_MAX_INPUTS, "between 1 and I8IE_CONCAT_MAX_INPUTS inputs");
  I8IE_REQUIRE(none_null(k, in), "null argument");
  I8IE_REQUIRE(n > 0 && h > 0 && w > 0 && out_border >= 0, "bad dimension");
  int64_t ctot = 0;
  bool plain = out_border == 0 && !out_s8;
  for (int i = 0; i < k; ++i) {
    I8IE_REQUIRE(c_in[i] > 0 && border_in[i] >= 0, "bad dimension");
    ctot += c_in[i];
    plain = plain && border_in[i] == 0 && !s8_in[i];
  }
  I8IE_REQUIRE(ctot <= 0x7FFFFFFF, "more than 2^31 - 1 channels in the result");
  I8IE_REQUIRE(scales_ok(k, s_in, s_out), "scales must be finite and the output scale positive");
  if (plain) {  // nothing bordered or re-biased: n * h * w runs of c_i bytes, the run form
    int64_t len[I8IE_CONCAT_MAX_INPUTS];
    for (int i = 0; i < k; ++i) len[i] = c_in[i];
    return run_form(ctx, "concat_u8_nhwc", k, (const void* const*)in, len, s_in, zp_in, out, (int64_t)n * h * w, 1, s_out, zp_out, relu);
  }
  CatArgs a;
  std::memset(&a, 0, sizeof(a));
  set_out(a.out, out, s_out, zp_out, relu, out_s8);
  a.out.c = (uint32_t)ctot;
  a.out.h = (uint32_t)h;
  a.out.w = (uint32_t)w;
  a.out.row = (int64_t)(w + 2 * out_border) * ctot;
  a.out.img = (int64_t)(h + 2 * out_border) * a.out.row;
  a.out.org = (int64_t)out_border * a.out.row + (int64_t)out_border * ctot;
  int64_t off = 0;
  for (int i = 0; i < k; ++i) {
    CatIn& d = a.in[i];
    const int b = border_in[i];
    d.p = in[i];
    d.c = (uint32_t)c_in[i];
    d.row = (int64_t)(w + 2 * b) * c_in[i];
    d.img = (int64_t)(h + 2 * b) * d.row;
    d.org = (int64_t)b * d.row + (int64_t)b * c_in[i];
    d.off = (uint32_t)off;
    d.vec = vec_of(c_in[i], off, ctot, in[i], out);
    d.mode = mode_of(s_in[i], zp_in[i], s_out, zp_out);
    d.x = s8_in[i] ? 0x80808080u : 0u;
    d.s = s_in[i];
    d.zp = (float)zp_in[i];
    off += c_in[i];
  }
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "concat_u8_nhwc", 0.0, 2.0 * (double)n * h * w * (double)ctot);
  return launch<true>(ctx, a, k, (int64_t)n * h * w);
}

int i8ie_concat_f32(i8ie_ctx* ctx, int k, const float* const* in, const int64_t* len, float* out, int64_t outer) {
  I8IE_REQUIRE(ctx && in && len && out, "null argument");
  I8IE_REQUIRE(k >= 1 && k <= I8IE_CONCAT_MAX_INPUTS, "between 1 and I8IE_CONCAT_MAX_INPUTS inputs");
  I8IE_REQUIRE(none_null(k, in), "null argument");
  I8IE_REQUIRE(outer >= 0 && all_positive(k, len), "bad dimension");
  I8IE_REQUIRE(aligned_to(out, 4), "buffers must be 4-byte aligned");
  for (int i = 0; i < k; ++i) I8IE_REQUIRE(aligned_to(in[i], 4), "buffers must be 4-byte aligned");
  return run_form(ctx, "concat_f32", k, (const void* const*)in, len, nullptr, nullptr, out, outer, 4, 1.0f, 0, 0);
}

}  // extern "C"
