// i8ie_mul.hip -- the quantized broadcast Mul: i8ie_mul_u8, i8ie_mul_u8_nhwc, i8ie_mul_f32.
//
// The reference has no multiply.  It is defined like the Add (i8ie_add.hip), as a composition of the reference's own
// expressions, dequantize (src/quantize_utils.cc:38-42) of both operands and down_scale's clamp and truncation
// (src/quantize_utils.cc:27-36), IEEE fp32, one rounding per operation, no contraction:
//     fa = (float)((int)a - (int)zp_a) * s_a;   fb = (float)((int)b - (int)zp_b) * s_b
//     t  = (fa * fb) / s_out + (float)zp_out
//     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t);   q = relu ? max(q, zp_out) : q        (relu<u8>, src/functional.cc:15-26)
// b has a's shape, or is a gate: one byte per image and channel, multiplied into every pixel of that image.
//
// Evaluation, bit-identical to that sequence for every byte pair (tests/test_gpu_mul.py runs all 65 536 of them through
// both forms).  Write x = fa * fb / s_out for the real-valued quotient of the fp32 numbers fa, fb, s_out.
//   exact    the sequence itself ((float)a - (float)zp_a is the exact integer difference).
//   guarded  an estimate e of t - 0.5, packed with v_cvt_pk_u8_f32 (round to nearest even, saturate).  A dword holding a
//            value closer than 2^-13 to a rounding boundary replays the exact sequence: the rule of i8ie_requant.h.
//            equal shapes:  P = fa * fb as above (the same three products), e = fma(P, r, zp_out - 0.5), r = fl(1 / s_out)
//                           from the host.  This is the Add's estimate with the product in the place of the sum, and its
//                           bound carries over: while |x| < 257 (which covers every t in (-1, 256), zp_out being in
//                           [0, 255]) the reference rounds twice behind P (the quotient, the sum: each <= 2^-16) and the
//                           estimate twice (r: 257 * 2^-24 < 2^-16, the fma: <= 2^-16), so |t - (e + 0.5)| < 6.2e-5 < 2^-13.
//            gate:          H = fl(fb * r) is computed once per gate byte and kept in a register; e = fma(fa, H, zp_out - 0.5),
//                           one fma per element where the equal-shape form has a product and an fma.  While |x| < 257 the
//                           reference rounds three times behind fa and fb (P: 257 * 2^-24 = 1.54e-5, the quotient and the
//                           sum: 2^-16 = 1.53e-5 each) and the estimate three times (r and H: 2 * 1.54e-5, the fma: 2^-16),
//                           so |t - (e + 0.5)| < 9.2e-5 < 2^-13: i8ie_requant.h's own figure.
//            Beyond |x| >= 257 both sides saturate whatever the guard says: t >= 255 or t < 0 on the one side,
//            e >= 256.4 or e <= -2.4 on the other (with the relu both give zp_out there).
//            Taken only for ordinary scales (i8ie_requant.h's rule): each scale, s_a * s_b and s_b / s_out in (1e-30, 1e30)
//            and the largest |x| below 1e30, so that P, r and H are normal numbers (or exact zeros) and the relative
//            bounds above hold.  Zero, denormal or huge scales run the exact sequence.
//
// The gate kernel.  An item is VEC bytes of one pixel's channels (VEC = 16 / 4 / 1 by c's divisibility and the buffers'
// alignment).  A block holds `rows` whole pixels of `lanes_c` items each (rows * lanes_c <= 256; consecutive lanes take
// consecutive channel items of one pixel, then the next pixel, so a wave's loads are contiguous), and every lane walks
// kWalk pixels of one image, `rows` pixels apart: its channel item never changes, so the gate's load, its VEC
// conversions and the multiply by r are paid once per kWalk * VEC output bytes.  Blocks stride over (image, channel
// chunk, pixel tile) units up to a grid cap.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kWalk = 8;  // pixels a lane of the gate kernel walks with one gate item in registers

struct MulParams {
  float sa, zpa, sb, zpb, sc, zpc;
  float rc, zph, lof;    // estimate: fl(1 / s_out), zp_out - 0.5, its lower clamp (relu: zp_out; else -1 = none, the pack saturates at 0)
  int lo;                // relu ? zp_out : 0
  int fast;              // the estimate may be used (ordinary scales)
  uint32_t xa, xb, xo;   // 0x80808080 where that buffer holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
};

// the exact sequence behind fb (plain bytes)
__device__ __forceinline__ uint32_t mul_exact_fb(uint32_t a, float fb, const MulParams& p) {
  const float fa = ((float)a - p.zpa) * p.sa;
  const float t = (fa * fb) / p.sc + p.zpc;
  const int u = (t >= 255.0f) ? 255 : ((t < 0.0f) ? 0 : (int)t);
  return (uint32_t)(u > p.lo ? u : p.lo);
}
__device__ __forceinline__ uint32_t mul_exact1(uint32_t a, uint32_t b, const MulParams& p) {
  return mul_exact_fb(a, ((float)b - p.zpb) * p.sb, p);
}

// four elements: a4 / b4 / the result as they lie in memory (re-biased or not)
__device__ __forceinline__ uint32_t mul4(uint32_t a4, uint32_t b4, const MulParams& p) {
  a4 ^= p.xa;
  b4 ^= p.xb;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = ((float)((a4 >> (8 * r)) & 0xFFu) - p.zpa) * p.sa;
      const float fb = ((float)((b4 >> (8 * r)) & 0xFFu) - p.zpb) * p.sb;
      const float e = __builtin_fmaf(fa * fb, p.rc, p.zph);
      packed = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaxf(e, p.lof), r, packed);
      worst = __builtin_fminf(worst, __builtin_fabsf(__builtin_amdgcn_fractf(e) - 0.5f));
    }
    if (worst >= 1.220703125e-4f) return packed ^ p.xo;  // 2^-13 > 6.2e-5, the proven bound
  }
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= mul_exact1((a4 >> (8 * r)) & 0xFFu, (b4 >> (8 * r)) & 0xFFu, p) << (8 * r);
  return packed ^ p.xo;
}
__device__ __forceinline__ uint8_t mul1(uint8_t a, uint8_t b, const MulParams& p) {
  return (uint8_t)(mul_exact1((a ^ p.xa) & 0xFFu, (b ^ p.xb) & 0xFFu, p) ^ (p.xo & 0xFFu));
}
__device__ __forceinline__ uint4 mul16(uint4 x, const uint4& y, const MulParams& p) {
  x.x = mul4(x.x, y.x, p);
  x.y = mul4(x.y, y.y, p);
  x.z = mul4(x.z, y.z, p);
  x.w = mul4(x.w, y.w, p);
  return x;
}

// ---- flat form: one physical order, no border.  out may alias a or b: a lane reads its 16 bytes before it stores them.
__global__ __launch_bounds__(kThreads) void mul_u8_flat_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n,
                                                               MulParams p) {
  const int64_t nvec = n >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    const uint4 x = reinterpret_cast<const uint4*>(a)[v];
    const uint4 y = reinterpret_cast<const uint4*>(b)[v];
    reinterpret_cast<uint4*>(out)[v] = mul16(x, y, p);
  }
  const int64_t t0 = nvec << 4;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = mul1(a[t0 + threadIdx.x], b[t0 + threadIdx.x], p);
}

// ---- bordered NHWC form, equal shapes: [n][h + 2b][w + 2b][c] per buffer, each with its own b.  The w * c interior bytes of
// an image row are the contiguous unit; an item is VEC bytes of one row.  Only the interior of `out` is written.
template <int VEC, typename Idx>
__global__ __launch_bounds__(kThreads) void mul_u8_nhwc_kernel(const uint8_t* __restrict__ a, NhwcGeom ga, const uint8_t* __restrict__ b,
                                                               NhwcGeom gb, uint8_t* __restrict__ out, NhwcGeom go, Idx items, Idx per_row,
                                                               Idx h, MulParams p) {
  const Idx stride = (Idx)gridDim.x * kThreads;
  for (Idx v = (Idx)blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const Idx r = v / per_row;
    const int64_t col = (int64_t)(v - r * per_row) * VEC;
    const Idx img = r / h;
    const int64_t y = (int64_t)(r - img * h);
    const uint8_t* pa = a + (int64_t)img * ga.img + ga.org + y * ga.row + col;
    const uint8_t* pb = b + (int64_t)img * gb.img + gb.org + y * gb.row + col;
    uint8_t* po = out + (int64_t)img * go.img + go.org + y * go.row + col;
    if (VEC == 16)
      *reinterpret_cast<uint4*>(po) = mul16(*reinterpret_cast<const uint4*>(pa), *reinterpret_cast<const uint4*>(pb), p);
    else if (VEC == 4)
      *reinterpret_cast<uint32_t*>(po) = mul4(*reinterpret_cast<const uint32_t*>(pa), *reinterpret_cast<const uint32_t*>(pb), p);
    else
      *po = mul1(*pa, *pb, p);
  }
}

// ---- gate form: a and out as above, the gate [n][1 + 2b][1 + 2b][c] (plain rows [n][c] at b = 0)
struct MulGate {
  int64_t g_img, g_org;    // the gate: bytes per image, offset of its one pixel
  int64_t units;           // n * chunks * tiles
  int cpv;                 // items per pixel: c / VEC
  int lanes_c, rows;       // a block's shape: lanes_c = min(cpv, 256) items by rows = 256 / lanes_c pixels
  int chunks, tiles;       // channel chunks of lanes_c items per pixel; tiles of rows * kWalk pixels per image
  int hw, w, c;
  int step_x;              // rows % w: how far a lane's column moves per step (its row moves by rows / w, +1 where the column wraps)
  int64_t a_step, a_wrap;  // ... and its byte offset in a: rows / w physical rows + step_x pixels; the extra 2 * border pixels of a wrap
  int64_t o_step, o_wrap;
};

// four elements against four gate values: h4 = fl(fb * r) of the four channels (estimate), g4 their plain bytes (replay)
__device__ __forceinline__ uint32_t gate4(uint32_t a4, const float* h4, uint32_t g4, const MulParams& p) {
  a4 ^= p.xa;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = ((float)((a4 >> (8 * r)) & 0xFFu) - p.zpa) * p.sa;
      const float e = __builtin_fmaf(fa, h4[r], p.zph);
      packed = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaxf(e, p.lof), r, packed);
      worst = __builtin_fminf(worst, __builtin_fabsf(__builtin_amdgcn_fractf(e) - 0.5f));
    }
    if (worst >= 1.220703125e-4f) return packed ^ p.xo;  // 2^-13 > 9.2e-5, the proven bound
  }
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= mul_exact1((a4 >> (8 * r)) & 0xFFu, (g4 >> (8 * r)) & 0xFFu, p) << (8 * r);
  return packed ^ p.xo;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void mul_u8_gate_kernel(const uint8_t* __restrict__ a, NhwcGeom ga, const uint8_t* __restrict__ g,
                                                               uint8_t* __restrict__ out, NhwcGeom go, MulGate t, MulParams p) {
  constexpr int W = VEC >= 4 ? VEC / 4 : 1;  // dwords per item
  const int pc = (int)threadIdx.x / t.lanes_c, ci = (int)threadIdx.x - pc * t.lanes_c;
  if (pc >= t.rows) return;  // (the lanes behind the block's last whole pixel)
  for (int64_t u = blockIdx.x; u < t.units; u += gridDim.x) {
    const int tile = (int)(u % t.tiles);
    const int64_t rest = u / t.tiles;
    const int chan = (int)(rest % t.chunks) * t.lanes_c + ci;
    const int64_t img = rest / t.chunks;
    int pix = tile * (t.rows * kWalk) + pc;
    if (chan >= t.cpv || pix >= t.hw) continue;
    // the gate item of (img, chan): its plain bytes, and for the estimate fl(fb * r) of each
    const uint8_t* pg = g + img * t.g_img + t.g_org + (int64_t)chan * VEC;
    uint32_t gw[W];
    float hv[VEC];
    if constexpr (VEC == 16) {
      const uint4 q = *reinterpret_cast<const uint4*>(pg);
      gw[0] = q.x ^ p.xb; gw[1] = q.y ^ p.xb; gw[2] = q.z ^ p.xb; gw[3] = q.w ^ p.xb;
    } else if constexpr (VEC == 4) {
      gw[0] = *reinterpret_cast<const uint32_t*>(pg) ^ p.xb;
    } else {
      gw[0] = (uint32_t)*pg ^ (p.xb & 0xFFu);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float fb = ((float)((gw[j / 4] >> (8 * (j % 4))) & 0xFFu) - p.zpb) * p.sb;
      hv[j] = VEC == 1 ? fb : fb * p.rc;  // (one byte per lane takes the exact sequence behind fb)
    }
    const int y = pix / t.w;
    int x = pix - y * t.w;
    int64_t oa = img * ga.img + ga.org + (int64_t)y * ga.row + (int64_t)x * t.c + (int64_t)chan * VEC;
    int64_t oo = img * go.img + go.org + (int64_t)y * go.row + (int64_t)x * t.c + (int64_t)chan * VEC;
#pragma unroll 2
    for (int k = 0; k < kWalk; ++k) {
      if constexpr (VEC == 16) {
        uint4 v = *reinterpret_cast<const uint4*>(a + oa);
        v.x = gate4(v.x, hv, gw[0], p);
        v.y = gate4(v.y, hv + 4, gw[1], p);
        v.z = gate4(v.z, hv + 8, gw[2], p);
        v.w = gate4(v.w, hv + 12, gw[3], p);
        *reinterpret_cast<uint4*>(out + oo) = v;
      } else if constexpr (VEC == 4) {
        *reinterpret_cast<uint32_t*>(out + oo) = gate4(*reinterpret_cast<const uint32_t*>(a + oa), hv, gw[0], p);
      } else {
        out[oo] = (uint8_t)(mul_exact_fb((a[oa] ^ p.xa) & 0xFFu, hv[0], p) ^ (p.xo & 0xFFu));
      }
      pix += t.rows;
      if (pix >= t.hw) break;
      x += t.step_x;
      oa += t.a_step;
      oo += t.o_step;
      if (x >= t.w) {
        x -= t.w;
        oa += t.a_wrap;
        oo += t.o_wrap;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void mul_f32_kernel(const float* a, const float* b, float* out, int64_t n) {
  const int64_t nvec = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    float4 x = reinterpret_cast<const float4*>(a)[v];
    const float4 y = reinterpret_cast<const float4*>(b)[v];
    x.x *= y.x; x.y *= y.y; x.z *= y.z; x.w *= y.w;
    reinterpret_cast<float4*>(out)[v] = x;
  }
  const int64_t t0 = nvec << 2;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = a[t0 + threadIdx.x] * b[t0 + threadIdx.x];
}
// the gate form in FP32 (NCHW: one gate value per run of h * w elements); the path of calibration, not of inference
__global__ __launch_bounds__(kThreads) void mul_f32_gate_kernel(const float* a, const float* g, float* out, int64_t n, int64_t run) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < n; v += stride) out[v] = a[v] * g[v / run];
}

// (in double, unlike the pointwise units' shared ordinary(float): the bound above is stated on the double products and quotients)
inline bool ordinary_d(double s) { return s > 1e-30 && s < 1e30; }

MulParams make_params(float s_a, int zp_a, float s_b, int zp_b, float s_out, int zp_out, int relu, int a_s8, int b_s8, int out_s8) {
  MulParams p;
  p.sa = s_a; p.zpa = (float)zp_a; p.sb = s_b; p.zpb = (float)zp_b; p.sc = s_out; p.zpc = (float)zp_out;
  p.rc = 1.0f / s_out;
  p.zph = (float)zp_out - 0.5f;
  p.lof = relu ? (float)zp_out : -1.0f;
  p.lo = relu ? zp_out : 0;
  // the estimate only where nothing can overflow or go denormal on the way: ordinary scales, an ordinary s_a * s_b (the
  // smallest nonzero |P|), an ordinary s_b / s_out (the smallest nonzero |H|) and an ordinary largest |P / s_out|
  const double top = 255.0 * 255.0 * (double)s_a * (double)s_b / (double)s_out;
  p.fast = (ordinary_d(s_a) && ordinary_d(s_b) && ordinary_d(s_out) && ordinary_d((double)s_a * (double)s_b) &&
            ordinary_d((double)s_b / (double)s_out) && top < 1e30) ? 1 : 0;
  p.xa = a_s8 ? 0x80808080u : 0u;
  p.xb = b_s8 ? 0x80808080u : 0u;
  p.xo = out_s8 ? 0x80808080u : 0u;
  return p;
}

template <int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* a, const NhwcGeom& ga, const uint8_t* b, const NhwcGeom& gb, uint8_t* out,
                 const NhwcGeom& go, int n, int c, int h, int w, const MulParams& p) {
  const int64_t per_row = (int64_t)w * c / VEC, items = (int64_t)n * h * per_row;
  if (items <= 0x7FFFFFFF)
    mul_u8_nhwc_kernel<VEC, uint32_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, (uint32_t)items,
                                                                                     (uint32_t)per_row, (uint32_t)h, p);
  else
    mul_u8_nhwc_kernel<VEC, int64_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, items, per_row,
                                                                                    (int64_t)h, p);
}

template <int VEC>
void launch_gate(i8ie_ctx* ctx, const uint8_t* a, const NhwcGeom& ga, const uint8_t* g, int g_border, uint8_t* out, const NhwcGeom& go,
                 int n, int c, int h, int w, const MulParams& p) {
  MulGate t;
  const NhwcGeom gg = buf_geom(c, 1, 1, g_border);
  t.g_img = gg.img;
  t.g_org = gg.org;
  t.cpv = c / VEC;
  t.lanes_c = t.cpv < kThreads ? t.cpv : kThreads;
  t.rows = kThreads / t.lanes_c;
  t.chunks = (t.cpv + t.lanes_c - 1) / t.lanes_c;
  t.hw = h * w;
  t.w = w;
  t.c = c;
  t.tiles = (t.hw + t.rows * kWalk - 1) / (t.rows * kWalk);
  t.units = (int64_t)n * t.chunks * t.tiles;
  const int step_y = t.rows / w;
  t.step_x = t.rows % w;
  t.a_step = step_y * ga.row + (int64_t)t.step_x * c;
  t.a_wrap = ga.row - (int64_t)w * c;
  t.o_step = step_y * go.row + (int64_t)t.step_x * c;
  t.o_wrap = go.row - (int64_t)w * c;
  const int blocks = (int)(t.units > kMaxBlocks ? kMaxBlocks : t.units);
  mul_u8_gate_kernel<VEC><<<blocks, kThreads, 0, ctx->stream>>>(a, ga, g, out, go, t, p);
}

}  // namespace

extern "C" {

int i8ie_mul_u8(i8ie_ctx* ctx, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, float s_a, uint8_t zp_a, float s_b,
                uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "mul_u8", 0.0, 3.0 * n);
  mul_u8_flat_kernel<<<grid_for((n >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n,
                                                                         make_params(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, 0, 0, 0));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_mul_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8, int b_gate,
                     uint8_t* out, int out_border, int out_s8, int n, int c, int h, int w, float s_a, uint8_t zp_a, float s_b,
                     uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && a_border >= 0 && b_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE((int64_t)h * w <= 0x3FFFFFFF, "bad dimension: more than 2^30 pixels per image");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const MulParams p = make_params(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, a_s8, b_s8, out_s8);
  const int64_t total = (int64_t)n * c * h * w;
  const bool al16 = aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16);
  const bool al4 = aligned_to(a, 4) && aligned_to(b, 4) && aligned_to(out, 4);
  const NhwcGeom ga = buf_geom(c, h, w, a_border), go = buf_geom(c, h, w, out_border);
  if (b_gate) {
    I8ieProfScope prof(ctx, "mul_u8_gate", 0.0, 2.0 * total + (double)n * c);
    if (c % 16 == 0 && al16) launch_gate<16>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
    else if (c % 4 == 0 && al4) launch_gate<4>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
    else launch_gate<1>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  I8ieProfScope prof(ctx, "mul_u8_nhwc", 0.0, 3.0 * total);
  if (a_border == 0 && b_border == 0 && out_border == 0 && al16) {  // one physical order, no border: the flat form
    mul_u8_flat_kernel<<<grid_for((total >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, total, p);
  } else {
    const NhwcGeom gb = buf_geom(c, h, w, b_border);
    if (c % 16 == 0 && al16) launch_nhwc<16>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else if (c % 4 == 0 && al4) launch_nhwc<4>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else launch_nhwc<1>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_mul_f32(i8ie_ctx* ctx, const float* a, const float* b, float* out, int64_t n, int64_t gate_run) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0 && gate_run >= 0, "negative size");
  I8IE_REQUIRE(gate_run == 0 || n % gate_run == 0, "the gate's run must divide the size");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(out, 16) && aligned_to(b, gate_run ? 4 : 16), "buffers must be 16-byte aligned (a gate: 4-byte)");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "mul_f32", 0.0, gate_run ? 8.0 * n : 12.0 * n);
  if (gate_run) mul_f32_gate_kernel<<<grid_for(n), kThreads, 0, ctx->stream>>>(a, b, out, n, gate_run);
  else mul_f32_kernel<<<grid_for((n >> 2) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
