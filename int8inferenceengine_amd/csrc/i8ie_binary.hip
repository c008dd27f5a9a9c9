// i8ie_binary.hip -- the two-operand quantized ops: the residual Add (i8ie_add_u8, i8ie_add_u8_nhwc,
// i8ie_add_f32) and the broadcast Mul (section 8g; i8ie_mul_u8, i8ie_mul_u8_nhwc, i8ie_mul_f32).  One kernel family,
// instantiated for (+) = + and (+) = x.
//
// The reference joins no two tensors.  Both ops are defined as a composition of the reference's own expressions, dequantize
// (src/quantize_utils.cc:38-42) of both operands and down_scale's clamp and truncation (src/quantize_utils.cc:27-36), IEEE
// fp32, one rounding per operation, no contraction:
//     fa = (float)((int)a - (int)zp_a) * s_a;   fb = (float)((int)b - (int)zp_b) * s_b
//     t  = (fa (+) fb) / s_out + (float)zp_out
//     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t);   q = relu ? max(q, zp_out) : q        (relu<u8>, src/functional.cc:15-26)
// Mul's b has a's shape, or is a gate: one byte per image and channel, multiplied into every pixel of that image.
//
// Evaluation, bit-identical to that sequence for every byte pair (tests/test_gpu_add.py and tests/test_gpu_mul.py run all
// 65 536 of them, Mul through both forms).  Write J = fa (+) fb and x = J / s_out for the real-valued quotient.
//   exact    the sequence itself ((float)a - (float)zp_a is the exact integer difference).
//   guarded  J as above (the same products, the same one sum), then e = fma(J, r, zp_out - 0.5) with r = fl(1 / s_out) from the
//            host, packed with v_cvt_pk_u8_f32 (round to nearest even, saturate).  A dword holding a value closer than 2^-13
//            to a rounding boundary replays the exact sequence: the guarded pack of i8ie_requant.h.
//            Bound: while |x| < 257 (which covers every t in (-1, 256), zp_out being in [0, 255]) the reference rounds twice
//            behind J (the quotient, the sum: each <= 2^-16) and the estimate twice (r: 257 * 2^-24 < 2^-16, the fma:
//            <= 2^-16), so |t - (e + 0.5)| < 6.2e-5 < 2^-13.  Beyond that range both sides saturate, both being monotone in J:
//            t >= 255 or t < 0 on the one side, e >= 256.4 or e <= -2.4 on the other (with the relu both give zp_out there).
//            Taken only for ordinary scales (i8ie_requant.h's rule), so that J, r (and H below) are normal numbers or exact
//            zeros and the relative bounds hold; zero, denormal or huge scales run the exact sequence.  Add: each scale
//            ordinary and the largest |x| = 255 (s_a + s_b) / s_out below 1e30.  Mul: each scale, s_a * s_b (the smallest
//            nonzero |J|) and s_b / s_out (the smallest nonzero |H|) in (1e-30, 1e30) and the largest |x| below 1e30.
//
// The gate's estimate rounds three times: H = fl(fb * r) is computed once per gate byte and kept in a register, and
// e = fma(fa, H, zp_out - 0.5) is one fma per element where the equal-shape form has a product and an fma.  While |x| < 257
// the reference rounds three times behind fa and fb (J: 257 * 2^-24 = 1.54e-5, the quotient and the sum: 2^-16 = 1.53e-5
// each) and the estimate three times (r and H: 2 * 1.54e-5, the fma: 2^-16), so |t - (e + 0.5)| < 9.2e-5 < 2^-13:
// i8ie_requant.h's own figure.
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
#include "i8ie_requant.h"

namespace {

constexpr int kWalk = 8;  // pixels a lane of the gate kernel walks with one gate item in registers

struct BinParams {
  float sa, zpa, sb, zpb, sc, zpc;
  float rc, zph, lof;    // estimate: fl(1 / s_out), zp_out - 0.5, its lower clamp (relu: zp_out; else -1 = none, the pack saturates at 0)
  int lo;                // relu ? zp_out : 0
  int fast;              // the estimate may be used (ordinary scales)
  uint32_t xa, xb, xo;   // 0x80808080 where that buffer holds re-biased bytes (I8IE_LAYOUT_NHWC_S8), else 0
};

// (+), and the rule under which its estimate may be used
struct Sum {
  static constexpr bool kSecondFirst = false;
  static __device__ __forceinline__ float join(float a, float b) { return a + b; }
  static bool fast(float s_a, float s_b, float s_out) {
    const double top = 255.0 * ((double)s_a + (double)s_b) / (double)s_out;
    return ordinary(s_a) && ordinary(s_b) && ordinary(s_out) && top < 1e30;
  }
};
struct Product {
  static constexpr bool kSecondFirst = true;
  static __device__ __forceinline__ float join(float a, float b) { return a * b; }
  // (in double, unlike the pointwise units' shared ordinary(float): the bound is stated on the double products and quotients)
  static bool ordinary_d(double s) { return s > 1e-30 && s < 1e30; }
  static bool fast(float s_a, float s_b, float s_out) {
    const double top = 255.0 * 255.0 * (double)s_a * (double)s_b / (double)s_out;
    return ordinary_d(s_a) && ordinary_d(s_b) && ordinary_d(s_out) && ordinary_d((double)s_a * (double)s_b) &&
           ordinary_d((double)s_b / (double)s_out) && top < 1e30;
  }
};

// the exact sequence behind fa and fb, and on plain bytes
template <typename Op>
__device__ __forceinline__ uint32_t exact_f(float fa, float fb, const BinParams& p) {
  const float t = Op::join(fa, fb) / p.sc + p.zpc;
  const int u = (t >= 255.0f) ? 255 : ((t < 0.0f) ? 0 : (int)t);
  return (uint32_t)(u > p.lo ? u : p.lo);
}
template <typename Op>
__device__ __forceinline__ uint32_t exact1(uint32_t a, uint32_t b, const BinParams& p) {
  // (the order of the two dequantisations is each op's own, as its unit had it before the two were merged: the numbers are the
  // same either way, but the order reaches the instruction scheduler, and the kernels keep their machine code with it)
  float fa, fb;
  if (Op::kSecondFirst) fb = ((float)b - p.zpb) * p.sb;
  fa = ((float)a - p.zpa) * p.sa;
  if (!Op::kSecondFirst) fb = ((float)b - p.zpb) * p.sb;
  return exact_f<Op>(fa, fb, p);
}
template <typename Op>
__device__ __forceinline__ uint32_t exact4(uint32_t a4, uint32_t b4, const BinParams& p) {
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= exact1<Op>((a4 >> (8 * r)) & 0xFFu, (b4 >> (8 * r)) & 0xFFu, p) << (8 * r);
  return packed;
}

// four elements: a4 / b4 / the result as they lie in memory (re-biased or not)
template <typename Op>
__device__ __forceinline__ uint32_t bin4(uint32_t a4, uint32_t b4, const BinParams& p) {
  a4 ^= p.xa;
  b4 ^= p.xb;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = ((float)((a4 >> (8 * r)) & 0xFFu) - p.zpa) * p.sa;
      const float fb = ((float)((b4 >> (8 * r)) & 0xFFu) - p.zpb) * p.sb;
      packed = i8ie_requant_est_step(__builtin_fmaf(Op::join(fa, fb), p.rc, p.zph), p.lof, r, packed, worst);
    }
    if (i8ie_requant_est_ok(worst)) return packed ^ p.xo;
  }
  return exact4<Op>(a4, b4, p) ^ p.xo;
}
template <typename Op>
__device__ __forceinline__ uint8_t bin1(uint8_t a, uint8_t b, const BinParams& p) {
  return (uint8_t)(exact1<Op>((a ^ p.xa) & 0xFFu, (b ^ p.xb) & 0xFFu, p) ^ (p.xo & 0xFFu));
}
template <typename Op>
__device__ __forceinline__ uint4 bin16(uint4 x, const uint4& y, const BinParams& p) {
  x.x = bin4<Op>(x.x, y.x, p);
  x.y = bin4<Op>(x.y, y.y, p);
  x.z = bin4<Op>(x.z, y.z, p);
  x.w = bin4<Op>(x.w, y.w, p);
  return x;
}

// ---- flat form: one physical order, no border.  out may alias a or b: a lane reads its 16 bytes before it stores them.
template <typename Op>
__global__ __launch_bounds__(kThreads) void bin_u8_flat_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, BinParams p) {
  const int64_t nvec = n >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    const uint4 x = reinterpret_cast<const uint4*>(a)[v];
    const uint4 y = reinterpret_cast<const uint4*>(b)[v];
    reinterpret_cast<uint4*>(out)[v] = bin16<Op>(x, y, p);
  }
  const int64_t t0 = nvec << 4;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = bin1<Op>(a[t0 + threadIdx.x], b[t0 + threadIdx.x], p);
}

// ---- bordered NHWC form, equal shapes: [n][h + 2b][w + 2b][c] per buffer, each with its own b.  The w * c interior bytes of
// an image row are the contiguous unit; an item is VEC bytes of one row (i8ie_pointwise.h).  Only the interior of `out` is
// written.
template <typename Op, int VEC, typename Idx>
__global__ __launch_bounds__(kThreads) void bin_u8_nhwc_kernel(const uint8_t* __restrict__ a, NhwcGeom ga, const uint8_t* __restrict__ b,
                                                               NhwcGeom gb, uint8_t* __restrict__ out, NhwcGeom go, Idx items, Idx per_row,
                                                               Idx h, BinParams p) {
  const Idx stride = (Idx)gridDim.x * kThreads;
  for (Idx v = (Idx)blockIdx.x * kThreads + threadIdx.x; v < items; v += stride) {
    const RowItem<Idx> it = row_item<VEC>(v, per_row, h);
    const uint8_t* pa = a + nhwc_at(ga, it);
    const uint8_t* pb = b + nhwc_at(gb, it);
    uint8_t* po = out + nhwc_at(go, it);
    if (VEC == 16)
      *reinterpret_cast<uint4*>(po) = bin16<Op>(*reinterpret_cast<const uint4*>(pa), *reinterpret_cast<const uint4*>(pb), p);
    else if (VEC == 4)
      *reinterpret_cast<uint32_t*>(po) = bin4<Op>(*reinterpret_cast<const uint32_t*>(pa), *reinterpret_cast<const uint32_t*>(pb), p);
    else
      *po = bin1<Op>(*pa, *pb, p);
  }
}

template <typename Op>
__global__ __launch_bounds__(kThreads) void bin_f32_kernel(const float* a, const float* b, float* out, int64_t n) {
  const int64_t nvec = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    float4 x = reinterpret_cast<const float4*>(a)[v];
    const float4 y = reinterpret_cast<const float4*>(b)[v];
    x.x = Op::join(x.x, y.x); x.y = Op::join(x.y, y.y); x.z = Op::join(x.z, y.z); x.w = Op::join(x.w, y.w);
    reinterpret_cast<float4*>(out)[v] = x;
  }
  const int64_t t0 = nvec << 2;
  if (blockIdx.x == 0 && threadIdx.x < (n - t0)) out[t0 + threadIdx.x] = Op::join(a[t0 + threadIdx.x], b[t0 + threadIdx.x]);
}

// ---- Mul's gate form: a and out as above, the gate [n][1 + 2b][1 + 2b][c] (plain rows [n][c] at b = 0)
struct MulGate : PixelWalk {  // (the walk: i8ie_pointwise.h)
  int64_t g_img, g_org;    // the gate: bytes per image, offset of its one pixel
};

// four elements against four gate values: h4 = fl(fb * r) of the four channels (estimate), g4 their plain bytes (replay)
__device__ __forceinline__ uint32_t gate4(uint32_t a4, const float* h4, uint32_t g4, const BinParams& p) {
  a4 ^= p.xa;
  if (p.fast) {
    uint32_t packed = 0;
    float worst = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float fa = ((float)((a4 >> (8 * r)) & 0xFFu) - p.zpa) * p.sa;
      packed = i8ie_requant_est_step(__builtin_fmaf(fa, h4[r], p.zph), p.lof, r, packed, worst);
    }
    if (i8ie_requant_est_ok(worst)) return packed ^ p.xo;
  }
  return exact4<Product>(a4, g4, p) ^ p.xo;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void mul_u8_gate_kernel(const uint8_t* __restrict__ a, NhwcGeom ga, const uint8_t* __restrict__ g,
                                                               uint8_t* __restrict__ out, NhwcGeom go, MulGate t, BinParams p) {
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
        const float fa = ((float)((a[oa] ^ p.xa) & 0xFFu) - p.zpa) * p.sa;
        out[oo] = (uint8_t)(exact_f<Product>(fa, hv[0], p) ^ (p.xo & 0xFFu));
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

// the gate form in FP32 (NCHW: one gate value per run of h * w elements); the path of calibration, not of inference
__global__ __launch_bounds__(kThreads) void mul_f32_gate_kernel(const float* a, const float* g, float* out, int64_t n, int64_t run) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < n; v += stride) out[v] = a[v] * g[v / run];
}

// ---- host side
template <typename Op>
BinParams make_params(float s_a, int zp_a, float s_b, int zp_b, float s_out, int zp_out, int relu, int a_s8, int b_s8, int out_s8) {
  BinParams p;
  p.sa = s_a; p.zpa = (float)zp_a; p.sb = s_b; p.zpb = (float)zp_b; p.sc = s_out; p.zpc = (float)zp_out;
  p.rc = 1.0f / s_out;
  p.zph = (float)zp_out - 0.5f;
  p.lof = relu ? (float)zp_out : -1.0f;
  p.lo = relu ? zp_out : 0;
  p.fast = Op::fast(s_a, s_b, s_out) ? 1 : 0;  // the estimate only where nothing can overflow or go denormal on the way
  p.xa = a_s8 ? 0x80808080u : 0u;
  p.xb = b_s8 ? 0x80808080u : 0u;
  p.xo = out_s8 ? 0x80808080u : 0u;
  return p;
}

template <typename Op, int VEC>
void launch_nhwc(i8ie_ctx* ctx, const uint8_t* a, const NhwcGeom& ga, const uint8_t* b, const NhwcGeom& gb, uint8_t* out,
                 const NhwcGeom& go, int n, int c, int h, int w, const BinParams& p) {
  const int64_t per_row = (int64_t)w * c / VEC, items = (int64_t)n * h * per_row;
  if (items <= 0x7FFFFFFF)
    bin_u8_nhwc_kernel<Op, VEC, uint32_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, (uint32_t)items,
                                                                                         (uint32_t)per_row, (uint32_t)h, p);
  else
    bin_u8_nhwc_kernel<Op, VEC, int64_t><<<grid_for(items), kThreads, 0, ctx->stream>>>(a, ga, b, gb, out, go, items, per_row,
                                                                                        (int64_t)h, p);
}

template <int VEC>
void launch_gate(i8ie_ctx* ctx, const uint8_t* a, const NhwcGeom& ga, const uint8_t* g, int g_border, uint8_t* out, const NhwcGeom& go,
                 int n, int c, int h, int w, const BinParams& p) {
  MulGate t;
  const NhwcGeom gg = buf_geom(c, 1, 1, g_border);
  t.g_img = gg.img;
  t.g_org = gg.org;
  pixel_walk_init(t, VEC, kWalk, n, c, h, w, ga, go);
  const int blocks = pixel_walk_blocks(t);
  mul_u8_gate_kernel<VEC><<<blocks, kThreads, 0, ctx->stream>>>(a, ga, g, out, go, t, p);
}

// ---- the bodies of the equal-shape entry points, behind their argument checks
template <typename Op>
int flat_body(i8ie_ctx* ctx, const char* scope, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, const BinParams& p) {
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, scope, 0.0, 3.0 * n);
  bin_u8_flat_kernel<Op><<<grid_for((n >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n, p);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
template <typename Op>
int nhwc_body(i8ie_ctx* ctx, const char* scope, const uint8_t* a, int a_border, const uint8_t* b, int b_border, uint8_t* out, int out_border,
              int n, int c, int h, int w, const BinParams& p) {
  const int64_t total = (int64_t)n * c * h * w;
  I8ieProfScope prof(ctx, scope, 0.0, 3.0 * total);
  const int vec = item_width({c}, {a, b, out});
  if (a_border == 0 && b_border == 0 && out_border == 0 && aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16)) {
    bin_u8_flat_kernel<Op><<<grid_for((total >> 4) + 1), kThreads, 0, ctx->stream>>>(a, b, out, total, p);  // one physical order, no border
  } else {
    const NhwcGeom ga = buf_geom(c, h, w, a_border), gb = buf_geom(c, h, w, b_border), go = buf_geom(c, h, w, out_border);
    if (vec == 16) launch_nhwc<Op, 16>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else if (vec == 4) launch_nhwc<Op, 4>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
    else launch_nhwc<Op, 1>(ctx, a, ga, b, gb, out, go, n, c, h, w, p);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
template <typename Op>
int f32_body(i8ie_ctx* ctx, const char* scope, const float* a, const float* b, float* out, int64_t n) {
  I8ieProfScope prof(ctx, scope, 0.0, 12.0 * n);
  bin_f32_kernel<Op><<<grid_for((n >> 2) + 1), kThreads, 0, ctx->stream>>>(a, b, out, n);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // namespace

extern "C" {

int i8ie_add_u8(i8ie_ctx* ctx, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, float s_a, uint8_t zp_a, float s_b,
                uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  return flat_body<Sum>(ctx, "add_u8", a, b, out, n, make_params<Sum>(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, 0, 0, 0));
}

int i8ie_add_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8,
                     uint8_t* out, int out_border, int out_s8, int n, int c, int h, int w, float s_a, uint8_t zp_a, float s_b,
                     uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && a_border >= 0 && b_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return nhwc_body<Sum>(ctx, "add_u8_nhwc", a, a_border, b, b_border, out, out_border, n, c, h, w,
                        make_params<Sum>(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, a_s8, b_s8, out_s8));
}

int i8ie_add_f32(i8ie_ctx* ctx, const float* a, const float* b, float* out, int64_t n) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  return f32_body<Sum>(ctx, "add_f32", a, b, out, n);
}

int i8ie_mul_u8(i8ie_ctx* ctx, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, float s_a, uint8_t zp_a, float s_b,
                uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(out, 16), "buffers must be 16-byte aligned");
  return flat_body<Product>(ctx, "mul_u8", a, b, out, n, make_params<Product>(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, 0, 0, 0));
}

int i8ie_mul_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8, int b_gate,
                     uint8_t* out, int out_border, int out_s8, int n, int c, int h, int w, float s_a, uint8_t zp_a, float s_b,
                     uint8_t zp_b, float s_out, uint8_t zp_out, int relu) {
  I8IE_REQUIRE(ctx && a && b && out, "null argument");
  I8IE_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && a_border >= 0 && b_border >= 0 && out_border >= 0, "bad dimension");
  I8IE_REQUIRE((int64_t)h * w <= 0x3FFFFFFF, "bad dimension: more than 2^30 pixels per image");
  I8IE_REQUIRE(scales_ok(s_a, s_b, s_out), "scales must be finite and the output scale positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const BinParams p = make_params<Product>(s_a, zp_a, s_b, zp_b, s_out, zp_out, relu, a_s8, b_s8, out_s8);
  if (!b_gate) return nhwc_body<Product>(ctx, "mul_u8_nhwc", a, a_border, b, b_border, out, out_border, n, c, h, w, p);
  const NhwcGeom ga = buf_geom(c, h, w, a_border), go = buf_geom(c, h, w, out_border);
  I8ieProfScope prof(ctx, "mul_u8_gate", 0.0, 2.0 * (double)((int64_t)n * c * h * w) + (double)n * c);
  const int vec = item_width({c}, {a, b, out});
  if (vec == 16) launch_gate<16>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
  else if (vec == 4) launch_gate<4>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
  else launch_gate<1>(ctx, a, ga, b, b_border, out, go, n, c, h, w, p);
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
  if (!gate_run) return f32_body<Product>(ctx, "mul_f32", a, b, out, n);
  I8ieProfScope prof(ctx, "mul_f32", 0.0, 8.0 * n);
  mul_f32_gate_kernel<<<grid_for(n), kThreads, 0, ctx->stream>>>(a, b, out, n, gate_run);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
