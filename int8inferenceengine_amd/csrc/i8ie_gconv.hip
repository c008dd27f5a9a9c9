// i8ie_gconv.hip -- grouped and depthwise Conv2d in INT8 (Conv2d groups=).
//   reference: src/conv2d.cc:100-142 per group; groups: not in the reference
//
// A grouped convolution is `groups` independent reference convolutions over channel slices that share the layer's
// (s_in, zp_in, s_w, s_out, zp_out): output features [g Ng, (g+1) Ng) see input channels [g Cg, (g+1) Cg).  Two kernels,
// both over NHWC activations (physical border `ib` holding zp_in; taps outside it read as zp_in) and weights packed once per
// layer as [groups][Ng padded to 16][Kg padded to 64], K ordered (kh, kw, cg), zero padded:
//   gconv_mfma    a block owns (group, 128 output pixels, up to 64 features of the group); each wave multiplies 32 pixels by
//                 the block's features on v_mfma_i32_16x16x64_i8, both operands read as fragments straight from global
//                 memory (the weights of a group are a few hundred KiB at most: they stay in L2 / the vector cache)
//   (both)        a dilation (Conv2d dilation=) multiplies a tap's pixel offset and nothing else: the
//                 weights, the tap table and the K order are those of the undilated layer.  Stride, padding and dilation are
//                 per axis (section 8p): a rectangular or anisotropic layer is the same walk with unequal pairs
//   gconv_direct  no matrix instruction: a lane owns up to 4 features of one (pixel, group) and walks the taps
//                 (v_dot4_i32_i8 where Cg % 4 == 0); depthwise, channel multipliers, tiny groups, and every grouped layer
//                 while I8IE_OPT_FORCE_FALLBACK is on
// Activations are re-biased ^0x80 on the way in (the term 128 * wsum[j] is in ocp), accumulation is exact INT32, the epilogue
// is the requantiser of i8ie_requant.h (per-tensor and per-channel instances) with the optional ReLU clamp.
#include "i8ie_internal.h"
#include "i8ie_epilogue.h"
#include "i8ie_gconv.h"
#include "i8ie_pointwise.h"

namespace {

struct GconvArgs {
  const uint8_t* A;  // [m][H + 2 ib][W + 2 ib][C]
  int H, W, C, ib;
  int OH, OW, KH, KW;
  int sh, sw, ph, pw, dh, dw;  // stride, padding, dilation per axis: tap (kh, kw) reads the pixel (kh * dh, kw * dw) of the
                               // window (DESIGN.md sections 8j, 8p)
  int Cg, Ng, Ngp, Kg, Kgp, kc;
  long long M;          // m * OH * OW output pixels
  const int8_t* Bp;     // [groups][Ngp][Kgp]
  const int2* ktab;     // K position (in units of the gather granularity) -> {(kh << 16) | kw, cg}
  I8ieEpiArgs ep;       // ocp, msv, sbv: [kc]; acc: nullptr or [M][kc]
  int zp_in;
  uint8_t* out;         // [m][OH + 2 ob][OW + 2 ob][kc], interior written
  int ob, vec_out;      // vec_out: 4 features of a lane go out as one dword
};

struct Pixel {
  long long in_base;   // byte offset of the window origin's channel 0 of this group (may lie outside the image: only
  int y0, x0;          // dereferenced for taps inside the physical tensor)
  long long out_pix;   // physical output pixel index
};

__device__ __forceinline__ Pixel locate(const GconvArgs& p, long long px, int g) {
  const int P = p.OH * p.OW;
  const long long img = px / P;
  const int rem = (int)(px - img * P), oy = rem / p.OW, ox = rem - oy * p.OW;
  Pixel q;
  q.y0 = oy * p.sh - p.ph;
  q.x0 = ox * p.sw - p.pw;
  const int Hp = p.H + 2 * p.ib, Wp = p.W + 2 * p.ib;
  q.in_base = ((img * Hp + (q.y0 + p.ib)) * Wp + (q.x0 + p.ib)) * p.C + (long long)g * p.Cg;
  q.out_pix = (img * (p.OH + 2 * p.ob) + oy + p.ob) * (p.OW + 2 * p.ob) + ox + p.ob;
  return q;
}

// (dy, dx): the tap's offset in pixels from the window origin, the dilation already in it
__device__ __forceinline__ bool tap_inside(const GconvArgs& p, const Pixel& q, int dy, int dx) {
  const int y = q.y0 + dy + p.ib, x = q.x0 + dx + p.ib;
  return (unsigned)y < (unsigned)(p.H + 2 * p.ib) && (unsigned)x < (unsigned)(p.W + 2 * p.ib);
}

// the quad epilogue (i8ie_epilogue.h) on 4 consecutive features f .. f + 3 of group g at one pixel
template <bool PC>
__device__ __forceinline__ void finish_quad(const GconvArgs& p, int (&c)[4], long long px, long long out_pix, int g, int f) {
  const int j0 = g * p.Ng + f, nf = p.Ng - f < 4 ? p.Ng - f : 4;
  i8ie_epi_finish<PC>(p.ep, c, i8ie_epi_cols<PC>(p.ep, j0, nf), nf, px * p.kc + j0, p.out + out_pix * p.kc + j0,
                      p.vec_out && nf == 4);
}

// ---- gconv_mfma ------------------------------------------------------------------------------------------------------
// v_mfma_i32_16x16x64_i8: lane (q, r) = (lane / 16, lane % 16) supplies bytes 16 q .. 16 q + 15 of a 64-byte K step for
// row r of each operand; with the weights as srcA it receives features 4 q .. 4 q + 3 of pixel r.
// G = gather granularity in bytes: 16 when Cg % 16 == 0 (a lane's 16 bytes lie inside one tap), 4 when Cg % 4 == 0, else 1.
constexpr int MT = 2, NT = 4;  // per wave: 2 x 16 pixels by 4 x 16 features

template <int G>
__device__ __forceinline__ v4i gather16(const GconvArgs& p, const Pixel& q, int kpos) {
  const uint32_t zp4 = (uint32_t)p.zp_in * 0x01010101u;
  const int Wp = p.W + 2 * p.ib;
  uint32_t d[4];
  if constexpr (G == 16) {
    const int2 t = p.ktab[kpos >> 4];
    const int dy = (t.x >> 16) * p.dh, dx = (t.x & 0xffff) * p.dw;
    v4i v = {(int)zp4, (int)zp4, (int)zp4, (int)zp4};
    if (tap_inside(p, q, dy, dx)) v = *reinterpret_cast<const v4i*>(p.A + q.in_base + (long long)(dy * Wp + dx) * p.C + t.y);
    return v;
  } else if constexpr (G == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int2 t = p.ktab[(kpos >> 2) + i];
      const int dy = (t.x >> 16) * p.dh, dx = (t.x & 0xffff) * p.dw;
      d[i] = zp4;
      if (tap_inside(p, q, dy, dx)) d[i] = *reinterpret_cast<const uint32_t*>(p.A + q.in_base + (long long)(dy * Wp + dx) * p.C + t.y);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[i] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int2 t = p.ktab[kpos + 4 * i + b];
        const int dy = (t.x >> 16) * p.dh, dx = (t.x & 0xffff) * p.dw;
        uint32_t v = (uint32_t)p.zp_in;
        if (tap_inside(p, q, dy, dx)) v = p.A[q.in_base + (long long)(dy * Wp + dx) * p.C + t.y];
        d[i] |= v << (8 * b);
      }
    }
  }
  return v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
}

template <int G, bool PC>
__global__ __launch_bounds__(256) void gconv_mfma_kernel(GconvArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
  const int g = blockIdx.z, f0 = blockIdx.y * (16 * NT);
  const long long p0 = ((long long)blockIdx.x * 4 + wave) * (16 * MT);
  if (p0 >= p.M) return;  // (no barrier in this kernel)
  Pixel px[MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const long long q = p0 + 16 * mi + lr;
    px[mi] = locate(p, q < p.M ? q : p.M - 1, g);  // ragged tile: the spare lanes redo the last pixel and store nothing
  }
  const int nt = (p.Ng - f0 + 15) / 16 < NT ? (p.Ng - f0 + 15) / 16 : NT;  // 16-feature fragments of this block
  const int8_t* brow = p.Bp + ((size_t)g * p.Ngp + f0 + lr) * p.Kgp + 16 * lq;
  v4i acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = v4i{0, 0, 0, 0};

  for (int k0 = 0; k0 < p.Kgp; k0 += 64) {
    v4i a[MT], b[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      b[ni] = v4i{0, 0, 0, 0};
      if (ni < nt) b[ni] = *reinterpret_cast<const v4i*>(brow + (size_t)ni * 16 * p.Kgp + k0);
    }
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) a[mi] = gather16<G>(p, px[mi], k0 + 16 * lq) ^ (int)0x80808080;  // u8 -> s8
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        if (ni < nt) acc[mi][ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], a[mi], acc[mi][ni], 0, 0, 0);
  }

#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const long long q = p0 + 16 * mi + lr;
    if (q >= p.M) continue;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int f = f0 + 16 * ni + 4 * lq;
      if (ni >= nt || f >= p.Ng) continue;
      int c[4] = {acc[mi][ni].x, acc[mi][ni].y, acc[mi][ni].z, acc[mi][ni].w};
      finish_quad<PC>(p, c, q, px[mi].out_pix, g, f);
    }
  }
}

// ---- gconv_direct ----------------------------------------------------------------------------------------------------
// item = (pixel, group, quad of features), quads fastest: neighbouring lanes store neighbouring bytes of an NHWC pixel.
// DOT4: Cg % 4 == 0 and dword-aligned activations; otherwise byte by byte.
template <bool DOT4, bool PC>
__global__ __launch_bounds__(256) void gconv_direct_kernel(GconvArgs p, int groups, long long items) {
  const int nq = (p.Ng + 3) / 4, Wp = p.W + 2 * p.ib;
  const long long gstride = (long long)gridDim.x * 256;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += gstride) {
    const int fq = (int)(it % nq);
    const long long t = it / nq;
    const int g = (int)(t % groups);
    const long long pxi = t / groups;
    const int f = 4 * fq;
    const Pixel q = locate(p, pxi, g);
    const int8_t* w = p.Bp + ((size_t)g * p.Ngp + f) * p.Kgp;  // rows f .. f + 3 < Ngp exist (zero beyond Ng)
    int c[4] = {0, 0, 0, 0};
    for (int dy = 0; dy < p.KH; ++dy)
      for (int dx = 0; dx < p.KW; ++dx) {
        const bool in = tap_inside(p, q, dy * p.dh, dx * p.dw);
        const uint8_t* a = p.A + q.in_base + (long long)(dy * p.dh * Wp + dx * p.dw) * p.C;
        const int8_t* wt = w + (dy * p.KW + dx) * p.Cg;
        if constexpr (DOT4) {
          for (int cg = 0; cg < p.Cg; cg += 4) {
            const uint32_t av = (in ? *reinterpret_cast<const uint32_t*>(a + cg) : (uint32_t)p.zp_in * 0x01010101u) ^ 0x80808080u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int wv;
              __builtin_memcpy(&wv, wt + (size_t)r * p.Kgp + cg, 4);  // (Kg % 4 == 0: aligned)
              c[r] = __builtin_amdgcn_sdot4((int)av, wv, c[r], false);
            }
          }
        } else {
          for (int cg = 0; cg < p.Cg; ++cg) {
            const int av = (in ? (int)a[cg] : p.zp_in) - 128;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] += av * (int)wt[(size_t)r * p.Kgp + cg];
          }
        }
      }
    finish_quad<PC>(p, c, pxi, q.out_pix, g, f);
  }
}

}  // namespace

// K position -> tap table of the MFMA kernel's gather, at granularity G(Cg) (i8ie_gconv_granularity)
int i8ie_gconv_granularity(int Cg) { return Cg % 16 == 0 ? 16 : (Cg % 4 == 0 ? 4 : 1); }

void i8ie_gconv_ktab(int Cg, int kh, int kw, int Kgp, std::vector<int>& tab) {
  const int G = i8ie_gconv_granularity(Cg), Kg = Cg * kh * kw;
  tab.assign((size_t)(Kgp / G) * 2, 0);  // padding positions: tap (0, 0), channel 0 (their weights are zero)
  for (int k = 0; k < Kg; k += G) {
    const int tap = k / Cg, cg = k - tap * Cg;
    tab[(size_t)(k / G) * 2] = ((tap / kw) << 16) | (tap % kw);
    tab[(size_t)(k / G) * 2 + 1] = cg;
  }
}

bool i8ie_gconv_mfma_takes(const i8ie_ctx* ctx, const I8ieGconvCall& c) {
  if ((ctx->options & 1) != 0 || c.Cg * c.KH * c.KW < 32) return false;
  const int G = i8ie_gconv_granularity(c.Cg);
  // (the gather reads G bytes at a time: the activations must be aligned to that)
  return aligned_to(c.A, G) && (G == 1 || c.C % G == 0) && aligned_to(c.Bp, 16);
}

int i8ie_gconv_launch(i8ie_ctx* ctx, const I8ieGconvCall& c) {
  I8IE_REQUIRE(c.groups >= 1 && c.groups <= 65535, "grouped conv: at most 65535 groups");
  I8IE_REQUIRE(c.KH < 65536 && c.KW < 65536, "grouped conv: kernel size");
  I8IE_REQUIRE(c.dil_h >= 1 && c.dil_w >= 1 && (long long)c.dil_h * c.KH < 65536 && (long long)c.dil_w * c.KW < 65536,
               "grouped conv: dilation");
  GconvArgs a{};
  a.A = c.A; a.H = c.H; a.W = c.W; a.C = c.C; a.ib = c.ib;
  a.OH = c.OH; a.OW = c.OW; a.KH = c.KH; a.KW = c.KW;
  a.sh = c.stride_h; a.sw = c.stride_w; a.ph = c.pad_h; a.pw = c.pad_w; a.dh = c.dil_h; a.dw = c.dil_w;
  a.Cg = c.Cg; a.Ng = c.Ng; a.Ngp = c.Ngp; a.Kg = c.Cg * c.KH * c.KW; a.Kgp = c.Kgp; a.kc = c.groups * c.Ng;
  a.M = (long long)c.m * c.OH * c.OW;
  a.Bp = c.Bp; a.ktab = reinterpret_cast<const int2*>(c.ktab);
  a.ep = i8ie_epi_args(c.ep); a.zp_in = c.zp_in;
  a.out = c.out; a.ob = c.ob;
  a.vec_out = (a.kc % 4 == 0 && c.Ng % 4 == 0 && aligned_to(c.out, 4)) ? 1 : 0;
  const bool pc = c.ep.msv != nullptr;
  const double ops = 2.0 * (double)a.M * a.kc * a.Kg;
  const double bytes = (double)c.m * c.H * c.W * c.C + (double)a.M * a.kc + (double)c.groups * c.Ngp * c.Kgp;
  if (i8ie_gconv_mfma_takes(ctx, c)) {
    const long long tiles = (a.M + 64 * MT - 1) / (64 * MT);
    I8IE_REQUIRE(tiles < ((long long)1 << 31), "grouped conv: too many output pixels in one call");
    const dim3 grid((unsigned)tiles, (unsigned)((c.Ng + 16 * NT - 1) / (16 * NT)), (unsigned)c.groups);
    I8IE_REQUIRE(grid.y <= 65535u, "grouped conv: too many features per group");
    I8ieProfScope prof(ctx, "gconv_mfma", ops, bytes);
    const int G = i8ie_gconv_granularity(c.Cg);
#define I8IE_GCONV_MFMA(GG)                                                            \
  do {                                                                                 \
    if (pc) gconv_mfma_kernel<GG, true><<<grid, 256, 0, ctx->stream>>>(a);             \
    else gconv_mfma_kernel<GG, false><<<grid, 256, 0, ctx->stream>>>(a);               \
  } while (0)
    if (G == 16) I8IE_GCONV_MFMA(16);
    else if (G == 4) I8IE_GCONV_MFMA(4);
    else I8IE_GCONV_MFMA(1);
#undef I8IE_GCONV_MFMA
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  const long long items = a.M * c.groups * ((c.Ng + 3) / 4);
  long long blocks = (items + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  const bool dot4 = c.Cg % 4 == 0 && c.C % 4 == 0 && aligned_to(c.A, 4) && aligned_to(c.Bp, 4);
  I8ieProfScope prof(ctx, "gconv_direct", ops, bytes);
  if (dot4) {
    if (pc) gconv_direct_kernel<true, true><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, c.groups, items);
    else gconv_direct_kernel<true, false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, c.groups, items);
  } else {
    if (pc) gconv_direct_kernel<false, true><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, c.groups, items);
    else gconv_direct_kernel<false, false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, c.groups, items);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
