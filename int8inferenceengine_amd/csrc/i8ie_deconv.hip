// i8ie_deconv.hip -- ConvTranspose2d in INT8 and FP32.
//   reference: src/conv2d.cc:100-142 applied to the equivalent problem; the transposed layer itself: not in the reference
//
// The layer is defined as the reference convolution (stride 1, padding 0) of x~ with W~: x~ is the input with s - 1 positions
// inserted between neighbouring pixels and k - 1 - p (+ output_padding below / right) positions around it, all holding zp_in,
// and W~[oc][ic][ky'][kx'] = W[ic][oc][k - 1 - ky'][k - 1 - kx'].  x~ is never built.  Output pixel (oy, ox) belongs to phase
// (ry, rx) = ((oy + p) mod s, (ox + p) mod s) and cell (qy, qx) = ((oy + p) / s, (ox + p) / s); of the k * k taps of W only
// ky = ry + s ty, kx = rx + s tx meet a real input pixel, (qy - ty, qx - tx), every other tap meets an inserted position:
//     sum over all of K of x~ w~  =  sum over the phase's taps of x w  +  zp_in * tph[phase][j]
// with tph the exact INT32 sum of feature j's weights at the taps the phase does not see.  A phase tap outside the image is a
// padding position of x~ and reads as zp_in, so a phase's tap set is always complete and the ^0x80 re-bias of the activations
// costs the constant 128 * (wsum[j] - tph[phase][j]) per (phase, feature); with ocp = oc + 128 wsum the epilogue adds
//     ocp[j] + (zp_in - 128) * tph[phase][j].
// Weights are packed once per layer as [s * s phases][N padded to 16][Kpp], K ordered (ty, tx, c), zero padded; Kpp is the
// longest phase's K rounded up to 64.  Two INT8 kernels over NHWC activations:
//   deconv_mfma    a block owns 128 cells (a flat tile of the (image, qy, qx) grid, 32 per wave) and up to 64 features and
//                  produces every phase of its cells on v_mfma_i32_16x16x64_i8.  k == s == 2 (each phase is one tap of the
//                  cell's own pixel): the activation fragment is fetched once per K step and multiplied against all four phase
//                  panels, 128 accumulator registers.  Any other geometry: phase after phase, each with its own gather.
//                  Both operands are read as fragments from global memory (no LDS stage, as gconv_mfma).
//   deconv_direct  no matrix instruction: a lane owns up to 4 features of one output pixel and walks that pixel's phase taps
//                  (v_dot4_i32_i8 where C % 4 == 0, byte by byte otherwise), 32-bit index arithmetic (the launcher refuses
//                  tensors of 2^31 bytes or more).  Tiny K (i8ie_deconv.h) and every transposed layer under
//                  I8IE_OPT_FORCE_FALLBACK.
// Accumulation is exact INT32; the epilogue is the requantiser of i8ie_requant.h (per-tensor and per-channel instances) with
// the optional ReLU clamp; a lane's 4 consecutive features of a pixel go out as one dword.
#include "i8ie_internal.h"
#include "i8ie_deconv.h"
#include "i8ie_pointwise.h"

namespace {

struct DeconvArgs {
  const uint8_t* A;  // [m][H + 2 ib][W + 2 ib][C]
  int H, W, C, ib;
  int OH, OW, k, s, p, QH, QW;  // QH x QW cells per image: qy = (oy + p) / s
  int N, Ngp, Kpp, ktab_pitch;  // ktab_pitch: table entries per phase (Kpp / granularity)
  long long Mq;                 // m * QH * QW cells
  const int8_t* Bp;
  const int2* ktab;
  const int32_t* ocp;
  const int32_t* tph;
  const float* msv;
  const float* sbv;
  I8ieRequant rq;
  int relu_lo, zp_in;
  uint8_t* out;  // [m][OH + 2 ob][OW + 2 ob][N], interior written
  int ob, vec_out;
  int32_t* acc;  // nullptr or [m * OH * OW][N]
};

// (Not on the quad epilogue of i8ie_epilogue.h: with it the one-phase-at-a-time instances measured 1 to 2 % slower.)
// oc', the accumulators' copy, requantise, store: 4 consecutive features f .. f + 3 of output pixel (img, oy, ox), phase ph
template <bool PC>
__device__ __forceinline__ void finish4(const DeconvArgs& p, int (&c)[4], long long img, int oy, int ox, int ph, int f) {
  const int nf = p.N - f < 4 ? p.N - f : 4;
  const int zb = p.zp_in - 128;
  float ms[4], sb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = f + (r < nf ? r : nf - 1);
    c[r] += p.ocp[j] + zb * p.tph[ph * p.Ngp + j];
    if (PC) {
      ms[r] = p.msv[j];
      sb[r] = p.sbv[j];
    }
  }
  if (p.acc != nullptr) {
    const long long px = (img * p.OH + oy) * p.OW + ox;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < nf) p.acc[px * p.N + f + r] = c[r];
  }
  const float lof = (float)p.relu_lo;
  uint32_t packed;
  if constexpr (PC)
    packed = i8ie_requant_pack4_pc(c, p.rq, make_float4(ms[0], ms[1], ms[2], ms[3]), sb, p.relu_lo, lof);
  else
    packed = i8ie_requant_pack4(c, p.rq, p.relu_lo, lof);
  const long long out_pix = (img * (p.OH + 2 * p.ob) + oy + p.ob) * (p.OW + 2 * p.ob) + ox + p.ob;
  uint8_t* o = p.out + out_pix * p.N + f;
  if (p.vec_out && nf == 4) {
    *reinterpret_cast<uint32_t*>(o) = packed;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < nf) o[r] = (uint8_t)(packed >> (8 * r));
  }
}

// ---- deconv_mfma -----------------------------------------------------------------------------------------------------
// v_mfma_i32_16x16x64_i8: lane (q, r) = (lane / 16, lane % 16) supplies bytes 16 q .. 16 q + 15 of a 64-byte K step for
// row r of each operand; with the weights as srcA it receives features 4 q .. 4 q + 3 of cell r.
// G = gather granularity in bytes: 16 when C % 16 == 0 (a lane's 16 bytes lie inside one tap), 4 when C % 4 == 0, else 1.
constexpr int MT = 2, NT = 4;  // per wave: 2 x 16 cells by 4 x 16 features

struct Cell {
  long long img, in_pix;  // in_pix: physical input pixel index of (img, qy, qx); only dereferenced for taps inside the image
  int qy, qx;
};

__device__ __forceinline__ Cell locate(const DeconvArgs& p, long long q) {
  const int Q = p.QH * p.QW;
  Cell cl;
  cl.img = q / Q;
  const int rem = (int)(q - cl.img * Q);
  cl.qy = rem / p.QW;
  cl.qx = rem - cl.qy * p.QW;
  cl.in_pix = (cl.img * (p.H + 2 * p.ib) + cl.qy + p.ib) * (p.W + 2 * p.ib) + cl.qx + p.ib;
  return cl;
}

__device__ __forceinline__ bool tap_inside(const DeconvArgs& p, const Cell& cl, int ty, int tx) {
  return (unsigned)(cl.qy - ty) < (unsigned)p.H && (unsigned)(cl.qx - tx) < (unsigned)p.W;
}

template <int G>
__device__ __forceinline__ v4i gather16(const DeconvArgs& p, const Cell& cl, const int2* tab, int kpos) {
  const uint32_t zp4 = (uint32_t)p.zp_in * 0x01010101u;
  const int Wp = p.W + 2 * p.ib;
  uint32_t d[4];
  if constexpr (G == 16) {
    const int2 t = tab[kpos >> 4];
    const int ty = t.x >> 16, tx = t.x & 0xffff;
    v4i v = {(int)zp4, (int)zp4, (int)zp4, (int)zp4};
    if (tap_inside(p, cl, ty, tx)) v = *reinterpret_cast<const v4i*>(p.A + (cl.in_pix - (long long)(ty * Wp + tx)) * p.C + t.y);
    return v;
  } else if constexpr (G == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int2 t = tab[(kpos >> 2) + i];
      const int ty = t.x >> 16, tx = t.x & 0xffff;
      d[i] = zp4;
      if (tap_inside(p, cl, ty, tx)) d[i] = *reinterpret_cast<const uint32_t*>(p.A + (cl.in_pix - (long long)(ty * Wp + tx)) * p.C + t.y);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[i] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int2 t = tab[kpos + 4 * i + b];
        const int ty = t.x >> 16, tx = t.x & 0xffff;
        uint32_t v = (uint32_t)p.zp_in;
        if (tap_inside(p, cl, ty, tx)) v = p.A[(cl.in_pix - (long long)(ty * Wp + tx)) * p.C + t.y];
        d[i] |= v << (8 * b);
      }
    }
  }
  return v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
}

// NPH phases share one activation fragment: 4 when k == s == 2 (every phase is tap (0, 0) of the cell's own pixel), else 1
template <int G, bool PC, int NPH>
__global__ __launch_bounds__(256) void deconv_mfma_kernel(DeconvArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
  const int f0 = blockIdx.y * (16 * NT);
  const long long q0 = ((long long)blockIdx.x * 4 + wave) * (16 * MT);
  if (q0 >= p.Mq) return;  // (no barrier in this kernel)
  Cell cl[MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const long long q = q0 + 16 * mi + lr;
    cl[mi] = locate(p, q < p.Mq ? q : p.Mq - 1);  // ragged tile: the spare lanes redo the last cell and store nothing
  }
  const int nt = (p.N - f0 + 15) / 16 < NT ? (p.N - f0 + 15) / 16 : NT;  // 16-feature fragments of this block
  const int8_t* brow = p.Bp + (size_t)(f0 + lr) * p.Kpp + 16 * lq;
  const size_t bphase = (size_t)p.Ngp * p.Kpp;

  for (int ph0 = 0; ph0 < p.s * p.s; ph0 += NPH) {
    const int ry0 = ph0 / p.s, rx0 = ph0 - ry0 * p.s;
    // (NPH == 4: every phase has the one tap, K = C)
    const int Kph = NPH == 1 ? i8ie_deconv_taps(p.k, p.s, ry0) * i8ie_deconv_taps(p.k, p.s, rx0) * p.C : p.C;
    const int Kp = (Kph + 63) / 64 * 64;  // (0 for a phase without taps: its outputs are the offsets alone)
    const int2* tab = p.ktab + (size_t)ph0 * p.ktab_pitch;
    v4i acc[NPH][MT][NT];
#pragma unroll
    for (int h = 0; h < NPH; ++h)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[h][mi][ni] = v4i{0, 0, 0, 0};

    for (int k0 = 0; k0 < Kp; k0 += 64) {
      v4i a[MT];
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) a[mi] = gather16<G>(p, cl[mi], tab, k0 + 16 * lq) ^ (int)0x80808080;  // u8 -> s8
#pragma unroll
      for (int h = 0; h < NPH; ++h) {
        v4i b[NT];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          b[ni] = v4i{0, 0, 0, 0};
          if (ni < nt) b[ni] = *reinterpret_cast<const v4i*>(brow + (size_t)(ph0 + h) * bphase + (size_t)ni * 16 * p.Kpp + k0);
        }
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni)
            if (ni < nt) acc[h][mi][ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], a[mi], acc[h][mi][ni], 0, 0, 0);
      }
    }

#pragma unroll
    for (int h = 0; h < NPH; ++h) {
      const int ph = ph0 + h, ry = ph / p.s, rx = ph - ry * p.s;
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) {
        if (q0 + 16 * mi + lr >= p.Mq) continue;
        const int oy = cl[mi].qy * p.s + ry - p.p, ox = cl[mi].qx * p.s + rx - p.p;
        if ((unsigned)oy >= (unsigned)p.OH || (unsigned)ox >= (unsigned)p.OW) continue;  // (a cell at the grid's rim)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int f = f0 + 16 * ni + 4 * lq;
          if (ni >= nt || f >= p.N) continue;
          int c[4] = {acc[h][mi][ni].x, acc[h][mi][ni].y, acc[h][mi][ni].z, acc[h][mi][ni].w};
          finish4<PC>(p, c, cl[mi].img, oy, ox, ph, f);
        }
      }
    }
  }
}

// ---- deconv_direct ---------------------------------------------------------------------------------------------------
// item = (output pixel, quad of features), quads fastest: neighbouring lanes store neighbouring bytes of an NHWC pixel.
// DOT4: C % 4 == 0 and dword-aligned activations; otherwise byte by byte.  Every index is an int (checked by the launcher).
template <bool DOT4, bool PC>
__global__ __launch_bounds__(256) void deconv_direct_kernel(DeconvArgs p, int items) {
  const int nq = (p.N + 3) / 4, Hp = p.H + 2 * p.ib, Wp = p.W + 2 * p.ib, P = p.OH * p.OW;
  const int gstride = (int)gridDim.x * 256;
  // (items < 2^31 - 2^23 and gstride <= 2^22: `it` does not wrap)
  for (int it = (int)blockIdx.x * 256 + (int)threadIdx.x; it < items; it += gstride) {
    const int fq = it % nq, px = it / nq, f = 4 * fq;
    const int img = px / P, rem = px - img * P, oy = rem / p.OW, ox = rem - oy * p.OW;
    const int qy = (oy + p.p) / p.s, ry = (oy + p.p) - qy * p.s, qx = (ox + p.p) / p.s, rx = (ox + p.p) - qx * p.s;
    const int ph = ry * p.s + rx, Ty = i8ie_deconv_taps(p.k, p.s, ry), Tx = i8ie_deconv_taps(p.k, p.s, rx);
    const int8_t* w = p.Bp + (ph * p.Ngp + f) * p.Kpp;  // rows f .. f + 3 < Ngp exist (zero beyond N)
    int c[4] = {0, 0, 0, 0};
    for (int ty = 0; ty < Ty; ++ty)
      for (int tx = 0; tx < Tx; ++tx) {
        const int iy = qy - ty, ix = qx - tx;
        const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const uint8_t* a = p.A + ((img * Hp + iy + p.ib) * Wp + ix + p.ib) * p.C;  // (dereferenced only when `in`)
        const int8_t* wt = w + (ty * Tx + tx) * p.C;
        if constexpr (DOT4) {
          for (int ch = 0; ch < p.C; ch += 4) {
            const uint32_t av = (in ? *reinterpret_cast<const uint32_t*>(a + ch) : (uint32_t)p.zp_in * 0x01010101u) ^ 0x80808080u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int wv;
              __builtin_memcpy(&wv, wt + r * p.Kpp + ch, 4);  // (Kpp % 64 == 0, C % 4 == 0: aligned)
              c[r] = __builtin_amdgcn_sdot4((int)av, wv, c[r], false);
            }
          }
        } else {
          for (int ch = 0; ch < p.C; ++ch) {
            const int av = (in ? (int)a[ch] : p.zp_in) - 128;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] += av * (int)wt[r * p.Kpp + ch];
          }
        }
      }
    finish4<PC>(p, c, img, oy, ox, ph, f);
  }
}

// ---- FP32 form: one thread per output element, the phase taps of its pixel, fp32 sum in (ic, ty, tx) order + bias --------
__global__ __launch_bounds__(256) void deconv_f32_kernel(const float* __restrict__ in, const float* __restrict__ wt,
                                                         const float* __restrict__ b, float* __restrict__ out, int64_t total,
                                                         int c, int h, int w, int kc, int k, int s, int pd, int oh, int ow) {
  const int64_t gstride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += gstride) {
    const int ox = (int)(e % ow);
    int64_t t = e / ow;
    const int oy = (int)(t % oh);
    t /= oh;
    const int oc = (int)(t % kc);
    const int64_t img = t / kc;
    const int qy = (oy + pd) / s, ry = (oy + pd) - qy * s, qx = (ox + pd) / s, rx = (ox + pd) - qx * s;
    float sum = 0.0f;
    for (int ic = 0; ic < c; ++ic) {
      const float* xi = in + (img * c + ic) * (int64_t)h * w;
      const float* wi = wt + ((int64_t)ic * kc + oc) * k * k;
      for (int ky = ry, iy = qy; ky < k; ky += s, --iy) {
        if ((unsigned)iy >= (unsigned)h) continue;
        for (int kx = rx, ix = qx; kx < k; kx += s, --ix) {
          if ((unsigned)ix >= (unsigned)w) continue;
          sum += xi[(int64_t)iy * w + ix] * wi[ky * k + kx];
        }
      }
    }
    out[e] = sum + b[oc];
  }
}

inline int granularity(int C) { return C % 16 == 0 ? 16 : (C % 4 == 0 ? 4 : 1); }

}  // namespace

int i8ie_deconv_check_args(int kc, int c, int k, int stride, int pad, int opad) {
  I8IE_REQUIRE(kc > 0 && c > 0 && k > 0, "non-positive dimension");
  I8IE_REQUIRE(k < 65536, "kernel size");
  I8IE_REQUIRE(stride >= 1 && stride < 65536, "stride must be >= 1");
  I8IE_REQUIRE(pad >= 0 && pad <= k - 1, "padding must be in [0, kernel_size - 1]");
  I8IE_REQUIRE(opad >= 0 && opad < stride, "output_padding must be in [0, stride)");
  I8IE_REQUIRE((long long)c * k * k < (1 << 30), "reduction length");
  return I8IE_OK;
}

int i8ie_deconv_kpitch(int C, int k, int s) {
  const int T = i8ie_deconv_taps(k, s, 0);
  return (C * T * T + 63) / 64 * 64;
}

void i8ie_deconv_pack(const int8_t* qw, int N, int C, int k, int s, std::vector<int8_t>& panels, std::vector<int32_t>& tph) {
  const int Ngp = (N + 15) / 16 * 16, Kpp = i8ie_deconv_kpitch(C, k, s);
  panels.assign((size_t)s * s * Ngp * Kpp, 0);
  tph.assign((size_t)s * s * Ngp, 0);
  std::vector<int32_t> wsum((size_t)N, 0);
  for (int j = 0; j < N; ++j)
    for (size_t i = 0; i < (size_t)C * k * k; ++i) wsum[j] += qw[(size_t)j * C * k * k + i];
  for (int ry = 0; ry < s; ++ry)
    for (int rx = 0; rx < s; ++rx) {
      const int ph = ry * s + rx, Ty = i8ie_deconv_taps(k, s, ry), Tx = i8ie_deconv_taps(k, s, rx);
      for (int j = 0; j < N; ++j) {
        int32_t seen = 0;
        int8_t* row = panels.data() + ((size_t)ph * Ngp + j) * Kpp;
        for (int ty = 0; ty < Ty; ++ty)
          for (int tx = 0; tx < Tx; ++tx)
            for (int c = 0; c < C; ++c) {
              const int ky = ry + s * ty, kx = rx + s * tx;
              const int8_t v = qw[(((size_t)j * C + c) * k + (k - 1 - ky)) * k + (k - 1 - kx)];
              row[(size_t)(ty * Tx + tx) * C + c] = v;
              seen += v;
            }
        tph[(size_t)ph * Ngp + j] = wsum[j] - seen;
      }
    }
}

void i8ie_deconv_ktab(int C, int k, int s, std::vector<int>& tab) {
  const int G = granularity(C), pitch = i8ie_deconv_kpitch(C, k, s) / G;
  tab.assign((size_t)s * s * pitch * 2, 0);  // padding positions: tap (0, 0), channel 0 (their weights are zero)
  for (int ry = 0; ry < s; ++ry)
    for (int rx = 0; rx < s; ++rx) {
      const int Tx = i8ie_deconv_taps(k, s, rx), Kph = i8ie_deconv_taps(k, s, ry) * Tx * C;
      int* t = tab.data() + (size_t)(ry * s + rx) * pitch * 2;
      for (int kk = 0; kk < Kph; kk += G) {
        const int tap = kk / C, c = kk - tap * C;
        t[(size_t)(kk / G) * 2] = ((tap / Tx) << 16) | (tap % Tx);
        t[(size_t)(kk / G) * 2 + 1] = c;
      }
    }
}

bool i8ie_deconv_mfma_takes(const i8ie_ctx* ctx, const I8ieDeconvCall& c) {
  const int T = i8ie_deconv_taps(c.k, c.s, 0);
  if ((ctx->options & 1) != 0 || c.C * T * T < 32) return false;
  // (the gather reads G bytes at a time: the activations must be aligned to that)
  return aligned_to(c.A, granularity(c.C)) && aligned_to(c.Bp, 16);
}

int i8ie_deconv_launch(i8ie_ctx* ctx, const I8ieDeconvCall& c) {
  I8IE_REQUIRE(c.k < 65536 && c.s >= 1 && c.s < 65536, "transposed conv: kernel size / stride");
  DeconvArgs a{};
  a.A = c.A; a.H = c.H; a.W = c.W; a.C = c.C; a.ib = c.ib;
  a.OH = c.OH; a.OW = c.OW; a.k = c.k; a.s = c.s; a.p = c.p;
  a.QH = (c.OH - 1 + c.p) / c.s + 1; a.QW = (c.OW - 1 + c.p) / c.s + 1;
  a.N = c.N; a.Ngp = c.Ngp; a.Kpp = c.Kpp; a.ktab_pitch = c.Kpp / granularity(c.C);
  a.Mq = (long long)c.m * a.QH * a.QW;
  a.Bp = c.Bp; a.ktab = reinterpret_cast<const int2*>(c.ktab); a.ocp = c.ep.ocp; a.tph = c.tph; a.msv = c.ep.msv; a.sbv = c.ep.sbv;
  a.rq = i8ie_make_requant(c.ep.s_in, c.ep.s_w, c.ep.s_out, c.ep.zp_out);
  a.relu_lo = c.ep.relu ? c.ep.zp_out : 0; a.zp_in = c.zp_in;
  a.out = c.out; a.ob = c.ob; a.acc = c.ep.acc;
  a.vec_out = (c.N % 4 == 0 && aligned_to(c.out, 4)) ? 1 : 0;
  const bool pc = c.ep.msv != nullptr;
  const double M = (double)c.m * c.OH * c.OW;
  const double ops = 2.0 * (double)c.m * c.H * c.W * c.C * c.N * c.k * c.k;  // the real MACs
  const double bytes = (double)c.m * c.H * c.W * c.C + M * c.N + (double)c.s * c.s * c.Ngp * c.Kpp;
  if (i8ie_deconv_mfma_takes(ctx, c)) {
    const long long tiles = (a.Mq + 64 * MT - 1) / (64 * MT);
    I8IE_REQUIRE(tiles < ((long long)1 << 31), "transposed conv: too many pixels in one call");
    const dim3 grid((unsigned)tiles, (unsigned)((c.N + 16 * NT - 1) / (16 * NT)), 1);
    I8IE_REQUIRE(grid.y <= 65535u, "transposed conv: too many features");
    I8ieProfScope prof(ctx, "deconv_mfma", ops, bytes);
    const int G = granularity(c.C);
    const bool ks2 = c.k == 2 && c.s == 2;
#define I8IE_DECONV_MFMA(GG)                                                                   \
  do {                                                                                         \
    if (ks2) {                                                                                 \
      if (pc) deconv_mfma_kernel<GG, true, 4><<<grid, 256, 0, ctx->stream>>>(a);               \
      else deconv_mfma_kernel<GG, false, 4><<<grid, 256, 0, ctx->stream>>>(a);                 \
    } else {                                                                                   \
      if (pc) deconv_mfma_kernel<GG, true, 1><<<grid, 256, 0, ctx->stream>>>(a);               \
      else deconv_mfma_kernel<GG, false, 1><<<grid, 256, 0, ctx->stream>>>(a);                 \
    }                                                                                          \
  } while (0)
    if (G == 16) I8IE_DECONV_MFMA(16);
    else if (G == 4) I8IE_DECONV_MFMA(4);
    else I8IE_DECONV_MFMA(1);
#undef I8IE_DECONV_MFMA
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  // deconv_direct: 32-bit index arithmetic
  const long long lim = ((long long)1 << 31) - ((long long)1 << 23);
  const long long items = (long long)c.m * c.OH * c.OW * ((c.N + 3) / 4);
  I8IE_REQUIRE((long long)c.m * (c.H + 2 * c.ib) * (c.W + 2 * c.ib) * c.C < lim &&
                   (long long)c.m * (c.OH + 2 * c.ob) * (c.OW + 2 * c.ob) * c.N < lim && items < lim &&
                   (long long)c.s * c.s * c.Ngp * c.Kpp < lim,
               "transposed conv: the direct kernel indexes with 32 bits");
  long long blocks = (items + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  const bool dot4 = c.C % 4 == 0 && aligned_to(c.A, 4) && aligned_to(c.Bp, 4);
  I8ieProfScope prof(ctx, "deconv_direct", ops, bytes);
  if (dot4) {
    if (pc) deconv_direct_kernel<true, true><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, (int)items);
    else deconv_direct_kernel<true, false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, (int)items);
  } else {
    if (pc) deconv_direct_kernel<false, true><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, (int)items);
    else deconv_direct_kernel<false, false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(a, (int)items);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_deconv_f32_launch(i8ie_ctx* ctx, const float* in, int n, int c, int h, int w, const float* wt, const float* b, int kc,
                           int k, int s, int p, int oh, int ow, float* out) {
  const int64_t total = (int64_t)n * kc * oh * ow;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  I8ieProfScope prof(ctx, "deconv_f32", 0.0, (double)total * 4 + (double)n * c * h * w * 4);
  deconv_f32_kernel<<<(unsigned)blocks, 256, 0, ctx->stream>>>(in, wt, b, out, total, c, h, w, kc, k, s, p, oh, ow);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
