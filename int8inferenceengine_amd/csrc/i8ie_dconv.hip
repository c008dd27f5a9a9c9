// i8ie_dconv.hip -- dense dilated Conv2d at stride 1 in INT8 (Conv2d dilation=, groups = 1).
//   reference: src/conv2d.cc:100-142 with the kernel inflated by zeros; dilation: not in the reference
//
// At stride 1 the output pixel (oy, ox) reads input pixels of one phase ((oy - p) mod d, (ox - p) mod d) only.  dconv_mfma works
// on the phase-subsampled planes: output pixels (py + d i, px + d j) of one image and phase (py, px) form a plane, cut into
// 4 x 4 tiles.  A tile's input patch, (k + 3) x (k + 3) pixels of that phase -- global pixel pitch d C, row pitch d Wp C -- is
// loaded densely into LDS, out-of-image positions filled with zp_in, every byte re-biased ^0x80 once on the way (the term
// 128 * wsum[j] is in ocp).  In LDS it is an ordinary dilation-1 patch: the halo does not grow with d, the K loop has no bounds
// predicate, and the dilation lives in the patch-load and the output-store addresses alone.
//   block   256 lanes = 4 waves; 8 slots (a slot = one tile of one (image, phase) plane = 16 MFMA rows, so the 128 rows of a
//           block come from up to 8 patches) by 64 features
//   wave    16 features by all 8 slots: a weight fragment, read once per block as a coalesced 16-byte-per-lane fragment from
//           global memory (the panel is a few hundred KiB at most: L2), meets 128 pixel rows
//   K       walked in channel chunks of CC <= 64 bytes per pixel (the patches of a chunk are staged between two barriers,
//           outside the tap loop), inside a chunk in (kh, kw, c) order, 64 bytes per v_mfma_i32_16x16x64_i8
// Accumulation is exact INT32, the epilogue the requantiser of i8ie_requant.h (per-tensor and per-channel instances) with the
// optional ReLU clamp, the border the consumer asks for and the INT32 sums on request.
#include "i8ie_internal.h"
#include "i8ie_epilogue.h"
#include "i8ie_dconv.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int SLOTS = 8, TS = 4;  // slots per block; a slot is a TS x TS tile

struct DconvArgs {
  const uint8_t* A;
  int H, W, C, ib, OH, OW, pad, k, dil;
  int N, Kgp, CC;         // CC: channel chunk (bytes per pixel in LDS), a multiple of 16 dividing C
  int tyN, txN, spi;      // tiles per plane (of the largest phase) and slots per image = dil^2 tyN txN
  long long S;            // m * spi slots
  const int8_t* Bp;
  I8ieEpiArgs ep;
  int zp_in;
  uint8_t* out;
  int ob, vec_out;
};

struct Slot {
  long long img;
  int py, px, ty, tx;
  bool ok;
};
__device__ __forceinline__ Slot decode(const DconvArgs& p, long long s) {
  Slot q;
  q.ok = s < p.S;
  if (!q.ok) s = 0;
  q.img = s / p.spi;
  const int r = (int)(s - q.img * p.spi), tpp = p.tyN * p.txN;
  const int ph = r / tpp, t = r - ph * tpp;
  q.py = ph / p.dil; q.px = ph - q.py * p.dil;
  q.ty = t / p.txN; q.tx = t - q.ty * p.txN;
  return q;
}

template <bool PC>
__global__ __launch_bounds__(256) void dconv_mfma_kernel(DconvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t patch[];  // [SLOTS][PW][PW][CC], re-biased
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
  const int PW = p.k + TS - 1, PP = PW * PW, CU = p.CC >> 4;
  const long long s0 = (long long)blockIdx.x * SLOTS;
  const int f0 = blockIdx.y * 64 + 16 * wave;  // this wave's 16 features
  const bool active = f0 < p.N;                // (an idle wave still loads patches and meets the barriers)
  const int Hp = p.H + 2 * p.ib, Wp = p.W + 2 * p.ib;
  const int ti = lr >> 2, tj = lr & 3;         // this lane's row inside a tile
  const int8_t* brow = p.Bp + (size_t)(active ? f0 + lr : 0) * p.Kgp;
  const int KC = p.k * p.k * p.CC;             // K bytes of one chunk
  v4i acc[SLOTS];
#pragma unroll
  for (int mi = 0; mi < SLOTS; ++mi) acc[mi] = v4i{0, 0, 0, 0};

  for (int c0 = 0; c0 < p.C; c0 += p.CC) {
    __syncthreads();  // everyone is done with the previous chunk
    for (int idx = threadIdx.x; idx < SLOTS * PP * CU; idx += 256) {
      const int sl = idx / (PP * CU), rem = idx - sl * (PP * CU), pos = rem / CU, e = rem - pos * CU;
      const int u = pos / PW, v = pos - u * PW;
      const Slot q = decode(p, s0 + sl);
      const int y = q.py - p.pad + p.dil * (TS * q.ty + u) + p.ib, x = q.px - p.pad + p.dil * (TS * q.tx + v) + p.ib;
      const int zp4 = (int)((uint32_t)p.zp_in * 0x01010101u);
      v4i val = {zp4, zp4, zp4, zp4};
      if (q.ok && (unsigned)y < (unsigned)Hp && (unsigned)x < (unsigned)Wp)
        val = *reinterpret_cast<const v4i*>(p.A + ((q.img * Hp + y) * Wp + x) * p.C + c0 + 16 * e);
      *reinterpret_cast<v4i*>(patch + (size_t)(sl * PP + pos) * p.CC + 16 * e) = val ^ (int)0x80808080;  // u8 -> s8, once
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < KC; j += 64) {
      const int kk = j + 16 * lq;
      const bool on = kk < KC;  // (the chunk's K tail: not a bounds test of a tap)
      const int tap = on ? kk / p.CC : 0, ch = on ? kk - tap * p.CC : 0;
      const int ky = tap / p.k, kx = tap - ky * p.k;
      v4i b = {0, 0, 0, 0};
      if (on) b = *reinterpret_cast<const v4i*>(brow + (size_t)tap * p.C + c0 + ch);
      const uint8_t* arow = patch + (size_t)((ti + ky) * PW + tj + kx) * p.CC + ch;
#pragma unroll
      for (int mi = 0; mi < SLOTS; ++mi) {
        v4i a = {0, 0, 0, 0};
        if (on) a = *reinterpret_cast<const v4i*>(arow + (size_t)mi * PP * p.CC);
        acc[mi] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a, acc[mi], 0, 0, 0);
      }
    }
  }
  if (!active) return;

  // ---- the quad epilogue (i8ie_epilogue.h): features f .. f + 3 of the pixel of row lr in each slot
  const int f = f0 + 4 * lq;
  if (f >= p.N) return;
  const int nf = p.N - f < 4 ? p.N - f : 4;
  const I8ieQuadCols<PC> cols = i8ie_epi_cols<PC>(p.ep, f, nf);
#pragma unroll
  for (int mi = 0; mi < SLOTS; ++mi) {
    const Slot q = decode(p, s0 + mi);
    const int oy = q.py + p.dil * (TS * q.ty + ti), ox = q.px + p.dil * (TS * q.tx + tj);
    if (!q.ok || oy >= p.OH || ox >= p.OW) continue;
    int c[4] = {acc[mi].x, acc[mi].y, acc[mi].z, acc[mi].w};
    const long long px = (q.img * p.OH + oy) * p.OW + ox;
    const long long opix = (q.img * (p.OH + 2 * p.ob) + oy + p.ob) * (p.OW + 2 * p.ob) + ox + p.ob;
    i8ie_epi_finish<PC>(p.ep, c, cols, nf, px * p.N + f, p.out + opix * p.N + f, p.vec_out && nf == 4);
  }
}

// the channel chunk: all of C up to 64, else the largest of 64 / 32 / 16 dividing C
int chunk_of(int C) { return C <= 64 ? C : (C % 64 == 0 ? 64 : (C % 32 == 0 ? 32 : 16)); }
size_t lds_bytes(const I8ieDconvCall& c) { return (size_t)SLOTS * (c.k + TS - 1) * (c.k + TS - 1) * chunk_of(c.C); }

}  // namespace

bool i8ie_dconv_takes(const i8ie_ctx* ctx, const I8ieDconvCall& c) {
  if ((ctx->options & 1) != 0 || c.dil < 2 || c.k < 2 || c.C % 16 != 0 || (long long)c.C * c.k * c.k < 32) return false;
  if (!aligned_to(c.A, 16) || !aligned_to(c.Bp, 16)) return false;
  return lds_bytes(c) <= (size_t)64 << 10;
}

int i8ie_dconv_launch(i8ie_ctx* ctx, const I8ieDconvCall& c) {
  I8IE_REQUIRE(i8ie_dconv_takes(ctx, c), "dilated conv: not a launch of the dense kernel");
  DconvArgs a{};
  a.A = c.A; a.H = c.H; a.W = c.W; a.C = c.C; a.ib = c.ib; a.OH = c.OH; a.OW = c.OW; a.pad = c.pad; a.k = c.k; a.dil = c.dil;
  a.N = c.N; a.Kgp = c.Kgp; a.CC = chunk_of(c.C);
  a.tyN = ((c.OH + c.dil - 1) / c.dil + TS - 1) / TS;
  a.txN = ((c.OW + c.dil - 1) / c.dil + TS - 1) / TS;
  const long long spi = (long long)c.dil * c.dil * a.tyN * a.txN;
  I8IE_REQUIRE(spi < ((long long)1 << 30), "dilated conv: too many tiles per image");
  a.spi = (int)spi;
  a.S = (long long)c.m * spi;
  a.Bp = c.Bp; a.ep = i8ie_epi_args(c.ep); a.zp_in = c.zp_in;
  a.out = c.out; a.ob = c.ob;
  a.vec_out = (c.N % 4 == 0 && aligned_to(c.out, 4)) ? 1 : 0;
  const long long blocks = (a.S + SLOTS - 1) / SLOTS;
  I8IE_REQUIRE(blocks < ((long long)1 << 31), "dilated conv: too many output pixels in one call");
  const dim3 grid((unsigned)blocks, (unsigned)((c.N + 63) / 64));
  I8IE_REQUIRE(grid.y <= 65535u, "dilated conv: too many features");
  const double M = (double)c.m * c.OH * c.OW;
  I8ieProfScope prof(ctx, "dconv_mfma", 2.0 * M * c.N * c.C * c.k * c.k,
                     (double)c.m * c.H * c.W * c.C + M * c.N + (double)c.Ngp * c.Kgp);
  const size_t lds = lds_bytes(c);
  if (c.ep.msv != nullptr) dconv_mfma_kernel<true><<<grid, 256, lds, ctx->stream>>>(a);
  else dconv_mfma_kernel<false><<<grid, 256, lds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
