// i8ie_sp24pw.hip -- pointwise (1 x 1, stride 1) Conv2d with 2:4 structured-sparse 8-bit weights on the sparse INT8 MFMA (DESIGN.md
// section 8zd), not in the reference: the qkv / proj / MLP layers that the transformer examples write as 1 x 1 convolutions on NHWC
// token maps.
//
//   C[g][j] = sum_c A_u8[g][c] * W_s8[j][c] + oc[j];  out = relu?(down_scale(C))       g: a pixel of any image, oc: with the bias
//
// A 2:4 pointwise conv is an INT8 Conv2d, per tensor or per channel, whose weight integers have at most two non-zeros in every
// aligned group of four channels: oc (src/conv2d.cc:117-124) and the requantiser (i8ie_epilogue.h, both forms) are unchanged.
// The channels of an NHWC pixel are contiguous, so the groups of four are and K needs no permutation.  Two existing pieces meet:
//   the weights  the compressed panel of i8ie_sp24lin.h, unchanged: chunks of 512 K, per feature tile and chunk four value
//                fragments and one position fragment of 1 KiB; a fragment is the `a` operand (or four `idx` dwords) of
//                v_smfmac_i32_16x16x128_i8 as it lies.  The instruction's pairing is written at the top of i8ie_sp24lin.hip.
//   the map      PwSide / pw_pixel of i8ie_w4pw.h: a pixel is a row of C contiguous bytes addressed per pixel, so a border byte
//                is never read as a channel; a row past M repeats pixel M - 1; re-biased input bytes enter as they are (128 *
//                wsum is in ocp), a re-biased output is the packed quad ^0x80808080, the output's border is the caller's.
//
// sp24pw_mfma: a block owns 16 RT pixels, 16 WF FPW features and all of K.  K is walked in STAGES of 128 KSTEPS values -- a whole
// panel chunk (KSTEPS = 4) or half of one (KSTEPS = 2: two value fragments plus the position fragment, 3 KiB per feature tile);
// per stage the block's pixel rows (128 KSTEPS bytes each, 16-byte slots swizzled by the row as in i8ie_flin.hip) and its
// fragments arrive by LDS-DMA in a ring, one barrier per stage.  The block's WF KS waves are a grid of their own: wave (wf, wk)
// owns feature tiles FPW wf .. FPW wf + FPW - 1, ALL row tiles, and the 128-steps v = wk (mod KS) of every stage.  So a weight
// fragment and an idx dword are read from LDS by exactly one wave, a 32-byte activation operand meets FPW sparse MFMAs, and a
// wave's register tile is RT x FPW output tiles however few waves share a feature tile.  The KS partial tiles meet in LDS behind
// the K loop, where every wave keeps 1 / KS of its tiles and requantises those: the epilogue is spread over all waves.
//   <1, 2, 1, 2, 4, 4>  up to kSp24pwFewRows pixels: 16 pixels x 32 features, 4 waves, 18 KiB per chunk of which 10 are weights,
//                       4 stages (80 KiB: two blocks per CU) -- a stream over the panel by many small blocks
//   <4, 2, 4, 2, 2, 2>  more pixels: 64 pixels x 128 features, 4 waves with 4 x 4 register tiles, a stage of HALF a chunk (16 KiB
//                       of pixels, 24 KiB of fragments), 2 stages (80 KiB: two blocks per CU).  A wave reads 12 KiB of LDS per
//                       16 sparse MFMAs (sp24lin_mfma's many-row shape: 26 KiB); a block's pixels are fetched once per 128 features
// A step at or past C is skipped; a step that straddles C multiplies the panel's zeros with what lies behind the pixel (or,
// past the buffer, the resource's zeros).  Blocks are numbered feature block fastest: the blocks that share 64 pixels run side
// by side and find them in L2.
// sp24pw_direct: the definition, one lane per output value, NHWC (any border) or NCHW at either end, plain or re-biased:
// C % 32 != 0, NCHW operands, unaligned buffers and the force-fallback option.
#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_sp24lin.h"
#include "i8ie_sp24pw.h"
#include "i8ie_w4pw.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

struct SpwArgs {
  const uint8_t* A;  // the whole input, border included
  unsigned a_bytes;
  int C, M, N, nch;  // M: pixels of all images; nch: panel chunks of 512 K
  PwSide in, os;
  unsigned a_xor;    // 0x80808080 for plain bytes (u8 -> s8), 0 for re-biased ones
  const uint8_t* B;  // the panel
  unsigned b_bytes;
  I8ieEpiArgs ep;    // ocp = oc + 128 * wsum; ocp, msv, sbv: [Npad]
  uint8_t* out;
  unsigned o_xor;
  int vec_out;       // N % 4 == 0 and `out` dword aligned: a whole quad is one store
};

// a block of 16 RT pixels x 16 WF FPW features; waves (wf, wk); a stage of KSTEPS 128-steps; a ring of STAGES stages
template <int RT, int WF, int FPW, int KS, int KSTEPS, int STAGES>
struct SpwShape {
  static constexpr int kWaves = WF * KS, kThreads = 64 * kWaves, kFT = WF * FPW;
  static constexpr int kRows = 16 * RT, kFeats = 16 * kFT, kTiles = RT * FPW;
  static constexpr int kRowBytes = 128 * KSTEPS, kSlots = 8 * KSTEPS;  // a pixel's bytes of a stage, as 16-byte slots
  static constexpr int kHalves = 4 / KSTEPS;                           // stages per panel chunk
  static constexpr int kFrags = KSTEPS + 1;                            // a feature tile's fragments of a stage: values, positions
  static constexpr int kPA = 2 * RT * KSTEPS, kPB = kFT * kFrags;      // 1-KiB DMA pieces of a stage: 64 / kSlots pixels / one fragment
  static constexpr int kPPW = (kPA + kPB + kWaves - 1) / kWaves;       // pieces per wave and stage (every wave issues the same number)
  static constexpr int kStageA = kPA * 1024;
  static constexpr int kStage = kPPW * kWaves * 1024;                  // (pieces past kPA + kPB land in the stage's padding)
  static constexpr int kLds = STAGES * kStage;
  static constexpr int kTPO = (kTiles + KS - 1) / KS;                  // tiles a wave keeps behind the K loop
  static constexpr int kXch = WF * KS * (KS - 1) * kTPO * 1024;        // the partial tiles on their way to their keepers
  static_assert(KSTEPS == 2 || KSTEPS == 4, "a stage is a panel chunk or half of one");
  static_assert(KSTEPS % KS == 0, "every wave of a feature tile takes the same number of steps");
  static_assert(STAGES >= 2 && (STAGES - 2) * kPPW < 64, "the vmcnt immediate");
  static_assert(kLds <= 80 * 1024, "two blocks per CU");
  static_assert(kXch <= kLds, "the exchange reuses the ring");
};

// c with oc' -> the accumulators' copy -> requantise -> (re-bias) -> store: the quad epilogue's steps (a conv has no float bias)
template <bool PC>
__device__ __forceinline__ void spw_finish(const I8ieEpiArgs& ep, int (&c)[4], const I8ieQuadCols<PC>& q, int nf, long long acc0,
                                           uint8_t* o, bool whole, uint32_t o_xor) {
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] += q.oc[r];
  i8ie_epi_copy_acc(ep, c, acc0, nf);
  i8ie_epi_store(o, i8ie_epi_pack<PC>(ep, c, q) ^ o_xor, whole, nf);
}

template <int RT, int WF, int FPW, int KS, int KSTEPS, int STAGES, bool PC>
__global__ __launch_bounds__(64 * WF * KS) void sp24pw_mfma_kernel(SpwArgs p, unsigned nfb) {
  using S = SpwShape<RT, WF, FPW, KS, KSTEPS, STAGES>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const int wf = wave % WF, wk = wave / WF;  // this wave's feature tiles / its steps of a stage
  const unsigned fb = blockIdx.x % nfb, rb = blockIdx.x / nfb;  // feature block fastest
  const int ft0 = (int)fb * S::kFT, row0 = (int)rb * S::kRows;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A), 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a stage: kPA of A (64 / kSlots pixels each; lane l: row, LDS slot l % kSlots, source slot that ^ (row & 15)),
  //      kPB of B (fragment (ft, 0 .. KSTEPS - 1 of this half | 4) as it lies), the rest padding; wave w issues pieces w, w + kWaves, ...
  //      A row past M repeats pixel M - 1 (nothing of it is stored).  A stage past C reads the bytes behind the pixel or, past
  //      the buffer, zeros, and so does a feature tile past the panel: the panel holds zeros there.
  const int nch = p.nch, nst = (p.C + S::kRowBytes - 1) / S::kRowBytes;  // (a half chunk wholly past C is never walked)
  const int rot = (int)(fb % (unsigned)nst);
  unsigned src[S::kPPW], chunk_bytes[S::kPPW], half_bytes[S::kPPW];
#pragma unroll
  for (int j = 0; j < S::kPPW; ++j) {
    const int pi = wave + S::kWaves * j;
    if (pi < S::kPA) {
      const int row = pi * (64 / S::kSlots) + lane / S::kSlots, slot = lane % S::kSlots;
      const int g = row0 + row < p.M ? row0 + row : p.M - 1;
      src[j] = (unsigned)(pw_pixel(p.in, g) * p.C) + (unsigned)((slot ^ (row & 15)) * 16);
      chunk_bytes[j] = 512;
      half_bytes[j] = S::kRowBytes;
    } else {
      const int f = (pi - S::kPA) % S::kPB;  // (padding pieces: a second copy of a B piece, unused)
      const int fr = f % S::kFrags;
      src[j] = (unsigned)((ft0 + f / S::kFrags) * nch * 5 + (fr < KSTEPS ? fr : 4)) * 1024u + (unsigned)lane * 16u;
      chunk_bytes[j] = 5120;
      half_bytes[j] = fr < KSTEPS ? KSTEPS * 1024 : 0;
    }
  }
  auto issue = [&](int step) {  // the stage of walk position `step` -> ring slot step % STAGES
    int t = step + rot;
    while (t >= nst) t -= nst;
    const unsigned ch = (unsigned)(t / S::kHalves), half = (unsigned)(t % S::kHalves);
    uint8_t* st = smem + (step % STAGES) * S::kStage;
#pragma unroll
    for (int j = 0; j < S::kPPW; ++j) {
      const int pi = wave + S::kWaves * j;
      const int off = (int)(src[j] + ch * chunk_bytes[j] + half * half_bytes[j]);
      if (pi < S::kPA)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16, off, 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16, off, 0, 0, 0);
    }
  };

  v4i acc[RT][FPW];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int f = 0; f < FPW; ++f) acc[rt][f] = v4i{0, 0, 0, 0};
  const int bfrag = S::kStageA + wf * FPW * S::kFrags * 1024 + lane * 16;  // fragment 0 of this wave's first feature tile, this lane's 16 bytes
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i) issue(nst > i ? i : 0);
  for (int step = 0; step < nst; ++step) {
    // my pieces of this stage (the STAGES - 2 stages after it may be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * S::kPPW) : "memory");
    asm volatile("s_barrier" ::: "memory");  // everyone's pieces; everyone is done with the previous stage
    issue(step + STAGES - 1);  // -> the slot of the previous stage (past the end the walk wraps: keeps the vmcnt counts uniform)
    const uint8_t* st = smem + (step % STAGES) * S::kStage;
    const int t = step + rot < nst ? step + rot : step + rot - nst;
    const int half = t % S::kHalves, k0 = t * S::kRowBytes;  // the stage's first K value (uniform)
#pragma unroll
    for (int v0 = 0; v0 < KSTEPS; v0 += KS) {
      const int v = v0 + wk;
      if (k0 + 128 * v >= p.C) break;
      v4i w[FPW];
      int idx[FPW];
#pragma unroll
      for (int f = 0; f < FPW; ++f) {
        w[f] = *reinterpret_cast<const v4i*>(st + bfrag + f * S::kFrags * 1024 + v * 1024);
        idx[f] = *reinterpret_cast<const int*>(st + bfrag + f * S::kFrags * 1024 + KSTEPS * 1024 + 4 * (half * KSTEPS + v));
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const uint8_t* arow = st + (rt * 16 + lr) * S::kRowBytes;  // slot s of row r at (s ^ (r & 15)) * 16
        const v4i lo = *reinterpret_cast<const v4i*>(arow + ((8 * v + lq) ^ lr) * 16) ^ (int)p.a_xor;
        const v4i hi = *reinterpret_cast<const v4i*>(arow + ((8 * v + 4 + lq) ^ lr) * 16) ^ (int)p.a_xor;
        const v8i a = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int f = 0; f < FPW; ++f) acc[rt][f] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(w[f], a, acc[rt][f], idx[f], 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wrapped pieces: nothing may land after the block is gone)

  // ---- the KS partial tiles of a feature tile group: tile ti = rt FPW + f is kept by wave (wf, ti % KS); the others hand theirs
  //      over through the ring's memory
  if constexpr (KS > 1) {
    asm volatile("s_barrier" ::: "memory");  // everyone has landed and is done reading the stages
    v4i* xch = reinterpret_cast<v4i*>(smem) + lane;
    auto slot = [&](int keeper, int from, int i) {  // (from != keeper)
      return (((wf * KS + keeper) * (KS - 1) + (from - (from > keeper ? 1 : 0))) * S::kTPO + i) * 64;
    };
#pragma unroll
    for (int ti = 0; ti < S::kTiles; ++ti)
      if (ti % KS != wk) xch[slot(ti % KS, wk, ti / KS)] = acc[ti / FPW][ti % FPW];
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < S::kTiles; ++ti)
      if (ti % KS == wk) {
#pragma unroll
        for (int o = 1; o < KS; ++o) acc[ti / FPW][ti % FPW] += xch[slot(wk, (wk + o) % KS, ti / KS)];
      }
  }

  // ---- the quad epilogue: lane (q, r) holds features 4 q .. 4 q + 3 of pixel row0 + 16 rt + r of each tile this wave keeps
#pragma unroll
  for (int ti = 0; ti < S::kTiles; ++ti) {
    if (ti % KS != wk) continue;
    const int rt = ti / FPW, f = ti % FPW;
    const int g = row0 + rt * 16 + lr, n = (ft0 + wf * FPW + f) * 16 + 4 * lq;
    if (g >= p.M || n >= p.N) continue;
    int cv[4] = {acc[rt][f].x, acc[rt][f].y, acc[rt][f].z, acc[rt][f].w};
    const int nf = p.N - n < 4 ? p.N - n : 4;
    // (n < N <= Npad, n % 4 == 0: the quad lies inside the padded arrays)
    spw_finish<PC>(p.ep, cv, i8ie_epi_cols_vec<PC>(p.ep, n), nf, (long long)g * p.N + n, p.out + pw_pixel(p.os, g) * p.N + n,
                   p.vec_out && nf == 4, p.o_xor);
  }
}

// ---- sp24pw_direct: the definition.  One lane per output (g, j): the sum over the kept values of feature j, each against the
// channel at its dense position; either side NHWC (any border) or NCHW ---------------------------------------------------------
struct SpwDirectArgs {
  const uint8_t* A;
  int C, M, N, nch, in_nchw, out_nchw;
  PwSide in, os;
  unsigned a_xor, o_xor;  // 0x80 where that side is stored re-biased
  const uint8_t* B;
  I8ieEpiArgs ep;         // ocp here: the plain oc (the activations enter as u8)
  uint8_t* out;
};

template <bool PC>
__global__ __launch_bounds__(256) void sp24pw_direct_kernel(SpwDirectArgs p) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.M * p.N) return;
  const long long g = item / p.N;
  const int j = (int)(item - g * p.N);
  const long long img = g / p.in.HW, rem = g - img * p.in.HW;
  const uint8_t* a = p.in_nchw ? p.A + img * p.C * p.in.HW + rem : p.A + pw_pixel(p.in, g) * p.C;
  const long long pitch = p.in_nchw ? p.in.HW : 1;
  int sum = 0;
  for (int g4 = 0; 4 * g4 < p.C; ++g4) {
    const unsigned nib = (p.B[i8ie_sp24_index_at(j, g4, p.nch)] >> (4 * (g4 & 1))) & 15u;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = 4 * g4 + (int)((nib >> (2 * e)) & 3u);
      if (k >= p.C) continue;  // (a partial last group: the value there is 0)
      sum += (int)(a[k * pitch] ^ p.a_xor) * (int)(int8_t)p.B[i8ie_sp24_value_at(j, g4, e, p.nch)];
    }
  }
  int cv[4] = {sum, 0, 0, 0};
  uint8_t* o = p.out_nchw ? p.out + (img * p.N + j) * p.os.HW + rem : p.out + pw_pixel(p.os, g) * p.N + j;
  spw_finish<PC>(p.ep, cv, i8ie_epi_cols<PC>(p.ep, j, 1), 1, item, o, false, p.o_xor);
}

// ---- the one-off kernel of a handle: sp24_offsets_kernel's conv form ---------------------------------------------------------
// src/conv2d.cc:117-124 from the compressed panel: one thread per feature replays the reference's sequential fp32 accumulation
// with k ascending (a group's first position is below its second; the zeros between add +0 and are skipped) and folds the
// bias in; also the exact row sum and oc'
__global__ __launch_bounds__(64) void sp24pw_offsets_kernel(const uint8_t* __restrict__ B, const int8_t* __restrict__ qb, int n, int K,
                                                            int nch, float s_in, int zp_in, int32_t* __restrict__ oc,
                                                            int32_t* __restrict__ wsum, int32_t* __restrict__ ocp) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  float t = 0.0f;
  int s = 0;
  for (int g = 0; 4 * g < K; ++g)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int q = (int)(int8_t)B[i8ie_sp24_value_at(j, g, e, nch)];
      t = t + (float)(zp_in * q);
      s += q;
    }
  oc[j] = (int)((float)qb[j] / s_in - t);
  wsum[j] = s;
  ocp[j] = oc[j] + 128 * s;
}

template <int RT, int WF, int FPW, int KS, int KSTEPS, int STAGES, bool PC>
int spw_launch_t(i8ie_ctx* ctx, const SpwArgs& a) {
  using S = SpwShape<RT, WF, FPW, KS, KSTEPS, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&sp24pw_mfma_kernel<RT, WF, FPW, KS, KSTEPS, STAGES, PC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kLds));
    raised[dev] = true;
  }
  const long long nfb = (a.N + S::kFeats - 1) / S::kFeats, nrb = (a.M + S::kRows - 1) / S::kRows;
  I8IE_REQUIRE(nfb * nrb < ((long long)1 << 31), "sp24pw_mfma: too many blocks in one call");
  sp24pw_mfma_kernel<RT, WF, FPW, KS, KSTEPS, STAGES, PC><<<(unsigned)(nfb * nrb), S::kThreads, S::kLds, ctx->stream>>>(a, (unsigned)nfb);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

template <bool PC>
int spw_launch_rows(i8ie_ctx* ctx, const SpwArgs& a) {
  if (a.M <= kSp24pwFewRows) return spw_launch_t<1, 2, 1, 2, 4, 4, PC>(ctx, a);
  return spw_launch_t<4, 2, 4, 2, 2, 2, PC>(ctx, a);
}

bool shape_ok(const I8ieSp24pwCall& c) {
  return c.m > 0 && c.H > 0 && c.W > 0 && c.C > 0 && c.C <= 65536 && c.N > 0 && c.ib >= 0 && c.ob >= 0 &&
         (long long)c.m * c.H * c.W < ((long long)1 << 31) - 64 && !(c.in_nchw && (c.ib || c.in_s8)) && !(c.out_nchw && (c.ob || c.out_s8));
}
bool epilogue_ok(const I8ieSp24pwCall& c) { return (c.ep.msv == nullptr) == (c.ep.sbv == nullptr) && c.ep.biasf == nullptr; }
size_t in_bytes(const I8ieSp24pwCall& c) { return (size_t)c.m * (c.H + 2 * c.ib) * (c.W + 2 * c.ib) * c.C; }
double algo_bytes(const I8ieSp24pwCall& c) {
  const double M = (double)c.m * c.H * c.W;
  return M * c.C + 0.625 * c.N * c.C + M * c.N;
}

}  // namespace

bool i8ie_sp24pw_mfma_takes(const I8ieSp24pwCall& c) {
  const size_t limit = ((size_t)1 << 32) - 8192;  // (32-bit buffer offsets)
  return shape_ok(c) && c.C % 32 == 0 && !c.in_nchw && !c.out_nchw && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 &&
         (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0 && in_bytes(c) < limit && i8ie_sp24_panel_bytes(c.N, c.C) < limit;
}

int i8ie_sp24pw_mfma_launch(i8ie_ctx* ctx, const I8ieSp24pwCall& c) {
  I8IE_REQUIRE(i8ie_sp24pw_mfma_takes(c), "sp24pw_mfma: shape, layout or alignment");
  I8IE_REQUIRE(epilogue_ok(c), "sp24pw_mfma: epilogue vectors (a conv's bias is in oc)");
  SpwArgs a{};
  a.A = c.A; a.a_bytes = (unsigned)in_bytes(c); a.C = c.C; a.M = c.m * c.H * c.W; a.N = c.N; a.nch = i8ie_sp24_chunks(c.C);
  a.in = pw_side(c.H, c.W, c.ib); a.os = pw_side(c.H, c.W, c.ob);
  a.a_xor = c.in_s8 ? 0u : 0x80808080u; a.o_xor = c.out_s8 ? 0x80808080u : 0u;
  a.B = c.B; a.b_bytes = (unsigned)i8ie_sp24_panel_bytes(c.N, c.C);
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  a.vec_out = (c.N % 4 == 0 && (reinterpret_cast<uintptr_t>(c.out) & 3u) == 0) ? 1 : 0;
  I8ieProfScope prof(ctx, a.M <= kSp24pwFewRows ? "sp24pw_mfma|few" : "sp24pw_mfma|many", 2.0 * a.M * c.N * c.C, algo_bytes(c));
  return c.ep.msv != nullptr ? spw_launch_rows<true>(ctx, a) : spw_launch_rows<false>(ctx, a);
}

int i8ie_sp24pw_direct_launch(i8ie_ctx* ctx, const I8ieSp24pwCall& c) {
  I8IE_REQUIRE(shape_ok(c), "sp24pw_direct: shape or layout");
  I8IE_REQUIRE(epilogue_ok(c), "sp24pw_direct: epilogue vectors (a conv's bias is in oc)");
  SpwDirectArgs a{};
  a.A = c.A; a.C = c.C; a.M = c.m * c.H * c.W; a.N = c.N; a.nch = i8ie_sp24_chunks(c.C);
  a.in_nchw = c.in_nchw; a.out_nchw = c.out_nchw;
  a.in = pw_side(c.H, c.W, c.ib); a.os = pw_side(c.H, c.W, c.ob);
  a.a_xor = c.in_s8 ? 0x80u : 0u; a.o_xor = c.out_s8 ? 0x80u : 0u;
  a.B = c.B;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)a.M * c.N;
  I8IE_REQUIRE(items < (1LL << 39), "sp24pw_direct: output too large");
  I8ieProfScope prof(ctx, "sp24pw_direct", 2.0 * a.M * c.N * c.C, algo_bytes(c));
  if (c.ep.msv != nullptr)
    sp24pw_direct_kernel<true><<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  else
    sp24pw_direct_kernel<false><<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_sp24pw_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in, int32_t* oc,
                               int32_t* wsum, int32_t* ocp) {
  I8ieProfScope prof(ctx, "sp24_offsets", 0.0, 0.5 * n * K);
  sp24pw_offsets_kernel<<<(n + 63) / 64, 64, 0, ctx->stream>>>(panel, qb, n, K, i8ie_sp24_chunks(K), s_in, zp_in, oc, wsum, ocp);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
