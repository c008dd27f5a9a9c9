// i8ie_w4glin.hip -- Linear with 4-bit weights and integer group scales along K (W4A8, group size gs = 64 / 128 / 256; DESIGN.md
// section 8za), not in the reference.
//
//   W_eff[j][k] = m[j][k / gs] * q[j][k]      q: nibbles in [-8, 7], m: u8 in [1, 32], so |W_eff| <= 256
//   C[r][j] = sum_k A_u8[r][k] * W_eff[j][k] + oc[j];  C += (int)(32 q_b / s_in);  out = relu?(down_scale_j(C))
//
// A grouped layer is the per-channel INT8 Linear on the integers W_eff: oc, the float bias step and the per-column requantiser
// (i8ie_epilogue.h, PC form) are those of i8ie_flin.hip.  Because m is an integer, C is an exact INT32 sum whatever the order
// of summation, and the kernel may cut K as it likes.  The nibbles lie in i8ie_w4lin.hip's panel, untouched: 1-KiB fragments
// [feature tile][chunk of 256 K][pair], lane (q, r) owning 16 bytes whose low nibbles are slot 8 p + q and whose high nibbles are
// slot 8 p + 4 + q of the chunk -- so the low-nibble MFMA of pair p covers K 128 p .. 128 p + 63 of the chunk and the
// high-nibble MFMA K 128 p + 64 .. 128 p + 127: each of a pair's two v_mfma_i32_16x16x64_i8 is 64 CONSECUTIVE K, and a group of
// 64, 128 or 256 is one MFMA, one pair or one chunk.
//
// w4glin_mfma keeps i8ie_w4lin.hip's stream: both operands by LDS-DMA in a ring of chunks with one barrier per chunk, the
// activations in swizzled 16-byte slots and re-biased by ^ 0x80 (128 * wsum_eff is in oc'), the MFMA fed (nibble << 4).  New is
// the accumulation.  A wave sums a group in a FRESH v4i from zero -- one MFMA (gs 64), the pair (gs 128), both pairs (gs 256;
// the few-row shape, whose wave pairs split the chunk, takes each pair as a half group with the same multiplier, which is the
// same integer) -- and then, per accumulator register, running += m * (group >> 4):
//   group    = 16 * sum over <= 256 K of (a - 128) * q:   |group| <= 16 * 256 * 128 * 8 = 2^22, an exact multiple of 16
//   group>>4 : |.| <= 2^18, fits the 24-bit multiply;  m * (group >> 4): |.| <= 2^23
//   running  : the sum over all K of (a - 128) * W_eff:   |.| <= 32768 * 128 * 256 = 2^30 for K <= 32768 (enforced at create)
//   C = running + oc' is the true sum, |C| <= 255 * 256 * 32768 < 2^31.  Every intermediate is exact in int32.
// A lane (q, r) of the accumulator tile holds features 4 q .. 4 q + 3 of row r, so it needs four multipliers per group: one dword
// of the [feature tile][group][16] array (i8ie_w4glin.h).  The block copies its feature tiles' whole multiplier columns into LDS
// once, ahead of the ring (FT * Gp * 16 bytes behind the stages: 16 KiB at gs 64, K 32768; 2.25 KiB for fc6 at gs 128); the read
// in the loop is one ds_read_b32 per group whose 64 lanes ask for four consecutive dwords (sixteen lanes each the same one: a
// broadcast, no bank conflict).
//   <1, 2, 2>  up to 16 rows: 4 waves, 8 stages of 8 KiB (64 KiB + multipliers: two blocks per CU), K split over wave pairs
//   <4, 2, 1>  any other row count: 8 waves, 64 rows x 32 features, 3 stages of 24 KiB (72 KiB + multipliers: two blocks per CU
//              while the multipliers take <= 8 KiB, one above -- K > 16384 at gs 64)
// w4glin_direct: the definition, one lane per output; K % 32 != 0, unaligned buffers, the force-fallback option and rows that
// are a flattened NHWC map (a K-permuted panel would scatter the groups).
#include <algorithm>

#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_w4glin.h"

namespace {

constexpr int kChunk = 256;          // K values per chunk: 256 activation bytes per row, 128 weight bytes per feature
constexpr int kMaxK = 32768;         // the int32 bound above
constexpr int kMaxMultLds = 16384;   // FT = 2 tiles * 512 groups * 16

struct W4gArgs {
  const uint8_t* A;  // [M][lda] u8
  size_t a_bytes;
  unsigned lda;
  int M, N, nch, Gp;
  const uint8_t* B;   // the panel: [ftiles][nch][2] fragments
  unsigned b_bytes;
  const uint8_t* Mg;  // the multipliers: [ftiles][Gp][16]
  I8ieEpiArgs ep;     // ocp = oc + 128 * wsum_eff (the activations enter re-biased by -128); ocp, biasf, msv, sbv: [Npad]
  uint8_t* out;
};

template <int RT, int FT, int KS, int STAGES>
struct W4gShape {
  static constexpr int kWaves = RT * FT * KS, kThreads = 64 * kWaves;
  static constexpr int kRows = RT * 16, kFeats = FT * 16;
  static constexpr int kPA = RT * 4, kPB = FT * 2;               // 1-KiB DMA pieces of a chunk: 4 activation rows / one fragment
  static constexpr int kPPW = (kPA + kPB + kWaves - 1) / kWaves;  // pieces per wave and chunk (every wave issues the same number)
  static constexpr int kStageA = kPA * 1024;
  static constexpr int kStage = kPPW * kWaves * 1024;            // (pieces past kPA + kPB land in the stage's padding)
  static constexpr int kRing = STAGES * kStage;                  // the multipliers lie behind it
  static_assert(KS == 1 || KS == 2, "a chunk has two pairs");
  static_assert(RT * FT * 1024 <= kStage, "the KS = 2 exchange reuses stage 0");
  static_assert(kRing + kMaxMultLds <= 160 * 1024, "LDS of a CU");
};

// running += m * (group >> 4) for the lane's four features; mw: their multipliers, feature 4 q + i in byte i
__device__ inline v4i w4g_fold(v4i run, v4i grp, unsigned mw) {
  run.x += __mul24(grp.x >> 4, (int)(mw & 255u));
  run.y += __mul24(grp.y >> 4, (int)((mw >> 8) & 255u));
  run.z += __mul24(grp.z >> 4, (int)((mw >> 16) & 255u));
  run.w += __mul24(grp.w >> 4, (int)(mw >> 24));
  return run;
}

template <int RT, int FT, int KS, int STAGES, int GS>
__global__ __launch_bounds__(64 * RT * FT * KS) void w4glin_mfma_kernel(W4gArgs p) {
  using S = W4gShape<RT, FT, KS, STAGES>;
  constexpr int kGPC = kChunk / GS;  // groups per chunk: 4, 2, 1
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const int wr = wave % RT, wf = (wave / RT) % FT, wk = wave / (RT * FT);  // this wave's row tile / feature tile / pair
  const int ft0 = blockIdx.x * FT, row0 = blockIdx.y * S::kRows;

  // ---- the block's multipliers: FT tiles' columns, contiguous in the array, into LDS behind the ring (16-byte copies; the
  //      array's tile count is even and FT = 2 divides it, so tile ft0 + FT - 1 exists)
  uint8_t* mlds = smem + S::kRing;
  {
    const uint4* msrc = reinterpret_cast<const uint4*>(p.Mg + (size_t)ft0 * p.Gp * 16);
    for (int i = tid; i < FT * p.Gp; i += S::kThreads) reinterpret_cast<uint4*>(mlds)[i] = msrc[i];
  }
  __syncthreads();  // (before the first DMA is issued: the ring's vmcnt counts below see only its own pieces)

  const size_t a_off = (size_t)row0 * p.lda;
  const size_t a_left = p.a_bytes - a_off;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A + a_off), 0,
                                                                       (unsigned)(a_left < 0xFFFFF000u ? a_left : 0xFFFFF000u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a chunk, as in i8ie_w4lin.hip: kPA of A (4 rows each; lane l: row 4 pi + (l >> 4), LDS slot l & 15, source
  //      slot (l & 15) ^ (row & 15)), kPB of B (fragment (ft, pair) as it lies), the rest padding; wave w issues pieces w,
  //      w + kWaves, ...  A chunk past K reads the next row's bytes or, past the buffer, zeros: the panel holds zeros there.
  const int nch = p.nch;
  const int rot = (int)(blockIdx.x % (unsigned)nch);
  unsigned src[S::kPPW], step_bytes[S::kPPW];
#pragma unroll
  for (int j = 0; j < S::kPPW; ++j) {
    const int pi = wave + S::kWaves * j;
    if (pi < S::kPA) {
      const int row = 4 * pi + (lane >> 4);
      src[j] = (unsigned)row * p.lda + (unsigned)(((lane & 15) ^ (row & 15)) * 16);
      step_bytes[j] = kChunk;
    } else {
      const int f = (pi - S::kPA) % S::kPB;  // (padding pieces: a second copy of a B piece, unused)
      src[j] = (unsigned)((ft0 + f / 2) * nch * 2 + (f & 1)) * 1024u + (unsigned)lane * 16u;
      step_bytes[j] = 2048;
    }
  }
  auto issue = [&](int step) {  // the chunk of walk position `step` -> stage step % STAGES
    int ch = step + rot;
    while (ch >= nch) ch -= nch;
    uint8_t* st = smem + (step % STAGES) * S::kStage;
#pragma unroll
    for (int j = 0; j < S::kPPW; ++j) {
      const int pi = wave + S::kWaves * j;
      if (pi < S::kPA)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16,
                                                 (int)(src[j] + (unsigned)ch * step_bytes[j]), 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16,
                                                 (int)(src[j] + (unsigned)ch * step_bytes[j]), 0, 0, 0);
    }
  };

  v4i run = {0, 0, 0, 0};
  const v4i zero = {0, 0, 0, 0};
  const int arow = (wr * 16 + lr) * kChunk;                 // row 16 wr + r of a stage; slot s of it at (s ^ r) * 16
  const int bfrag = S::kStageA + wf * 2048 + lane * 16;     // fragment (wf, pair 0) of a stage, this lane's 16 bytes
  const uint8_t* mcol = mlds + wf * p.Gp * 16 + 4 * lq;     // this lane's dword of group g of its tile: mcol + 16 g
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i) issue(nch > i ? i : 0);
  int ch = rot;  // the chunk of this step (the walk starts at `rot`: the order does not matter to an integer sum)
  for (int step = 0; step < nch; ++step) {
    // my pieces of this chunk (the STAGES - 2 chunks after it may be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * S::kPPW) : "memory");
    asm volatile("s_barrier" ::: "memory");  // everyone's pieces; everyone is done with the previous chunk
    issue(step + STAGES - 1);  // -> the stage of the previous chunk (past the end the walk wraps: keeps the vmcnt counts uniform)
    const uint8_t* st = smem + (step % STAGES) * S::kStage;
    const uint8_t* mch = mcol + ch * (kGPC * 16);           // group kGPC * ch
    v4i grp = zero;                                          // (gs 256, one wave per chunk: both pairs)
#pragma unroll
    for (int pr = (KS == 2 ? wk : 0); pr < 2; pr += KS) {
      const v4i x = *reinterpret_cast<const v4i*>(st + bfrag + pr * 1024);                              // 32 nibbles
      const v4i a_lo = *reinterpret_cast<const v4i*>(st + arow + ((8 * pr + lq) ^ lr) * 16) ^ (int)0x80808080;      // u8 -> s8
      const v4i a_hi = *reinterpret_cast<const v4i*>(st + arow + ((8 * pr + 4 + lq) ^ lr) * 16) ^ (int)0x80808080;  // (128 * wsum_eff is in ocp)
      const v4i b_lo = (x << 4) & (int)0xF0F0F0F0, b_hi = x & (int)0xF0F0F0F0;                         // nibble << 4 as s8
      if constexpr (GS == 64) {  // K 128 pr .. + 63 is group 4 ch + 2 pr, K 128 pr + 64 .. + 127 the next
        const v4i g0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_lo, a_lo, zero, 0, 0, 0);
        const v4i g1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_hi, a_hi, zero, 0, 0, 0);
        run = w4g_fold(run, g0, *reinterpret_cast<const unsigned*>(mch + (2 * pr) * 16));
        run = w4g_fold(run, g1, *reinterpret_cast<const unsigned*>(mch + (2 * pr + 1) * 16));
      } else if constexpr (GS == 128 || KS == 2) {  // the pair is group 2 ch + pr (gs 128) or half of group ch (gs 256)
        v4i g = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_lo, a_lo, zero, 0, 0, 0);
        g = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_hi, a_hi, g, 0, 0, 0);
        run = w4g_fold(run, g, *reinterpret_cast<const unsigned*>(mch + (GS == 128 ? pr : 0) * 16));
      } else {
        grp = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_lo, a_lo, grp, 0, 0, 0);
        grp = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_hi, a_hi, grp, 0, 0, 0);
      }
    }
    if constexpr (GS == 256 && KS == 1) run = w4g_fold(run, grp, *reinterpret_cast<const unsigned*>(mch));
    if (++ch == nch) ch = 0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wrapped pieces: nothing may land after the block is gone)

  if constexpr (KS == 2) {  // the two pairs' partial tiles: pair 1 hands its to pair 0 through stage 0
    asm volatile("s_barrier" ::: "memory");  // everyone has landed and is done reading the stages
    v4i* xch = reinterpret_cast<v4i*>(smem) + (wr + RT * wf) * 64 + lane;
    if (wk == 1) *xch = run;
    __syncthreads();
    if (wk == 1) return;
    run += *xch;
  }

  // ---- epilogue of src/fully_connected.cc:42-48: lane (q, r) holds features 4 q .. 4 q + 3 of row 16 wr + r
  const int row = row0 + wr * 16 + lr, n = (ft0 + wf) * 16 + 4 * lq;
  if (row < p.M && n < p.N) {
    int cv[4] = {run.x, run.y, run.z, run.w};
    const int nf = p.N - n < 4 ? p.N - n : 4;
    // (n < N <= Npad, n % 4 == 0: the quad lies inside the padded arrays)
    i8ie_epi_finish<true>(p.ep, cv, i8ie_epi_cols_vec<true>(p.ep, n), nf, (long long)row * p.N + n, p.out + (size_t)row * p.N + n,
                          nf == 4 && (p.N & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 3u) == 0, [&](int (&c)[4]) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                              if (r < nf) c[r] = (int)((float)c[r] + p.ep.biasf[n + r]);
                          });
  }
}

// W_eff[j][k] from panel and multipliers (k: the weight's own in_features index)
__device__ inline int w4g_weight(const uint8_t* B, const uint8_t* Mg, int j, int k, int nch, int Gp, int gshift) {
  return i8ie_w4_get(B, j, k, nch) * (int)Mg[i8ie_w4g_mult_at(j, k >> gshift, Gp)];
}

// ---- w4glin_direct: the definition.  One lane per output (row, j): the sum over k in the caller's K order (c, hw: rows that are
// a flattened NHWC activation walk k' = pix * c + ch against weight k = ch * hw + pix, whose group is k / gs) ----
struct W4gDirectArgs {
  const uint8_t* A;
  int M, N, K, nch, Gp, gshift, c, hw;
  const uint8_t* B;
  const uint8_t* Mg;
  I8ieEpiArgs ep;  // ocp here: the plain oc (the activations enter as they are)
  uint8_t* out;
};

__global__ __launch_bounds__(256) void w4glin_direct_kernel(W4gDirectArgs p) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.M * p.N) return;
  const int row = (int)(item / p.N), j = (int)(item - (long long)row * p.N);
  const uint8_t* a = p.A + (size_t)row * p.K;
  int sum = 0;
  for (int kq = 0; kq < p.K; ++kq) {
    int k = kq;
    if (p.hw > 1) {
      const int pix = kq / p.c;
      k = (kq - pix * p.c) * p.hw + pix;
    }
    sum += (int)a[kq] * w4g_weight(p.B, p.Mg, j, k, p.nch, p.Gp, p.gshift);
  }
  int cv[4] = {sum, 0, 0, 0};
  i8ie_epi_finish<true>(p.ep, cv, i8ie_epi_cols<true>(p.ep, j, 1), 1, item, p.out + item, false, [&](int (&c)[4]) {
    c[0] = (int)((float)c[0] + p.ep.biasf[j]);
  });
}

// ---- w4g_offsets: src/fully_connected.cc:30-38 on W_eff.  One thread per feature replays the reference's sequential fp32
// accumulation (k ascending; zp_in * W_eff is an exact integer below 2^16); also the exact row sum, oc' and the float bias of the
// bias integer 32 q_b ----
__global__ __launch_bounds__(64) void w4g_offsets_kernel(const uint8_t* __restrict__ B, const uint8_t* __restrict__ Mg,
                                                         const int8_t* __restrict__ qb, int n, int K, int nch, int Gp, int gshift,
                                                         float s_in, int zp_in, int32_t* __restrict__ oc, int32_t* __restrict__ wsum,
                                                         int32_t* __restrict__ ocp, float* __restrict__ biasf) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  float t = 0.0f;
  int s = 0;
  for (int k = 0; k < K; ++k) {
    const int w = w4g_weight(B, Mg, j, k, nch, Gp, gshift);
    t = t + (float)(zp_in * w);
    s += w;
  }
  oc[j] = (int)(-t);
  wsum[j] = s;
  ocp[j] = oc[j] + 128 * s;
  biasf[j] = (float)(32 * (int)qb[j]) / s_in;
}

template <int RT, int FT, int KS, int STAGES, int GS>
int w4g_launch_t(i8ie_ctx* ctx, const W4gArgs& a) {
  using S = W4gShape<RT, FT, KS, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4glin_mfma_kernel<RT, FT, KS, STAGES, GS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kRing + kMaxMultLds));
    raised[dev] = true;
  }
  const int lds = S::kRing + (FT * a.Gp * 16 + 1023) / 1024 * 1024;
  const dim3 grid((unsigned)((a.N + S::kFeats - 1) / S::kFeats), (unsigned)((a.M + S::kRows - 1) / S::kRows));
  w4glin_mfma_kernel<RT, FT, KS, STAGES, GS><<<grid, S::kThreads, lds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

template <int GS>
int w4g_launch_gs(i8ie_ctx* ctx, const W4gArgs& a) {
  if (a.M <= 16) return w4g_launch_t<1, 2, 2, 8, GS>(ctx, a);
  return w4g_launch_t<4, 2, 1, 3, GS>(ctx, a);
}

int w4g_shift(int gs) { return gs == 64 ? 6 : (gs == 128 ? 7 : 8); }

}  // namespace

void i8ie_w4g_pack_mult(const uint8_t* m_host, int n, int K, int gs, uint8_t* out) {
  const int G = i8ie_w4g_groups(K, gs), Gp = i8ie_w4g_padded_groups(K, gs);
  std::fill(out, out + i8ie_w4g_mult_bytes(n, K, gs), (uint8_t)1);
  for (int j = 0; j < n; ++j)
    for (int g = 0; g < G; ++g) out[i8ie_w4g_mult_at(j, g, Gp)] = m_host[(size_t)j * G + g];
}

bool i8ie_w4glin_mfma_takes(const I8ieW4gCall& c) {
  return c.K % 32 == 0 && c.hw <= 1 && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 && (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0 &&
         (reinterpret_cast<uintptr_t>(c.Mg) & 15u) == 0;
}

int i8ie_w4glin_mfma_launch(i8ie_ctx* ctx, const I8ieW4gCall& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= kMaxK && i8ie_w4g_size_ok(c.gs) && i8ie_w4glin_mfma_takes(c),
               "w4glin_mfma: shape, group size or alignment");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf != nullptr, "w4glin_mfma: a grouped layer is per-feature");
  const size_t b_bytes = i8ie_w4_panel_bytes(c.N, c.K);
  I8IE_REQUIRE(b_bytes < ((size_t)1 << 32) - 4096, "w4glin_mfma: panel offsets exceed 32 bits");
  W4gArgs a{};
  a.A = c.A; a.a_bytes = (size_t)c.M * c.K; a.lda = (unsigned)c.K; a.M = c.M; a.N = c.N; a.nch = i8ie_w4_chunks(c.K);
  a.Gp = i8ie_w4g_padded_groups(c.K, c.gs);
  a.B = c.B; a.b_bytes = (unsigned)b_bytes; a.Mg = c.Mg;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  // the nibbles and one multiplier byte per group once from HBM; every row block reads its rows' activations once per feature block
  I8ieProfScope prof(ctx, "w4glin_mfma", 2.0 * c.M * c.N * c.K,
                     (double)c.M * c.K + (0.5 + 1.0 / c.gs) * c.N * c.K + (double)c.M * c.N);
  if (c.gs == 64) return w4g_launch_gs<64>(ctx, a);
  if (c.gs == 128) return w4g_launch_gs<128>(ctx, a);
  return w4g_launch_gs<256>(ctx, a);
}

int i8ie_w4glin_direct_launch(i8ie_ctx* ctx, const I8ieW4gCall& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= kMaxK && i8ie_w4g_size_ok(c.gs), "w4glin_direct: shape or group size");
  I8IE_REQUIRE(c.hw >= 1 && c.K % c.hw == 0, "w4glin_direct: in_features is not c * h * w");
  I8IE_REQUIRE((long long)c.M * c.N < (1LL << 39), "w4glin_direct: output too large");
  W4gDirectArgs a{};
  a.A = c.A; a.M = c.M; a.N = c.N; a.K = c.K; a.nch = i8ie_w4_chunks(c.K); a.c = c.K / c.hw; a.hw = c.hw;
  a.Gp = i8ie_w4g_padded_groups(c.K, c.gs); a.gshift = w4g_shift(c.gs);
  a.B = c.B; a.Mg = c.Mg;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)c.M * c.N;
  I8ieProfScope prof(ctx, "w4glin_direct", 2.0 * c.M * c.N * c.K,
                     (double)c.M * c.K + (0.5 + 1.0 / c.gs) * c.N * c.K + (double)c.M * c.N);
  w4glin_direct_kernel<<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_w4g_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const uint8_t* mg, const int8_t* qb, int n, int K, int gs, float s_in,
                            int zp_in, int32_t* oc, int32_t* wsum, int32_t* ocp, float* biasf) {
  I8ieProfScope prof(ctx, "w4g_offsets", 0.0, (0.5 + 1.0 / gs) * n * K);
  w4g_offsets_kernel<<<(n + 63) / 64, 64, 0, ctx->stream>>>(panel, mg, qb, n, K, i8ie_w4_chunks(K), i8ie_w4g_padded_groups(K, gs),
                                                            w4g_shift(gs), s_in, zp_in, oc, wsum, ocp, biasf);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
