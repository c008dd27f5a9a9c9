// i8ie_w4lin.hip -- Linear with 4-bit weights and 8-bit activations (W4A8), not in the reference.
//
//   C[r][j] = sum_k A_u8[r][k] * W_s4[j][k] + oc[j];  C += (int)bias;  out = relu?(down_scale_j(C))
//
// A 4-bit layer is a per-channel INT8 layer whose weight integers lie in [-8, 7]: oc, the float bias step and the per-column
// requantiser (i8ie_epilogue.h, PC form) are those of i8ie_flin.hip.  What is new is that the weights stay nibbles from HBM
// through LDS into the registers, half the bytes of the INT8 stream that bounds fc6 / fc7 at few rows.
//
// The panel (w4_at below).  K is cut into chunks of 256, a chunk into sixteen 16-value slots, the features into tiles of 16.
// One FRAGMENT is 1 KiB: lane (q, r) = 16 q + r of a wave owns 16 bytes of it, and byte i holds
//     low nibble   W[16 ft + r][256 ch + 16 (8 p + q) + i]          p = 0, 1: the fragment's pair of the chunk
//     high nibble  W[16 ft + r][256 ch + 16 (8 p + 4 + q) + i]
// so ONE 16-byte read is the lane's B operand of TWO v_mfma_i32_16x16x64_i8: slots 8 p + q (low) and 8 p + 4 + q (high) are
// exactly the slots lane q feeds to MFMAs 2 p and 2 p + 1 of the chunk in i8ie_flin.hip's walk, so the activations are read
// as that kernel reads them, with no byte shuffle.  Fragments lie as [feature tile][chunk][pair]: a wave's read of one is a
// contiguous KiB in HBM (one LDS-DMA instruction) and a conflict-free ds_read_b128 in LDS (lane l at 16 l).
//
// Nibble -> s8 without a sign extension: the MFMA gets (nibble << 4) as its s8 operand -- x & 0xF0F0F0F0 for the high
// nibbles, (x << 4) & 0xF0F0F0F0 for the low ones, two vector operations per four weights -- and the accumulator is exactly
// 16 C; one arithmetic shift by 4 before the epilogue.  |16 C| <= K * 128 * 128 stays inside int32 for K <= 131071; the
// create entry enforces K <= 65536.
//
// w4lin_mfma: a block owns 16 FT features, 16 RT rows and all of K; wave (rt, ft, ks) owns one 16 x 16 output tile and, with
// KS = 2, one of the chunk's two pairs (the two partial tiles meet in LDS at the end).  Both operands arrive by LDS-DMA in a
// ring of STAGES chunks, one barrier per chunk (i8ie_flin.hip's ring; the activations keep its 16-byte-slot swizzle).
//   <1, 2, 2>  up to 16 rows: 4 waves, 8 KiB per chunk of which 4 are weights, 8 stages (64 KiB: two blocks per CU) -- the
//              launch is a stream over the nibbles and wants bytes in flight, not MFMA rate
//   <4, 2, 1>  any other row count: 8 waves, 64 rows x 32 features, 24 KiB per chunk, 3 stages, row blocks over grid.y
// w4lin_direct: the definition, one lane per output; K % 32 != 0, unaligned buffers and the force-fallback option.
#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_w4lin.h"

namespace {

constexpr int kChunk = 256;  // K values per chunk: 256 activation bytes per row, 128 weight bytes per feature

struct W4Args {
  const uint8_t* A;  // [M][lda] u8
  size_t a_bytes;
  unsigned lda;
  int M, N, nch;
  const uint8_t* B;  // the panel: [ftiles][nch][2] fragments
  unsigned b_bytes;
  I8ieEpiArgs ep;    // ocp = oc + 128 * wsum (the activations enter re-biased by -128); ocp, biasf, msv, sbv: [Npad]
  uint8_t* out;
};

template <int RT, int FT, int KS, int STAGES>
struct W4Shape {
  static constexpr int kWaves = RT * FT * KS, kThreads = 64 * kWaves;
  static constexpr int kRows = RT * 16, kFeats = FT * 16;
  static constexpr int kPA = RT * 4, kPB = FT * 2;               // 1-KiB DMA pieces of a chunk: 4 activation rows / one fragment
  static constexpr int kPPW = (kPA + kPB + kWaves - 1) / kWaves;  // pieces per wave and chunk (every wave issues the same number)
  static constexpr int kStageA = kPA * 1024;
  static constexpr int kStage = kPPW * kWaves * 1024;            // (pieces past kPA + kPB land in the stage's padding)
  static constexpr int kLds = STAGES * kStage;
  static_assert(KS == 1 || KS == 2, "a chunk has two pairs");
  static_assert(RT * FT * 1024 <= kStage, "the KS = 2 exchange reuses stage 0");
};

template <int RT, int FT, int KS, int STAGES>
__global__ __launch_bounds__(64 * RT * FT * KS) void w4lin_mfma_kernel(W4Args p) {
  using S = W4Shape<RT, FT, KS, STAGES>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const int wr = wave % RT, wf = (wave / RT) % FT, wk = wave / (RT * FT);  // this wave's row tile / feature tile / pair
  const int ft0 = blockIdx.x * FT, row0 = blockIdx.y * S::kRows;

  const size_t a_off = (size_t)row0 * p.lda;
  const size_t a_left = p.a_bytes - a_off;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A + a_off), 0,
                                                                       (unsigned)(a_left < 0xFFFFF000u ? a_left : 0xFFFFF000u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a chunk: kPA of A (4 rows each; lane l: row 4 pi + (l >> 4), LDS slot l & 15, source slot
  //      (l & 15) ^ (row & 15)), kPB of B (fragment (ft, pair) as it lies), the rest padding; wave w issues pieces w, w + kWaves, ...
  //      A chunk past K (K % 256 != 0) reads the next row's bytes or, past the buffer, zeros: the panel holds zeros there.
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

  v4i acc = {0, 0, 0, 0};
  const int arow = (wr * 16 + lr) * kChunk;                 // row 16 wr + r of a stage; slot s of it at (s ^ r) * 16
  const int bfrag = S::kStageA + wf * 2048 + lane * 16;     // fragment (wf, pair 0) of a stage, this lane's 16 bytes
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i) issue(nch > i ? i : 0);
  for (int step = 0; step < nch; ++step) {
    // my pieces of this chunk (the STAGES - 2 chunks after it may be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * S::kPPW) : "memory");
    asm volatile("s_barrier" ::: "memory");  // everyone's pieces; everyone is done with the previous chunk
    issue(step + STAGES - 1);  // -> the stage of the previous chunk (past the end the walk wraps: keeps the vmcnt counts uniform)
    const uint8_t* st = smem + (step % STAGES) * S::kStage;
#pragma unroll
    for (int pr = (KS == 2 ? wk : 0); pr < 2; pr += KS) {
      const v4i x = *reinterpret_cast<const v4i*>(st + bfrag + pr * 1024);                              // 32 nibbles
      const v4i a_lo = *reinterpret_cast<const v4i*>(st + arow + ((8 * pr + lq) ^ lr) * 16) ^ (int)0x80808080;      // u8 -> s8
      const v4i a_hi = *reinterpret_cast<const v4i*>(st + arow + ((8 * pr + 4 + lq) ^ lr) * 16) ^ (int)0x80808080;  // (128 * wsum is in ocp)
      const v4i b_lo = (x << 4) & (int)0xF0F0F0F0, b_hi = x & (int)0xF0F0F0F0;                         // nibble << 4 as s8
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_lo, a_lo, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_hi, a_hi, acc, 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wrapped pieces: nothing may land after the block is gone)

  if constexpr (KS == 2) {  // the two pairs' partial tiles: pair 1 hands its to pair 0 through stage 0
    asm volatile("s_barrier" ::: "memory");  // everyone has landed and is done reading the stages
    v4i* xch = reinterpret_cast<v4i*>(smem) + (wr + RT * wf) * 64 + lane;
    if (wk == 1) *xch = acc;
    __syncthreads();
    if (wk == 1) return;
    acc += *xch;
  }

  // ---- epilogue of src/fully_connected.cc:42-48: lane (q, r) holds 16 C of features 4 q .. 4 q + 3 of row 16 wr + r
  const int row = row0 + wr * 16 + lr, n = (ft0 + wf) * 16 + 4 * lq;
  if (row < p.M && n < p.N) {
    int cv[4] = {acc.x >> 4, acc.y >> 4, acc.z >> 4, acc.w >> 4};
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

// ---- w4lin_direct: the definition.  One lane per output (row, j): the sum over k in the caller's K order, the nibble looked up
// in the panel (c, hw: rows that are a flattened NHWC activation walk k' = pix * c + ch against weight k = ch * hw + pix) ----
struct W4DirectArgs {
  const uint8_t* A;
  int M, N, K, nch, c, hw;
  const uint8_t* B;
  I8ieEpiArgs ep;  // ocp here: the plain oc (the activations enter as they are)
  uint8_t* out;
};

__global__ __launch_bounds__(256) void w4lin_direct_kernel(W4DirectArgs p) {
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
    sum += (int)a[kq] * i8ie_w4_get(p.B, j, k, p.nch);
  }
  int cv[4] = {sum, 0, 0, 0};
  i8ie_epi_finish<true>(p.ep, cv, i8ie_epi_cols<true>(p.ep, j, 1), 1, item, p.out + item, false, [&](int (&c)[4]) {
    c[0] = (int)((float)c[0] + p.ep.biasf[j]);
  });
}

// ---- one-off kernels of a handle --------------------------------------------------------------------------------------------
// src/fully_connected.cc:30-38 from the nibbles: one thread per feature replays the reference's sequential fp32 accumulation
// (k ascending), as offsets_kernel of i8ie_gemm.hip does from bytes; also the exact row sum, oc' and the float bias.  cpad > 0:
// the panel of a k x k conv (i8ie_w4conv.h) -- reference weight k = (c, tap) lies at position tap * cpad + c
__global__ __launch_bounds__(64) void w4_offsets_kernel(const uint8_t* __restrict__ B, const int8_t* __restrict__ qb, int n, int K,
                                                        int nch, float s_in, int zp_in, int32_t* __restrict__ oc,
                                                        int32_t* __restrict__ wsum, int32_t* __restrict__ ocp,
                                                        float* __restrict__ biasf, int conv, int taps, int cpad) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  float t = 0.0f;
  int s = 0;
  for (int k = 0, c = 0, tap = 0; k < K; ++k) {
    const int q = i8ie_w4_get(B, j, cpad > 0 ? tap * cpad + c : k, nch);
    t = t + (float)(zp_in * q);
    s += q;
    if (++tap == taps) {
      tap = 0;
      ++c;
    }
  }
  oc[j] = conv ? (int)((float)qb[j] / s_in - t) : (int)(-t);  // src/conv2d.cc:123 / src/fully_connected.cc:37
  wsum[j] = s;
  ocp[j] = oc[j] + 128 * s;
  biasf[j] = conv ? 0.0f : (float)qb[j] / s_in;
}

// the panel with K reordered (h, w, c): weight k = ch * hw + pix goes where k' = pix * c + ch lies.  One thread per byte of
// the new panel (two nibbles); bytes past K and feature rows past n stay zero.
__global__ __launch_bounds__(256) void w4_permute_kernel(const uint8_t* __restrict__ B, uint8_t* __restrict__ Bp, size_t bytes,
                                                         int n, int K, int nch, int c, int hw) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= bytes) return;
  const int i = (int)(e & 15), r = (int)((e >> 4) & 15), q = (int)((e >> 8) & 3), pr = (int)((e >> 10) & 1);
  const size_t fc = e >> 11;
  const int ch = (int)(fc % (unsigned)nch), j = (int)(fc / (unsigned)nch) * 16 + r;
  unsigned v = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kq = ch * kChunk + 16 * (8 * pr + 4 * h + q) + i;
    if (j < n && kq < K) {
      const int pix = kq / c;
      v |= (unsigned)(i8ie_w4_get(B, j, (kq - pix * c) * hw + pix, nch) & 15) << (4 * h);
    }
  }
  Bp[e] = (uint8_t)v;
}

template <int RT, int FT, int KS, int STAGES>
int w4_launch_t(i8ie_ctx* ctx, const W4Args& a) {
  using S = W4Shape<RT, FT, KS, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4lin_mfma_kernel<RT, FT, KS, STAGES>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kLds));
    raised[dev] = true;
  }
  const dim3 grid((unsigned)((a.N + S::kFeats - 1) / S::kFeats), (unsigned)((a.M + S::kRows - 1) / S::kRows));
  w4lin_mfma_kernel<RT, FT, KS, STAGES><<<grid, S::kThreads, S::kLds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // namespace

size_t i8ie_w4_panel_bytes(int n, int K) { return (size_t)i8ie_w4_ftiles(n) * i8ie_w4_chunks(K) * 2048; }

void i8ie_w4_pack_panel(const uint8_t* packed, int n, int K, uint8_t* panel) {
  const int nch = i8ie_w4_chunks(K);
  const size_t pitch = ((size_t)K + 1) / 2;
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < K; ++k) {
      const unsigned v = (packed[j * pitch + k / 2] >> (4 * (k & 1))) & 15u;
      int hi;
      const size_t at = i8ie_w4_at(j, k, nch, &hi);
      panel[at] = (uint8_t)(panel[at] | (v << (4 * hi)));
    }
}

bool i8ie_w4lin_mfma_takes(const I8ieW4Call& c) {
  return c.K % 32 == 0 && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 && (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0;
}

int i8ie_w4lin_mfma_launch(i8ie_ctx* ctx, const I8ieW4Call& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= 65536 && i8ie_w4lin_mfma_takes(c), "w4lin_mfma: shape or alignment");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf != nullptr, "w4lin_mfma: a 4-bit layer is per-feature");
  const size_t b_bytes = i8ie_w4_panel_bytes(c.N, c.K);
  I8IE_REQUIRE(b_bytes < ((size_t)1 << 32) - 4096, "w4lin_mfma: panel offsets exceed 32 bits");
  W4Args a{};
  a.A = c.A; a.a_bytes = (size_t)c.M * c.K; a.lda = (unsigned)c.K; a.M = c.M; a.N = c.N; a.nch = i8ie_w4_chunks(c.K);
  a.B = c.B; a.b_bytes = (unsigned)b_bytes;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  // the nibbles once from HBM; every row block reads its rows' activations once per feature block
  I8ieProfScope prof(ctx, "w4lin_mfma", 2.0 * c.M * c.N * c.K, (double)c.M * c.K + 0.5 * c.N * c.K + (double)c.M * c.N);
  if (c.M <= 16) return w4_launch_t<1, 2, 2, 8>(ctx, a);
  return w4_launch_t<4, 2, 1, 3>(ctx, a);  // (72 KB of LDS: two blocks per CU)
}

int i8ie_w4lin_direct_launch(i8ie_ctx* ctx, const I8ieW4Call& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= 65536, "w4lin_direct: shape");
  I8IE_REQUIRE(c.hw >= 1 && c.K % c.hw == 0, "w4lin_direct: in_features is not c * h * w");
  I8IE_REQUIRE((long long)c.M * c.N < (1LL << 39), "w4lin_direct: output too large");
  W4DirectArgs a{};
  a.A = c.A; a.M = c.M; a.N = c.N; a.K = c.K; a.nch = i8ie_w4_chunks(c.K); a.c = c.K / c.hw; a.hw = c.hw;
  a.B = c.B;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)c.M * c.N;
  I8ieProfScope prof(ctx, "w4lin_direct", 2.0 * c.M * c.N * c.K, (double)c.M * c.K + 0.5 * c.N * c.K + (double)c.M * c.N);
  w4lin_direct_kernel<<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_w4_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in,
                           int32_t* oc, int32_t* wsum, int32_t* ocp, float* biasf, bool conv, int taps, int cpad) {
  I8ieProfScope prof(ctx, "w4_offsets", 0.0, 0.5 * n * K);
  w4_offsets_kernel<<<(n + 63) / 64, 64, 0, ctx->stream>>>(panel, qb, n, K, i8ie_w4_chunks(cpad > 0 ? taps * cpad : K), s_in, zp_in,
                                                           oc, wsum, ocp, biasf, conv ? 1 : 0, taps, cpad);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_w4_launch_permute(i8ie_ctx* ctx, const uint8_t* panel, uint8_t* out, int n, int K, int c, int hw) {
  const size_t bytes = i8ie_w4_panel_bytes(n, K);
  I8ieProfScope prof(ctx, "w4_permute_k", 0.0, 2.0 * bytes);
  w4_permute_kernel<<<(unsigned)((bytes + 255) / 256), 256, 0, ctx->stream>>>(panel, out, bytes, n, K, i8ie_w4_chunks(K), c, hw);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
