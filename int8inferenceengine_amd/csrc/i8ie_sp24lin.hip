// i8ie_sp24lin.hip -- Linear with 2:4 structured-sparse 8-bit weights on the sparse INT8 MFMA, not in the
// reference.
//
//   C[r][j] = sum_k A_u8[r][k] * W_s8[j][k] + oc[j];  C += (int)bias;  out = relu?(down_scale(C))
//
// A 2:4 layer is an INT8 layer whose weight integers have at most two non-zeros in every aligned group k = 4 g .. 4 g + 3: oc,
// the float bias step and the requantiser (i8ie_epilogue.h, both forms) are those of i8ie_flin.hip.  What is new is that only
// the two kept values of a group and their 2-bit positions travel from HBM through LDS into the registers (0.625 of the dense
// bytes) and that one v_smfmac_i32_16x16x128_i8 covers 128 dense K.
//
// The instruction's pairing, measured with one-hot operands on an MI355X (acc = smfmac(a: v4i, b: v8i, acc, idx); lane (q, r) =
// 16 q + r; K is the instruction's 128 dense values):
//   a   compressed bytes 2 g, 2 g + 1 of lane (q, r) are the two kept values of row r's group K = 32 q + 4 g .. 32 q + 4 g + 3
//       (g = 0 .. 7): a lane's sixteen bytes are the compressed form of 32 consecutive dense K
//   idx bits 4 g + 1 : 4 g are the position (0 .. 3) inside that group of byte 2 g, bits 4 g + 3 : 4 g + 2 that of byte 2 g + 1
//   b   byte i of lane (q, c) is column c's dense K = 16 q + i for i < 16 and K = 64 + 16 q + (i - 16) for i >= 16: two stacked
//       16x16x64 operands -- NOT the 32 consecutive K of the a lane with the same q.  Compressed byte c of a lane (q, r) thus
//       selects among the bytes 16 (q >> 1) + 4 ((c & 7) >> 1) .. + 3 of the b lane 2 (q & 1) + (c >> 3)
//   acc lane (q, c) holds rows 4 q .. 4 q + 3 of column c, as the dense 16x16 instructions do
// With the weights as `a` the compressed rows of the C-ABI (values [n][K / 2], one position nibble per group, group 2 i in the low
// nibble of byte i) are what a lane wants as they lie: sixteen consecutive value bytes, and four consecutive position bytes as
// one little-endian dword.
//
// The panel (i8ie_sp24_value_at / i8ie_sp24_index_at).  K is cut into chunks of 512 dense values, a chunk into four steps of 128
// (one instruction each), the features into tiles of 16.  A chunk of a tile is five FRAGMENTS of 1 KiB:
//     fragment v = 0 .. 3   lane (q, r) owns 16 bytes: the kept values of W[16 ft + r][512 ch + 128 v + 32 q .. + 31]
//     fragment 4            lane (q, r) owns 16 bytes: dword v is that lane's idx operand of step v
// so the positions of four steps ride in one 16-byte-per-lane piece, like a values fragment.  Fragments lie as
// [feature tile][chunk][5]: a wave's read of one is a contiguous KiB in HBM (one LDS-DMA instruction) and a conflict-free
// ds_read_b128 in LDS (lane l at 16 l).  The panel is zero past n and past K (value 0 at position 0 adds nothing).
//
// The activations: a stage holds 512 bytes per row as 32 slots of 16 bytes, slot s of row r at (s ^ (r & 15)) * 16 -- i8ie_flin.hip's
// swizzle on a longer row; lane (q, r) reads slots 8 v + q and 8 v + 4 + q of its row for step v, exactly the b layout above,
// XORs them with 0x80 (u8 -> s8; 128 * wsum is in ocp) and has its v8i.
//
// sp24lin_mfma: a block owns 16 WF BF features, 16 WR BR rows and all of K; a wave owns WR x WF output tiles of 16 x 16 and, with
// KS = 4, one of a chunk's four steps (the partial tiles meet in LDS at the end).  Both operands arrive by LDS-DMA in a ring of
// STAGES chunks, one barrier per chunk.
//   <1, 1, 1, 1, 4, 8>  up to 16 rows: 4 waves, 16 features, 5 KiB of weights per chunk, 8 stages of 16 KiB -- a stream over the
//                       panel that wants bytes in flight and many blocks (n / 16), not MFMA rate
//   <2, 1, 2, 2, 1, 3>  up to 128 rows: 4 waves, 64 rows x 32 features, 3 stages of 44 KiB
//   <2, 2, 2, 4, 1, 2>  more rows: 8 waves with 32 x 32 wave tiles, 64 rows x 128 features, 2 stages of 72 KiB: a row block
//                       reads its activations once per 128 features
// sp24lin_direct: the definition, one lane per output; every other K, unaligned buffers, rows in (h, w, c) order, force-fallback.
#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_sp24lin.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kChunk = 512;  // dense K values per chunk: 512 activation bytes per row, 256 + 64 panel bytes per feature

struct Sp24Args {
  const uint8_t* A;  // [M][lda] u8
  size_t a_bytes;
  unsigned lda;
  int M, N, nch;
  const uint8_t* B;  // the panel: [ftiles][nch][5] fragments
  unsigned b_bytes;
  I8ieEpiArgs ep;    // ocp = oc + 128 * wsum (the activations enter re-biased by -128); ocp, biasf, msv, sbv: [Npad]
  uint8_t* out;
};

template <int WR, int WF, int BR, int BF, int KS, int STAGES>
struct Sp24Shape {
  static constexpr int kWaves = BR * BF * KS, kThreads = 64 * kWaves;
  static constexpr int kRows = 16 * WR * BR, kFeats = 16 * WF * BF, kTiles = WR * WF;
  static constexpr int kPA = kRows / 2, kPB = 5 * WF * BF;       // 1-KiB DMA pieces of a chunk: 2 activation rows / one fragment
  static constexpr int kPPW = (kPA + kPB + kWaves - 1) / kWaves;  // pieces per wave and chunk (every wave issues the same number)
  static constexpr int kStageA = kPA * 1024;
  static constexpr int kStage = kPPW * kWaves * 1024;            // (pieces past kPA + kPB land in the stage's padding)
  static constexpr int kLds = STAGES * kStage;
  static_assert(KS == 1 || KS == 4, "a chunk has four steps");
  static_assert(STAGES >= 2 && kLds <= 160 * 1024, "the ring must fit the CU's LDS");
  static_assert((KS - 1) * BR * BF * kTiles * 1024 <= kStage, "the KS = 4 exchange reuses stage 0");
};

template <int WR, int WF, int BR, int BF, int KS, int STAGES, bool PC>
__global__ __launch_bounds__(64 * BR * BF * KS) void sp24lin_mfma_kernel(Sp24Args p) {
  using S = Sp24Shape<WR, WF, BR, BF, KS, STAGES>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const int wr = wave % BR, wf = (wave / BR) % BF, wk = wave / (BR * BF);  // this wave's row tiles / feature tiles / step
  const int ft0 = blockIdx.x * (WF * BF), row0 = blockIdx.y * S::kRows;

  const size_t a_off = (size_t)row0 * p.lda;
  const size_t a_left = p.a_bytes - a_off;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A + a_off), 0,
                                                                       (unsigned)(a_left < 0xFFFFF000u ? a_left : 0xFFFFF000u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a chunk: kPA of A (2 rows each; lane l: row 2 pi + (l >> 5), LDS slot l & 31, source slot
  //      (l & 31) ^ (row & 15)), kPB of B (fragment (ft, 0 .. 4) as it lies), the rest padding; wave w issues pieces w, w + kWaves, ...
  //      A chunk past K (K % 512 != 0) reads the next row's bytes or, past the buffer, zeros: the panel holds zeros there.  A
  //      feature tile past the panel reads zeros (the buffer's bound).
  const int nch = p.nch;
  const int rot = (int)(blockIdx.x % (unsigned)nch);
  unsigned src[S::kPPW], step_bytes[S::kPPW];
#pragma unroll
  for (int j = 0; j < S::kPPW; ++j) {
    const int pi = wave + S::kWaves * j;
    if (pi < S::kPA) {
      const int row = 2 * pi + (lane >> 5);
      src[j] = (unsigned)row * p.lda + (unsigned)(((lane & 31) ^ (row & 15)) * 16);
      step_bytes[j] = kChunk;
    } else {
      const int f = (pi - S::kPA) % S::kPB;  // (padding pieces: a second copy of a B piece, unused)
      src[j] = (unsigned)((ft0 + f / 5) * nch * 5 + f % 5) * 1024u + (unsigned)lane * 16u;
      step_bytes[j] = 5120;
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

  v4i acc[WR][WF];
#pragma unroll
  for (int i = 0; i < WR; ++i)
#pragma unroll
    for (int f = 0; f < WF; ++f) acc[i][f] = v4i{0, 0, 0, 0};
  const int arow = (wr * WR * 16 + lr) * kChunk;                  // row lr of this wave's first row tile; slot s of it at (s ^ lr) * 16
  const int bfrag = S::kStageA + wf * WF * 5120 + lane * 16;      // fragment 0 of this wave's first feature tile, this lane's 16 bytes
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i) issue(nch > i ? i : 0);
  for (int step = 0; step < nch; ++step) {
    // my pieces of this chunk (the STAGES - 2 chunks after it may be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * S::kPPW) : "memory");
    asm volatile("s_barrier" ::: "memory");  // everyone's pieces; everyone is done with the previous chunk
    issue(step + STAGES - 1);  // -> the stage of the previous chunk (past the end the walk wraps: keeps the vmcnt counts uniform)
    const uint8_t* st = smem + (step % STAGES) * S::kStage;
    int idx[WF][4];
#pragma unroll
    for (int f = 0; f < WF; ++f) {
      if constexpr (KS == 1) {
        const v4i x = *reinterpret_cast<const v4i*>(st + bfrag + f * 5120 + 4096);
        idx[f][0] = x.x; idx[f][1] = x.y; idx[f][2] = x.z; idx[f][3] = x.w;
      } else {
        idx[f][0] = idx[f][1] = idx[f][2] = idx[f][3] = *reinterpret_cast<const int*>(st + bfrag + f * 5120 + 4096 + 4 * wk);
      }
    }
#pragma unroll
    for (int v = (KS == 4 ? wk : 0); v < 4; v += KS) {
      v4i w[WF];
#pragma unroll
      for (int f = 0; f < WF; ++f) w[f] = *reinterpret_cast<const v4i*>(st + bfrag + f * 5120 + v * 1024);
#pragma unroll
      for (int i = 0; i < WR; ++i) {
        const v4i lo = *reinterpret_cast<const v4i*>(st + arow + i * 16 * kChunk + ((8 * v + lq) ^ lr) * 16) ^ (int)0x80808080;      // u8 -> s8
        const v4i hi = *reinterpret_cast<const v4i*>(st + arow + i * 16 * kChunk + ((8 * v + 4 + lq) ^ lr) * 16) ^ (int)0x80808080;  // (128 * wsum is in ocp)
        const v8i a = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int f = 0; f < WF; ++f) acc[i][f] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(w[f], a, acc[i][f], idx[f][KS == 4 ? 0 : v], 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wrapped pieces: nothing may land after the block is gone)

  if constexpr (KS == 4) {  // the four steps' partial tiles: steps 1 .. 3 hand theirs to step 0 through stage 0
    asm volatile("s_barrier" ::: "memory");  // everyone has landed and is done reading the stages
    v4i* xch = reinterpret_cast<v4i*>(smem) + (wr + BR * wf) * S::kTiles * 64 + lane;
    constexpr int kPer = BR * BF * S::kTiles * 64;  // v4i per step
    if (wk != 0) {
#pragma unroll
      for (int i = 0; i < WR; ++i)
#pragma unroll
        for (int f = 0; f < WF; ++f) xch[(wk - 1) * kPer + (i * WF + f) * 64] = acc[i][f];
    }
    __syncthreads();
    if (wk != 0) return;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int i = 0; i < WR; ++i)
#pragma unroll
        for (int f = 0; f < WF; ++f) acc[i][f] += xch[s * kPer + (i * WF + f) * 64];
  }

  // ---- epilogue of src/fully_connected.cc:42-48: lane (q, r) holds features 4 q .. 4 q + 3 of row r of each of its tiles
#pragma unroll
  for (int i = 0; i < WR; ++i)
#pragma unroll
    for (int f = 0; f < WF; ++f) {
      const int row = row0 + (wr * WR + i) * 16 + lr, n = (ft0 + wf * WF + f) * 16 + 4 * lq;
      if (row < p.M && n < p.N) {
        int cv[4] = {acc[i][f].x, acc[i][f].y, acc[i][f].z, acc[i][f].w};
        const int nf = p.N - n < 4 ? p.N - n : 4;
        // (n < N <= Npad, n % 4 == 0: the quad lies inside the padded arrays)
        i8ie_epi_finish<PC>(p.ep, cv, i8ie_epi_cols_vec<PC>(p.ep, n), nf, (long long)row * p.N + n, p.out + (size_t)row * p.N + n,
                            nf == 4 && (p.N & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 3u) == 0, [&](int (&c)[4]) {
#pragma unroll
                              for (int r = 0; r < 4; ++r)
                                if (r < nf) c[r] = (int)((float)c[r] + p.ep.biasf[n + r]);
                            });
      }
    }
}

// ---- sp24lin_direct: the definition.  One lane per output (row, j): the sum over the kept values of feature j, each against the
// activation at its dense k (c, hw: rows that are a flattened NHWC activation hold weight k = ch * hw + pix at k' = pix * c + ch) ----
struct Sp24DirectArgs {
  const uint8_t* A;
  int M, N, K, nch, c, hw;
  const uint8_t* B;
  I8ieEpiArgs ep;  // ocp here: the plain oc (the activations enter as they are)
  uint8_t* out;
};

template <bool PC>
__global__ __launch_bounds__(256) void sp24lin_direct_kernel(Sp24DirectArgs p) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.M * p.N) return;
  const int row = (int)(item / p.N), j = (int)(item - (long long)row * p.N);
  const uint8_t* a = p.A + (size_t)row * p.K;
  int sum = 0;
  for (int g = 0; 4 * g < p.K; ++g) {
    const unsigned nib = (p.B[i8ie_sp24_index_at(j, g, p.nch)] >> (4 * (g & 1))) & 15u;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = 4 * g + (int)((nib >> (2 * e)) & 3u);
      if (k >= p.K) continue;  // (a partial last group: the value there is 0)
      const int kq = p.hw > 1 ? (k % p.hw) * p.c + k / p.hw : k;
      sum += (int)a[kq] * (int)(int8_t)p.B[i8ie_sp24_value_at(j, g, e, p.nch)];
    }
  }
  int cv[4] = {sum, 0, 0, 0};
  i8ie_epi_finish<PC>(p.ep, cv, i8ie_epi_cols<PC>(p.ep, j, 1), 1, item, p.out + item, false, [&](int (&c)[4]) {
    c[0] = (int)((float)c[0] + p.ep.biasf[j]);
  });
}

// ---- the one-off kernel of a handle --------------------------------------------------------------------------------------------
// src/fully_connected.cc:30-38 from the compressed panel: one thread per feature replays the reference's sequential fp32
// accumulation with k ascending (a group's first position is below its second; the zeros between add +0 and are skipped);
// also the exact row sum, oc' and the float bias
__global__ __launch_bounds__(64) void sp24_offsets_kernel(const uint8_t* __restrict__ B, const int8_t* __restrict__ qb, int n, int K,
                                                          int nch, float s_in, int zp_in, int32_t* __restrict__ oc,
                                                          int32_t* __restrict__ wsum, int32_t* __restrict__ ocp,
                                                          float* __restrict__ biasf) {
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
  oc[j] = (int)(-t);
  wsum[j] = s;
  ocp[j] = oc[j] + 128 * s;
  biasf[j] = (float)qb[j] / s_in;
}

template <int WR, int WF, int BR, int BF, int KS, int STAGES, bool PC>
int sp24_launch_t(i8ie_ctx* ctx, const Sp24Args& a) {
  using S = Sp24Shape<WR, WF, BR, BF, KS, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&sp24lin_mfma_kernel<WR, WF, BR, BF, KS, STAGES, PC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kLds));
    raised[dev] = true;
  }
  const dim3 grid((unsigned)((a.N + S::kFeats - 1) / S::kFeats), (unsigned)((a.M + S::kRows - 1) / S::kRows));
  sp24lin_mfma_kernel<WR, WF, BR, BF, KS, STAGES, PC><<<grid, S::kThreads, S::kLds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

template <bool PC>
int sp24_launch_rows(i8ie_ctx* ctx, const Sp24Args& a) {
  if (a.M <= 16) return sp24_launch_t<1, 1, 1, 1, 4, 8, PC>(ctx, a);
  if (a.M <= 128) return sp24_launch_t<2, 1, 2, 2, 1, 3, PC>(ctx, a);
  return sp24_launch_t<2, 2, 2, 4, 1, 2, PC>(ctx, a);
}

}  // namespace

void i8ie_sp24_pack_panel(const int8_t* values, const uint8_t* index, int n, int K, uint8_t* panel) {
  const int nch = i8ie_sp24_chunks(K), groups = (K + 3) / 4;
  for (int j = 0; j < n; ++j)
    for (int g = 0; g < groups; ++g) {
      const unsigned nib = (index[(size_t)j * ((groups + 1) / 2) + g / 2] >> (4 * (g & 1))) & 15u;
      const size_t at = i8ie_sp24_index_at(j, g, nch);
      panel[at] = (uint8_t)(panel[at] | (nib << (4 * (g & 1))));
      for (int e = 0; e < 2; ++e) panel[i8ie_sp24_value_at(j, g, e, nch)] = (uint8_t)values[((size_t)j * groups + g) * 2 + e];
    }
}

bool i8ie_sp24lin_mfma_takes(const I8ieSp24Call& c) {
  return c.K % 32 == 0 && c.hw == 1 && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 && (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0;
}

int i8ie_sp24lin_mfma_launch(i8ie_ctx* ctx, const I8ieSp24Call& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= 65536 && i8ie_sp24lin_mfma_takes(c), "sp24lin_mfma: shape or alignment");
  I8IE_REQUIRE(c.ep.biasf != nullptr && (c.ep.msv == nullptr) == (c.ep.sbv == nullptr), "sp24lin_mfma: epilogue vectors");
  const size_t b_bytes = i8ie_sp24_panel_bytes(c.N, c.K);
  I8IE_REQUIRE(b_bytes < ((size_t)1 << 32) - 8192, "sp24lin_mfma: panel offsets exceed 32 bits");
  Sp24Args a{};
  a.A = c.A; a.a_bytes = (size_t)c.M * c.K; a.lda = (unsigned)c.K; a.M = c.M; a.N = c.N; a.nch = i8ie_sp24_chunks(c.K);
  a.B = c.B; a.b_bytes = (unsigned)b_bytes;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  // the compressed panel once from HBM; every row block reads its rows' activations once per feature block
  I8ieProfScope prof(ctx, "sp24lin_mfma", 2.0 * c.M * c.N * c.K, (double)c.M * c.K + 0.625 * c.N * c.K + (double)c.M * c.N);
  return c.ep.msv != nullptr ? sp24_launch_rows<true>(ctx, a) : sp24_launch_rows<false>(ctx, a);
}

int i8ie_sp24lin_direct_launch(i8ie_ctx* ctx, const I8ieSp24Call& c) {
  I8IE_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.K <= 65536, "sp24lin_direct: shape");
  I8IE_REQUIRE(c.hw >= 1 && c.K % c.hw == 0, "sp24lin_direct: in_features is not c * h * w");
  I8IE_REQUIRE((long long)c.M * c.N < (1LL << 39), "sp24lin_direct: output too large");
  I8IE_REQUIRE(c.ep.biasf != nullptr && (c.ep.msv == nullptr) == (c.ep.sbv == nullptr), "sp24lin_direct: epilogue vectors");
  Sp24DirectArgs a{};
  a.A = c.A; a.M = c.M; a.N = c.N; a.K = c.K; a.nch = i8ie_sp24_chunks(c.K); a.c = c.K / c.hw; a.hw = c.hw;
  a.B = c.B;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)c.M * c.N;
  I8ieProfScope prof(ctx, "sp24lin_direct", 2.0 * c.M * c.N * c.K, (double)c.M * c.K + 0.625 * c.N * c.K + (double)c.M * c.N);
  if (c.ep.msv != nullptr)
    sp24lin_direct_kernel<true><<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  else
    sp24lin_direct_kernel<false><<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_sp24_launch_offsets(i8ie_ctx* ctx, const uint8_t* panel, const int8_t* qb, int n, int K, float s_in, int zp_in,
                             int32_t* oc, int32_t* wsum, int32_t* ocp, float* biasf) {
  I8ieProfScope prof(ctx, "sp24_offsets", 0.0, 0.5 * n * K);
  sp24_offsets_kernel<<<(n + 63) / 64, 64, 0, ctx->stream>>>(panel, qb, n, K, i8ie_sp24_chunks(K), s_in, zp_in, oc, wsum, ocp, biasf);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
