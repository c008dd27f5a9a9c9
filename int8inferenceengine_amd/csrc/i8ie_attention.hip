// i8ie_attention.hip -- fused multi-head attention: i8ie_attention_u8, i8ie_attention_f32.
// The arithmetic is defined in include/i8ie_hip.h as a composition of entries that exist: per (batch item, head)
//     S = bmm_u8(Q_h, K_h^T -> s_s, zp_s);  P = softmax_u8(S, s_s);  O_h = bmm_u8(P, V_h; 1/256, 0, s_v, zp_v -> s_o, zp_o), relu
// Head h is columns h*d .. h*d + d - 1 of [b, t, c]: Q_h and K_h are K-contiguous "rows x k" operands with the token stride as
// row stride, V_h is K-strided (its k is the token axis), exactly the two operand forms of i8ie_bmm_tile.h.
//
//   attn_mfma    d % 16 == 0, operand pointers and strides 16-byte aligned, tk <= 1024.  A block of 4 waves owns 64 query
//                rows of one (batch item, head) and runs three phases with the scores and probabilities in an LDS strip
//                [64][SP], SP = roundup(tk, 64) + 16 bytes.
//                1  scores: for each 64-row tile of K, walk d in steps of 64; the Q and K tiles are staged by stage_tile
//                   (re-biased, zero-filled past tq, tk and d) and multiplied with v_mfma_i32_16x16x64_i8, 2 x 2 waves of
//                   32 x 32 as in bmm_mfma; the row sums of Q' and K' for the zero-point correction
//                       C = P - za' colsum - zb' rowsum + d za' zb'
//                   come from the staged fragments by an MFMA against a fragment of ones (bmm_mfma's choice: they arrive in
//                   the accumulators' lane layout).  The tile is requantised through i8ie_requant_pack4 (no relu) and written
//                   into the strip as dwords.  Q is re-staged for every K tile (it comes from the cache after the first).
//                2  softmax in the strip, in place: a wave takes 16 rows, one after the other; a lane keeps 4 dwords of the
//                   row in registers (i8ie_softmax.hip's wave form), the max and S go through wave reductions, the quotient
//                   is i8ie_softmax_dev.h's div_by.  Columns >= tk hold the score of a zero-filled K row, which is not
//                   neutral: they are masked out of the max and of S.  The probabilities are written back re-biased
//                   (p ^ 0x80), and 0 -- the s8 zero -- in columns tk .. roundup(tk, 64) - 1, so that phase 3 has no bounds
//                   test; the row's sum of probabilities is kept for phase 3's correction.
//                3  O = P V: for each 64 columns of d, walk tk in steps of 64; the P fragments are 16-byte reads straight
//                   from the strip (SP / 16 is odd: the 16 lanes of a ds_read_b128 quarter land on 16 distinct 16-byte
//                   slots, the 80-byte-row argument of section 8k), V is staged through stage_tile's 4 x 4 register transpose.
//                   Correction with zp_p = 0 (za' = -128), rowsum = (sum of the row's probabilities) - 128 tk from phase 2,
//                   colsum of V' by an MFMA against ones.  Requantised with (1/256, s_v, s_o, zp_o), relu folded, four
//                   columns packed: a dword store where the address allows, else bytes.
//                Rows >= tq are computed on zeros and never stored.
//   attn_direct  everything else and everything under I8IE_OPT_FORCE_FALLBACK: one block per (batch item, head, query row),
//                the score row in LDS (tk <= 32768 bytes), plain loops, i8ie_requant_exact: the definition verbatim.
//   FP32         i8ie_bmm_f32, i8ie_softmax_f32, i8ie_bmm_f32 per head through strides, the scores in the ctx workspace.
//
// The windowed form (i8ie_attention_window_u8 / _f32): attention inside non-overlapping wh x ww windows
// of an [n, h, w, c] map.  Both kernels are templates on WIN; with WIN a "batch item" is one (image, window), token j of it is
// pixel (wy * wh + j / ww, wx * ww + j % ww), and every place that turned a token into an address -- stage_tile's row (Q, K) or
// k (V) offset, attn_direct's three reads, the result's pixel -- goes through WindowRows: (j / ww) * pitch + (j % ww) * stride,
// the pitch being one physical map row, border included, and j / ww a multiply by a host-made reciprocal.  One window per 64-row
// tile.  Everything between the addresses (the strip, the softmax, the corrections, the requantiser, the debug outputs, which
// count (image, window) as the batch) is the same code; without WIN the kernels compile to what they were.
//   FP32         part / unpart: gather the windows of NCHW floats into [n * nW, T, c] in the ctx workspace, i8ie_attention_f32
//                on them, scatter the result back.  The calibration path.
#include <algorithm>
#include <cmath>

#include "i8ie_bmm_tile.h"
#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_requant.h"
#include "i8ie_softmax_dev.h"

namespace {

constexpr int kMaxTk = 32768;       // the second product's k
constexpr int kStripMaxTk = 1024;   // attn_mfma: 64 x (1024 + 16) bytes of strip
constexpr int kStripPad = 16;
constexpr int kMaxBorder = 65535;   // the windowed entries: a border in pixels (i8ie_pad2d's limit on an amount)

struct AttnParams {
  BmmOp Q, K, V;        // Q, K: rows are tokens, k the head's columns (ks == 1); V: rows are the head's columns, k the tokens
  int H, D, Tq, Tk, tiles_q;
  int Tk64, SP;         // attn_mfma: tk rounded up to 64, bytes per strip row
  uint8_t* out;         // interior pixel (0, 0) of a bordered map
  int64_t o_batch, o_tok;
  uint32_t xout;
  int pix_w, pix_pad;   // physical token index = i + (i / pix_w) * pix_pad (pix_pad = 2B, 0: plain)
  uint8_t* sdbg;
  uint8_t* pdbg;
  int32_t* acc;
  I8ieRequant rq_s, rq_o;
  int lo;               // the relu's lower bound on the result (zp_o, or 0)
  // the windowed form alone (WIN kernels): `out` is then interior pixel (0, 0) and pix_w / pix_pad are unused
  uint32_t w_mult;      // ceil(2^30 / ww): j / ww == umulhi(j << 2, w_mult) for j, ww <= 32768
  int wh, ww, nwx, nw;  // the window; windows per map row and per image
  int64_t q_pitch, k_pitch, v_pitch, o_pitch;  // bytes between two physical map rows of each operand and of the result
};

// token j of a window -> the byte offset of its pixel from the window's first pixel; `stride` is one physical pixel
struct WindowRows {
  uint32_t mult;
  int ww;
  int64_t pitch;
  __device__ __forceinline__ int64_t operator()(int j, int64_t stride) const {
    const int y = (int)__umulhi((uint32_t)j << 2, mult);
    return (int64_t)y * pitch + (int64_t)(j - y * ww) * stride;
  }
};
template <bool WIN> struct RowsOf;
template <> struct RowsOf<false> {
  using type = LinearRows;
  static __device__ __forceinline__ type make(const AttnParams&, int64_t) { return LinearRows(); }
};
template <> struct RowsOf<true> {
  using type = WindowRows;
  static __device__ __forceinline__ type make(const AttnParams& p, int64_t pitch) { return WindowRows{p.w_mult, p.ww, pitch}; }
};

// A block's sequence `seq` is a batch item, or with WIN one (image, window): the image, and the byte offsets of the window's
// first pixel inside the image for q, k, v and the result.
template <bool WIN>
struct AttnSeq {
  int batch;
  int64_t q0 = 0, k0 = 0, v0 = 0, o0 = 0;
  __device__ __forceinline__ AttnSeq(const AttnParams& p, int seq) : batch(seq) {
    if (WIN) {
      batch = seq / p.nw;
      const int wi = seq - batch * p.nw;
      const int wy = wi / p.nwx, wx = wi - wy * p.nwx;
      const int64_t y0 = (int64_t)wy * p.wh, x0 = (int64_t)wx * p.ww;
      q0 = y0 * p.q_pitch + x0 * p.Q.rs;
      k0 = y0 * p.k_pitch + x0 * p.K.rs;
      v0 = y0 * p.v_pitch + x0 * p.V.ks;
      o0 = y0 * p.o_pitch + x0 * p.o_tok;
    }
  }
};

__device__ __forceinline__ int64_t out_token_index(const AttnParams& p, int i) {
  return p.pix_pad ? (int64_t)i + (int64_t)(i / p.pix_w) * p.pix_pad : (int64_t)i;
}
// the byte offset of result token i from the sequence's first result byte
template <bool WIN>
__device__ __forceinline__ int64_t out_token_offset(const AttnParams& p, int i) {
  if (WIN) return WindowRows{p.w_mult, p.ww, p.o_pitch}(i, p.o_tok);
  return out_token_index(p, i) * p.o_tok;
}

extern __shared__ __attribute__((aligned(16))) uint8_t attn_smem[];

template <bool WIN>
__global__ __launch_bounds__(256) void attn_mfma_kernel(AttnParams p, SoftmaxTable tab) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[2 * TM * LROW];
  __shared__ uint32_t E[256];
  __shared__ uint32_t psum[TM];
  uint8_t* As = stage;
  uint8_t* Bs = stage + TM * LROW;
  uint8_t* strip = attn_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  E[tid] = tab.e[tid];
  const int tile = blockIdx.x % p.tiles_q, bh = blockIdx.x / p.tiles_q;
  const int h = bh % p.H, seq = bh / p.H;
  const AttnSeq<WIN> sq(p, seq);
  const int batch = sq.batch;
  const int m0 = tile * TM;
  const uint8_t* Qb = p.Q.p + (int64_t)batch * p.Q.batch + sq.q0 + (int64_t)h * p.D;
  const uint8_t* Kb = p.K.p + (int64_t)batch * p.K.batch + sq.k0 + (int64_t)h * p.D;
  const uint8_t* Vb = p.V.p + (int64_t)batch * p.V.batch + sq.v0 + (int64_t)h * p.D;
  const typename RowsOf<WIN>::type q_at = RowsOf<WIN>::make(p, p.q_pitch), k_at = RowsOf<WIN>::make(p, p.k_pitch),
                                   v_at = RowsOf<WIN>::make(p, p.v_pitch);
  const int q = lane >> 4, r = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const int64_t dbg_head = ((int64_t)seq * p.H + h) * p.Tq;  // row index of this head's first query row in [b, H, tq, tk]

  // ---- phase 1: the u8 scores of the 64 query rows, into the strip ----
  {
    const uint32_t za = (uint32_t)(p.Q.zp - 128), zb = (uint32_t)(p.K.zp - 128);
    const uint32_t kzz = (uint32_t)p.D * za * zb;
    for (int j0 = 0; j0 < p.Tk; j0 += TN) {
      v4i acc[2][2], rsum[2], csum[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        rsum[i] = v4i{0, 0, 0, 0};
        csum[i] = v4i{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = v4i{0, 0, 0, 0};
      }
      for (int k0 = 0; k0 < p.D; k0 += TK) {
        stage_tile(p.Q, Qb, p.Tq, p.D, m0, k0, As, q_at);
        stage_tile(p.K, Kb, p.Tk, p.D, j0, k0, Bs, k_at);
        __syncthreads();
        v4i a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const v4i*>(As + (wm * 32 + i * 16 + r) * LROW + 16 * q);
          b[i] = *reinterpret_cast<const v4i*>(Bs + (wn * 32 + i * 16 + r) * LROW + 16 * q);
        }
        // with K's fragment as srcA, lane (q, r) receives columns 4q .. 4q + 3 of row r; the sums arrive in the same layout
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          rsum[mi] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, a[mi], rsum[mi], 0, 0, 0);
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], a[mi], acc[mi][ni], 0, 0, 0);
        }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) csum[ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], ones, csum[ni], 0, 0, 0);
        __syncthreads();
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int lr = wm * 32 + mi * 16 + r;
        const int m = m0 + lr;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int nb = j0 + wn * 32 + ni * 16 + 4 * q;   // < Tk64: inside the strip row
          int c[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            c[e] = (int)((uint32_t)acc[mi][ni][e] - za * (uint32_t)csum[ni][e] - zb * (uint32_t)rsum[mi][e] + kzz);
          const uint32_t packed = i8ie_requant_pack4(c, p.rq_s, 0, 0.0f);
          *reinterpret_cast<uint32_t*>(strip + lr * p.SP + nb) = packed;
          if (p.sdbg && m < p.Tq) {
            uint8_t* sp = p.sdbg + (dbg_head + m) * p.Tk + nb;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (nb + e < p.Tk) sp[e] = (uint8_t)(packed >> (8 * e));
          }
        }
      }
    }
  }
  __syncthreads();  // (also: E is complete)

  // ---- phase 2: softmax of each strip row over its first tk columns, in place, written back re-biased ----
  for (int lr = wave * 16; lr < wave * 16 + 16; ++lr) {
    uint8_t* row = strip + lr * p.SP;
    uint32_t v[16];
    uint32_t mx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * (lane + 64 * i);
      uint32_t w = 0;
      if (j < p.Tk) w = *reinterpret_cast<const uint32_t*>(row + j);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        v[4 * i + b] = j + b < p.Tk ? (w >> (8 * b)) & 0xFFu : 0u;   // (a masked 0 never raises the max)
        mx = v[4 * i + b] > mx ? v[4 * i + b] : mx;
      }
    }
    mx = wave_max(mx);
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = 4 * (lane + 64 * (i >> 2)) + (i & 3);
      v[i] = E[mx - v[i]];
      sum += j < p.Tk ? v[i] : 0u;
    }
    const uint32_t S = wave_sum(sum);
    const float rinv = 1.0f / (float)S;
    const uint32_t half = S >> 1;
    const int m = m0 + lr;
    uint32_t ps = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * (lane + 64 * i);
      if (j >= p.Tk64) continue;
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (j + b < p.Tk) {
          const uint32_t pr = div_by(v[4 * i + b] * 256u + half, S, rinv);
          ps += pr;
          w |= (pr ^ 0x80u) << (8 * b);
          if (p.pdbg && m < p.Tq) p.pdbg[(dbg_head + m) * p.Tk + j + b] = (uint8_t)pr;
        }
      }
      *reinterpret_cast<uint32_t*>(row + j) = w;
    }
    ps = wave_sum(ps);
    if (lane == 0) psum[lr] = ps;
  }
  __syncthreads();

  // ---- phase 3: O = P V, requantised into the result ----
  {
    const uint32_t za = (uint32_t)(0 - 128), zb = (uint32_t)(p.V.zp - 128);
    const uint32_t kzz = (uint32_t)p.Tk * za * zb;
    const float lof = (float)p.lo;
    for (int n0 = 0; n0 < p.D; n0 += TN) {
      v4i acc[2][2], csum[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        csum[i] = v4i{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = v4i{0, 0, 0, 0};
      }
      for (int k0 = 0; k0 < p.Tk; k0 += TK) {
        stage_tile(p.V, Vb, p.D, p.Tk, n0, k0, Bs, v_at);
        __syncthreads();
        v4i a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const v4i*>(strip + (wm * 32 + i * 16 + r) * p.SP + k0 + 16 * q);
          b[i] = *reinterpret_cast<const v4i*>(Bs + (wn * 32 + i * 16 + r) * LROW + 16 * q);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], a[mi], acc[mi][ni], 0, 0, 0);
        }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) csum[ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[ni], ones, csum[ni], 0, 0, 0);
        __syncthreads();
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int lr = wm * 32 + mi * 16 + r;
        const int m = m0 + lr;
        if (m >= p.Tq) continue;
        const uint32_t rs = psum[lr] - 128u * (uint32_t)p.Tk;   // the row sum of P' = P - 128 over the true tk
        uint8_t* orow = p.out + (int64_t)batch * p.o_batch + sq.o0 + out_token_offset<WIN>(p, m) + (int64_t)h * p.D;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int nb = n0 + wn * 32 + ni * 16 + 4 * q;
          if (nb >= p.D) continue;   // (d % 16 == 0: a group of four columns is inside the head or outside)
          int c[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) c[e] = (int)((uint32_t)acc[mi][ni][e] - za * (uint32_t)csum[ni][e] - zb * rs + kzz);
          if (p.acc) {
            int32_t* ap = p.acc + ((int64_t)seq * p.Tq + m) * ((int64_t)p.H * p.D) + (int64_t)h * p.D + nb;
#pragma unroll
            for (int e = 0; e < 4; ++e) ap[e] = c[e];
          }
          const uint32_t packed = i8ie_requant_pack4(c, p.rq_o, p.lo, lof) ^ p.xout;
          uint8_t* op = orow + nb;
          if ((reinterpret_cast<uintptr_t>(op) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(op) = packed;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) op[e] = (uint8_t)(packed >> (8 * e));
          }
        }
      }
    }
  }
}

// one block per (batch item, head, query row); attn_smem holds the row's tk scores, then its probabilities
template <bool WIN>
__global__ __launch_bounds__(kThreads) void attn_direct_kernel(AttnParams p, SoftmaxTable tab) {
  __shared__ uint32_t E[256];
  __shared__ uint32_t red[kThreads / 64];
  uint8_t* sc = attn_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  E[tid] = tab.e[tid];
  const int i = blockIdx.x % p.Tq, bh = blockIdx.x / p.Tq;
  const int h = bh % p.H, seq = bh / p.H;
  const AttnSeq<WIN> sq(p, seq);
  const int batch = sq.batch;
  const typename RowsOf<WIN>::type q_at = RowsOf<WIN>::make(p, p.q_pitch), k_at = RowsOf<WIN>::make(p, p.k_pitch),
                                   v_at = RowsOf<WIN>::make(p, p.v_pitch);
  const uint32_t xq = (p.Q.x & 0xFFu) ^ 0x80u, xk = (p.K.x & 0xFFu) ^ 0x80u, xv = (p.V.x & 0xFFu) ^ 0x80u;  // to plain bytes
  const uint8_t* qr = p.Q.p + (int64_t)batch * p.Q.batch + sq.q0 + q_at(i, p.Q.rs) + (int64_t)h * p.D;
  const uint8_t* kb = p.K.p + (int64_t)batch * p.K.batch + sq.k0 + (int64_t)h * p.D;
  const uint8_t* vb = p.V.p + (int64_t)batch * p.V.batch + sq.v0 + (int64_t)h * p.D;
  const int64_t dbg_row = (((int64_t)seq * p.H + h) * p.Tq + i) * p.Tk;
  uint32_t mx = 0;
  for (int j = tid; j < p.Tk; j += kThreads) {
    const uint8_t* kr = kb + k_at(j, p.K.rs);
    uint32_t sum = 0;
    for (int c = 0; c < p.D; ++c) {
      const int av = (int)((uint32_t)qr[c] ^ xq) - p.Q.zp;
      const int bv = (int)((uint32_t)kr[c] ^ xk) - p.K.zp;
      sum += (uint32_t)(av * bv);
    }
    const uint32_t s = (uint32_t)i8ie_requant_exact((float)(int)sum, p.rq_s, 0);
    sc[j] = (uint8_t)s;
    if (p.sdbg) p.sdbg[dbg_row + j] = (uint8_t)s;
    mx = s > mx ? s : mx;
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();  // (also: E and the score row are complete)
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) mx = red[w] > mx ? red[w] : mx;
  __syncthreads();
  uint32_t sum = 0;
  for (int j = tid; j < p.Tk; j += kThreads) sum += E[mx - (uint32_t)sc[j]];
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  uint32_t S = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) S += red[w];
  const float rinv = 1.0f / (float)S;
  const uint32_t half = S >> 1;
  for (int j = tid; j < p.Tk; j += kThreads) {   // (a lane rewrites only the bytes it read itself)
    const uint32_t pr = div_by(E[mx - (uint32_t)sc[j]] * 256u + half, S, rinv);
    sc[j] = (uint8_t)pr;
    if (p.pdbg) p.pdbg[dbg_row + j] = (uint8_t)pr;
  }
  __syncthreads();
  for (int c = tid; c < p.D; c += kThreads) {
    uint32_t acc = 0;
    for (int j = 0; j < p.Tk; ++j) {
      const int bv = (int)((uint32_t)vb[v_at(j, p.V.ks) + c] ^ xv) - p.V.zp;
      acc += (uint32_t)((int)sc[j] * bv);
    }
    const int64_t col = (int64_t)h * p.D + c;
    if (p.acc) p.acc[((int64_t)seq * p.Tq + i) * ((int64_t)p.H * p.D) + col] = (int)acc;
    const int qv = i8ie_requant_exact((float)(int)acc, p.rq_o, p.lo);
    p.out[(int64_t)batch * p.o_batch + sq.o0 + out_token_offset<WIN>(p, i) + col] = (uint8_t)((uint32_t)qv ^ (p.xout & 0xFFu));
  }
}

// ---- FP32 windowed form: gather / scatter between an NCHW map and its windows [n * nW, T, c] ----
struct PartParams {
  int64_t total;            // n * c * h * w
  int c, T, ww, nwx, nw, W; // W: map width
  int64_t batch, chan;      // floats between two images / two channels of the map
};
// item e = (seq, j, col) of the dense [n * nW, T, c] side; the map element it mirrors
__device__ __forceinline__ int64_t part_map_index(const PartParams& p, int64_t e, int wh) {
  const int col = (int)(e % p.c);
  const int64_t t = e / p.c;
  const int j = (int)(t % p.T);
  const int64_t seq = t / p.T;
  const int wi = (int)(seq % p.nw);
  const int64_t img = seq / p.nw;
  const int y = (wi / p.nwx) * wh + j / p.ww, x = (wi % p.nwx) * p.ww + j % p.ww;
  return img * p.batch + (int64_t)col * p.chan + (int64_t)y * p.W + x;
}
__global__ __launch_bounds__(kThreads) void attn_part_f32_kernel(const float* __restrict__ map, float* __restrict__ win, PartParams p, int wh) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < p.total; e += (int64_t)gridDim.x * kThreads)
    win[e] = map[part_map_index(p, e, wh)];
}
__global__ __launch_bounds__(kThreads) void attn_unpart_f32_kernel(const float* __restrict__ win, float* __restrict__ map, PartParams p, int wh) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < p.total; e += (int64_t)gridDim.x * kThreads)
    map[part_map_index(p, e, wh)] = win[e];
}

bool mat_ok(const i8ie_attn_mat& m, int64_t c) { return m.ptr != nullptr && m.batch_stride >= 0 && m.token_stride >= c; }
bool fits31(const i8ie_attn_mat& m) { return m.batch_stride <= 0x7FFFFFFF && m.token_stride <= 0x7FFFFFFF; }
bool aligned16(const i8ie_attn_mat& m) { return aligned_to(m.ptr, 16) && m.batch_stride % 16 == 0 && m.token_stride % 16 == 0; }

// the checks both entries share
int check_sizes(const i8ie_attention_args* g) {
  I8IE_REQUIRE(g->b > 0 && g->heads > 0 && g->d > 0 && g->tq > 0 && g->tk > 0, "non-positive size");
  I8IE_REQUIRE(g->tk <= kMaxTk, "tk > 32768: the second product's int32 sum could overflow");
  I8IE_REQUIRE((int64_t)g->heads * g->d <= 0x7FFFFFFF, "heads * d does not fit");
  const int64_t c = (int64_t)g->heads * g->d;
  I8IE_REQUIRE(mat_ok(g->q, c) && mat_ok(g->k, c) && mat_ok(g->v, c) && mat_ok(g->out, c),
               "null pointer, negative batch stride, or a token stride below heads * d");
  I8IE_REQUIRE((int64_t)g->b * g->heads * g->tq <= 0x7FFFFFFF, "too many query rows for one launch");
  return I8IE_OK;
}

// the checks both windowed entries share; the least token stride is heads * d, or for the FP32 form (NCHW, where it is the
// channel stride) the map's pixel count
int check_window(const i8ie_attention_args* g, const i8ie_attention_window* w, bool f32) {
  I8IE_REQUIRE(g->b > 0 && g->heads > 0 && g->d > 0, "non-positive size");
  I8IE_REQUIRE((int64_t)g->heads * g->d <= 0x7FFFFFFF, "heads * d does not fit");
  I8IE_REQUIRE(w->map_h > 0 && w->map_w > 0 && w->win_h > 0 && w->win_w > 0, "non-positive map or window");
  I8IE_REQUIRE(w->map_h % w->win_h == 0 && w->map_w % w->win_w == 0, "the window does not divide the map");
  I8IE_REQUIRE((int64_t)w->win_h * w->win_w <= kMaxTk, "more than 32768 pixels in a window");
  I8IE_REQUIRE(g->tq == w->win_h * w->win_w && g->tk == g->tq, "tq and tk must both be win_h * win_w");
  I8IE_REQUIRE(w->q_border >= 0 && w->k_border >= 0 && w->v_border >= 0 && w->q_border <= kMaxBorder && w->k_border <= kMaxBorder &&
                   w->v_border <= kMaxBorder,
               "an operand border is negative or above 65535");
  I8IE_REQUIRE(g->out_h == w->map_h && g->out_w == w->map_w && g->out_border >= 0 && g->out_border <= kMaxBorder,
               "out_h / out_w must be the map, 0 <= out_border <= 65535");
  const int64_t least = f32 ? (int64_t)w->map_h * w->map_w : (int64_t)g->heads * g->d;
  I8IE_REQUIRE(mat_ok(g->q, least) && mat_ok(g->k, least) && mat_ok(g->v, least) && mat_ok(g->out, least),
               "null pointer, negative batch stride, or a stride below its least value");
  // (two factors at a time: each product of two ints fits int64, and the last one multiplies two values below 2^31)
  const int64_t pixels = (int64_t)w->map_h * w->map_w, rows = (int64_t)g->b * g->heads;
  I8IE_REQUIRE(pixels <= 0x7FFFFFFF && rows <= 0x7FFFFFFF && pixels * rows <= 0x7FFFFFFF, "too many query rows for one launch");
  return I8IE_OK;
}

// the first byte of interior pixel (0, 0) of a bordered [.][h + 2B][w + 2B][.] buffer, and the bytes of one of its rows
int64_t padded(int w, int border) { return (int64_t)w + 2 * (int64_t)border; }
int64_t interior_origin(int w, int border, int64_t pixel_stride) { return ((int64_t)border * padded(w, border) + border) * pixel_stride; }

// What both u8 entries do once their arguments are checked.  win == nullptr: the global form, the result's pixel rule in
// pix_w / pix_pad and `origin`, the first result byte's offset.
int launch_u8(i8ie_ctx* ctx, const i8ie_attention_args* g, const i8ie_attention_window* win, int pix_w, int pix_pad, int64_t origin) {
  AttnParams p{};
  const uint32_t plain = 0x80808080u;
  const uint8_t *qp = (const uint8_t*)g->q.ptr, *kp = (const uint8_t*)g->k.ptr, *vp = (const uint8_t*)g->v.ptr;
  int64_t seqs = g->b;
  if (win) {
    qp += interior_origin(win->map_w, win->q_border, g->q.token_stride);
    kp += interior_origin(win->map_w, win->k_border, g->k.token_stride);
    vp += interior_origin(win->map_w, win->v_border, g->v.token_stride);
    p.wh = win->win_h; p.ww = win->win_w;
    p.nwx = win->map_w / win->win_w;
    p.nw = p.nwx * (win->map_h / win->win_h);
    p.w_mult = (uint32_t)((((uint64_t)1 << 30) + (uint32_t)win->win_w - 1) / (uint32_t)win->win_w);
    p.q_pitch = padded(win->map_w, win->q_border) * g->q.token_stride;
    p.k_pitch = padded(win->map_w, win->k_border) * g->k.token_stride;
    p.v_pitch = padded(win->map_w, win->v_border) * g->v.token_stride;
    p.o_pitch = padded(win->map_w, g->out_border) * g->out.token_stride;
    seqs *= p.nw;
  }
  p.Q = BmmOp{qp, g->q.batch_stride, g->q.token_stride, 1, g->q.s8 ? 0u : plain, 16, (int)g->zp_q};
  p.K = BmmOp{kp, g->k.batch_stride, g->k.token_stride, 1, g->k.s8 ? 0u : plain, 16, (int)g->zp_k};
  p.V = BmmOp{vp, g->v.batch_stride, 1, g->v.token_stride, g->v.s8 ? 0u : plain, 16, (int)g->zp_v};
  p.H = g->heads; p.D = g->d; p.Tq = g->tq; p.Tk = g->tk;
  p.tiles_q = (g->tq + TM - 1) / TM;
  p.Tk64 = (g->tk + 63) / 64 * 64;
  p.SP = p.Tk64 + kStripPad;
  p.out = (uint8_t*)g->out.ptr + origin;
  p.o_batch = g->out.batch_stride;
  p.o_tok = g->out.token_stride;
  p.xout = g->out.s8 ? plain : 0u;
  p.pix_w = pix_w;
  p.pix_pad = pix_pad;
  p.sdbg = g->scores_dbg_dev;
  p.pdbg = g->probs_dbg_dev;
  p.acc = g->acc_dbg_dev;
  p.rq_s = i8ie_make_requant(g->s_q, g->s_k, g->s_s, (int)g->zp_s);
  p.rq_o = i8ie_make_requant((float)(1.0 / 256), g->s_v, g->s_o, (int)g->zp_o);
  p.lo = g->relu ? (int)g->zp_o : 0;
  SoftmaxTable tab;
  I8IE_TRY(i8ie_softmax_table(g->s_s, tab.e));
  const int64_t blocks = seqs * g->heads * p.tiles_q;
  const bool mfma = (ctx->options & 1) == 0 && g->d % 16 == 0 && g->tk <= kStripMaxTk && aligned16(g->q) && aligned16(g->k) &&
                    aligned16(g->v) && fits31(g->q) && fits31(g->k) && fits31(g->v) &&
                    (g->acc_dbg_dev == nullptr || aligned_to(g->acc_dbg_dev, 4));
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const double pairs = (double)seqs * g->heads * g->tq * g->tk;
  I8ieProfScope prof(ctx, mfma ? (win ? "attn_mfma_win" : "attn_mfma") : (win ? "attn_direct_win" : "attn_direct"), 4.0 * pairs * g->d,
                     (double)seqs * g->heads * g->d * (2.0 * g->tq + 2.0 * g->tk));
  if (mfma) {
    const size_t lds = (size_t)TM * p.SP;
    // The flag is read and written without a lock, and devices 64 apart share one: either can only repeat the attribute call,
    // which is idempotent (the same kernel, the same limit).  A forward is run eagerly before it is captured into a graph
    // (GraphedForward warms up), so the call is made outside any capture; launch_pc_t (i8ie_pconv.hip) does the same.
    static bool raised[2][64] = {};
    const int dev = ctx->device & 63;
    if (!raised[win ? 1 : 0][dev]) {
      const void* fn = win ? reinterpret_cast<const void*>(&attn_mfma_kernel<true>) : reinterpret_cast<const void*>(&attn_mfma_kernel<false>);
      I8IE_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, TM * (kStripMaxTk + kStripPad)));
      raised[win ? 1 : 0][dev] = true;
    }
    if (win) attn_mfma_kernel<true><<<(unsigned)blocks, 256, lds, ctx->stream>>>(p, tab);
    else attn_mfma_kernel<false><<<(unsigned)blocks, 256, lds, ctx->stream>>>(p, tab);
  } else {
    const size_t lds = i8ie_align_up((size_t)g->tk, 16);
    const unsigned rows = (unsigned)(seqs * g->heads * g->tq);
    if (win) attn_direct_kernel<true><<<rows, kThreads, lds, ctx->stream>>>(p, tab);
    else attn_direct_kernel<false><<<rows, kThreads, lds, ctx->stream>>>(p, tab);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // namespace

extern "C" {

int i8ie_attention_u8(i8ie_ctx* ctx, const i8ie_attention_args* g) {
  I8IE_REQUIRE(ctx && g, "null argument");
  I8IE_TRY(check_sizes(g));
  I8IE_REQUIRE(g->scores_out_dev == nullptr, "scores_out_dev belongs to the FP32 entry");
  I8IE_REQUIRE(std::isfinite(g->s_q) && std::isfinite(g->s_k) && std::isfinite(g->s_v) && std::isfinite(g->s_s) && std::isfinite(g->s_o) &&
                   g->s_s > 0.0f && g->s_o > 0.0f,
               "scales must be finite, s_s > 0 and s_o > 0");
  int pix_w = 1, pix_pad = 0;
  int64_t origin = 0;
  if (g->out_h != 0) {
    I8IE_REQUIRE(g->out_h > 0 && g->out_w > 0 && g->out_border >= 0, "bad pixel geometry");
    I8IE_REQUIRE((int64_t)g->out_h * g->out_w == g->tq, "tq is not out_h * out_w");
    pix_w = g->out_w;
    pix_pad = 2 * g->out_border;
    origin = interior_origin(g->out_w, g->out_border, g->out.token_stride);
  } else {
    I8IE_REQUIRE(g->out_w == 0 && g->out_border == 0, "out_w / out_border without out_h");
  }
  return launch_u8(ctx, g, nullptr, pix_w, pix_pad, origin);
}

int i8ie_attention_window_u8(i8ie_ctx* ctx, const i8ie_attention_args* g, const i8ie_attention_window* w) {
  I8IE_REQUIRE(ctx && g && w, "null argument");
  I8IE_TRY(check_window(g, w, false));
  I8IE_REQUIRE(g->scores_out_dev == nullptr, "scores_out_dev belongs to the FP32 entry");
  I8IE_REQUIRE(std::isfinite(g->s_q) && std::isfinite(g->s_k) && std::isfinite(g->s_v) && std::isfinite(g->s_s) && std::isfinite(g->s_o) &&
                   g->s_s > 0.0f && g->s_o > 0.0f,
               "scales must be finite, s_s > 0 and s_o > 0");
  return launch_u8(ctx, g, w, 1, 0, interior_origin(g->out_w, g->out_border, g->out.token_stride));
}

int i8ie_attention_f32(i8ie_ctx* ctx, const i8ie_attention_args* g) {
  I8IE_REQUIRE(ctx && g, "null argument");
  I8IE_TRY(check_sizes(g));
  I8IE_REQUIRE(g->out_h == 0 && g->out_w == 0 && g->out_border == 0 && !g->q.s8 && !g->k.s8 && !g->v.s8 && !g->out.s8 && !g->relu &&
                   g->scores_dbg_dev == nullptr && g->probs_dbg_dev == nullptr && g->acc_dbg_dev == nullptr,
               "an INT8-only field is set");
  const int64_t per_head = (int64_t)g->tq * g->tk;
  I8IE_TRY(i8ie_ws_reserve(ctx, (size_t)g->b * per_head * sizeof(float)));
  float* ws = (float*)ctx->ws;
  for (int h = 0; h < g->heads; ++h) {
    const int64_t off = (int64_t)h * g->d;
    i8ie_bmm_args s{};   // S = Q_h K_h^T
    s.b = g->b; s.m = g->tq; s.n = g->tk; s.k = g->d;
    s.a = i8ie_bmm_mat{(float*)g->q.ptr + off, g->q.batch_stride, g->q.token_stride, 1, 0};
    s.bm = i8ie_bmm_mat{(float*)g->k.ptr + off, g->k.batch_stride, 1, g->k.token_stride, 0};
    s.out = i8ie_bmm_mat{ws, per_head, (int64_t)g->tk, 1, 0};
    I8IE_TRY(i8ie_bmm_f32(ctx, &s));
    if (g->scores_out_dev) {   // the same product again, into the caller's [b, H, tq, tk] (off the timed path)
      s.out = i8ie_bmm_mat{g->scores_out_dev + (int64_t)h * per_head, (int64_t)g->heads * per_head, (int64_t)g->tk, 1, 0};
      I8IE_TRY(i8ie_bmm_f32(ctx, &s));
    }
    I8IE_TRY(i8ie_softmax_f32(ctx, ws, ws, (int64_t)g->b * g->tq, g->tk));
    i8ie_bmm_args o{};   // O_h = P V_h
    o.b = g->b; o.m = g->tq; o.n = g->d; o.k = g->tk;
    o.a = i8ie_bmm_mat{ws, per_head, (int64_t)g->tk, 1, 0};
    o.bm = i8ie_bmm_mat{(float*)g->v.ptr + off, g->v.batch_stride, g->v.token_stride, 1, 0};
    o.out = i8ie_bmm_mat{(float*)g->out.ptr + off, g->out.batch_stride, g->out.token_stride, 1, 0};
    I8IE_TRY(i8ie_bmm_f32(ctx, &o));
  }
  return I8IE_OK;
}

int i8ie_attention_window_f32(i8ie_ctx* ctx, const i8ie_attention_args* g, const i8ie_attention_window* w) {
  I8IE_REQUIRE(ctx && g && w, "null argument");
  I8IE_TRY(check_window(g, w, true));
  I8IE_REQUIRE(w->q_border == 0 && w->k_border == 0 && w->v_border == 0 && g->out_border == 0 && !g->q.s8 && !g->k.s8 && !g->v.s8 &&
                   !g->out.s8 && !g->relu && g->scores_dbg_dev == nullptr && g->probs_dbg_dev == nullptr && g->acc_dbg_dev == nullptr,
               "an INT8-only field is set");
  const int T = g->tq, c = g->heads * g->d;
  const int nwx = w->map_w / w->win_w, nw = nwx * (w->map_h / w->win_h);
  const int64_t seqs = (int64_t)g->b * nw;
  I8IE_REQUIRE(seqs <= 0x7FFFFFFF, "too many windows");
  // the workspace: i8ie_attention_f32's scores first (its own reservation then finds room and moves nothing), then the
  // windows of q, k, v and of the result
  const size_t scores = i8ie_align_up((size_t)seqs * T * T * sizeof(float), 256);
  const int64_t dense = seqs * T * c;   // == n * c * h * w
  I8IE_TRY(i8ie_ws_reserve(ctx, scores + 4 * (size_t)dense * sizeof(float)));
  float* part = (float*)((char*)ctx->ws + scores);
  PartParams pp{dense, c, T, w->win_w, nwx, nw, w->map_w, 0, 0};
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned blocks = (unsigned)std::min<int64_t>((dense + kThreads - 1) / kThreads, 65535);
  const i8ie_attn_mat* ops[3] = {&g->q, &g->k, &g->v};
  for (int i = 0; i < 3; ++i) {
    pp.batch = ops[i]->batch_stride;
    pp.chan = ops[i]->token_stride;
    attn_part_f32_kernel<<<blocks, kThreads, 0, ctx->stream>>>((const float*)ops[i]->ptr, part + i * dense, pp, w->win_h);
    I8IE_LAUNCH_CHECK();
  }
  i8ie_attention_args a{};
  a.b = (int)seqs; a.heads = g->heads; a.d = g->d; a.tq = T; a.tk = T;
  i8ie_attn_mat* ms[4] = {&a.q, &a.k, &a.v, &a.out};
  for (int i = 0; i < 4; ++i) *ms[i] = i8ie_attn_mat{part + i * dense, (int64_t)T * c, (int64_t)c, 0};
  a.scores_out_dev = g->scores_out_dev;
  I8IE_TRY(i8ie_attention_f32(ctx, &a));
  pp.batch = g->out.batch_stride;
  pp.chan = g->out.token_stride;
  attn_unpart_f32_kernel<<<blocks, kThreads, 0, ctx->stream>>>(part + 3 * dense, (float*)g->out.ptr, pp, w->win_h);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
