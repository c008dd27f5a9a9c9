// i8ie_matmul.hip -- quantized batched matmul of two activation tensors: i8ie_bmm_u8, i8ie_bmm_f32.
// The arithmetic and the physical descriptor are defined in include/i8ie_hip.h:
//     C[b,i,j] = sum_k (a[b,i,k] - zp_a) (b[b,k,j] - zp_b);  out = down_scale(C, s_a, s_b, s_out, zp_out), then the relu.
//
// Both operands are dynamic, so neither zero-point correction can be prepared on the host.  v_mfma_i32_16x16x64_i8 multiplies
// signed bytes, so both operands are taken to s8 by the ^0x80 re-bias (a' = a - 128 as a number); with za' = zp_a - 128,
// zb' = zp_b - 128 and P the sum of the re-biased products,
//     C = P - za' colsum_b[j] - zb' rowsum_a[i] + k za' zb',     rowsum_a[i] = sum_k a'[i,k],  colsum_b[j] = sum_k b'[k,j].
// All partial sums wrap in 32 bits; only C is guaranteed to fit (|P| <= 2^29, the sums <= 2^22, each product term <= 2^29).
//
// The host first brings every problem to one orientation: the result's contiguous axis becomes the columns (and the pixels
// of a bordered NHWC result the rows), by computing C^T = B^T A^T where needed -- an exchange of the operands' roles and of
// every pair of strides, nothing in memory.  Behind that, each operand is "rows x k" with a row stride and a k stride.
//
//   bmm_mfma    a block of 4 waves owns a 64 x 64 output tile of one batch item and walks K in steps of 64.  Both operand
//               tiles are staged into LDS as [64 rows][64 k bytes] (rows padded to 80 bytes: the 16 lanes of a ds_read_b128
//               quarter land on 16 distinct 16-byte slots), re-biased once: a plain operand is XORed while staging, a re-biased
//               one is copied.  A K-contiguous operand moves in 16-byte pieces (16 / 4 / 1 bytes per load by its strides); a
//               K-strided operand is transposed while staging, 4 x 4 bytes per lane in registers, so that every MFMA fragment
//               is a 16-byte K-contiguous LDS read.  Rows past the tile's end and the K tail are zero-filled in LDS: zero in
//               the s8 domain adds nothing to P or to the sums, and the true k goes into the constant term, so the MFMA loop
//               has no bounds test.  The row and column sums come from the same fragments by an MFMA against a fragment of
//               ones, which leaves them in exactly the accumulators' lane layout.  2 x 2 waves of 32 x 32: per K step 4
//               fragments read, 4 product MFMAs and 4 sum MFMAs.  LDS: 2 x 64 x 80 = 10 KiB.  The epilogue applies the
//               correction, stores C where asked, and requantises through i8ie_requant_pack4; 4 consecutive columns per lane
//               are one dword store where the address allows, else bytes.
//   bmm_direct  one output per lane, plain loops, the exact requantiser: k < 16, buffers that are not 16-byte aligned, and
//               everything under I8IE_OPT_FORCE_FALLBACK.  Same bytes.
//   bmm_f32     one output per lane, products added in ascending k (off the timed path).
#include <cmath>

#include "i8ie_bmm_tile.h"
#include "i8ie_internal.h"
#include "i8ie_pointwise.h"
#include "i8ie_requant.h"

namespace {

constexpr int kMaxK = 32768;
// (the block tile TM, TN, TK, LROW, the operand BmmOp and stage_tile live in i8ie_bmm_tile.h: attn_mfma stages with them too)
struct BmmParams {
  BmmOp A, B;           // rows of A are the result's rows, rows of B its columns
  int M, N, K, tiles_m, tiles_n;
  uint8_t* out;
  int64_t o_batch, o_row, o_col;
  uint32_t xout;
  int pix_w, pix_pad;   // rows are pixels of a bordered map: physical row index = i + (i / pix_w) * pix_pad (pix_pad = 2B, 0: plain)
  int32_t* acc;
  int64_t acc_batch, acc_row, acc_col;
  I8ieRequant rq;
  int lo;
};

__device__ __forceinline__ int64_t out_row_index(const BmmParams& p, int i) {
  return p.pix_pad ? (int64_t)i + (int64_t)(i / p.pix_w) * p.pix_pad : (int64_t)i;
}

__global__ __launch_bounds__(256) void bmm_mfma_kernel(BmmParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * TM * LROW];
  uint8_t* As = lds;
  uint8_t* Bs = lds + TM * LROW;
  const int per_batch = p.tiles_m * p.tiles_n;
  const int batch = blockIdx.x / per_batch, tile = blockIdx.x - batch * per_batch;
  const int m0 = (tile / p.tiles_n) * TM, n0 = (tile % p.tiles_n) * TN;
  const uint8_t* Ab = p.A.p + (int64_t)batch * p.A.batch;
  const uint8_t* Bb = p.B.p + (int64_t)batch * p.B.batch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, r = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;

  v4i acc[2][2], rsum[2], csum[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    rsum[i] = v4i{0, 0, 0, 0};
    csum[i] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v4i{0, 0, 0, 0};
  }
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};

  for (int k0 = 0; k0 < p.K; k0 += TK) {
    stage_tile(p.A, Ab, p.M, p.K, m0, k0, As);
    stage_tile(p.B, Bb, p.N, p.K, n0, k0, Bs);
    __syncthreads();
    v4i a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i] = *reinterpret_cast<const v4i*>(As + (wm * 32 + i * 16 + r) * LROW + 16 * q);
      b[i] = *reinterpret_cast<const v4i*>(Bs + (wn * 32 + i * 16 + r) * LROW + 16 * q);
    }
    // with B's fragment as srcA, lane (q, r) receives columns 4q .. 4q + 3 of row r; the sums arrive in the same layout
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

  const uint32_t za = (uint32_t)(p.A.zp - 128), zb = (uint32_t)(p.B.zp - 128);
  const uint32_t kzz = (uint32_t)p.K * za * zb;
  const float lof = (float)p.lo;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + wm * 32 + mi * 16 + r;
    if (m >= p.M) continue;
    uint8_t* orow = p.out + (int64_t)batch * p.o_batch + out_row_index(p, m) * p.o_row;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int nb = n0 + wn * 32 + ni * 16 + 4 * q;
      if (nb >= p.N) continue;
      int c[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        c[e] = (int)((uint32_t)acc[mi][ni][e] - za * (uint32_t)csum[ni][e] - zb * (uint32_t)rsum[mi][e] + kzz);
      if (p.acc) {
        int32_t* ap = p.acc + (int64_t)batch * p.acc_batch + (int64_t)m * p.acc_row + (int64_t)nb * p.acc_col;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (nb + e < p.N) ap[(int64_t)e * p.acc_col] = c[e];
      }
      const uint32_t packed = i8ie_requant_pack4(c, p.rq, p.lo, lof) ^ p.xout;
      uint8_t* op = orow + (int64_t)nb * p.o_col;
      if (p.o_col == 1 && nb + 4 <= p.N && (reinterpret_cast<uintptr_t>(op) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(op) = packed;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (nb + e < p.N) op[(int64_t)e * p.o_col] = (uint8_t)(packed >> (8 * e));
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void bmm_direct_kernel(BmmParams p, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const uint32_t xa = (p.A.x & 0xFFu) ^ 0x80u, xb = (p.B.x & 0xFFu) ^ 0x80u;  // to plain bytes
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int n = (int)(e % p.N);
    const int64_t t = e / p.N;
    const int m = (int)(t % p.M);
    const int64_t batch = t / p.M;
    const uint8_t* a = p.A.p + batch * p.A.batch + (int64_t)m * p.A.rs;
    const uint8_t* b = p.B.p + batch * p.B.batch + (int64_t)n * p.B.rs;
    uint32_t sum = 0;
    for (int k = 0; k < p.K; ++k) {
      const int av = (int)((uint32_t)a[(int64_t)k * p.A.ks] ^ xa) - p.A.zp;
      const int bv = (int)((uint32_t)b[(int64_t)k * p.B.ks] ^ xb) - p.B.zp;
      sum += (uint32_t)(av * bv);
    }
    const int c = (int)sum;
    if (p.acc) p.acc[batch * p.acc_batch + (int64_t)m * p.acc_row + (int64_t)n * p.acc_col] = c;
    const int qv = i8ie_requant_exact((float)c, p.rq, p.lo);
    p.out[batch * p.o_batch + out_row_index(p, m) * p.o_row + (int64_t)n * p.o_col] = (uint8_t)((uint32_t)qv ^ (p.xout & 0xFFu));
  }
}

struct BmmF32Params {
  const float *a, *b;
  float* out;
  int64_t a_batch, a_row, a_col, b_batch, b_row, b_col, o_batch, o_row, o_col;
  int M, N, K;
};
__global__ __launch_bounds__(kThreads) void bmm_f32_kernel(BmmF32Params p, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int n = (int)(e % p.N);
    const int64_t t = e / p.N;
    const int m = (int)(t % p.M);
    const int64_t batch = t / p.M;
    const float* a = p.a + batch * p.a_batch + (int64_t)m * p.a_row;
    const float* b = p.b + batch * p.b_batch + (int64_t)n * p.b_col;
    float sum = 0.0f;
    for (int k = 0; k < p.K; ++k) sum += a[(int64_t)k * p.a_col] * b[(int64_t)k * p.b_row];
    p.out[batch * p.o_batch + (int64_t)m * p.o_row + (int64_t)n * p.o_col] = sum;
  }
}

bool mat_ok(const i8ie_bmm_mat& m) {
  return m.ptr != nullptr && m.batch_stride >= 0 && m.row_stride >= 0 && m.col_stride >= 0 && (m.row_stride == 1 || m.col_stride == 1);
}
bool fits31(const i8ie_bmm_mat& m) { return m.batch_stride <= 0x7FFFFFFF && m.row_stride <= 0x7FFFFFFF && m.col_stride <= 0x7FFFFFFF; }

// bytes per load along an operand's contiguous axis: every other stride must keep the pieces aligned
int op_vec(const BmmOp& o) {
  const int64_t other = o.ks == 1 ? o.rs : o.ks;
  if (o.ks == 1 && other % 16 == 0 && o.batch % 16 == 0) return 16;
  if (other % 4 == 0 && o.batch % 4 == 0) return 4;
  return 1;
}

}  // namespace

extern "C" {

int i8ie_bmm_u8(i8ie_ctx* ctx, const i8ie_bmm_args* g) {
  I8IE_REQUIRE(ctx && g, "null argument");
  I8IE_REQUIRE(g->b > 0 && g->m > 0 && g->n > 0 && g->k > 0, "non-positive size");
  I8IE_REQUIRE(g->k <= kMaxK, "k > 32768: the int32 sum could overflow");
  I8IE_REQUIRE(mat_ok(g->a) && mat_ok(g->bm) && mat_ok(g->out), "null pointer, negative stride, or neither stride of a matrix is 1");
  I8IE_REQUIRE(g->b == 1 || g->out.batch_stride > 0, "the result's batch_stride is 0: its batch items would share their bytes");
  I8IE_REQUIRE(scales_ok(g->s_a, g->s_b, g->s_out), "scales must be finite and s_out > 0");
  I8IE_REQUIRE(g->out_pix_axis >= 0 && g->out_pix_axis <= 2, "out_pix_axis must be 0, 1 or 2");
  I8IE_REQUIRE((int64_t)g->b * g->m * g->n <= 0x7FFFFFFFFFFFll / 4, "too many outputs");
  bool swap = g->out.col_stride != 1;
  int pix_w = 1, pix_pad = 0;
  int64_t origin = 0;
  if (g->out_pix_axis != 0) {
    I8IE_REQUIRE(g->out_h > 0 && g->out_w > 0 && g->out_border >= 0, "bad pixel geometry");
    I8IE_REQUIRE((int64_t)g->out_h * g->out_w == (g->out_pix_axis == 1 ? g->m : g->n), "the pixel axis is not out_h * out_w long");
    I8IE_REQUIRE((g->out_pix_axis == 1 ? g->out.col_stride : g->out.row_stride) == 1, "the channel axis of an NHWC result must have stride 1");
    swap = g->out_pix_axis == 2;
    const int64_t c = g->out_pix_axis == 1 ? g->out.row_stride : g->out.col_stride;
    pix_w = g->out_w;
    pix_pad = 2 * g->out_border;
    origin = ((int64_t)g->out_border * (g->out_w + 2 * g->out_border) + g->out_border) * c;
  }
  BmmParams p;
  const i8ie_bmm_mat &ma = g->a, &mb = g->bm;
  BmmOp opa{(const uint8_t*)ma.ptr, ma.batch_stride, ma.row_stride, ma.col_stride, ma.s8 ? 0u : 0x80808080u, 1, (int)g->zp_a};
  BmmOp opb{(const uint8_t*)mb.ptr, mb.batch_stride, mb.col_stride, mb.row_stride, mb.s8 ? 0u : 0x80808080u, 1, (int)g->zp_b};
  opa.vec = op_vec(opa);
  opb.vec = op_vec(opb);
  p.A = swap ? opb : opa;
  p.B = swap ? opa : opb;
  p.M = swap ? g->n : g->m;
  p.N = swap ? g->m : g->n;
  p.K = g->k;
  p.tiles_m = (p.M + TM - 1) / TM;
  p.tiles_n = (p.N + TN - 1) / TN;
  p.out = (uint8_t*)g->out.ptr + origin;
  p.o_batch = g->out.batch_stride;
  p.o_row = swap ? g->out.col_stride : g->out.row_stride;
  p.o_col = swap ? g->out.row_stride : g->out.col_stride;
  p.xout = g->out.s8 ? 0x80808080u : 0u;
  p.pix_w = pix_w;
  p.pix_pad = pix_pad;
  p.acc = g->acc_dbg_dev;
  p.acc_batch = (int64_t)g->m * g->n;
  p.acc_row = swap ? 1 : g->n;
  p.acc_col = swap ? g->n : 1;
  p.rq = i8ie_make_requant(g->s_a, g->s_b, g->s_out, (int)g->zp_out);
  p.lo = g->relu ? (int)g->zp_out : 0;
  const bool aligned = aligned_to(ma.ptr, 16) && aligned_to(mb.ptr, 16) && aligned_to(g->out.ptr, 16) &&
                       (g->acc_dbg_dev == nullptr || aligned_to(g->acc_dbg_dev, 4));
  const int64_t blocks = (int64_t)g->b * p.tiles_m * p.tiles_n;
  const bool mfma = (ctx->options & 1) == 0 && g->k >= 16 && aligned && fits31(ma) && fits31(mb) && fits31(g->out) && blocks <= 0x7FFFFFFF;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const double outs = (double)g->b * g->m * g->n;
  I8ieProfScope prof(ctx, mfma ? "bmm_mfma" : "bmm_direct", 2.0 * outs * g->k, (double)g->b * g->k * ((double)g->m + g->n) + outs);
  if (mfma) {
    bmm_mfma_kernel<<<(unsigned)blocks, 256, 0, ctx->stream>>>(p);
  } else {
    const int64_t total = (int64_t)g->b * g->m * g->n;
    bmm_direct_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(p, total);
  }
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_bmm_f32(i8ie_ctx* ctx, const i8ie_bmm_args* g) {
  I8IE_REQUIRE(ctx && g, "null argument");
  I8IE_REQUIRE(g->b > 0 && g->m > 0 && g->n > 0 && g->k > 0, "non-positive size");
  I8IE_REQUIRE(mat_ok(g->a) && mat_ok(g->bm) && mat_ok(g->out), "null pointer, negative stride, or neither stride of a matrix is 1");
  I8IE_REQUIRE(g->b == 1 || g->out.batch_stride > 0, "the result's batch_stride is 0: its batch items would share their bytes");
  I8IE_REQUIRE(g->out_pix_axis == 0 && g->acc_dbg_dev == nullptr && !g->a.s8 && !g->bm.s8 && !g->out.s8, "an INT8-only field is set");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  BmmF32Params p;
  p.a = (const float*)g->a.ptr; p.b = (const float*)g->bm.ptr; p.out = (float*)g->out.ptr;
  p.a_batch = g->a.batch_stride; p.a_row = g->a.row_stride; p.a_col = g->a.col_stride;
  p.b_batch = g->bm.batch_stride; p.b_row = g->bm.row_stride; p.b_col = g->bm.col_stride;
  p.o_batch = g->out.batch_stride; p.o_row = g->out.row_stride; p.o_col = g->out.col_stride;
  p.M = g->m; p.N = g->n; p.K = g->k;
  const int64_t total = (int64_t)g->b * g->m * g->n;
  I8ieProfScope prof(ctx, "bmm_f32", 0.0, 4.0 * ((double)g->b * g->k * ((double)g->m + g->n) + (double)total));
  bmm_f32_kernel<<<grid_for(total), kThreads, 0, ctx->stream>>>(p, total);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
