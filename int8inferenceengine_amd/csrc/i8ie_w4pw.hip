// i8ie_w4pw.hip -- pointwise (1 x 1, stride 1) Conv2d with 4-bit weights and 8-bit activations (W4A8), not
// in the reference: the qkv / proj / MLP layers that the transformer examples write as 1 x 1 convolutions on NHWC token maps.
//
//   C[g][j] = sum_c A_u8[g][c] * W_s4[j][c] + oc[j];  out = relu?(down_scale_j(C))       g: a pixel of any image, oc: with the bias
//
// A 4-bit pointwise conv is a per-channel INT8 Conv2d whose weight integers lie in [-8, 7]: oc (src/conv2d.cc:117-124) and the
// per-column requantiser (i8ie_epilogue.h, PC form) are unchanged.  The weights are the nibble panel of i8ie_w4lin.hip -- one
// 16-byte read is a lane's operand of two v_mfma_i32_16x16x64_i8, the MFMA gets nibble << 4 as s8 and the sums are shifted right
// by 4 -- and what is new is the map at both ends and the block tile.
//
// The map.  A pixel is a row of C contiguous bytes; pixel g of the m H W pixels lies at physical pixel
//     img (H + 2 b)(W + 2 b) + (y + b)(W + 2 b) + x + b        b: the border its neighbour keeps (pw_pixel below)
// so a row is addressed per pixel and a border byte is never read as a pixel's channel: the 1 x 1 window needs no padding, and
// the border of the output belongs to the caller (i8ie_fill_border_u8), as for every NHWC producer.  Bytes stored re-biased
// (^0x80) enter the MFMA as they are -- the kernel computes with a - 128 anyway, the term 128 * wsum[j] is in ocp -- and a
// consumer that reads re-biased bytes gets the packed quad ^0x80808080.
//
// w4pw_mfma: a block owns 16 RT pixels, 16 FT = 16 WAVES FPW features and all of K.  K is walked in the panel's chunks of 256;
// per chunk the block's 16 RT activation rows (256 bytes each, 16-byte slots swizzled by the row as in i8ie_flin.hip) and the
// 2 FT fragments of its feature tiles arrive by LDS-DMA in a ring of STAGES chunks, one barrier per chunk.  Wave w owns feature
// tiles FPW w .. FPW w + FPW - 1 and ALL row tiles: it alone reads its fragments from LDS and widens them, once per block and
// chunk, in registers (two vector operations per four weights); an activation fragment read from LDS meets FPW weight
// fragments.  A chunk's MFMAs past K are skipped (K = 192: three of four).
//   <1, 4, 1, 4>  up to kW4pwFewRows pixels: 16 pixels x 64 features, 12 KiB per chunk of which 8 are nibbles, 4 stages
//                 (48 KiB: three blocks per CU) -- a stream over the panel by many small blocks, as w4lin_mfma's few-row shape
//   <4, 4, 2, 2>  more pixels: 64 pixels x 128 features, 32 KiB per chunk, half activations and half nibbles, 2 stages (64 KiB:
//                 two blocks per CU).  A block's activations are fetched once per 128 features (w4lin_mfma: 32) and a 16-byte
//                 activation read from LDS feeds two MFMAs per wave, so the panel costs a block as many bytes as the map does.
// Blocks are numbered feature block fastest: the blocks that share 64 pixels run side by side and find them in L2.
// w4pw_direct: the definition, one lane per output value, NHWC or NCHW at either end: C % 32 != 0, NCHW operands, unaligned
// buffers and the force-fallback option.
#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_w4lin.h"
#include "i8ie_w4pw.h"

namespace {

struct PwArgs {
  const uint8_t* A;  // the whole input, border included
  unsigned a_bytes;
  int C, M, N, nch;  // M: pixels of all images
  PwSide in, os;
  unsigned a_xor;    // 0x80808080 for plain bytes (u8 -> s8), 0 for re-biased ones
  const uint8_t* B;  // the panel
  unsigned b_bytes;
  I8ieEpiArgs ep;    // ocp = oc + 128 * wsum; ocp, msv, sbv: [Npad]
  uint8_t* out;
  unsigned o_xor;
  int vec_out;       // N % 4 == 0 and `out` dword aligned: a whole quad is one store
};

template <int RT, int WAVES, int FPW, int STAGES>
__global__ __launch_bounds__(64 * WAVES) void w4pw_mfma_kernel(PwArgs p, unsigned nfb) {
  using S = PwShape<RT, WAVES, FPW, STAGES>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const unsigned fb = blockIdx.x % nfb, rb = blockIdx.x / nfb;  // feature block fastest
  const int ft0 = (int)fb * S::kFT, row0 = (int)rb * S::kRows;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A), 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a chunk: kPA of A (4 pixels each; lane l: row 4 pi + (l >> 4), LDS slot l & 15, source slot
  //      (l & 15) ^ (row & 15)), kPB of B (fragment (ft, pair) as it lies), the rest padding; wave w issues pieces w, w + WAVES, ...
  //      A row past M repeats pixel M - 1 (nothing of it is stored).  A chunk past C (C % 256 != 0) reads the bytes behind the
  //      pixel or, past the buffer, zeros, and so does a feature tile past the panel: the panel holds zero nibbles there.
  const int nch = p.nch;
  const int rot = (int)(fb % (unsigned)nch);
  unsigned src[S::kPPW], step_bytes[S::kPPW];
#pragma unroll
  for (int j = 0; j < S::kPPW; ++j) {
    const int pi = wave + WAVES * j;
    if (pi < S::kPA) {
      const int row = 4 * pi + (lane >> 4);
      const int g = row0 + row < p.M ? row0 + row : p.M - 1;
      src[j] = (unsigned)(pw_pixel(p.in, g) * p.C) + (unsigned)(((lane & 15) ^ (row & 15)) * 16);
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
      const int pi = wave + WAVES * j;
      if (pi < S::kPA)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16,
                                                 (int)(src[j] + (unsigned)ch * step_bytes[j]), 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16,
                                                 (int)(src[j] + (unsigned)ch * step_bytes[j]), 0, 0, 0);
    }
  };

  v4i acc[RT][FPW];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int f = 0; f < FPW; ++f) acc[rt][f] = v4i{0, 0, 0, 0};
  const int bfrag = S::kStageA + wave * FPW * 2048 + lane * 16;  // fragment (first tile of this wave, pair 0) of a stage
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i) issue(nch > i ? i : 0);
  for (int step = 0; step < nch; ++step) {
    // my pieces of this chunk (the STAGES - 2 chunks after it may be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * S::kPPW) : "memory");
    asm volatile("s_barrier" ::: "memory");  // everyone's pieces; everyone is done with the previous chunk
    issue(step + STAGES - 1);  // -> the stage of the previous chunk (past the end the walk wraps: keeps the vmcnt counts uniform)
    const uint8_t* st = smem + (step % STAGES) * S::kStage;
    const int ch = step + rot < nch ? step + rot : step + rot - nch;
    const int klim = p.C - ch * kChunk;  // K values of this chunk (uniform)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      if (128 * pr >= klim) break;
      const bool high = 128 * pr + 64 < klim;
      v4i b_lo[FPW], b_hi[FPW];
#pragma unroll
      for (int f = 0; f < FPW; ++f) {  // 32 nibbles -> nibble << 4 as s8, here and nowhere else in the block
        const v4i x = *reinterpret_cast<const v4i*>(st + bfrag + f * 2048 + pr * 1024);
        b_lo[f] = (x << 4) & (int)0xF0F0F0F0;
        b_hi[f] = x & (int)0xF0F0F0F0;
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const uint8_t* arow = st + (rt * 16 + lr) * kChunk;  // slot s of row r at (s ^ r) * 16
        const v4i a_lo = *reinterpret_cast<const v4i*>(arow + ((8 * pr + lq) ^ lr) * 16) ^ (int)p.a_xor;
#pragma unroll
        for (int f = 0; f < FPW; ++f) acc[rt][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_lo[f], a_lo, acc[rt][f], 0, 0, 0);
        if (high) {
          const v4i a_hi = *reinterpret_cast<const v4i*>(arow + ((8 * pr + 4 + lq) ^ lr) * 16) ^ (int)p.a_xor;
#pragma unroll
          for (int f = 0; f < FPW; ++f) acc[rt][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b_hi[f], a_hi, acc[rt][f], 0, 0, 0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wrapped pieces: nothing may land after the block is gone)

  // ---- the quad epilogue: lane (q, r) holds 16 C of features 4 q .. 4 q + 3 of pixel row0 + 16 rt + r
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int g = row0 + rt * 16 + lr;
    if (g >= p.M) continue;
    const long long opix = pw_pixel(p.os, g);
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
      const int n = (ft0 + wave * FPW + f) * 16 + 4 * lq;
      if (n >= p.N) continue;
      int cv[4] = {acc[rt][f].x >> 4, acc[rt][f].y >> 4, acc[rt][f].z >> 4, acc[rt][f].w >> 4};
      const int nf = p.N - n < 4 ? p.N - n : 4;
      // (n < N <= Npad, n % 4 == 0: the quad lies inside the padded arrays)
      pw_finish(p.ep, cv, i8ie_epi_cols_vec<true>(p.ep, n), nf, (long long)g * p.N + n, p.out + opix * p.N + n,
                p.vec_out && nf == 4, p.o_xor);
    }
  }
}

// ---- w4pw_direct: the definition.  One lane per output (g, j); either side NHWC (any border) or NCHW ----------------------------
struct PwDirectArgs {
  const uint8_t* A;
  int C, M, N, nch, in_nchw, out_nchw;
  PwSide in, os;
  unsigned a_xor, o_xor;  // 0x80 where that side is stored re-biased
  const uint8_t* B;
  I8ieEpiArgs ep;         // ocp here: the plain oc (the activations enter as u8)
  uint8_t* out;
};

__global__ __launch_bounds__(256) void w4pw_direct_kernel(PwDirectArgs p) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.M * p.N) return;
  const long long g = item / p.N;
  const int j = (int)(item - g * p.N);
  const long long img = g / p.in.HW, rem = g - img * p.in.HW;
  const uint8_t* a = p.in_nchw ? p.A + img * p.C * p.in.HW + rem : p.A + pw_pixel(p.in, g) * p.C;
  const long long pitch = p.in_nchw ? p.in.HW : 1;
  int sum = 0;
  for (int k = 0; k < p.C; ++k) sum += (int)(a[k * pitch] ^ p.a_xor) * i8ie_w4_get(p.B, j, k, p.nch);
  int cv[4] = {sum, 0, 0, 0};
  uint8_t* o = p.out_nchw ? p.out + (img * p.N + j) * p.os.HW + rem : p.out + pw_pixel(p.os, g) * p.N + j;
  pw_finish(p.ep, cv, i8ie_epi_cols<true>(p.ep, j, 1), 1, item, o, false, p.o_xor);
}

template <int RT, int WAVES, int FPW, int STAGES>
int pw_launch_t(i8ie_ctx* ctx, const PwArgs& a) {
  using S = PwShape<RT, WAVES, FPW, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4pw_mfma_kernel<RT, WAVES, FPW, STAGES>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kLds));
    raised[dev] = true;
  }
  const long long nfb = (a.N + S::kFeats - 1) / S::kFeats, nrb = (a.M + S::kRows - 1) / S::kRows;
  I8IE_REQUIRE(nfb * nrb < ((long long)1 << 31), "w4pw_mfma: too many blocks in one call");
  w4pw_mfma_kernel<RT, WAVES, FPW, STAGES><<<(unsigned)(nfb * nrb), S::kThreads, S::kLds, ctx->stream>>>(a, (unsigned)nfb);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

bool shape_ok(const I8ieW4pwCall& c) {
  return c.m > 0 && c.H > 0 && c.W > 0 && c.C > 0 && c.C <= 65536 && c.N > 0 && c.ib >= 0 && c.ob >= 0 &&
         (long long)c.m * c.H * c.W < ((long long)1 << 31) - 64 && !(c.in_nchw && (c.ib || c.in_s8)) && !(c.out_nchw && (c.ob || c.out_s8));
}
size_t in_bytes(const I8ieW4pwCall& c) { return (size_t)c.m * (c.H + 2 * c.ib) * (c.W + 2 * c.ib) * c.C; }
double algo_bytes(const I8ieW4pwCall& c) {
  const double M = (double)c.m * c.H * c.W;
  return M * c.C + 0.5 * c.N * c.C + M * c.N;
}

}  // namespace

bool i8ie_w4pw_mfma_takes(const I8ieW4pwCall& c) {
  const size_t limit = ((size_t)1 << 32) - 4096;  // (32-bit buffer offsets)
  return shape_ok(c) && c.C % 32 == 0 && !c.in_nchw && !c.out_nchw && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 &&
         (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0 && in_bytes(c) < limit && i8ie_w4_panel_bytes(c.N, c.C) < limit;
}

int i8ie_w4pw_mfma_launch(i8ie_ctx* ctx, const I8ieW4pwCall& c) {
  I8IE_REQUIRE(i8ie_w4pw_mfma_takes(c), "w4pw_mfma: shape, layout or alignment");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf == nullptr, "w4pw_mfma: a 4-bit conv is per-feature, its bias in oc");
  PwArgs a{};
  a.A = c.A; a.a_bytes = (unsigned)in_bytes(c); a.C = c.C; a.M = c.m * c.H * c.W; a.N = c.N; a.nch = i8ie_w4_chunks(c.C);
  a.in = pw_side(c.H, c.W, c.ib); a.os = pw_side(c.H, c.W, c.ob);
  a.a_xor = c.in_s8 ? 0u : 0x80808080u; a.o_xor = c.out_s8 ? 0x80808080u : 0u;
  a.B = c.B; a.b_bytes = (unsigned)i8ie_w4_panel_bytes(c.N, c.C);
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  a.vec_out = (c.N % 4 == 0 && (reinterpret_cast<uintptr_t>(c.out) & 3u) == 0) ? 1 : 0;
  const bool few = a.M <= kW4pwFewRows;
  I8ieProfScope prof(ctx, few ? "w4pw_mfma|few" : "w4pw_mfma|many", 2.0 * a.M * c.N * c.C, algo_bytes(c));
  if (few) return pw_launch_t<1, 4, 1, 4>(ctx, a);
  return pw_launch_t<4, 4, 2, 2>(ctx, a);
}

int i8ie_w4pw_direct_launch(i8ie_ctx* ctx, const I8ieW4pwCall& c) {
  I8IE_REQUIRE(shape_ok(c), "w4pw_direct: shape or layout");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf == nullptr, "w4pw_direct: a 4-bit conv is per-feature, its bias in oc");
  PwDirectArgs a{};
  a.A = c.A; a.C = c.C; a.M = c.m * c.H * c.W; a.N = c.N; a.nch = i8ie_w4_chunks(c.C);
  a.in_nchw = c.in_nchw; a.out_nchw = c.out_nchw;
  a.in = pw_side(c.H, c.W, c.ib); a.os = pw_side(c.H, c.W, c.ob);
  a.a_xor = c.in_s8 ? 0x80u : 0u; a.o_xor = c.out_s8 ? 0x80u : 0u;
  a.B = c.B;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)a.M * c.N;
  I8IE_REQUIRE(items < (1LL << 39), "w4pw_direct: output too large");
  I8ieProfScope prof(ctx, "w4pw_direct", 2.0 * a.M * c.N * c.C, algo_bytes(c));
  w4pw_direct_kernel<<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
