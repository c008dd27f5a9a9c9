// i8ie_w4conv.hip -- k x k Conv2d (groups 1, one stride, padding and dilation) with 4-bit weights and 8-bit activations (W4A8;
// DESIGN.md section 8zc), not in the reference: the 3 x 3 layers and strided shortcuts that hold almost all weights of a CNN.
//
//   C[g][j] = sum_{ky, kx, c} A_u8[pixel(g) + (ky, kx) dil][c] * W_s4[j][c][ky][kx] + oc[j];  out = relu?(down_scale_j(C))
//
// A 4-bit k x k conv is a per-channel INT8 Conv2d whose weight integers lie in [-8, 7]: oc (src/conv2d.cc:117-124, the bias folded
// in) and the per-column requantiser (i8ie_epilogue.h, PC form) are unchanged.  The nibble fragments, their widening (nibble << 4
// as s8, sums shifted right by 4), the block tile and the quad epilogue are those of i8ie_w4pw.hip; what is new is where a row's
// bytes come from.
//
// The kernel's K order is tap major, channels minor, every tap's channels padded to 64 (i8ie_w4conv.h): a unit of 64 K values --
// one MFMA -- lies inside one tap, and the bytes it reads behind a short tap (C % 64 == 32: the next pixel's first channels, or
// zeros past the buffer) multiply zero nibbles.  A row is an output pixel g = (img, oy, ox) of all images; its bytes for unit u =
// (tap (ky, kx), channels c0 .. c0 + 63) lie at
//     base(g) + tab[u],   base(g) = ((img Hp + oy stride + b - pad) Wp + ox stride + b - pad) C,  tab[u] = (ky dil Wp + kx dil) C + c0
// in the NHWC input whose border b >= pad holds zp_in (zp_in ^ 0x80 in a re-biased map), as every NHWC producer writes it.  tab is
// uniform over pixels: the block writes it into LDS behind the stages once, one entry per unit (the idiom of ktab in
// i8ie_gconv.hip), and a DMA lane -- one 16-byte slot of one row per chunk -- adds its row's base and its slot to the entry it
// looks up.  Entries past the last unit are 0: those chunks' nibbles are zero.
//
// w4conv_mfma: a block owns 16 RT output pixels, 16 WAVES FPW features and all of K, walked in chunks of 256 (four units) through
// a ring of STAGES stages filled by LDS-DMA, slots swizzled by the row, one barrier per chunk; wave w owns its feature tiles over
// all row tiles and alone reads and widens their fragments.  MFMA halves past the last unit are skipped.  The two instances are
// w4pw_mfma's: <1, 4, 1, 4> (16 pixels x 64 features) up to kW4pwFewRows output pixels, <4, 4, 2, 2> (64 x 128) above; blocks
// are numbered feature block fastest.  Rows past M repeat row M - 1 and are not stored.
// w4conv_direct: the definition, one lane per output value, taps bounds-checked against zp_in (no border needed), NHWC or NCHW at
// either end: C % 32 != 0, NCHW operands, unaligned buffers and the force-fallback option.
// Not here (follow-up): a tile's input patch resident in LDS with the taps read as shifted fragments, as dconv_mfma does -- this
// kernel fetches every tap's bytes from L2 / HBM again.
#include "i8ie_calls.h"
#include "i8ie_epilogue.h"
#include "i8ie_internal.h"
#include "i8ie_w4conv.h"
#include "i8ie_w4lin.h"
#include "i8ie_w4pw.h"

namespace {

constexpr int kMaxTabBytes = 8192;  // c k k <= 65536 and cpad <= 2 c: at most 512 chunks of four entries

struct CvArgs {
  const uint8_t* A;  // the whole input, border included
  unsigned a_bytes;
  int C, M, N, nch;  // M: output pixels of all images; nch: chunks of the panel
  int nunits, upt;   // units of 64 K values in all, and per tap
  int k, dil, stride;
  int OW, OHW;       // output pixels per line and per image
  int Wp, HpWp;      // the physical input line and image, in pixels
  int org;           // ib - pad: where the window of output pixel (0, 0) starts
  PwSide os;
  unsigned a_xor;    // 0x80808080 for plain bytes (u8 -> s8), 0 for re-biased ones
  const uint8_t* B;  // the panel
  unsigned b_bytes;
  I8ieEpiArgs ep;    // ocp = oc + 128 * wsum; ocp, msv, sbv: [Npad]
  uint8_t* out;
  unsigned o_xor;
  int vec_out;       // N % 4 == 0 and `out` dword aligned: a whole quad is one store
};

__device__ __forceinline__ unsigned cv_base(const CvArgs& p, int g) {
  const int img = g / p.OHW, rem = g - img * p.OHW, oy = rem / p.OW, ox = rem - oy * p.OW;
  return (unsigned)(img * p.HpWp + (oy * p.stride + p.org) * p.Wp + ox * p.stride + p.org) * (unsigned)p.C;
}

template <int RT, int WAVES, int FPW, int STAGES>
__global__ __launch_bounds__(64 * WAVES) void w4conv_mfma_kernel(CvArgs p, unsigned nfb) {
  using S = PwShape<RT, WAVES, FPW, STAGES>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const unsigned fb = blockIdx.x % nfb, rb = blockIdx.x / nfb;  // feature block fastest
  const int ft0 = (int)fb * S::kFT, row0 = (int)rb * S::kRows;
  const int nch = p.nch;

  // ---- the offset table: one entry per unit of 64 K values, zeros behind the last unit
  unsigned* tab = reinterpret_cast<unsigned*>(smem + S::kLds);
  for (int u = tid; u < 4 * nch; u += S::kThreads) {
    unsigned off = 0;
    if (u < p.nunits) {
      const int t = u / p.upt, ky = t / p.k, kx = t - ky * p.k;
      off = (unsigned)(ky * p.dil * p.Wp + kx * p.dil) * (unsigned)p.C + (unsigned)(u - t * p.upt) * 64u;
    }
    tab[u] = off;
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A), 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.B), 0, p.b_bytes, 0x00020000);

  // ---- DMA pieces of a chunk: kPA of A (4 rows each; lane l: row 4 pi + (l >> 4), LDS slot l & 15, source slot s = (l & 15) ^
  //      (row & 15): unit s >> 2 of the chunk, bytes 16 (s & 3) of it), kPB of B (fragment (ft, pair) as it lies), the rest
  //      padding; wave w issues pieces w, w + WAVES, ...  A row past M repeats row M - 1 (nothing of it is stored).
  const int rot = (int)(fb % (unsigned)nch);
  unsigned src[S::kPPW], var[S::kPPW];  // var: the lane's unit inside a chunk (A) / the panel's chunk pitch (B)
#pragma unroll
  for (int j = 0; j < S::kPPW; ++j) {
    const int pi = wave + WAVES * j;
    if (pi < S::kPA) {
      const int row = 4 * pi + (lane >> 4);
      const int g = row0 + row < p.M ? row0 + row : p.M - 1;
      const int s = (lane & 15) ^ (row & 15);
      src[j] = cv_base(p, g) + (unsigned)((s & 3) * 16);
      var[j] = (unsigned)(s >> 2);
    } else {
      const int f = (pi - S::kPA) % S::kPB;  // (padding pieces: a second copy of a B piece, unused)
      src[j] = (unsigned)((ft0 + f / 2) * nch * 2 + (f & 1)) * 1024u + (unsigned)lane * 16u;
      var[j] = 2048;
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
                                                 (int)(src[j] + tab[4 * ch + (int)var[j]]), 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + pi * 1024), 16,
                                                 (int)(src[j] + (unsigned)ch * var[j]), 0, 0, 0);
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
    const int klim = (p.nunits - 4 * ch) * 64;  // K values of this chunk (uniform)
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

  // ---- the quad epilogue: lane (q, r) holds 16 C of features 4 q .. 4 q + 3 of output pixel row0 + 16 rt + r
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

// ---- w4conv_direct: the definition.  One lane per output (g, j); either side NHWC (any border) or NCHW ---------------------------
struct CvDirectArgs {
  const uint8_t* A;
  int C, H, W, ib, M, N, nch, cpad, in_nchw, out_nchw;
  int k, dil, stride, pad, OW, OHW, zp_in;
  PwSide os;
  unsigned a_xor, o_xor;  // 0x80 where that side is stored re-biased
  const uint8_t* B;
  I8ieEpiArgs ep;         // ocp here: the plain oc (the activations enter as u8)
  uint8_t* out;
};

__global__ __launch_bounds__(256) void w4conv_direct_kernel(CvDirectArgs p) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.M * p.N) return;
  const long long g = item / p.N;
  const int j = (int)(item - g * p.N);
  const long long img = g / p.OHW;
  const int rem = (int)(g - img * p.OHW), oy = rem / p.OW, ox = rem - oy * p.OW;
  const long long Wp = p.W + 2 * p.ib, Hp = p.H + 2 * p.ib;
  int sum = 0;
  for (int ky = 0; ky < p.k; ++ky)
    for (int kx = 0; kx < p.k; ++kx) {
      const int iy = oy * p.stride - p.pad + ky * p.dil, ix = ox * p.stride - p.pad + kx * p.dil;
      const bool inside = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const uint8_t* a = p.in_nchw ? p.A + (img * p.C * p.H + iy) * p.W + ix : p.A + ((img * Hp + iy + p.ib) * Wp + ix + p.ib) * p.C;
      const long long pitch = p.in_nchw ? (long long)p.H * p.W : 1;
      const int k0 = (ky * p.k + kx) * p.cpad;
      for (int c = 0; c < p.C; ++c) {
        const int v = inside ? (int)(a[c * pitch] ^ p.a_xor) : p.zp_in;
        sum += v * i8ie_w4_get(p.B, j, k0 + c, p.nch);
      }
    }
  int cv[4] = {sum, 0, 0, 0};
  uint8_t* o = p.out_nchw ? p.out + (img * p.N + j) * p.OHW + rem : p.out + pw_pixel(p.os, g) * p.N + j;
  pw_finish(p.ep, cv, i8ie_epi_cols<true>(p.ep, j, 1), 1, item, o, false, p.o_xor);
}

template <int RT, int WAVES, int FPW, int STAGES>
int cv_launch_t(i8ie_ctx* ctx, const CvArgs& a) {
  using S = PwShape<RT, WAVES, FPW, STAGES>;
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4conv_mfma_kernel<RT, WAVES, FPW, STAGES>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, S::kLds + kMaxTabBytes));
    raised[dev] = true;
  }
  const long long nfb = (a.N + S::kFeats - 1) / S::kFeats, nrb = (a.M + S::kRows - 1) / S::kRows;
  I8IE_REQUIRE(nfb * nrb < ((long long)1 << 31), "w4conv_mfma: too many blocks in one call");
  const int tab_bytes = a.nch * 16;
  I8IE_REQUIRE(tab_bytes <= kMaxTabBytes, "w4conv_mfma: offset table too large");
  w4conv_mfma_kernel<RT, WAVES, FPW, STAGES><<<(unsigned)(nfb * nrb), S::kThreads, S::kLds + tab_bytes, ctx->stream>>>(a, (unsigned)nfb);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

bool shape_ok(const I8ieW4convCall& c) {
  if (!(c.m > 0 && c.H > 0 && c.W > 0 && c.C > 0 && c.N > 0 && c.ib >= 0 && c.ob >= 0 && c.k > 0 && c.stride > 0 && c.pad >= 0 && c.dil >= 1))
    return false;
  const long long e = (long long)c.dil * (c.k - 1) + 1;
  return (long long)c.C * c.k * c.k <= 65536 && c.H + 2LL * c.pad >= e && c.W + 2LL * c.pad >= e &&
         c.OH == (int)((c.H + 2LL * c.pad - e) / c.stride) + 1 && c.OW == (int)((c.W + 2LL * c.pad - e) / c.stride) + 1 &&
         (long long)c.m * c.OH * c.OW < ((long long)1 << 31) - 64 && !(c.in_nchw && (c.ib || c.in_s8)) && !(c.out_nchw && (c.ob || c.out_s8));
}
size_t in_bytes(const I8ieW4convCall& c) { return (size_t)c.m * (c.H + 2 * c.ib) * (c.W + 2 * c.ib) * c.C; }
double algo_bytes(const I8ieW4convCall& c) {
  const double M = (double)c.m * c.OH * c.OW;
  return (double)c.m * c.H * c.W * c.C + 0.5 * c.N * c.C * c.k * c.k + M * c.N;
}

}  // namespace

void i8ie_w4conv_pack_panel(const uint8_t* packed, int n, int c, int k, uint8_t* panel) {
  const int K = c * k * k, kk = k * k, cpad = i8ie_w4conv_cpad(c), nch = i8ie_w4_chunks(kk * cpad);
  const size_t pitch = ((size_t)K + 1) / 2;
  for (int j = 0; j < n; ++j)
    for (int r = 0; r < K; ++r) {  // reference order (c, ky, kx)
      const unsigned v = (packed[j * pitch + r / 2] >> (4 * (r & 1))) & 15u;
      int hi;
      const size_t at = i8ie_w4_at(j, (r % kk) * cpad + r / kk, nch, &hi);
      panel[at] = (uint8_t)(panel[at] | (v << (4 * hi)));
    }
}

bool i8ie_w4conv_mfma_takes(const I8ieW4convCall& c) {
  const size_t limit = ((size_t)1 << 32) - 4096;  // (32-bit buffer offsets)
  return shape_ok(c) && c.C % 32 == 0 && !c.in_nchw && !c.out_nchw && c.ib >= c.pad && (reinterpret_cast<uintptr_t>(c.A) & 15u) == 0 &&
         (reinterpret_cast<uintptr_t>(c.B) & 15u) == 0 && in_bytes(c) < limit &&
         i8ie_w4_panel_bytes(c.N, i8ie_w4conv_kpanel(c.C, c.k)) < limit;
}

int i8ie_w4conv_mfma_launch(i8ie_ctx* ctx, const I8ieW4convCall& c) {
  I8IE_REQUIRE(i8ie_w4conv_mfma_takes(c), "w4conv_mfma: shape, layout, border or alignment");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf == nullptr, "w4conv_mfma: a 4-bit conv is per-feature, its bias in oc");
  const int kp = i8ie_w4conv_kpanel(c.C, c.k);
  CvArgs a{};
  a.A = c.A; a.a_bytes = (unsigned)in_bytes(c); a.C = c.C; a.M = c.m * c.OH * c.OW; a.N = c.N; a.nch = i8ie_w4_chunks(kp);
  a.nunits = kp / 64; a.upt = i8ie_w4conv_cpad(c.C) / 64;
  a.k = c.k; a.dil = c.dil; a.stride = c.stride;
  a.OW = c.OW; a.OHW = c.OH * c.OW;
  a.Wp = c.W + 2 * c.ib; a.HpWp = (c.H + 2 * c.ib) * a.Wp; a.org = c.ib - c.pad;
  a.os = pw_side(c.OH, c.OW, c.ob);
  a.a_xor = c.in_s8 ? 0u : 0x80808080u; a.o_xor = c.out_s8 ? 0x80808080u : 0u;
  a.B = c.B; a.b_bytes = (unsigned)i8ie_w4_panel_bytes(c.N, kp);
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  a.vec_out = (c.N % 4 == 0 && (reinterpret_cast<uintptr_t>(c.out) & 3u) == 0) ? 1 : 0;
  const bool few = a.M <= kW4pwFewRows;
  I8ieProfScope prof(ctx, few ? "w4conv_mfma|few" : "w4conv_mfma|many", 2.0 * a.M * c.N * c.C * c.k * c.k, algo_bytes(c));
  if (few) return cv_launch_t<1, 4, 1, 4>(ctx, a);
  return cv_launch_t<4, 4, 2, 2>(ctx, a);
}

int i8ie_w4conv_direct_launch(i8ie_ctx* ctx, const I8ieW4convCall& c) {
  I8IE_REQUIRE(shape_ok(c), "w4conv_direct: shape or layout");
  I8IE_REQUIRE(c.ep.msv != nullptr && c.ep.sbv != nullptr && c.ep.biasf == nullptr, "w4conv_direct: a 4-bit conv is per-feature, its bias in oc");
  CvDirectArgs a{};
  a.A = c.A; a.C = c.C; a.H = c.H; a.W = c.W; a.ib = c.ib; a.M = c.m * c.OH * c.OW; a.N = c.N;
  a.cpad = i8ie_w4conv_cpad(c.C); a.nch = i8ie_w4_chunks(i8ie_w4conv_kpanel(c.C, c.k));
  a.in_nchw = c.in_nchw; a.out_nchw = c.out_nchw;
  a.k = c.k; a.dil = c.dil; a.stride = c.stride; a.pad = c.pad; a.OW = c.OW; a.OHW = c.OH * c.OW;
  a.zp_in = c.zp_in;
  a.os = pw_side(c.OH, c.OW, c.ob);
  a.a_xor = c.in_s8 ? 0x80u : 0u; a.o_xor = c.out_s8 ? 0x80u : 0u;
  a.B = c.B;
  a.ep = i8ie_epi_args(c.ep);
  a.out = c.out;
  const long long items = (long long)a.M * c.N;
  I8IE_REQUIRE(items < (1LL << 39), "w4conv_direct: output too large");
  I8ieProfScope prof(ctx, "w4conv_direct", 2.0 * a.M * c.N * c.C * c.k * c.k, algo_bytes(c));
  w4conv_direct_kernel<<<(unsigned)((items + 255) / 256), 256, 0, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
