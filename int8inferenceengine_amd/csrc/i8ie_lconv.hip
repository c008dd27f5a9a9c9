// i8ie_lconv.hip -- dense 1 x k and k x 1 Conv2d at stride 1, dilation 1, in INT8 (Conv2d with pair arguments, groups = 1; DESIGN.md
// section 8p): the factorised 7 x 7 and 3 x 3 convolutions of the Inception B / C / E blocks.
//   reference: src/conv2d.cc:100-142 with the kernel embedded in a square of zeros; rectangular kernels: not in the reference
//
// In NHWC both orientations are one problem, a convolution along a LINE of pixels: an image row at pixel pitch C bytes for
// 1 x k, an image column at pixel pitch Wp C bytes for k x 1, every pixel at least 16 contiguous bytes of a channel chunk.  The
// two differ in two address patterns (the staging load, the output store) and nowhere else; nothing is transposed.
//   rows    the output pixels of all lines of all images, numbered line by line (line = (image, row) for 1 x k, (image, column)
//           for k x 1), are cut into runs of 128: a block's 128 MFMA rows are the pixels g0 .. g0 + 127 of that numbering, so they
//           come from as many lines as it takes (a 17-pixel line fills 17 rows, not two 16-row slots) of any images
//   LDS     the block stages every line it touches whole and padded, Lo + k - 1 pixels by one channel chunk of CC <= 64 bytes (pixel
//           pitch CC + 16: neighbouring pixels start in different banks), out-of-image positions filled with zp_in, every byte
//           re-biased ^0x80 once on the way (the term 128 * wsum[j] is in ocp)
//   K       walked as (channel chunk, tap, channel): the A fragment of tap t for line pixel x is the LDS bytes of pixel x + t, so a
//           staged byte is used k times from LDS and the K loop has no bounds test
//   wave    16 features by all 128 rows: a weight fragment, read coalesced (16 bytes per lane) from route G's panel [Ngp][Kgp],
//           K ordered (tap, c), once per block and K step, meets 8 A fragments
// Accumulation is exact INT32, the epilogue the quad epilogue of i8ie_epilogue.h (per-tensor and per-channel instances) with the
// optional ReLU clamp, the border the consumer asks for and the INT32 sums on request.
#include "i8ie_internal.h"
#include "i8ie_epilogue.h"
#include "i8ie_lconv.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int ROWS = 128, SLOTS = ROWS / 16;

struct LconvArgs {
  const uint8_t* A;
  int H, W, C, ib, OH, OW;
  int vert;               // 0: 1 x k, lines are image rows; 1: k x 1, lines are image columns
  int k, pl, pc;          // taps; padding along the line and across it
  int Lo, LP, NL;         // output pixels of a line; staged pixels of a line, Lo + k - 1; lines per image
  long long M, lines;     // m * NL * Lo output pixels, m * NL lines
  int N, Kgp, CC, PCH;    // CC: channel chunk, a multiple of 16 dividing C; PCH = CC + 16: the pixel pitch in LDS
  const int8_t* Bp;
  I8ieEpiArgs ep;
  int zp_in;
  uint8_t* out;
  int ob, vec_out;
};

template <bool PC>
__global__ __launch_bounds__(256) void lconv_mfma_kernel(LconvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lines[];  // [lines of this block][LP][PCH], re-biased
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
  const long long g0 = (long long)blockIdx.x * ROWS;
  const long long glast = g0 + ROWS - 1 < p.M - 1 ? g0 + ROWS - 1 : p.M - 1;
  const long long l0 = g0 / p.Lo;
  const int nl = (int)(glast / p.Lo - l0) + 1;  // the lines this block touches
  const int f0 = blockIdx.y * 64 + 16 * wave;   // this wave's 16 features
  const bool active = f0 < p.N;                 // (an idle wave still stages lines and meets the barriers)
  const int Hp = p.H + 2 * p.ib, Wp = p.W + 2 * p.ib, CU = p.CC >> 4;
  const int8_t* brow = p.Bp + (size_t)(active ? f0 + lr : 0) * p.Kgp;
  const int KC = p.k * p.CC;                    // K bytes of one chunk

  // this lane's row of each slot: the LDS offset of its line pixel (tap 0)
  int rowoff[SLOTS];
#pragma unroll
  for (int mi = 0; mi < SLOTS; ++mi) {
    const long long g = g0 + 16 * mi + lr;
    const long long l = g / p.Lo;
    rowoff[mi] = g < p.M ? ((int)(l - l0) * p.LP + (int)(g - l * p.Lo)) * p.PCH : 0;  // (spare rows redo pixel 0 and store nothing)
  }
  v4i acc[SLOTS];
#pragma unroll
  for (int mi = 0; mi < SLOTS; ++mi) acc[mi] = v4i{0, 0, 0, 0};

  for (int c0 = 0; c0 < p.C; c0 += p.CC) {
    __syncthreads();  // everyone is done with the previous chunk
    for (int idx = threadIdx.x; idx < nl * p.LP * CU; idx += 256) {
      const int ll = idx / (p.LP * CU), rem = idx - ll * (p.LP * CU), s = rem / CU, e = rem - s * CU;
      const long long l = l0 + ll;  // (< p.lines: the block's last row lies on it)
      const long long img = l / p.NL;
      const int across = (int)(l - img * p.NL) - p.pc + p.ib, along = s - p.pl + p.ib;
      const int y = p.vert ? along : across, x = p.vert ? across : along;
      const int zp4 = (int)((uint32_t)p.zp_in * 0x01010101u);
      v4i val = {zp4, zp4, zp4, zp4};
      if ((unsigned)y < (unsigned)Hp && (unsigned)x < (unsigned)Wp)
        val = *reinterpret_cast<const v4i*>(p.A + ((img * Hp + y) * Wp + x) * p.C + c0 + 16 * e);
      *reinterpret_cast<v4i*>(lines + (size_t)(ll * p.LP + s) * p.PCH + 16 * e) = val ^ (int)0x80808080;  // u8 -> s8, once
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < KC; j += 64) {
      const int kk = j + 16 * lq;
      const bool on = kk < KC;  // (the chunk's K tail: not a bounds test of a tap)
      const int tap = on ? kk / p.CC : 0, ch = on ? kk - tap * p.CC : 0;
      v4i b = {0, 0, 0, 0};
      if (on) b = *reinterpret_cast<const v4i*>(brow + (size_t)tap * p.C + c0 + ch);
      const uint8_t* arow = lines + tap * p.PCH + ch;
#pragma unroll
      for (int mi = 0; mi < SLOTS; ++mi) {
        v4i a = {0, 0, 0, 0};
        if (on) a = *reinterpret_cast<const v4i*>(arow + rowoff[mi]);
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
    const long long g = g0 + 16 * mi + lr;
    if (g >= p.M) continue;
    const long long l = g / p.Lo, img = l / p.NL;
    const int along = (int)(g - l * p.Lo), across = (int)(l - img * p.NL);
    const int oy = p.vert ? along : across, ox = p.vert ? across : along;
    int c[4] = {acc[mi].x, acc[mi].y, acc[mi].z, acc[mi].w};
    const long long px = (img * p.OH + oy) * p.OW + ox;
    const long long opix = (img * (p.OH + 2 * p.ob) + oy + p.ob) * (p.OW + 2 * p.ob) + ox + p.ob;
    i8ie_epi_finish<PC>(p.ep, c, cols, nf, px * p.N + f, p.out + opix * p.N + f, p.vec_out && nf == 4);
  }
}

// the channel chunk: all of C up to 64, else the largest of 64 / 32 / 16 dividing C
int chunk_of(int C) { return C <= 64 ? C : (C % 64 == 0 ? 64 : (C % 32 == 0 ? 32 : 16)); }
int line_out(const I8ieLconvCall& c) { return c.KH == 1 ? c.OW : c.OH; }

}  // namespace

size_t i8ie_lconv_lds_bytes(int C, int k, int Lo) {
  const size_t nlb = (size_t)(ROWS - 2 + Lo) / Lo + 1;  // lines a run of 128 pixels can touch
  return nlb * ((size_t)Lo + k - 1) * (chunk_of(C) + 16);
}

bool i8ie_lconv_takes(const i8ie_ctx* ctx, const I8ieLconvCall& c) {
  const int k = c.KH == 1 ? c.KW : c.KH;
  if ((ctx->options & 1) != 0 || (c.KH != 1 && c.KW != 1) || k < 2 || c.C % 16 != 0) return false;
  if (!aligned_to(c.A, 16) || !aligned_to(c.Bp, 16)) return false;
  return i8ie_lconv_lds_bytes(c.C, k, line_out(c)) <= I8IE_LCONV_LDS_BUDGET;
}

int i8ie_lconv_launch(i8ie_ctx* ctx, const I8ieLconvCall& c) {
  I8IE_REQUIRE(i8ie_lconv_takes(ctx, c), "line conv: not a launch of the line kernel");
  LconvArgs a{};
  a.A = c.A; a.H = c.H; a.W = c.W; a.C = c.C; a.ib = c.ib; a.OH = c.OH; a.OW = c.OW;
  a.vert = c.KW == 1 ? 1 : 0;
  a.k = a.vert ? c.KH : c.KW; a.pl = a.vert ? c.pad_h : c.pad_w; a.pc = a.vert ? c.pad_w : c.pad_h;
  a.Lo = line_out(c); a.LP = a.Lo + a.k - 1; a.NL = a.vert ? c.OW : c.OH;
  a.lines = (long long)c.m * a.NL;
  a.M = a.lines * a.Lo;
  a.N = c.N; a.Kgp = c.Kgp; a.CC = chunk_of(c.C); a.PCH = a.CC + 16;
  a.Bp = c.Bp; a.ep = i8ie_epi_args(c.ep); a.zp_in = c.zp_in;
  a.out = c.out; a.ob = c.ob;
  a.vec_out = (c.N % 4 == 0 && aligned_to(c.out, 4)) ? 1 : 0;
  const long long blocks = (a.M + ROWS - 1) / ROWS;
  I8IE_REQUIRE(blocks < ((long long)1 << 31), "line conv: too many output pixels in one call");
  const dim3 grid((unsigned)blocks, (unsigned)((c.N + 63) / 64));
  I8IE_REQUIRE(grid.y <= 65535u, "line conv: too many features");
  I8ieProfScope prof(ctx, "lconv_mfma", 2.0 * (double)a.M * c.N * c.C * a.k,
                     (double)c.m * c.H * c.W * c.C + (double)a.M * c.N + (double)c.Ngp * c.Kgp);
  const size_t lds = i8ie_lconv_lds_bytes(c.C, a.k, a.Lo);
  if (c.ep.msv != nullptr) lconv_mfma_kernel<true><<<grid, 256, lds, ctx->stream>>>(a);
  else lconv_mfma_kernel<false><<<grid, 256, lds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
