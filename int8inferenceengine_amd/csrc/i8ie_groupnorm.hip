// i8ie_groupnorm.hip -- quantized GroupNorm over the pixels of an image: i8ie_groupnorm_u8_nhwc,
// i8ie_groupnorm_workspace_bytes, i8ie_groupnorm_f32.  The arithmetic is defined in include/i8ie_hip.h; row (i, g) is the
// N = cg h w bytes of image i in the channels of group g, and per row it is the LayerNorm's with C read as N:
//     S1 = sum a, S2 = sum a^2, V = N S2 - S1^2 (integers), r = (float)(1 / sqrt((double)V + E)),
//     d = N a - S1, t = (float)d * r, u = t * g[c], v = u + b[c], q = clamp(trunc(v)), relu: q = max(q, zp_out)
// Every kernel evaluates the last line as it is written (three fp32 operations; the library is built with
// -ffp-contract=off).  In NHWC storage a row is spread over the whole image at a stride of C bytes, so the fast forms do not
// walk rows: a lane owns one 16-byte channel item (channels 16 ci .. 16 ci + 15) and walks pixels, lane t of a block at item
// ci = t % (C / 16) of pixel slot t / (C / 16) (lanes past the last whole slot idle), so that the lanes of a slot read C
// contiguous bytes.  The sums are kept per accumulator unit of the item: the whole item where cg % 16 == 0 (two dot-4
// accumulators), a dword where cg % 4 == 0 (eight), a byte otherwise (thirty-two); a unit never straddles a group.  Lanes of
// a wave that own the same item are folded with __shfl_xor where C / 16 is a power of two below 64; units are then folded into
// their groups by integer adds on LDS (exact, so the order does not matter), runs of units of one group first.
//
// Three forms, identical bytes:
//   image   h w C <= 98304 (I8IE_GROUPNORM_IMAGE_BYTES), C % 16 == 0, C <= 4096: one launch, one block of 512 lanes per
//           image.  The interior is staged into LDS with 16-byte loads (the border skipped, the re-bias undone) while the
//           sums are taken, so the image is read from memory once; one double-precision r per group; the bytes are normalised
//           out of LDS and written with 16-byte stores at the result's border offset and re-bias.  LDS: h w C + 12 G bytes
//           (at most 96 KiB + 48 KiB of the CU's 160 KiB).  A block always owns a whole image: the variant in which a block
//           owns a slab of whole groups, for batches smaller than the CU count, is not built (section 8n, "next").
//   split   larger images: groupnorm_u8_stats on a grid over (image, chunk of max(1, 32768 / C) pixels) writes per-group
//           partial sums to ws[image][chunk][S1 | S2][G] (written, never accumulated: ws need not be zeroed and there is no
//           atomic on memory); groupnorm_u8_apply on the same grid sums its image's partials in chunk order (integers), takes r
//           per group and streams its chunk a second time.
//   direct  the definition verbatim: one wave per (image, group), lanes striding over the row's N bytes, the row walked
//           twice.  For C % 16 != 0, C > 4096, in, out, g or b not 16-byte aligned and everything under
//           I8IE_OPT_FORCE_FALLBACK.  Grid-strides.
// out may alias in: the image form has read every byte before its first store, the split form's stats launch has ended
// before apply starts and an apply lane writes only the item it has just read, a direct wave owns its row.
#include <cmath>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kMaxC = 16384;
constexpr int kMaxN = I8IE_GROUPNORM_MAX_N;
constexpr int kFastMaxC = 4096;  // C / 16 <= 256: every channel item has a lane in a block of kThreads
constexpr int kImageBytes = I8IE_GROUPNORM_IMAGE_BYTES;
constexpr int kChunkBytes = I8IE_GROUPNORM_CHUNK_BYTES;
constexpr int kImageThreads = 512;

struct GnSide {
  int64_t img, row, org;  // NhwcGeom
  int flat;               // border 0: interior pixel p lies at p * C
  uint32_t x4;            // 0x80808080 where this side is stored re-biased
};
struct GnArgs {
  const uint8_t* in;
  uint8_t* out;
  GnSide si, so;
  int n, C, G, cg, w, hw, n16, N;
  const float* g;
  const float* b;
  double E;
  int lo;  // relu: zp_out, else 0
  uint32_t* ws;
  int chunks, chunk_px;
};

extern __shared__ __attribute__((aligned(16))) uint8_t gn_smem[];

// byte offset of interior pixel p of an image (from the image's start)
__device__ __forceinline__ int64_t gn_px(const GnSide& s, int p, int C, int w) {
  if (s.flat) return (int64_t)p * C;
  const int y = p / w, x = p - y * w;
  return s.org + (int64_t)y * s.row + (int64_t)x * C;
}

__device__ __forceinline__ float gn_rstd(uint32_t S1, uint32_t S2, int N, double E) {
  const int64_t V = (int64_t)N * (int64_t)S2 - (int64_t)S1 * (int64_t)S1;
  return (float)__ddiv_rn(1.0, __dsqrt_rn(__dadd_rn((double)V, E)));
}
__device__ __forceinline__ uint32_t gn_byte(uint32_t a, int N, uint32_t S1, float r, float g, float b, int lo) {
  const int d = N * (int)a - (int)S1;  // |d| <= 255 * 65536 < 2^24
  const float t = (float)d * r;
  const float u = t * g;
  const float v = u + b;
  const int q = v >= 255.0f ? 255 : (v < 0.0f ? 0 : (int)v);
  return (uint32_t)(q > lo ? q : lo);
}

// PER accumulator units per 16-byte item: 1 (the item), 4 (a dword) or 16 (a byte)
template <int PER>
__device__ __forceinline__ void gn_acc(const uint32_t (&w)[4], uint32_t (&s1)[PER], uint32_t (&s2)[PER]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (PER == 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t v = (w[k] >> (8 * e)) & 0xFFu;
        s1[(4 * k + e) % PER] += v;
        s2[(4 * k + e) % PER] += v * v;
      }
    } else {
      const int u = PER == 4 ? k : 0;
      s1[u % PER] = __builtin_amdgcn_udot4(w[k], 0x01010101u, s1[u % PER], false);
      s2[u % PER] = __builtin_amdgcn_udot4(w[k], w[k], s2[u % PER], false);
    }
  }
}

// the lanes' unit sums into gS1[G], gS2[G] (LDS, zeroed, a barrier behind the zeroing).  Every lane of a wave calls this;
// `active` lanes own item ci.
template <int PER>
__device__ __forceinline__ void gn_fold(uint32_t (&s1)[PER], uint32_t (&s2)[PER], bool active, int ci, int n16, int cg, uint32_t* gS1,
                                        uint32_t* gS2) {
  bool mine = active;
  if (n16 < 64 && (n16 & (n16 - 1)) == 0) {  // (block-uniform; every lane of the block is active then)
    for (int o = 32; o >= n16; o >>= 1) {
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        s1[u] += (uint32_t)__shfl_xor((int)s1[u], o, 64);
        s2[u] += (uint32_t)__shfl_xor((int)s2[u], o, 64);
      }
    }
    mine = active && ((int)threadIdx.x & 63) < n16;
  }
  if (!mine) return;
  constexpr int W = 16 / PER;
  int gcur = 16 * ci / cg;
  uint32_t a1 = 0, a2 = 0;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int g = (16 * ci + W * u) / cg;
    if (g != gcur) {
      atomicAdd(&gS1[gcur], a1);
      atomicAdd(&gS2[gcur], a2);
      gcur = g;
      a1 = a2 = 0;
    }
    a1 += s1[u];
    a2 += s2[u];
  }
  atomicAdd(&gS1[gcur], a1);
  atomicAdd(&gS2[gcur], a2);
}

// what a lane needs to normalise bytes of item ci: S1 and r of every unit's group, g and b of its 16 channels
template <int PER>
struct GnLane {
  uint32_t S1[PER];
  float r[PER];
  float gg[16], bb[16];
};
template <int PER>
__device__ __forceinline__ void gn_lane(GnLane<PER>& L, int ci, int cg, const uint32_t* gS1, const float* gR, const float* g, const float* b) {
  constexpr int W = 16 / PER;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int grp = (16 * ci + W * u) / cg;
    L.S1[u] = gS1[grp];
    L.r[u] = gR[grp];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 g4 = *reinterpret_cast<const float4*>(g + 16 * ci + 4 * k), b4 = *reinterpret_cast<const float4*>(b + 16 * ci + 4 * k);
    L.gg[4 * k] = g4.x; L.gg[4 * k + 1] = g4.y; L.gg[4 * k + 2] = g4.z; L.gg[4 * k + 3] = g4.w;
    L.bb[4 * k] = b4.x; L.bb[4 * k + 1] = b4.y; L.bb[4 * k + 2] = b4.z; L.bb[4 * k + 3] = b4.w;
  }
}
template <int PER>
__device__ __forceinline__ uint4 gn_item(const uint32_t (&w)[4], const GnLane<PER>& L, int N, int lo, uint32_t x4) {
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * k + e, u = (PER == 16 ? j : PER == 4 ? k : 0) % PER;
      v |= gn_byte((w[k] >> (8 * e)) & 0xFFu, N, L.S1[u], L.r[u], L.gg[j], L.bb[j], lo) << (8 * e);
    }
    o[k] = v ^ x4;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// one block per image; LDS: [hw * C] the interior, plain bytes | gS1[G] | gS2[G] | gR[G]
template <int PER>
__global__ __launch_bounds__(kImageThreads) void groupnorm_u8_image_kernel(const GnArgs a) {
  const int C = a.C, G = a.G, hw = a.hw, n16 = a.n16, t = (int)threadIdx.x;
  uint8_t* img = gn_smem;
  uint32_t* gS1 = reinterpret_cast<uint32_t*>(gn_smem + (size_t)hw * C);
  uint32_t* gS2 = gS1 + G;
  float* gR = reinterpret_cast<float*>(gS2 + G);
  const int slots = kImageThreads / n16, slot = t / n16, ci = t - slot * n16;
  const bool active = slot < slots;
  for (int g = t; g < G; g += kImageThreads) gS1[g] = gS2[g] = 0u;
  uint32_t s1[PER], s2[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) s1[u] = s2[u] = 0u;
  if (active) {
    const uint8_t* src = a.in + (int64_t)blockIdx.x * a.si.img + 16 * ci;
#pragma unroll 4
    for (int p = slot; p < hw; p += slots) {
      const uint4 x = *reinterpret_cast<const uint4*>(src + gn_px(a.si, p, C, a.w));
      const uint32_t w[4] = {x.x ^ a.si.x4, x.y ^ a.si.x4, x.z ^ a.si.x4, x.w ^ a.si.x4};
      *reinterpret_cast<uint4*>(img + (size_t)p * C + 16 * ci) = make_uint4(w[0], w[1], w[2], w[3]);
      gn_acc<PER>(w, s1, s2);
    }
  }
  __syncthreads();
  gn_fold<PER>(s1, s2, active, ci, n16, a.cg, gS1, gS2);
  __syncthreads();
  for (int g = t; g < G; g += kImageThreads) gR[g] = gn_rstd(gS1[g], gS2[g], a.N, a.E);
  __syncthreads();
  if (!active) return;
  GnLane<PER> L;
  gn_lane<PER>(L, ci, a.cg, gS1, gR, a.g, a.b);
  uint8_t* dst = a.out + (int64_t)blockIdx.x * a.so.img + 16 * ci;
  for (int p = slot; p < hw; p += slots) {
    const uint4 x = *reinterpret_cast<const uint4*>(img + (size_t)p * C + 16 * ci);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    *reinterpret_cast<uint4*>(dst + gn_px(a.so, p, C, a.w)) = gn_item<PER>(w, L, a.N, a.lo, a.so.x4);
  }
}

// block (image, chunk): ws[image][chunk][0][g] = S1, [1][g] = S2 of the chunk's pixels.  LDS: gS1[G] | gS2[G]
template <int PER>
__global__ __launch_bounds__(kThreads) void groupnorm_u8_stats_kernel(const GnArgs a) {
  const int C = a.C, G = a.G, n16 = a.n16, t = (int)threadIdx.x;
  uint32_t* gS1 = reinterpret_cast<uint32_t*>(gn_smem);
  uint32_t* gS2 = gS1 + G;
  const int image = (int)(blockIdx.x / (unsigned)a.chunks), ch = (int)blockIdx.x - image * a.chunks;
  const int p0 = ch * a.chunk_px, p1 = min(a.hw, p0 + a.chunk_px);
  const int slots = kThreads / n16, slot = t / n16, ci = t - slot * n16;
  const bool active = slot < slots;
  for (int g = t; g < G; g += kThreads) gS1[g] = gS2[g] = 0u;
  uint32_t s1[PER], s2[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) s1[u] = s2[u] = 0u;
  if (active) {
    const uint8_t* src = a.in + (int64_t)image * a.si.img + 16 * ci;
    for (int p = p0 + slot; p < p1; p += slots) {
      const uint4 x = *reinterpret_cast<const uint4*>(src + gn_px(a.si, p, C, a.w));
      const uint32_t w[4] = {x.x ^ a.si.x4, x.y ^ a.si.x4, x.z ^ a.si.x4, x.w ^ a.si.x4};
      gn_acc<PER>(w, s1, s2);
    }
  }
  __syncthreads();
  gn_fold<PER>(s1, s2, active, ci, n16, a.cg, gS1, gS2);
  __syncthreads();
  uint32_t* part = a.ws + (size_t)blockIdx.x * 2 * G;
  for (int g = t; g < G; g += kThreads) {
    part[g] = gS1[g];
    part[G + g] = gS2[g];
  }
}

// block (image, chunk): the image's partials summed in chunk order, r per group, the chunk streamed.  LDS: gS1[G] | gR[G]
template <int PER>
__global__ __launch_bounds__(kThreads) void groupnorm_u8_apply_kernel(const GnArgs a) {
  const int C = a.C, G = a.G, n16 = a.n16, t = (int)threadIdx.x;
  uint32_t* gS1 = reinterpret_cast<uint32_t*>(gn_smem);
  float* gR = reinterpret_cast<float*>(gS1 + G);
  const int image = (int)(blockIdx.x / (unsigned)a.chunks), ch = (int)blockIdx.x - image * a.chunks;
  const int p0 = ch * a.chunk_px, p1 = min(a.hw, p0 + a.chunk_px);
  const uint32_t* part = a.ws + (size_t)image * a.chunks * 2 * G;
  for (int g = t; g < G; g += kThreads) {
    uint32_t S1 = 0, S2 = 0;
    for (int k = 0; k < a.chunks; ++k) {
      S1 += part[(size_t)k * 2 * G + g];
      S2 += part[(size_t)k * 2 * G + G + g];
    }
    gS1[g] = S1;
    gR[g] = gn_rstd(S1, S2, a.N, a.E);
  }
  __syncthreads();
  const int slots = kThreads / n16, slot = t / n16, ci = t - slot * n16;
  if (slot >= slots) return;
  GnLane<PER> L;
  gn_lane<PER>(L, ci, a.cg, gS1, gR, a.g, a.b);
  const uint8_t* src = a.in + (int64_t)image * a.si.img + 16 * ci;
  uint8_t* dst = a.out + (int64_t)image * a.so.img + 16 * ci;
  for (int p = p0 + slot; p < p1; p += slots) {
    const uint4 x = *reinterpret_cast<const uint4*>(src + gn_px(a.si, p, C, a.w));
    const uint32_t w[4] = {x.x ^ a.si.x4, x.y ^ a.si.x4, x.z ^ a.si.x4, x.w ^ a.si.x4};
    *reinterpret_cast<uint4*>(dst + gn_px(a.so, p, C, a.w)) = gn_item<PER>(w, L, a.N, a.lo, a.so.x4);
  }
}

// the definition verbatim: one wave per row (image, group), element e = (pixel e / cg, channel g cg + e % cg), the row walked twice
__global__ __launch_bounds__(kThreads) void groupnorm_u8_direct_kernel(const GnArgs a) {
  const int lane = (int)threadIdx.x & 63, cg = a.cg, N = a.N;
  const int64_t rows = (int64_t)a.n * a.G, stride = (int64_t)gridDim.x * (kThreads / 64);
  const uint32_t xi = a.si.x4 & 0xFFu, xo = a.so.x4 & 0xFFu;
  for (int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + ((int)threadIdx.x >> 6); row < rows; row += stride) {
    const int64_t image = row / a.G;
    const int c0 = (int)(row - image * a.G) * cg;
    const uint8_t* src = a.in + image * a.si.img + c0;
    uint8_t* dst = a.out + image * a.so.img + c0;
    uint32_t S1 = 0, S2 = 0;
    for (int e = lane; e < N; e += 64) {
      const int p = e / cg, k = e - p * cg;
      const uint32_t v = (uint32_t)src[gn_px(a.si, p, a.C, a.w) + k] ^ xi;
      S1 += v;
      S2 += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      S1 += (uint32_t)__shfl_xor((int)S1, o, 64);
      S2 += (uint32_t)__shfl_xor((int)S2, o, 64);
    }
    const float r = gn_rstd(S1, S2, N, a.E);
    for (int e = lane; e < N; e += 64) {
      const int p = e / cg, k = e - p * cg;
      const uint32_t v = (uint32_t)src[gn_px(a.si, p, a.C, a.w) + k] ^ xi;
      dst[gn_px(a.so, p, a.C, a.w) + k] = (uint8_t)(gn_byte(v, N, S1, r, a.g[c0 + k], a.b[c0 + k], a.lo) ^ xo);
    }
  }
}

// FP32, off the timed path: one lane per row of N contiguous floats, plain loops in ascending address order
__global__ __launch_bounds__(kThreads) void groupnorm_f32_kernel(const float* in, float* out, int64_t rows, int G, int cg, int64_t hw,
                                                                 const float* gamma, const float* beta, float eps) {
  const int64_t stride = (int64_t)gridDim.x * kThreads, N = (int64_t)cg * hw;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += stride) {
    const float* src = in + r * N;
    float* dst = out + r * N;
    const int c0 = (int)(r % G) * cg;
    float sum = 0.0f;
    for (int64_t e = 0; e < N; ++e) sum = sum + src[e];
    const float mean = sum / (float)N;
    float sq = 0.0f;
    for (int64_t e = 0; e < N; ++e) {
      const float dx = src[e] - mean;
      const float p = dx * dx;
      sq = sq + p;
    }
    const float var = sq / (float)N;
    const float sd = sqrtf(var + eps);
    for (int k = 0; k < cg; ++k) {
      const float g = gamma[c0 + k], b = beta[c0 + k];
      for (int64_t e = (int64_t)k * hw; e < (int64_t)(k + 1) * hw; ++e) {
        const float dx = src[e] - mean;
        const float nrm = dx / sd;
        const float sc = nrm * g;
        dst[e] = sc + b;
      }
    }
  }
}

// E of the definition, or a negative value where the arguments do not allow it
double gn_E(int N, float s_in, float eps) {
  if (!(std::isfinite(eps) && eps > 0.0f && std::isfinite(s_in) && s_in > 0.0f)) return -1.0;
  const double E = (double)N * (double)N * (double)eps / ((double)s_in * (double)s_in);
  if (!(std::isfinite(E) && E > 0.0 && std::isfinite((float)(1.0 / std::sqrt(E))))) return -1.0;
  return E;
}

GnSide gn_side(int C, int h, int w, int border, int s8) {
  const NhwcGeom g = buf_geom(C, h, w, border);
  return {g.img, g.row, g.org, border == 0 ? 1 : 0, s8 ? 0x80808080u : 0u};
}

// the shapes the 16-byte forms take (given aligned pointers and no forced fallback)
inline bool gn_fast_shape(int C) { return C % 16 == 0 && C <= kFastMaxC; }
inline int gn_chunk_px(int C) { return kChunkBytes / C > 1 ? kChunkBytes / C : 1; }
inline int gn_per(int cg) { return cg % 16 == 0 ? 1 : (cg % 4 == 0 ? 4 : 16); }

template <int PER>
int gn_launch_image(i8ie_ctx* ctx, const GnArgs& a) {
  const size_t lds = (size_t)a.hw * a.C + 12 * (size_t)a.G;
  // (the flag: see attn_run in i8ie_attention.hip -- unlocked, idempotent, first raised by an eager run before any capture)
  static bool raised[64] = {};
  const int dev = ctx->device & 63;
  if (!raised[dev]) {
    I8IE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&groupnorm_u8_image_kernel<PER>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kImageBytes + 12 * kFastMaxC));
    raised[dev] = true;
  }
  groupnorm_u8_image_kernel<PER><<<(unsigned)a.n, kImageThreads, lds, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}
template <int PER>
int gn_launch_split(i8ie_ctx* ctx, const GnArgs& a, double bytes) {
  const unsigned grid = (unsigned)((int64_t)a.n * a.chunks);
  {
    I8ieProfScope prof(ctx, "groupnorm_u8_stats", 0.0, bytes);
    groupnorm_u8_stats_kernel<PER><<<grid, kThreads, 8 * (size_t)a.G, ctx->stream>>>(a);
    I8IE_LAUNCH_CHECK();
  }
  I8ieProfScope prof(ctx, "groupnorm_u8_apply", 0.0, 2.0 * bytes);
  groupnorm_u8_apply_kernel<PER><<<grid, kThreads, 8 * (size_t)a.G, ctx->stream>>>(a);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

// the size rules the two u8 entries share: a message, or NULL and the row length
const char* gn_size_error(int n, int C, int G, int h, int w, int* N) {
  if (!(n > 0 && h > 0 && w > 0)) return "bad dimension (n, h, w >= 1)";
  if (!(C >= 1 && C <= kMaxC)) return "bad dimension (1 <= C <= 16384)";
  if (!(G >= 1 && C % G == 0)) return "the channel count must be a multiple of the group count";
  const int64_t rowlen = (int64_t)(C / G) * h * w;
  if (rowlen > kMaxN) return "a group of one image has more than 65536 values";
  if ((int64_t)n * h * w > 0x7FFFFFFF) return "too many pixels for one launch";
  *N = (int)rowlen;
  return nullptr;
}

}  // namespace

extern "C" {

int64_t i8ie_groupnorm_workspace_bytes(int n, int C, int G, int h, int w) {
  int N = 0;
  if (const char* bad_size = gn_size_error(n, C, G, h, w, &N)) {
    i8ie_set_error("%s: %s", __func__, bad_size);
    return -1;
  }
  if (!gn_fast_shape(C) || (int64_t)h * w * C <= kImageBytes) return 0;
  const int px = gn_chunk_px(C), chunks = (h * w + px - 1) / px;
  return (int64_t)n * chunks * 2 * G * (int64_t)sizeof(uint32_t);
}

int i8ie_groupnorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in, int in_border, int in_s8, uint8_t* out, int out_border, int out_s8, int n,
                           int C, int G, int h, int w, const float* g, const float* b, float s_in, float eps, int relu, uint8_t zp_out,
                           void* ws) {
  I8IE_REQUIRE(ctx && in && out && g && b, "null argument");
  I8IE_REQUIRE(in_border >= 0 && out_border >= 0, "bad dimension");
  int N = 0;
  const char* bad_size = gn_size_error(n, C, G, h, w, &N);
  I8IE_REQUIRE(!bad_size, bad_size);
  const double E = gn_E(N, s_in, eps);
  I8IE_REQUIRE(E > 0.0, "eps and the input scale must be finite and positive (and N^2 eps / s_in^2 an ordinary number)");
  I8IE_REQUIRE(aligned_to(g, 4) && aligned_to(b, 4), "g and b must be 4-byte aligned");
  const bool split_shape = gn_fast_shape(C) && (int64_t)h * w * C > kImageBytes;
  // (the direct form takes no workspace: ws_dev is asked for only where the split form runs)
  const bool direct = (ctx->options & 1u) || !gn_fast_shape(C) || !aligned_to(in, 16) || !aligned_to(out, 16) || !aligned_to(g, 16) ||
                      !aligned_to(b, 16);
  I8IE_REQUIRE(direct || !split_shape || (ws && aligned_to(ws, 4)), "ws_dev must hold i8ie_groupnorm_workspace_bytes() bytes, 4-byte aligned");
  GnArgs a;
  a.in = in;
  a.out = out;
  a.si = gn_side(C, h, w, in_border, in_s8);
  a.so = gn_side(C, h, w, out_border, out_s8);
  a.n = n; a.C = C; a.G = G; a.cg = C / G; a.w = w; a.hw = h * w; a.n16 = C / 16; a.N = N;
  a.g = g;
  a.b = b;
  a.E = E;
  a.lo = relu ? (int)zp_out : 0;
  a.ws = static_cast<uint32_t*>(ws);
  a.chunk_px = gn_chunk_px(C);
  a.chunks = (a.hw + a.chunk_px - 1) / a.chunk_px;
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const double bytes = (double)n * a.hw * C;
  const int per = gn_per(a.cg);
  if (direct) {
    I8ieProfScope prof(ctx, "groupnorm_u8_direct", 0.0, 3.0 * bytes);
    const int64_t blocks = ((int64_t)n * G + kThreads / 64 - 1) / (kThreads / 64);
    groupnorm_u8_direct_kernel<<<(unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks), kThreads, 0, ctx->stream>>>(a);
    I8IE_LAUNCH_CHECK();
    return I8IE_OK;
  }
  if (!split_shape) {
    I8ieProfScope prof(ctx, "groupnorm_u8_image", 0.0, 2.0 * bytes);
    return per == 1 ? gn_launch_image<1>(ctx, a) : per == 4 ? gn_launch_image<4>(ctx, a) : gn_launch_image<16>(ctx, a);
  }
  return per == 1 ? gn_launch_split<1>(ctx, a, bytes) : per == 4 ? gn_launch_split<4>(ctx, a, bytes) : gn_launch_split<16>(ctx, a, bytes);
}

int i8ie_groupnorm_f32(i8ie_ctx* ctx, const float* in, float* out, int n, int C, int G, int64_t hw, const float* gamma, const float* beta,
                       float eps) {
  I8IE_REQUIRE(ctx && in && out && gamma && beta, "null argument");
  I8IE_REQUIRE(n > 0 && hw > 0, "bad dimension");
  I8IE_REQUIRE(C >= 1 && C <= kMaxC, "bad dimension (1 <= C <= 16384)");
  I8IE_REQUIRE(G >= 1 && C % G == 0, "the channel count must be a multiple of the group count");
  I8IE_REQUIRE(hw <= kMaxN && (int64_t)(C / G) * hw <= kMaxN, "a group of one image has more than 65536 values");
  I8IE_REQUIRE(std::isfinite(eps) && eps > 0.0f, "eps must be finite and positive");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t rows = (int64_t)n * G;
  I8ieProfScope prof(ctx, "groupnorm_f32", 0.0, 8.0 * (double)n * C * (double)hw);
  groupnorm_f32_kernel<<<grid_for(rows), kThreads, 0, ctx->stream>>>(in, out, rows, G, C / G, hw, gamma, beta, eps);
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

}  // extern "C"
