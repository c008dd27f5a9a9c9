// i8ie_calib_hist.hip -- the histogram observer of calibration (include/i8ie_hip.h, "Histogram calibration"): exact min / max,
// a count of the non-finite values and 2048 power-of-two-wide bins over every finite value a layer's FP32 output took, kept in
// one caller-owned device buffer; and the host function that turns a state read back into a range (minmax, percentile, mse).
//
// One observe is two launches on the ctx stream and never meets the host:
//   calib_hist_stats  min / max / non-finite count of the chunk (16-byte loads, grid-strided, at most 512 blocks: each ends in an
//                     atomic on one ticket word, and one word takes about 90 atomics per microsecond); the block that finishes last
//                     merges them into the state, computes the exponent and, when it grew, folds the 2048 counters in place
//   calib_hist_count  reads the exponent from the state and counts: one 8 KiB table of 32-bit counters per wave in LDS
//                     (LDS atomics), flushed once per block with 64-bit global atomic adds of the non-zero counters
// Both read the data once: 8n bytes for n values, what a read and a write of an elementwise FP32 op move.  Lanes of a wave that
// hit the same LDS counter are served one per LDS cycle, so a wave takes the bin of its first lane, and then of the first lane
// that differs, out of the atomics: the lanes that hold it are counted with a ballot and added by one lane.  All-equal data costs
// one add per wave instead of 64 serialised ones, and a dominant bin (the zeros behind a ReLU) is taken out in 3 of 4 waves.
// Measured, the kind of data then hardly matters: an observe is bound by its fixed costs, the ticket
// atomics of the statistics pass and the flush of the count pass.
#include <cstring>

#include "i8ie_internal.h"
#include "i8ie_pointwise.h"

namespace {

constexpr int kBins = I8IE_CALIB_HIST_BINS;
constexpr int kMinExp = -100;
constexpr int kCountThreads = 512;                 // 8 waves, one table each: 64 KiB of LDS, two blocks per CU
constexpr int kCountWaves = kCountThreads / 64;
constexpr int kCountGrid = 512;                    // capped grid of the count pass (2 blocks x 256 CUs)
constexpr int kCountUnroll = 4;                    // 16-byte loads in flight per lane
constexpr int kStatsGrid = 512;                    // capped grid of the statistics pass: every block ends in one ticket atomic
constexpr int kStatsUnroll = 4;
constexpr int64_t kCountMaxValues = (int64_t)1 << 30;  // values per count launch: a block's LDS counters stay below 2^32

struct State {
  i8ie_calib_hist_header h;
  unsigned long long hist[kBins];
};
static_assert(sizeof(i8ie_calib_hist_header) == 32, "the header is 32 bytes: hist[] starts 16-byte aligned");
static_assert(sizeof(State) == 32 + 8 * kBins, "state layout");

// |x| < 2^-126 (a denormal, +-0) counts as +0; NaN and +-Inf are not finite
__device__ __forceinline__ bool is_finite_bits(uint32_t b) { return (b & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float canonical(uint32_t b) { return (b & 0x7F800000u) == 0 ? 0.0f : __uint_as_float(b); }
// a key that orders the finite floats as unsigned integers; no finite value has key 0 or 0xFFFFFFFF
__host__ __device__ __forceinline__ uint32_t order_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t key_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

// the smallest e >= -100 with absmax < 1024 * 2^e: absmax in [2^x, 2^(x+1)) gives e = x - 9
__device__ __forceinline__ int exponent_for(float absmax) {
  const uint32_t b = __float_as_uint(absmax);
  if ((b & 0x7F800000u) == 0) return kMinExp;
  const int e = (int)((b >> 23) & 0xFF) - 127 - 9;
  return e < kMinExp ? kMinExp : e;
}

struct Stats {
  float lo, hi;
  unsigned nonfinite;
};
__device__ __forceinline__ void take(Stats& s, float x) {
  const uint32_t b = __float_as_uint(x);
  if (is_finite_bits(b)) {
    const float c = canonical(b);
    s.lo = fminf(s.lo, c);
    s.hi = fmaxf(s.hi, c);
  } else {
    ++s.nonfinite;
  }
}

// the scalar head (up to the first 16-byte boundary) and tail of a buffer aligned to 4 bytes, and the 16-byte body between
struct Span {
  int64_t head, nvec, tail_at, n;
};
inline Span span_of(const float* p, int64_t n) {
  Span s;
  const int64_t to_boundary = (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;
  s.head = to_boundary < n ? to_boundary : n;
  s.nvec = (n - s.head) / 4;
  s.tail_at = s.head + 4 * s.nvec;
  s.n = n;
  return s;
}

__global__ __launch_bounds__(256) void calib_hist_stats_kernel(const float* __restrict__ data, Span sp, State* __restrict__ st) {
  Stats s{INFINITY, -INFINITY, 0u};
  const float4* body = reinterpret_cast<const float4*>(data + sp.head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256 + threadIdx.x; base < sp.nvec; base += stride * kStatsUnroll) {
    float4 f[kStatsUnroll];
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u)  // (a lane past the end reads its first vector again: the minimum and maximum do not change,
      f[u] = body[base + u * stride < sp.nvec ? base + u * stride : base];  // and take() is not called for it)
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u) {
      if (base + u * stride >= sp.nvec) continue;
      take(s, f[u].x);
      take(s, f[u].y);
      take(s, f[u].z);
      take(s, f[u].w);
    }
  }
  if (blockIdx.x == 0) {  // head and tail: at most 3 values each
    if ((int64_t)threadIdx.x < sp.head) take(s, data[threadIdx.x]);
    if (sp.tail_at + threadIdx.x < sp.n) take(s, data[sp.tail_at + threadIdx.x]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    s.lo = fminf(s.lo, __shfl_xor(s.lo, off));
    s.hi = fmaxf(s.hi, __shfl_xor(s.hi, off));
    s.nonfinite += __shfl_xor(s.nonfinite, off);
  }
  __shared__ float w_lo[4], w_hi[4];
  __shared__ unsigned w_nf[4];
  __shared__ int last_block, shift;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    w_lo[wave] = s.lo;
    w_hi[wave] = s.hi;
    w_nf[wave] = s.nonfinite;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float lo = fminf(fminf(w_lo[0], w_lo[1]), fminf(w_lo[2], w_lo[3]));
    const float hi = fmaxf(fmaxf(w_hi[0], w_hi[1]), fmaxf(w_hi[2], w_hi[3]));
    const unsigned nf = w_nf[0] + w_nf[1] + w_nf[2] + w_nf[3];
    if (lo <= hi) {  // the block saw a finite value; only a block that may improve on what has arrived pays for an atomic
      const uint32_t klo = ~order_key(__float_as_uint(lo)), khi = order_key(__float_as_uint(hi));
      if (klo > __atomic_load_n(&st->h.scratch[0], __ATOMIC_RELAXED)) atomicMax(&st->h.scratch[0], klo);
      if (khi > __atomic_load_n(&st->h.scratch[1], __ATOMIC_RELAXED)) atomicMax(&st->h.scratch[1], khi);
    }
    if (nf) atomicAdd(reinterpret_cast<unsigned long long*>(&st->h.nonfinite), (unsigned long long)nf);
    __threadfence();
    last_block = atomicAdd(&st->h.scratch[2], 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last_block) return;
  // ---- the one-block step: every block's minimum and maximum have arrived ----
  __threadfence();
  if (threadIdx.x == 0) {
    const uint32_t klo = ~atomicAdd(&st->h.scratch[0], 0u), khi = atomicAdd(&st->h.scratch[1], 0u);
    float lo = st->h.min, hi = st->h.max;
    if (khi != 0) {
      lo = fminf(lo, __uint_as_float(key_bits(klo)));
      hi = fmaxf(hi, __uint_as_float(key_bits(khi)));
    }
    const int e_old = st->h.exponent;
    const int e_new = lo <= hi ? exponent_for(fmaxf(fabsf(lo), fabsf(hi))) : e_old;
    st->h.min = lo;
    st->h.max = hi;
    st->h.exponent = e_new;
    st->h.scratch[0] = st->h.scratch[1] = st->h.scratch[2] = 0;  // at rest again
    shift = e_new - e_old;  // never negative: the running absmax only grows
  }
  __syncthreads();
  int d = shift;
  if (d <= 0) return;
  if (d > 11) d = 11;  // eleven folds take every bin to 1023 or 1024, which further folds leave where they are
  unsigned long long c[kBins / 256];
#pragma unroll
  for (int j = 0; j < kBins / 256; ++j) {
    c[j] = st->hist[threadIdx.x + 256 * j];
    st->hist[threadIdx.x + 256 * j] = 0;
  }
  __threadfence();  // the zeros are in memory before another thread's add can land on them
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kBins / 256; ++j) {
    if (c[j] == 0) continue;
    int i = threadIdx.x + 256 * j;
    for (int f = 0; f < d; ++f) i = kBins / 4 + (i >> 1);
    atomicAdd(&st->hist[i], c[j]);
  }
}

// floor(x * 2^-e) + 1024 of a canonical finite x with |x| < 1024 * 2^e.  The product is exact unless it underflows, and then
// it is below one in magnitude: floor is 0 for a positive x and -1 for a negative one, whatever the flush mode made of it.
__device__ __forceinline__ int bin_of(float x, float inv_width) {
  int f = (int)floorf(x * inv_width);
  if (x < 0.0f && f > -1) f = -1;
  f += kBins / 2;
  return f < 0 ? 0 : (f > kBins - 1 ? kBins - 1 : f);  // (in range already for a state that observe() itself wrote)
}

// one value per lane into the wave's table.  The bin of the first lane, and then of the first lane that holds another, are
// counted with a ballot and added once; what is left goes through one LDS atomic per lane.
__device__ __forceinline__ void count_wave(uint32_t* table, int bin) {  // bin < 0: nothing to count in this lane
  bool pending = bin >= 0;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long active = __ballot(pending);
    if (active == 0) return;
    const int first = __ffsll((long long)active) - 1;
    const int b = __shfl(bin, first);
    const bool mine = pending && bin == b;
    const unsigned long long same = __ballot(mine);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&table[b], (uint32_t)__popcll(same));
    pending = pending && !mine;
  }
  if (pending) atomicAdd(&table[bin], 1u);
}

__device__ __forceinline__ int bin_or_none(float x, float inv_width) {
  const uint32_t b = __float_as_uint(x);
  return is_finite_bits(b) ? bin_of(canonical(b), inv_width) : -1;
}

__global__ __launch_bounds__(kCountThreads) void calib_hist_count_kernel(const float* __restrict__ data, Span sp,
                                                                         State* __restrict__ st) {
  __shared__ uint32_t tables[kCountWaves][kBins];
  for (int i = threadIdx.x; i < kCountWaves * kBins; i += kCountThreads) (&tables[0][0])[i] = 0;
  __syncthreads();
  const float inv_width = __uint_as_float((uint32_t)(127 - st->h.exponent) << 23);  // 2^-e, e in [-100, 118]
  uint32_t* table = tables[threadIdx.x >> 6];
  const float4* body = reinterpret_cast<const float4*>(data + sp.head);
  // every wave runs the same number of rounds of the loop (count_wave uses wave-wide ballots): a lane past the end counts nothing
  const int64_t stride = (int64_t)gridDim.x * kCountThreads;
  for (int64_t base = (int64_t)blockIdx.x * kCountThreads; base < sp.nvec; base += stride * kCountUnroll) {
    float4 f[kCountUnroll];
    bool have[kCountUnroll];
#pragma unroll
    for (int u = 0; u < kCountUnroll; ++u) {
      const int64_t v = base + u * stride + threadIdx.x;
      have[u] = v < sp.nvec;
      if (have[u]) f[u] = body[v];
    }
#pragma unroll
    for (int u = 0; u < kCountUnroll; ++u) {
      count_wave(table, have[u] ? bin_or_none(f[u].x, inv_width) : -1);
      count_wave(table, have[u] ? bin_or_none(f[u].y, inv_width) : -1);
      count_wave(table, have[u] ? bin_or_none(f[u].z, inv_width) : -1);
      count_wave(table, have[u] ? bin_or_none(f[u].w, inv_width) : -1);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // head and tail, by the first wave
    const int64_t t = threadIdx.x;
    int bin = -1;
    if (t < sp.head) bin = bin_or_none(data[t], inv_width);
    else if (t >= 4 && sp.tail_at + (t - 4) < sp.n) bin = bin_or_none(data[sp.tail_at + (t - 4)], inv_width);
    count_wave(table, bin);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBins; i += kCountThreads) {
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kCountWaves; ++w) c += tables[w][i];
    if (c) atomicAdd(&st->hist[i], c);
  }
}

__global__ __launch_bounds__(256) void calib_hist_reset_kernel(State* __restrict__ st) {
  for (int i = threadIdx.x; i < kBins; i += 256) st->hist[i] = 0;
  if (threadIdx.x == 0) {
    st->h.min = INFINITY;
    st->h.max = -INFINITY;
    st->h.exponent = kMinExp;
    st->h.scratch[0] = st->h.scratch[1] = st->h.scratch[2] = 0;
    st->h.nonfinite = 0;
  }
}

// ---- host: a state read back -> a range ----------------------------------------------------------------------------------
#pragma clang fp contract(off)

double bin_width(int e) { return std::ldexp(1.0, e); }

uint64_t total_of(const uint64_t* hist) {
  uint64_t t = 0;
  for (int i = 0; i < kBins; ++i) t += hist[i];
  return t;
}

// sum_i h_i * (c_i - d(c_i))^2 of one candidate (scale, zero_point), in ascending i, in double; d is down_scale's clamp and
// truncation.  (A term with h_i == 0 is zero and is skipped.)
double mse_of(const uint64_t* hist, int e, float scale, uint8_t zp) {
  const double w = bin_width(e), s = (double)scale, z = (double)zp;
  double err = 0.0;
  for (int i = 0; i < kBins; ++i) {
    if (hist[i] == 0) continue;
    const double c = ((double)i - 1023.5) * w;
    double q = std::trunc(c / s + z);
    q = q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q);
    const double r = c - (q - z) * s;
    err += (double)hist[i] * (r * r);
  }
  return err;
}

}  // namespace

extern "C" {

size_t i8ie_calib_hist_state_bytes(void) { return sizeof(State); }

int i8ie_calib_hist_reset(i8ie_ctx* ctx, void* state_dev) {
  I8IE_REQUIRE(ctx && state_dev, "null argument");
  I8IE_REQUIRE(aligned_to(state_dev, 16), "the state must be 16-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  I8ieProfScope prof(ctx, "calib_hist_reset", 0.0, (double)sizeof(State));
  calib_hist_reset_kernel<<<1, 256, 0, ctx->stream>>>(static_cast<State*>(state_dev));
  I8IE_LAUNCH_CHECK();
  return I8IE_OK;
}

int i8ie_calib_hist_observe_f32(i8ie_ctx* ctx, const float* data_dev, int64_t n, void* state_dev) {
  I8IE_REQUIRE(ctx && state_dev, "null argument");
  I8IE_REQUIRE(n >= 0, "negative size");
  I8IE_REQUIRE(aligned_to(state_dev, 16), "the state must be 16-byte aligned");
  if (n == 0) return I8IE_OK;
  I8IE_REQUIRE(data_dev, "null argument");
  I8IE_REQUIRE(aligned_to(data_dev, 4), "the data must be 4-byte aligned");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  State* st = static_cast<State*>(state_dev);
  {
    const Span sp = span_of(data_dev, n);
    I8ieProfScope prof(ctx, "calib_hist_stats", 0.0, 4.0 * n);
    int64_t blocks = (sp.nvec + 256 * kStatsUnroll - 1) / (256 * kStatsUnroll);
    blocks = blocks < 1 ? 1 : (blocks > kStatsGrid ? kStatsGrid : blocks);
    calib_hist_stats_kernel<<<(int)blocks, 256, 0, ctx->stream>>>(data_dev, sp, st);
    I8IE_LAUNCH_CHECK();
  }
  for (int64_t at = 0; at < n; at += kCountMaxValues) {  // (one launch unless n > 2^30)
    const int64_t len = n - at < kCountMaxValues ? n - at : kCountMaxValues;
    const Span sp = span_of(data_dev + at, len);
    const int64_t per_block = (int64_t)kCountThreads * kCountUnroll;
    int64_t blocks = (sp.nvec + per_block - 1) / per_block;
    blocks = blocks < 1 ? 1 : (blocks > kCountGrid ? kCountGrid : blocks);
    I8ieProfScope prof(ctx, "calib_hist_count", 0.0, 4.0 * len);
    calib_hist_count_kernel<<<(int)blocks, kCountThreads, 0, ctx->stream>>>(data_dev + at, sp, st);
    I8IE_LAUNCH_CHECK();
  }
  return I8IE_OK;
}

int i8ie_calib_hist_read(i8ie_ctx* ctx, const void* state_dev, i8ie_calib_hist_header* header, uint64_t* hist) {
  I8IE_REQUIRE(ctx && state_dev && header && hist, "null argument");
  I8IE_HIP_TRY(hipSetDevice(ctx->device));
  State host;
  I8IE_HIP_TRY(hipMemcpyAsync(&host, state_dev, sizeof(State), hipMemcpyDeviceToHost, ctx->stream));
  I8IE_HIP_TRY(hipStreamSynchronize(ctx->stream));
  *header = host.h;
  std::memcpy(hist, host.hist, sizeof(host.hist));
  return I8IE_OK;
}

void i8ie_calib_range_qparams(float out_min, float out_max, float* scale_out, uint8_t* zero_point_out) {
  // src/calibrator.cc:31-36
  out_min = std::fmin(out_min, 0.);
  out_max = std::fmax(out_max, 0.);
  uint8_t zp = (uint8_t)(255 * (0 - out_min) / (out_max - out_min + 1e-09));
  float scale = (zp == 0) ? (out_max - out_min) / 255 : (0 - out_min) / zp;
  if (scale == 0) scale = 1;
  *scale_out = scale;
  *zero_point_out = zp;
}

int i8ie_calib_hist_range(const i8ie_calib_hist_header* header, const uint64_t* hist, int method, double param, float* lo_out,
                          float* hi_out) {
  I8IE_REQUIRE(header && hist && lo_out && hi_out, "null argument");
  I8IE_REQUIRE(method == I8IE_CALIB_MINMAX || method == I8IE_CALIB_PERCENTILE || method == I8IE_CALIB_MSE, "unknown range method");
  I8IE_REQUIRE(method != I8IE_CALIB_PERCENTILE || (param > 50.0 && param <= 100.0), "the percentile must lie in (50, 100]");
  I8IE_REQUIRE(header->exponent >= kMinExp && header->exponent <= 118, "exponent out of range");
  *lo_out = *hi_out = 0.0f;
  const uint64_t total = total_of(hist);
  if (total == 0 || !(header->min <= header->max)) return I8IE_OK;  // nothing finite was seen
  const float mn = header->min, mx = header->max;
  if (method == I8IE_CALIB_MINMAX) {
    *lo_out = mn;
    *hi_out = mx;
    return I8IE_OK;
  }
  if (method == I8IE_CALIB_PERCENTILE) {
    const double w = bin_width(header->exponent);
    const uint64_t k = (uint64_t)std::floor((1.0 - param / 100.0) * (double)total);
    uint64_t cum = 0;
    int i = 0;
    for (; i < kBins - 1; ++i)
      if ((cum += hist[i]) > k) break;
    const double lower = (double)(i - kBins / 2) * w;
    cum = 0;
    for (i = kBins - 1; i > 0; --i)
      if ((cum += hist[i]) > k) break;
    const double upper = (double)(i - kBins / 2 + 1) * w;
    *lo_out = lower > (double)mn ? (float)lower : mn;
    *hi_out = upper < (double)mx ? (float)upper : mx;
    return I8IE_OK;
  }
  const float lo0 = std::fmin(mn, 0.0f), hi0 = std::fmax(mx, 0.0f);
  double best = 0.0;
  for (int j = 16; j <= 64; ++j) {
    const float lo = (float)((double)lo0 * (double)j / 64.0), hi = (float)((double)hi0 * (double)j / 64.0);
    float s;
    uint8_t z;
    i8ie_calib_range_qparams(lo, hi, &s, &z);
    const double err = mse_of(hist, header->exponent, s, z);
    if (j == 16 || err <= best) {  // ties go to the larger j
      best = err;
      *lo_out = lo;
      *hi_out = hi;
    }
  }
  return I8IE_OK;
}

}  // extern "C"
