// i8ie_requant.h -- the one requantiser of libi8ie_hip.so (every kernel's epilogue includes this file).
//
// Reference: down_scale, src/quantize_utils.cc:27-36
//     deq = ((float)C * s_in) * s_w;  q = deq / s_out + (float)zp_out;
//     out = q >= 255 ? 255 : (q < 0 ? 0 : (u8)q)                      (IEEE fp32, no contraction)
// optionally followed by relu<u8> (src/functional.cc:15-26): out = max(out, zp_out).
//
// Evaluation modes, both bit-identical to that sequence:
//   I8IE_RQ_EXACT    the sequence itself.
//   I8IE_RQ_GUARDED  e = fma((float)C, ms, zp - 0.5), ms = fl(s_in*s_w/s_out), packed with v_cvt_pk_u8_f32
//                    (round-to-nearest-even, saturate); any dword holding a value closer than 2^-13 to a
//                    rounding boundary replays the exact sequence (error analysis below).
// (An unguarded estimate with host-fitted ms', bias' was measured in round 2: the fit fails on every AlexNet conv
// layer, so the guard stays.  The fit is at 9e2c9d6.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

enum { I8IE_RQ_EXACT = 0, I8IE_RQ_GUARDED = 1 };

struct I8ieRequant {
  float sa, sb, sc, zpf, ms;
  int fast;  // I8IE_RQ_*
};

// src/quantize_utils.cc:30-33, the exact sequence (+ relu lower bound `lo`, 0 when relu is not fused)
__host__ __device__ __forceinline__ int i8ie_requant_exact(float cf, const I8ieRequant& q, int lo) {
  const float deq = (cf * q.sa) * q.sb;
  const float v = deq / q.sc + q.zpf;
  const int u = (v >= 255.0f) ? 255 : ((v < 0.0f) ? 0 : (int)v);
  return u > lo ? u : lo;
}

#if defined(__HIPCC__)
// e = fma(cf, ms, zp - 0.5): an estimate of (reference value v) - 0.5.  While -1 < v < 256,
// |v - (e + 0.5)| < 9.2e-5 (reference: 3 roundings on |C*s_in*s_w/s_out| < 256 and one on |v| < 257; e: one
// rounding of ms, one of the fma).  So if e is further than 2^-13 from every half-integer, v lies strictly
// inside the unit interval [k, k+1) with k = rne(e), and the reference's trunc + clamp equals sat_u8(rne(e)),
// which is what v_cvt_pk_u8_f32 computes.  Outside (-1, 256) both sides clamp, with the same margin.  relu
// (max with zp_out) commutes with the monotone rounding: rne(max(e, lo)) for the integer lo.
//
// The guard exists once.  A pack is four steps, one per estimate e of (value) - 0.5, whatever e was computed from: byte r of
// `packed` becomes sat_u8(rne(max(e, lof))) (v_cvt_pk_u8_f32; lof = -1 is no clamp at all, the pack saturates at 0, and
// CLAMP = false leaves the max out), and `worst` keeps the smallest distance of any e to a rounding boundary.  It starts at 1,
// or at 0 for a pack that must not stand (scales that do not allow the estimate).  The dword stands where
// i8ie_requant_est_ok(worst): the threshold 2^-13 lies above every bound proven for an estimate in this library (9.2e-5 here
// and for the gate multiply, 6.2e-5 for add, multiply and concat: i8ie_binary.hip, i8ie_concat.hip).  Otherwise the caller
// replays its exact sequence.
template <bool CLAMP = true>
__device__ __forceinline__ uint32_t i8ie_requant_est_step(float e, float lof, int r, uint32_t packed, float& worst) {
  packed = __builtin_amdgcn_cvt_pk_u8_f32(CLAMP ? __builtin_fmaxf(e, lof) : e, r, packed);
  worst = __builtin_fminf(worst, __builtin_fabsf(__builtin_amdgcn_fractf(e) - 0.5f));
  return packed;
}
__device__ __forceinline__ bool i8ie_requant_est_ok(float worst) { return worst >= 1.220703125e-4f; }

__device__ __forceinline__ uint32_t i8ie_requant_pack4(const int (&c)[4], const I8ieRequant& q, int lo, float lof) {
  uint32_t packed = 0;
  float worst = q.fast ? 1.0f : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    packed = i8ie_requant_est_step(__builtin_fmaf((float)c[r], q.ms, q.zpf - 0.5f), lof, r, packed, worst);
  }
  if (i8ie_requant_est_ok(worst)) return packed;
  packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= (uint32_t)i8ie_requant_exact((float)c[r], q, lo) << (8 * r);
  return packed;
}

// Without the ReLU (callers that apply max(., zp_out) later, e.g. behind a max-pool, which it commutes with): the
// estimate needs no lower clamp at all -- v_cvt_pk_u8_f32 saturates at 0 -- so a value costs one instruction less.
__device__ __forceinline__ uint32_t i8ie_requant_pack4_norelu(const int (&c)[4], const I8ieRequant& q) {
  uint32_t packed = 0;
  float worst = q.fast ? 1.0f : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    packed = i8ie_requant_est_step<false>(__builtin_fmaf((float)c[r], q.ms, q.zpf - 0.5f), 0.0f, r, packed, worst);
  }
  if (i8ie_requant_est_ok(worst)) return packed;
  packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= (uint32_t)i8ie_requant_exact((float)c[r], q, 0) << (8 * r);
  return packed;
}

// The same in two halves, for epilogues that keep several independent packs in flight without a branch between them:
// the estimate (+ how far the closest value is from a rounding boundary), and the exact replay for a pack whose
// `worst` came out below 2^-13 (or whose scales do not allow the estimate: worst = 0 then).
__device__ __forceinline__ uint32_t i8ie_requant_est4(const int (&c)[4], const I8ieRequant& q, float lof, float& worst) {
  uint32_t packed = 0;
  float w = q.fast ? 1.0f : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    packed = i8ie_requant_est_step(__builtin_fmaf((float)c[r], q.ms, q.zpf - 0.5f), lof, r, packed, w);
  }
  worst = w;
  return packed;
}
__device__ __forceinline__ uint32_t i8ie_requant_exact4(const int (&c)[4], const I8ieRequant& q, int lo) {
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= (uint32_t)i8ie_requant_exact((float)c[r], q, lo) << (8 * r);
  return packed;
}

// ---- per-output-channel weight scales (i8ie_linear_create_per_channel / i8ie_conv2d_create_per_channel) ---------------
// Column j has its own multiplier ms[j] = fl(s_in * s_w[j] / s_out) (host, in double) and its own s_w[j] for the exact
// replay.  The guard's bound is per value, so it holds column by column; q.fast is decided for the whole layer on the host
// (every column's scales ordinary, or the layer takes the exact sequence).  A column with ms[j] == 0 has e = zp - 0.5,
// fract(e) = 0.5: it always replays.  `ms` holds the multipliers of 4 consecutive columns, `sb` points at s_w of the first
// of them; sb is read in the replay only.
__device__ __forceinline__ int i8ie_requant_exact_col(float cf, const I8ieRequant& q, float sb, int lo) {
  I8ieRequant qc = q;
  qc.sb = sb;
  return i8ie_requant_exact(cf, qc, lo);
}
__device__ __forceinline__ uint32_t i8ie_requant_exact4_pc(const int (&c)[4], const I8ieRequant& q, const float* sb, int lo) {
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) packed |= (uint32_t)i8ie_requant_exact_col((float)c[r], q, sb[r], lo) << (8 * r);
  return packed;
}
__device__ __forceinline__ uint32_t i8ie_requant_est4_pc(const int (&c)[4], const I8ieRequant& q, const float4& ms, float lof,
                                                         float& worst) {
  const float m[4] = {ms.x, ms.y, ms.z, ms.w};
  uint32_t packed = 0;
  float w = q.fast ? 1.0f : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    packed = i8ie_requant_est_step(__builtin_fmaf((float)c[r], m[r], q.zpf - 0.5f), lof, r, packed, w);
  }
  worst = w;
  return packed;
}
__device__ __forceinline__ uint32_t i8ie_requant_pack4_pc(const int (&c)[4], const I8ieRequant& q, const float4& ms,
                                                          const float* sb, int lo, float lof) {
  float worst;
  const uint32_t packed = i8ie_requant_est4_pc(c, q, ms, lof, worst);
  if (i8ie_requant_est_ok(worst)) return packed;
  return i8ie_requant_exact4_pc(c, q, sb, lo);
}
// (v_cvt_pk_u8_f32 saturates at 0: lof = -1 is no clamp at all, as in i8ie_requant_pack4_norelu)
__device__ __forceinline__ uint32_t i8ie_requant_pack4_norelu_pc(const int (&c)[4], const I8ieRequant& q, const float4& ms,
                                                                 const float* sb) {
  return i8ie_requant_pack4_pc(c, q, ms, sb, 0, -1.0f);
}

#endif

// ---- host side --------------------------------------------------------------------------------------------
inline I8ieRequant i8ie_make_requant(float s_in, float s_w, float s_out, int zp_out) {
  I8ieRequant r;
  r.sa = s_in; r.sb = s_w; r.sc = s_out; r.zpf = (float)zp_out;
  const double ms = (double)s_in * (double)s_w / (double)s_out;
  r.ms = (float)ms;
  // estimate only for ordinary positive finite scales; anything else takes the exact sequence
  r.fast = (s_in > 1e-30f && s_w > 1e-30f && s_out > 1e-30f && s_in < 1e30f && s_w < 1e30f && s_out < 1e30f &&
            ms > 1e-30 && ms < 1e30) ? I8IE_RQ_GUARDED : I8IE_RQ_EXACT;
  return r;
}

// Per-channel layers: the multiplier of column j (0 for s_w[j] == 0, see above), and whether the estimate may be used for
// the whole layer -- every s_w[j] zero or ordinary, and every nonzero multiplier ordinary.
inline float i8ie_requant_ms(float s_in, float s_w, float s_out) { return (float)((double)s_in * (double)s_w / (double)s_out); }
inline bool i8ie_requant_pc_fast(float s_in, const float* s_w, int n, float s_out) {
  if (!(s_in > 1e-30f && s_out > 1e-30f && s_in < 1e30f && s_out < 1e30f)) return false;
  for (int j = 0; j < n; ++j) {
    if (s_w[j] == 0.0f) continue;
    const double ms = (double)s_in * (double)s_w[j] / (double)s_out;
    if (!(s_w[j] > 1e-30f && s_w[j] < 1e30f && ms > 1e-30 && ms < 1e30)) return false;
  }
  return true;
}
