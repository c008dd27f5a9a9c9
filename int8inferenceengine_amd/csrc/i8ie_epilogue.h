// i8ie_epilogue.h -- the quad epilogue of the contraction kernels whose lanes end with four consecutive output features of one
// pixel or row as INT32: gconv_mfma, gconv_direct, dconv_mfma and the flin kernels.
//     c += oc'  ->  (the accumulators' copy)  ->  (what the kernel puts in between: Linear's float bias)  ->  requantise  ->  store
// The order is the reference's (src/fully_connected.cc:42-48): the copy holds the sums with oc' and without the float bias.
// What differs between the kernels stays in them: which column a quad starts at, where the pixel lies, Linear's float bias.
// The kernels with an epilogue shaped by their store path (i8ie_igemm.hip's tiled kernel, i8ie_pconv.hip, i8ie_tconv.hip,
// i8ie_stem.hip, i8ie_first.hip, i8ie_mlin.hip, the head) keep theirs; so do deconv_mfma / deconv_direct and splitk_reduce,
// which measured slower on this form (deconv's one-phase instances 1 to 2 %, splitk_reduce 1.4 us per launch).
#pragma once
#include "i8ie_calls.h"
#include "i8ie_requant.h"

// the epilogue's part of a kernel argument block
struct I8ieEpiArgs {
  const int32_t* ocp;
  const float* biasf;
  const float* msv;  // PC instances (per-channel layers): multipliers and weight scales per column (i8ie_requant.h)
  const float* sbv;
  I8ieRequant rq;
  int relu_lo;   // zp_out when relu is fused, else 0
  int32_t* acc;  // nullptr or [rows][N]
};

inline I8ieEpiArgs i8ie_epi_args(const I8ieEpilogue& e) {
  I8ieEpiArgs a;
  a.ocp = e.ocp; a.biasf = e.biasf; a.msv = e.msv; a.sbv = e.sbv;
  a.rq = i8ie_make_requant(e.s_in, e.s_w, e.s_out, e.zp_out);
  a.relu_lo = e.relu ? e.zp_out : 0;
  a.acc = e.acc;
  return a;
}

#if defined(__HIPCC__)
// what a quad reads per column: oc', and under PC the multiplier and the weight scale
template <bool PC>
struct I8ieQuadCols {
  int oc[4];
  float4 ms;
  float sb[4];
};
template <>
struct I8ieQuadCols<false> {
  int oc[4];
};

// Columns j0 .. j0 + nf - 1 are live (1 <= nf <= 4): a dead byte repeats the last live column, so nothing is read past N and
// no value is made up (a zero multiplier would send the whole dword to the replay).
template <bool PC>
__device__ __forceinline__ I8ieQuadCols<PC> i8ie_epi_cols(const I8ieEpiArgs& ep, int j0, int nf) {
  I8ieQuadCols<PC> q;
  float ms[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + (r < nf ? r : nf - 1);
    q.oc[r] = ep.ocp[j];
    if constexpr (PC) {
      ms[r] = ep.msv[j];
      q.sb[r] = ep.sbv[j];
    }
  }
  if constexpr (PC) q.ms = make_float4(ms[0], ms[1], ms[2], ms[3]);
  return q;
}
// The same as 16-byte loads, for a caller whose arrays are padded to whole quads and 16-byte aligned at j0 (Linear: [Npad])
template <bool PC>
__device__ __forceinline__ I8ieQuadCols<PC> i8ie_epi_cols_vec(const I8ieEpiArgs& ep, int j0) {
  I8ieQuadCols<PC> q;
  const int4 o = *reinterpret_cast<const int4*>(ep.ocp + j0);
  q.oc[0] = o.x; q.oc[1] = o.y; q.oc[2] = o.z; q.oc[3] = o.w;
  if constexpr (PC) {
    q.ms = *reinterpret_cast<const float4*>(ep.msv + j0);
    const float4 s = *reinterpret_cast<const float4*>(ep.sbv + j0);
    q.sb[0] = s.x; q.sb[1] = s.y; q.sb[2] = s.z; q.sb[3] = s.w;
  }
  return q;
}

template <bool PC>
__device__ __forceinline__ uint32_t i8ie_epi_pack(const I8ieEpiArgs& ep, const int (&c)[4], const I8ieQuadCols<PC>& q) {
  if constexpr (PC)
    return i8ie_requant_pack4_pc(c, ep.rq, q.ms, q.sb, ep.relu_lo, (float)ep.relu_lo);
  else
    return i8ie_requant_pack4(c, ep.rq, ep.relu_lo, (float)ep.relu_lo);
}

// the accumulators' copy: acc0 = the quad's first element, row * N + j0
__device__ __forceinline__ void i8ie_epi_copy_acc(const I8ieEpiArgs& ep, const int (&c)[4], long long acc0, int nf) {
  if (ep.acc == nullptr) return;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r < nf) ep.acc[acc0 + r] = c[r];
}

// `whole`: all four bytes are live and `o` is dword aligned
__device__ __forceinline__ void i8ie_epi_store(uint8_t* o, uint32_t packed, bool whole, int nf) {
  if (whole) {
    *reinterpret_cast<uint32_t*>(o) = packed;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < nf) o[r] = (uint8_t)(packed >> (8 * r));
  }
}

// `c`: the quad's sums without oc'; `pre_pack(c)` runs between the accumulators' copy and the requantiser
template <bool PC, class Pre>
__device__ __forceinline__ void i8ie_epi_finish(const I8ieEpiArgs& ep, int (&c)[4], const I8ieQuadCols<PC>& q, int nf,
                                                long long acc0, uint8_t* o, bool whole, Pre&& pre_pack) {
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] += q.oc[r];
  i8ie_epi_copy_acc(ep, c, acc0, nf);
  pre_pack(c);
  i8ie_epi_store(o, i8ie_epi_pack<PC>(ep, c, q), whole, nf);
}
template <bool PC>
__device__ __forceinline__ void i8ie_epi_finish(const I8ieEpiArgs& ep, int (&c)[4], const I8ieQuadCols<PC>& q, int nf,
                                                long long acc0, uint8_t* o, bool whole) {
  i8ie_epi_finish<PC>(ep, c, q, nf, acc0, o, whole, [](int (&)[4]) {});
}
#endif
