// i8ie_calls.h -- argument blocks passed between the translation units of libi8ie_hip.so
#pragma once
#include <cstddef>
#include <cstdint>

#include <vector>

struct i8ie_ctx;

// Weights re-packed by a contraction kernel for its own K walk, cached in the layer handle: one buffer per packing
// key (the fragment order depends on the pass width, which depends on the batch size), never overwritten once made --
// a captured HIP graph keeps replaying the address it was captured with -- and freed with the layer.
struct I8ieWCache {
  struct Ent {
    unsigned long long key;
    void* buf;
  };
  std::vector<Ent> ents;
  void* find(unsigned long long key) const {
    for (const Ent& e : ents)
      if (e.key == key) return e.buf;
    return nullptr;
  }
};

// What every contraction launch hands its epilogue (oc', Linear's float bias, the requantiser of i8ie_requant.h, the optional
// ReLU, the accumulators' copy): one member `ep` of every call block, filled once per launch by i8ie_layer.hip.
struct I8ieEpilogue {
  const int32_t* ocp;  // oc[j] + 128 * wsum[j]
  const float* biasf;  // Linear: (float)q_b[j] / s_in (src/fully_connected.cc:44); nullptr for a convolution
  // per-channel layers: [Npad] multipliers fl(s_in * s_w[j] / s_out) and [Npad] weight scales s_w[j] (i8ie_requant.h);
  // s_w is then 1 when every column allows the guarded estimate and 0 when the layer takes the exact sequence.
  // nullptr: a per-tensor layer (the kernels' per-tensor instances).  The classifier head reads sbv alone.
  const float* msv;
  const float* sbv;
  float s_in, s_w, s_out;
  int zp_out, relu;
  int32_t* acc;  // nullptr, or where the INT32 sums (with oc', before the float bias) go
};

// one contraction launch: Linear (amode 0) or implicit-GEMM Conv2d over bordered NHWC (amode 1)
struct I8ieIgemmCall {
  const uint8_t* A;   // amode 0: [M][lda]; amode 1: window origin of pixel (0,0) in a bordered NHWC input
  size_t a_bytes;     // bytes readable from A
  int amode;
  long lda;
  int M, Kchunks;
  int Hp, Wp, C, KH, KW, sh, sw, OH, OW;  // amode 1: physical input dims, kernel, strides, output dims
  const int8_t* B;
  int Kpad, Npad, N;
  I8ieEpilogue ep;
  uint8_t* out;
  int ob;  // physical border of the NHWC output (amode 1 only)
  double Ktrue;
  int ksplit;        // amode 0 only: > 1 = split K over that many slices (partial must hold ksplit*M*N int32)
  int32_t* partial;
  I8ieWCache* wcache;  // amode 1: the layer handle's cache of weights re-packed by i8ie_pconv.hip / i8ie_tconv.hip; may be null
  // amode 1, honoured by i8ie_pconv.hip only (ask i8ie_pconv_takes first; the tiled kernel ignores them):
  int pool_k, pool_s;  // max_pool2d behind the (relu'd) convolution: `out` is then the pooled tensor, ob its border
  int a_s8, out_s8;    // input bytes / output bytes stored re-biased (^0x80: I8IE_LAYOUT_NHWC_S8)
};
// ONE definition of "this call carries a max-pool" for every file: a 1 x 1 window with a stride > 1 subsamples, so it IS a
// pool (src/functional.cc:36-64 makes no exception for it); kernels that fold pools take k > 1 only and must decline it
inline bool i8ie_is_pool(int pool_k, int pool_s) { return pool_k > 1 || (pool_k == 1 && pool_s > 1); }
int i8ie_igemm_launch(i8ie_ctx* ctx, const I8ieIgemmCall& c);
size_t i8ie_igemm_chunk_limit();  // activations at or beyond this many bytes run as several launches

// i8ie_pconv.hip: the patch-stationary form of the amode-1 contraction (input patch resident in LDS, weights
// streamed in fragment order).  Returns 1 when it took the launch, 0 when the shape is not its (the caller then
// runs the tiled kernel), < 0 on error.
int i8ie_pconv_try_launch(i8ie_ctx* ctx, const I8ieIgemmCall& c);
int i8ie_pconv_takes(i8ie_ctx* ctx, const I8ieIgemmCall& c);  // dry run of the same decision: 1 / 0

// i8ie_tconv.hip: the patch-stationary contraction with two wave teams half a tile apart (epilogues, patch waits
// and re-bias passes of one team under the MFMAs of the other).  Same return convention.
int i8ie_tconv_try_launch(i8ie_ctx* ctx, const I8ieIgemmCall& c);

// i8ie_flin.hip: Linear for few rows (m <= 256) in one launch: 16 features x 128 rows x all of K per block, both
// operands through LDS stages.  Takes the amode-0 fields of the call (ksplit / partial unused).
bool i8ie_flin_wants(int m, int n, int Kpad, bool force);
int i8ie_flin_launch(i8ie_ctx* ctx, const I8ieIgemmCall& c);

// i8ie_mlin.hip: Linear for many rows (m > 256) in one launch: 128 rows x 128 features x all of K per block (one per CU), both
// operands through a four-stage LDS-DMA ring fed by dedicated loader waves.  Takes the amode-0 fields of the call.
bool i8ie_mlin_wants(int m, int n, int Kpad, bool force);
int i8ie_mlin_launch(i8ie_ctx* ctx, const I8ieIgemmCall& c);

// ---- launch helpers of i8ie_gemm.hip (the first three) and i8ie_igemm.hip, called by i8ie_layer.hip and, where a handle is
// made or a stateless call runs (pad_rows, offsets, finish_offsets), by i8ie_layer_create.hip ---------------------------
int i8ie_launch_pad_rows(i8ie_ctx* ctx, const void* src, int rows, int k, void* dst, int rows_pad, int k_pad, int fill);
int i8ie_launch_offsets(i8ie_ctx* ctx, bool conv, const int8_t* qw, const int8_t* qb, int n, int K, float s_in, int zp_in,
                        int32_t* oc, int32_t* wsum);
int i8ie_launch_im2col(i8ie_ctx* ctx, const uint8_t* in, uint8_t* col, int n, int c, int h, int w, int kh, int kw, int oh,
                       int ow, int stride, int pad, int K, int Kpad, int zp);
int i8ie_launch_finish_offsets(i8ie_ctx* ctx, const int32_t* oc, const int32_t* wsum, const int8_t* qb, float s_in, int n,
                               int32_t* ocp, float* biasf);
int i8ie_launch_nchw_to_nhwc(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int b);
int i8ie_launch_nhwc_to_nchw(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int b);
int i8ie_launch_reborder(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int ib, int ob, int zp);
int i8ie_launch_fill_border(i8ie_ctx* ctx, uint8_t* out, int n, int c, int h, int w, int b, int zp);
int i8ie_launch_permute_k(i8ie_ctx* ctx, const int8_t* B, int8_t* Bp, int rows, int Kpad, int K, int c, int hw);
int i8ie_launch_repack_smallc(i8ie_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int c, int h, int w, int Hp, int Wg,
                              int ph, int pw, int zp, int rebias);
int i8ie_launch_maxpool_nhwc(i8ie_ctx* ctx, const uint8_t* in, int ib, uint8_t* out, int ob, int n, int c, int h, int w, int k,
                             int s, int relu_zp);

// i8ie_igemm.hip: the classifier head, Linear with at most i8ie_smalln_max_features() outputs in one launch (one wave per
// row, epilogue and, with out_f32, the dequantize fused)
struct I8ieSmallNCall {
  const uint8_t* A;
  size_t lda;
  int M, K;
  const int8_t* B;
  int Kpad, N;
  I8ieEpilogue ep;  // (msv unused: the head takes the exact sequence)
  uint8_t* out;
  float* out_f32;
};
int i8ie_smalln_max_features();
int i8ie_launch_linear_smalln(i8ie_ctx* ctx, const I8ieSmallNCall& c);
