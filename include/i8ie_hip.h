/*
 * i8ie_hip.h -- C-ABI of libi8ie_hip.so: the MI355X (gfx950) implementation of
 * the INT8 hot path of t0037799/INT8InferenceEngine.
 *
 * This is the boundary the rebuilt pybind11 module `_CXX_i8ie` (and any other
 * FFI: ctypes, cgo, JNI) binds.  Plain pointers and sizes only; no C++ types,
 * no torch types, no exceptions cross it.  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - every function returns an int status: I8IE_OK (0) or a negative code;
 *     i8ie_last_error() returns a thread-local message for the last failure.
 *     (The reference throws message-less std::exception or segfaults on
 *     misuse: include/tensor.h:114-130, src/conv2d.cc:105.)
 *   - "dev" pointers are device (HBM) pointers, obtained from i8ie_malloc or
 *     from any other HIP allocation in the same process (e.g. a torch tensor's
 *     data_ptr()).  Ops enqueue on the ctx's HIP stream and return without
 *     waiting; i8ie_sync() or a D2H copy waits.
 *   - tensors use the reference's layouts: activations u8 NCHW / [m,k]
 *     row-major, weights s8 [out, in*kh*kw] row-major (K ordered c,kh,kw),
 *     per-tensor fp32 scale + u8 zero point (include/tensor.h:152-154).
 *   - arithmetic is the reference's, bit for bit: exact int32 accumulation,
 *     fp32 epilogue without contraction or reassociation.
 */
#ifndef I8IE_HIP_H
#define I8IE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I8IE_OK 0
#define I8IE_ERR_ARG (-1)   /* bad argument (null pointer, non-positive size, stride 0 ...) */
#define I8IE_ERR_STATE (-2) /* call made in the wrong state (e.g. forward before qparams set) */
#define I8IE_ERR_HIP (-3)   /* a HIP runtime call failed; message has hipGetErrorString */
#define I8IE_ERR_OOM (-4)   /* device allocation failed */

typedef struct i8ie_ctx i8ie_ctx;     /* one per (thread-of-control, device): stream + workspace */
typedef struct i8ie_layer i8ie_layer; /* a converted (INT8) Linear or Conv2d with device-resident weights */
/* Threading: a ctx and the layer handles created on it belong to ONE host thread at a time.  A layer handle caches
 * state keyed by the call (offset vectors per (s_in, zp_in), weight panels re-packed per kernel shape) without locks:
 * do not forward the same handle from two host threads at once; one ctx + its own handles per thread is the model. */

/* ---- library / context ------------------------------------------------- */
const char* i8ie_last_error(void);
int i8ie_version(void);                 /* ABI version, currently 1 */
int i8ie_device_count(int* n);
int i8ie_ctx_create(int device, i8ie_ctx** out);                       /* own stream */
int i8ie_ctx_create_on_stream(int device, void* hip_stream, i8ie_ctx** out); /* borrow a hipStream_t */
int i8ie_ctx_destroy(i8ie_ctx* ctx);
void* i8ie_ctx_stream(i8ie_ctx* ctx);   /* the hipStream_t, as void* */
int i8ie_sync(i8ie_ctx* ctx);

/* Options.  I8IE_OPT_FORCE_FALLBACK = 1 makes every layer handle take the any-geometry
 * path (materialised im2col + v1 GEMM, separate ReLU) instead of the implicit-GEMM paths;
 * results are identical, it exists so that tests can cover both. */
#define I8IE_OPT_FORCE_FALLBACK 1
/* I8IE_OPT_KERNEL_VARIANT = 2 selects among compiled variants of the contraction kernel (all
 * produce identical bytes; a tuning / A-B timing aid, 0 = default). */
#define I8IE_OPT_KERNEL_VARIANT 2
/* The values the library understands.  Anything else behaves like 0 (earlier numbers named timing experiments,
 * retired at 9e2c9d6).  A value changes the one thing it names and leaves every other choice automatic.  A
 * convolution with a max-pool or a re-biased layout (below) folds them into the patch-stationary kernel only where
 * that kernel is tried and takes the launch; otherwise the pool and the re-bias run as launches of their own. */
#define I8IE_VARIANT_AUTO 0            /* automatic selection per launch */
#define I8IE_VARIANT_IGEMM_REGSTAGE 3  /* conv: the tiled contraction kernel only, 128 x 128 tiles, one LDS stage filled through registers;
                                          Linear: the tiled kernel where the many-row kernel would run */
#define I8IE_VARIANT_IGEMM_DMA 5       /* conv: the tiled contraction kernel only, 128 x 128 tiles, one LDS stage filled by LDS-DMA;
                                          Linear: where the tiled kernel runs, DMA staging (its default: registers) */
#define I8IE_VARIANT_TILED 11          /* tiled contraction kernel everywhere: no patch-stationary conv, no first-stage kernel,
                                          split-K Linear, classifier head without its MFMA form */
#define I8IE_VARIANT_STEM_WHOLE 12     /* first-stage kernel (csrc/i8ie_stem.hip): whole images per block at any batch size (no parts) */
#define I8IE_VARIANT_STEM_SIMD_ROLES 13 /* first-stage kernel with its two wave roles on separate SIMDs (A/B of the placement: 8 % slower, profiles/r04_stem_roles.txt) */
#define I8IE_VARIANT_PCONV 50          /* conv: patch-stationary kernel (csrc/i8ie_pconv.hip) at any batch size, else the tiled kernel */
#define I8IE_VARIANT_PCONV_2PASS 54    /* the same, N = 384 as two passes of 192 and no 128-wide pass split */
#define I8IE_VARIANT_TCONV 70          /* conv: two-team patch-stationary kernel (csrc/i8ie_tconv.hip) wherever its shape rules allow, else the tiled kernel */
#define I8IE_VARIANT_FLIN 80           /* few-row Linear kernel (csrc/i8ie_flin.hip) below its automatic feature threshold */
#define I8IE_VARIANT_FLIN_128 81       /* the same in its 128-row x 16-feature form at up to 128 rows (default above 64 rows: 64 x 32) */
#define I8IE_VARIANT_MLIN 83           /* many-row Linear kernel (csrc/i8ie_mlin.hip) from 257 rows on and below its automatic feature threshold */
#define I8IE_VARIANT_MLIN_64 84        /* the same with 64-row block tiles (automatic where 128-row tiles give at most half the CUs a block) */
#define I8IE_VARIANT_MLIN_128 85       /* the same with 128-row block tiles at any row count above 256 */
/* I8IE_OPT_PROFILE_STRIDE = 3: while profiling, bracket only every value-th eligible launch
 * (default 1 = all).  Event packets cost a few microseconds each on the stream; a stride that is
 * coprime with the launches per batch samples every kernel over a few batches. */
#define I8IE_OPT_PROFILE_STRIDE 3
/* I8IE_OPT_CU_LIMIT = 4: the compute units the ctx's stream may use, for a ctx created on a stream with a CU mask
 * (hipExtStreamCreateWithCUMask + i8ie_ctx_create_on_stream): one-block-per-CU kernels size their grids and their
 * work splits by min(device CUs, value).  0 (default) = all of the device's. */
#define I8IE_OPT_CU_LIMIT 4
int i8ie_ctx_set_option(i8ie_ctx* ctx, int option, int value);

/* Activation layouts accepted by the *_fused / *_nhwc entry points.  NCHW is the
 * reference's layout (include/tensor.h); NHWC is the engine's internal layout between
 * layers (the reference's own GEMM output is HWC before its transpose, src/conv2d.cc:134-136). */
#define I8IE_LAYOUT_NCHW 0
#define I8IE_LAYOUT_NHWC 1
/* NHWC with every byte stored as value ^ 0x80 (= value - 128 as s8; border bytes: zero point ^ 0x80).  The matrix
 * cores have no unsigned 8-bit operand: a conv kernel re-biases its activations on the way in (the exact term
 * 128 * sum_k q_w[j,k] joins oc[j]).  Between two conv layers of this library the producer can store that form
 * directly and the consumer skip its re-bias pass.  Accepted as in_layout / out_layout of the conv layer forwards;
 * i8ie_rebias_u8 converts a whole buffer either way. */
#define I8IE_LAYOUT_NHWC_S8 2

/* ---- per-kernel timing (measurement aid; nothing like it in the reference) ---
 * Between start and stop every kernel launch of this ctx is bracketed by HIP
 * events on the ctx's stream; stop waits for the stream and returns one entry
 * per kernel name: launches, summed device time, summed algorithmic integer
 * ops (2 x MACs, unpadded dimensions) and algorithmic bytes. */
typedef struct i8ie_profile_entry {
  char name[64];
  uint64_t launches;
  double total_ms;
  double total_ops;
  double total_bytes;
} i8ie_profile_entry;
/* mfma_kernels_only != 0: bracket only the contraction kernels (those with algorithmic
 * ops), which keeps the instrumentation overhead of a timed region small */
int i8ie_profile_start(i8ie_ctx* ctx, int mfma_kernels_only);
int i8ie_profile_stop(i8ie_ctx* ctx, i8ie_profile_entry* entries, int max_entries, int* n_entries);

/* ---- device memory (replaces `new T[]` + py::capsule, include/tensor.h:26-61) */
/* Blocks come from a per-ctx caching allocator: i8ie_free() never blocks, and a freed
 * block may be handed to the next i8ie_malloc() at once.  That is safe because every
 * consumer of ctx memory runs on the ctx's stream; do not read a block from another
 * stream after freeing it.  i8ie_trim() returns cached blocks to the driver. */
int i8ie_malloc(i8ie_ctx* ctx, size_t bytes, void** dev);
int i8ie_free(i8ie_ctx* ctx, void* dev);
int i8ie_trim(i8ie_ctx* ctx);
int i8ie_memory_stats(i8ie_ctx* ctx, size_t* bytes_live, size_t* bytes_cached, size_t* n_device_allocs);
int i8ie_memcpy_h2d(i8ie_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int i8ie_memcpy_d2h(i8ie_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* waits */
int i8ie_memcpy_d2d(i8ie_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int i8ie_memset(i8ie_ctx* ctx, void* dst_dev, int byte, size_t bytes);

/* ---- whole-forward replay as one HIP graph (small per-GPU batches are launch-bound) ----------
 * Nothing like it in the reference (its forward is a chain of host calls, i8ie/module.py); on the GPU a 125-image
 * AlexNet shard spends more time between its ~14 dependent launches than inside them.  Between begin and end every
 * launch and asynchronous copy this ctx issues is recorded instead of run; device blocks freed meanwhile stay owned
 * by the graph (their addresses are baked into it) until i8ie_graph_destroy.  Run the same calls once eagerly
 * first: workspace growth, weight re-packing caches and offset vectors must exist before the capture (anything
 * that would synchronise inside it fails the capture with I8IE_ERR_HIP).  Replays are ordered on the ctx's
 * stream like any other launch; inputs and outputs are the device buffers the captured calls used. */
typedef struct i8ie_graph i8ie_graph;
/* While graphs captured on a ctx are alive its workspace is pinned: a later call that needs a larger one gets a new
 * allocation and the old one stays until the last graph is destroyed.  Weights re-packed by a kernel are kept per
 * packing key in the layer handle and never overwritten, so a replay after an eager forward at another batch size
 * still finds its own.  A layer handle must outlive the graphs that captured its forward.
 * i8ie_ctx_is_capturing: *yes = 1 between begin and end (owners of cached device blocks use it to route frees
 * to i8ie_free, which hands the block to the graph, instead of to a cache of their own). */
int i8ie_ctx_is_capturing(i8ie_ctx* ctx, int* yes);
int i8ie_graph_begin(i8ie_ctx* ctx);
int i8ie_graph_end(i8ie_ctx* ctx, i8ie_graph** out);
int i8ie_graph_launch(i8ie_graph* g);
int i8ie_graph_nodes(i8ie_graph* g, int* kernel_nodes, int* all_nodes);
int i8ie_graph_destroy(i8ie_graph* g);

/* ---- asynchronous host<->device transfers -------
 * Nothing like it in the reference (its tensors are host arrays, include/tensor.h:26-61); this is
 * what lets a caller overlap the logits read-back and the next batch's upload with the kernels.
 * Host buffers given to the *_async copies must come from i8ie_host_malloc (pinned); a pageable
 * pointer is refused with I8IE_ERR_ARG.  `on_copy_stream` != 0 issues the copy on the ctx's second
 * (transfer) stream so that it runs beside the kernels; order it against the compute stream with
 * events: record on one stream, i8ie_stream_wait_event on the other (device-side wait, the host
 * does not block), or i8ie_event_synchronize to block the host until the recorded point. */
typedef struct i8ie_event i8ie_event;
int i8ie_host_malloc(i8ie_ctx* ctx, size_t bytes, void** host);
int i8ie_host_free(i8ie_ctx* ctx, void* host);
/* *yes = 1 when [p, p+bytes) lies inside one live i8ie_host_malloc block of this ctx */
int i8ie_host_is_pinned(i8ie_ctx* ctx, const void* p, size_t bytes, int* yes);
int i8ie_memcpy_h2d_async(i8ie_ctx* ctx, void* dst_dev, const void* src_pinned, size_t bytes, int on_copy_stream);
int i8ie_memcpy_d2h_async(i8ie_ctx* ctx, void* dst_pinned, const void* src_dev, size_t bytes, int on_copy_stream);
int i8ie_event_create(i8ie_ctx* ctx, i8ie_event** out);
int i8ie_event_record(i8ie_ctx* ctx, i8ie_event* ev, int on_copy_stream);
int i8ie_stream_wait_event(i8ie_ctx* ctx, i8ie_event* ev, int copy_stream_waits);
int i8ie_event_synchronize(i8ie_event* ev);
int i8ie_event_query(i8ie_event* ev, int* done);
int i8ie_event_destroy(i8ie_event* ev);

/* ---- elementwise ops ---------------------------------------------------- */
/* quantize(Tensor<float>&, scale, zp)  src/quantize_utils.cc:44-52, src/pybind11.cc:41-45
 * q = (u8)(x / scale + zp): fp32 divide, add, truncate, low 8 bits (no clamp). */
int i8ie_quantize_f32_u8(i8ie_ctx* ctx, const float* in_dev, uint8_t* out_dev, int64_t n,
                         float scale, uint8_t zero_point);
/* dequantize(Tensor<u8>&)  src/quantize_utils.cc:38-42,54-58, src/pybind11.cc:46-48 */
int i8ie_dequantize_u8_f32(i8ie_ctx* ctx, const uint8_t* in_dev, float* out_dev, int64_t n,
                           float scale, uint8_t zero_point);
/* out = in ^ 0x80 over n bytes (in place allowed): plain u8 <-> the re-biased bytes of I8IE_LAYOUT_NHWC_S8 */
int i8ie_rebias_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t n);
/* relu<u8_t>  src/functional.cc:15-26:  out = in > zp ? in : zp */
int i8ie_relu_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t n,
                 uint8_t zero_point);
/* max_pool2d<u8_t>  src/functional.cc:36-64: NCHW, k x k window, stride s, floor, no padding */
int i8ie_maxpool2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c,
                      int h, int w, int kernel_size, int stride);
/* the s8 instantiations the reference registers as well (src/functional.cc:78-82): the generic templates,
 * relu = x > 0 ? x : 0 (src/functional.cc:5-13), max-pool with a running maximum starting at -127
 * (src/functional.cc:28-31, 36-64).  NCHW, no quantisation parameters involved. */
int i8ie_relu_s8(i8ie_ctx* ctx, const int8_t* in_dev, int8_t* out_dev, int64_t n);
int i8ie_maxpool2d_s8(i8ie_ctx* ctx, const int8_t* in_dev, int8_t* out_dev, int n, int c, int h, int w,
                      int kernel_size, int stride);
/* Calibrator::sample  src/calibrator.cc:6-23 on the device, without copying the layer output to the host.
 * The reference keeps 1000 samples: the first 1000 values seen fill the slots, every later value draws
 * idx uniform in [0, 2000] from an UNSEEDED mt19937 (std::random_device) and overwrites slot idx when idx < 1000, so
 * each slot ends up holding the last value that drew it.  Here the draw of global element number g is a
 * counter-based hash of (seed, g): same distribution of slot contents, a different (and, unlike the reference's,
 * reproducible) random stream.  `samples_dev` holds 1000 floats, `scratch_dev` 1000 ints; `seen_before` = values
 * already sampled by earlier calls on this layer.  The host-side replay of the reference's own mt19937 stream
 * (golden-pinned, tests/golden/ref_calibrator*.npz) stays in _CXX_i8ie for seeded runs. */
int i8ie_calib_sample_f32(i8ie_ctx* ctx, const float* data_dev, int64_t n, int64_t seen_before, uint64_t seed,
                          float* samples_dev, int* scratch_dev);

/* ---- Histogram calibration (additive, not in the reference) ----------------
 * A second observer beside the 1000-slot reservoir above: it sees EVERY value of a layer's FP32 output.  Over all finite
 * values observed so far it keeps the exact `min` and `max`, a count of the non-finite values (NaN, +-Inf: counted, otherwise
 * ignored), B = 2048 counters of 64 bits and one integer exponent e.  A value with |x| < 2^-126 (a denormal, +-0) counts as
 * +0, for the minimum and maximum too, whatever the device's flush mode.
 *   bins      bin i covers [(i - 1024) * 2^e, (i - 1023) * 2^e); a finite x falls in bin floor(x * 2^-e) + 1024, the floor of
 *             the exact product (it does not depend on rounding mode, FMA contraction or summation order).
 *   exponent  e is the smallest integer >= -100 with absmax < 1024 * 2^e, strictly, over everything seen so far.  When a
 *             later tensor raises absmax, e grows by d and the histogram is folded d times: old bin i goes to
 *             512 + floor(i / 2), counts add.  The state is therefore a function of the multiset of values alone: not of the
 *             chunking, the order of the chunks or the order of the atomics.
 * The state is one caller-owned device buffer of i8ie_calib_hist_state_bytes() bytes, 16-byte aligned: this header, then
 * uint64_t hist[2048].  At rest (between calls) `scratch` is zero; a state that was never observed has min = +Inf,
 * max = -Inf, exponent = -100 and zero counters (i8ie_calib_hist_reset). */
#define I8IE_CALIB_HIST_BINS 2048
typedef struct i8ie_calib_hist_header {
  float min, max;      /* of the finite values seen; +Inf / -Inf while there were none */
  int32_t exponent;    /* e */
  uint32_t scratch[3]; /* of an observe in flight (the chunk's minimum and maximum as ordered keys, a block ticket); 0 at rest */
  uint64_t nonfinite;  /* NaN and +-Inf seen */
} i8ie_calib_hist_header;
size_t i8ie_calib_hist_state_bytes(void);
int i8ie_calib_hist_reset(i8ie_ctx* ctx, void* state_dev);
/* Observe n floats (n >= 0; data_dev aligned to 4 bytes, any offset from a 16-byte boundary).  Asynchronous on the ctx stream,
 * never synchronises with the host: the exponent lives on the device.  Two launches (three above 2^30 values, one more per
 * 2^30): "calib_hist_stats" takes min / max / absmax / the non-finite count, and its last block computes the new e and folds the
 * counters in place when e grew; "calib_hist_count" reads e from the state and counts in LDS (32-bit LDS atomics, one table
 * per wave), then adds the non-zero counters to the 64-bit global ones.  n == 0 launches nothing. */
int i8ie_calib_hist_observe_f32(i8ie_ctx* ctx, const float* data_dev, int64_t n, void* state_dev);
/* The state, read back once (synchronises the ctx stream): the header and the 2048 counters. */
int i8ie_calib_hist_read(i8ie_ctx* ctx, const void* state_dev, i8ie_calib_hist_header* header, uint64_t* hist_host);
/* Host only.  The last step of Calibrator::get_range (src/calibrator.cc:31-36), from `out_min = fmin(...)` on: the range is
 * widened to include 0, zero_point = (u8)(255 * (0 - min) / (max - min + 1e-09)) in double, scale = (max - min) / 255 when
 * zero_point == 0 and (0 - min) / zero_point otherwise in float, and a scale of 0 becomes 1.  Shared by the reservoir and by
 * every method below. */
void i8ie_calib_range_qparams(float out_min, float out_max, float* scale, uint8_t* zero_point);
/* Host only, no ctx.  (lo, hi) of a state read back; (scale, zero_point) is i8ie_calib_range_qparams(lo, hi).  With T the
 * total count:
 *   I8IE_CALIB_MINMAX      lo = min, hi = max.
 *   I8IE_CALIB_PERCENTILE  param = p, 50 < p <= 100 (I8IE_ERR_ARG otherwise); k = floor((1 - p / 100) * T) in double.  lo is the
 *                          lower edge of the first bin at which the ascending cumulative count exceeds k, but not below min;
 *                          hi the upper edge of the first bin at which the descending cumulative count exceeds k, but not
 *                          above max.  p = 100 is MINMAX exactly.
 *   I8IE_CALIB_MSE         (lo0, hi0) = (fmin(min, 0), fmax(max, 0)).  Candidate j = 16..64 is (float(lo0 * j / 64),
 *                          float(hi0 * j / 64)) (the product and quotient in double) with its (s_j, z_j); its error is
 *                          E_j = sum_i h_i * (c_i - d_j(c_i))^2 over the bins in ascending i, accumulated sequentially in double
 *                          without contraction, c_i = (i - 1023.5) * 2^e, d_j(c) = (q - z_j) * s_j, q = min(255, max(0,
 *                          trunc(c / s_j + z_j))): down_scale's clamp and truncation in double.  The smallest E_j wins, ties
 *                          go to the larger j.
 * A state that saw no finite value gives (0, 0), hence (scale, zero_point) = (1, 0), as an empty reservoir does. */
enum { I8IE_CALIB_MINMAX = 0, I8IE_CALIB_PERCENTILE = 1, I8IE_CALIB_MSE = 2 };
int i8ie_calib_hist_range(const i8ie_calib_hist_header* header, const uint64_t* hist, int method, double param, float* lo,
                          float* hi);

/* down_scale  src/quantize_utils.cc:27-36 (standalone requantiser; the layers fuse it) */
int i8ie_down_scale(i8ie_ctx* ctx, const int32_t* acc_dev, uint8_t* out_dev, int64_t n, float sa,
                    float sb, float sc, uint8_t zp_c);
/* the same per column: acc [rows, cols] int32, column j requantised with its own weight scale sb_dev[j]
 * (device, float [cols]):  deq = ((float)C[., j] * sa) * sb[j];  q = deq / sc + (float)zp_c;  clamp / truncate */
int i8ie_down_scale_per_channel(i8ie_ctx* ctx, const int32_t* acc_dev, uint8_t* out_dev, int64_t rows, int cols,
                                float sa, const float* sb_dev, float sc, uint8_t zp_c);

/* ---- FP32 ops: the path taken before convert() and while calibrating -------
 * Conv2d/Linear::forward_prop(Tensor<float>&&)  src/conv2d.cc:63-98, src/fully_connected.cc:5-21
 * (cblas_sgemm + bias); relu<float>, max_pool2d<float>  src/functional.cc:5-13,36-64.
 * Off the timed INT8 path: plain correct kernels, pinned to the reference's own
 * tolerance (atol 0.1 vs torch, unittest/test_layers.py:10-11). */
int i8ie_linear_f32(i8ie_ctx* ctx, const float* in_dev, int m, int k, const float* w_dev,
                    const float* b_dev, int n, float* out_dev);
int i8ie_conv2d_f32(i8ie_ctx* ctx, const float* in_dev, int n, int c, int h, int w,
                    const float* w_dev, const float* b_dev, int kc, int kh, int kw, int stride,
                    int pad, float* out_dev);
/* i8ie_conv2d_f32 with groups (src/conv2d.cc:63-98 per group; groups: not in the reference): w_dev is
 * [kc, c/groups, kh, kw], output features [g*kc/groups, (g+1)*kc/groups) see input channels [g*c/groups, (g+1)*c/groups).
 * groups must divide c and kc (I8IE_ERR_ARG otherwise); groups == 1 is i8ie_conv2d_f32.  One launch, the group index
 * a grid dimension.  The path taken before convert() and while calibrating. */
int i8ie_conv2d_f32_grouped(i8ie_ctx* ctx, const float* in_dev, int n, int c, int h, int w,
                            const float* w_dev, const float* b_dev, int kc, int kh, int kw, int stride,
                            int pad, int groups, float* out_dev);
/* i8ie_conv2d_f32_grouped with a dilation (not in the reference; torch.nn.Conv2d's dilation=): tap (ky, kx) of the window
 * of output pixel (oy, ox) reads input pixel (oy*stride - pad + ky*dilation, ox*stride - pad + kx*dilation), i.e.
 * src/conv2d.cc:63-98 per group with the kernel inflated by zeros to dilation*(k-1)+1 (see i8ie_conv2d_create_dilated).
 * oh = (h + 2*pad - dilation*(kh-1) - 1)/stride + 1.  dilation >= 1 and the inflated kernel no larger than the padded
 * input (I8IE_ERR_ARG otherwise, before any device call).  dilation == 1 is i8ie_conv2d_f32_grouped bit for bit: the same
 * kernel, the dilation only in its gather table.  The path taken before convert() and while calibrating. */
int i8ie_conv2d_f32_dilated(i8ie_ctx* ctx, const float* in_dev, int n, int c, int h, int w,
                            const float* w_dev, const float* b_dev, int kc, int kh, int kw, int stride,
                            int pad, int groups, int dilation, float* out_dev);
/* i8ie_conv2d_f32_dilated with the geometry per axis (see i8ie_conv2d_create_rect): the same FP32 implicit-GEMM kernel, the
 * per-axis geometry only in its gather table and window origin.  With equal pairs it is i8ie_conv2d_f32_dilated bit for bit.
 * A bad geometry is I8IE_ERR_ARG before any device call. */
struct i8ie_conv_geom;
int i8ie_conv2d_f32_rect(i8ie_ctx* ctx, const float* in_dev, int n, int c, int h, int w, const float* w_dev,
                         const float* b_dev, int kc, int groups, const struct i8ie_conv_geom* geom, float* out_dev);
/* ConvTranspose2d in FP32 (not in the reference; the definition of torch.nn.ConvTranspose2d with groups = 1,
 * dilation = 1, a square kernel): out[n, oc, iy*s - p + ky, ix*s - p + kx] += in[n, ic, iy, ix] * w[ic, oc, ky, kx], + b[oc].
 * w_dev is [c, kc, k, k], out_dev [n, kc, oh, ow] with oh = (h - 1)*stride - 2*pad + k + output_pad.  stride >= 1,
 * 0 <= pad <= k - 1, 0 <= output_pad < stride (I8IE_ERR_ARG otherwise, before any device call).  Equivalently
 * src/conv2d.cc:63-98 (stride 1, padding 0) of the zero-inserted, padded input with the flipped, transposed kernel; the
 * kernel sums only the taps that meet a real pixel, in (ic, ky, kx) order.  The path taken before convert() and while
 * calibrating. */
int i8ie_conv_transpose2d_f32(i8ie_ctx* ctx, const float* in_dev, int n, int c, int h, int w,
                              const float* w_dev, const float* b_dev, int kc, int k, int stride, int pad,
                              int output_pad, float* out_dev);
int i8ie_relu_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int64_t n);
int i8ie_maxpool2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h,
                       int w, int kernel_size, int stride);

/* ---- weight preparation (host side, one-shot) --------------------------- */
/* quantize_weight  src/layer.cc:6-26: joint min/max over weight and bias,
 * s_w = (max - min) / 127, q = (s8)(x / s_w) truncating, unclamped.  Host pointers. */
int i8ie_quantize_weight(const float* w_host, int64_t nw, const float* b_host, int64_t nb,
                         int8_t* qw_host, int8_t* qb_host, float* scale_out);
/* per-output-channel weights (opt-in; not the reference's rule).  Row j = w[j*row_len .. +row_len) (Conv2d:
 * in*kh*kw values, Linear: in), with its bias b[j] (b_host may be NULL: zero bias).  IEEE fp32:
 *   a_j = max(max_k |w[j,k]|, |b[j]|);  s_w[j] = a_j / 127  (a_j == 0: 1)
 *   q_w[j,k] = (s8) clamp(rint(w[j,k] / s_w[j]), -127, 127),  q_b[j] likewise   (rint: round half to even)
 * scales_host: float [rows].  The bias stays s8 at its row's scale, so the offset vector and Linear's float bias
 * step are unchanged; only the requantiser reads s_w[j] ("Per-channel weight scales"). */
int i8ie_quantize_weight_per_channel(const float* w_host, int rows, int64_t row_len, const float* b_host,
                                     int8_t* qw_host, int8_t* qb_host, float* scales_host);

/* ---- zero-point offset vectors (device) --------------------------------- */
/* src/conv2d.cc:117-124:  t_j = sum_k zp_in*q_w[j,k] accumulated sequentially in fp32;
 * oc[j] = (int)((float)q_b[j] / s_in - t_j).  qw_dev: s8 [kc, K]; oc_dev: int32 [kc]. */
int i8ie_conv_offsets(i8ie_ctx* ctx, const int8_t* qw_dev, const int8_t* qb_dev, int kc, int K,
                      float s_in, uint8_t zp_in, int32_t* oc_dev);
/* src/fully_connected.cc:30-38:  oc[i] = (int)(-t_i) */
int i8ie_linear_offsets(i8ie_ctx* ctx, const int8_t* qw_dev, int n, int k, uint8_t zp_in,
                        int32_t* oc_dev);

/* ---- stateless layer entry points (raw device pointers) ------------------ */
/* Linear::forward_prop(Tensor<u8>&&)  src/fully_connected.cc:22-52
 *   C = X*W^T + oc (exact int32);  C = (int)((float)C + (float)q_b[j]/s_in);
 *   out = down_scale(C, s_in, s_w, s_out, zp_out).
 * in [m,k] u8, qw [n,k] s8, qb [n] s8, oc [n] int32 (from i8ie_linear_offsets), out [m,n] u8.
 * acc_dbg_dev: NULL, or int32 [m,n] receiving C BEFORE the float bias step (the
 * MKL cblas_gemm_s8u8s32 result, src/fully_connected.cc:39-41).               */
int i8ie_linear_u8s8(i8ie_ctx* ctx, const uint8_t* in_dev, int m, int k, const int8_t* qw_dev,
                     const int8_t* qb_dev, int n, const int32_t* oc_dev, float s_in, float s_w,
                     float s_out, uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);
/* Conv2d::forward_prop(Tensor<u8>&&)  src/conv2d.cc:100-142
 *   per image: im2col (pad value zp_in) -> C = A*W^T + oc -> down_scale -> HWC->CHW.
 * in NCHW [n,c,h,w] u8, qw [kc, c*kh*kw] s8, oc [kc] int32 (from i8ie_conv_offsets),
 * out NCHW [n,kc,oh,ow] u8, oh = (h - kh + 2*pad)/stride + 1.
 * acc_dbg_dev: NULL, or int32 [n, oh*ow, kc]: the pre-requant accumulators
 * (the MKL result, src/conv2d.cc:131-133).                                   */
int i8ie_conv2d_u8s8(i8ie_ctx* ctx, const uint8_t* in_dev, int n, int c, int h, int w,
                     const int8_t* qw_dev, int kc, int kh, int kw, int stride, int pad,
                     uint8_t zp_in, const int32_t* oc_dev, float s_in, float s_w, float s_out,
                     uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);

/* Conv2d::forward_prop(Tensor<u8>&&)  src/conv2d.cc:100-142, one reference convolution per group; groups: not in the
 * reference.  i8ie_conv2d_u8s8 with `groups` dividing c and kc (I8IE_ERR_ARG otherwise): qw [kc, (c/groups)*kh*kw],
 * oc [kc] from i8ie_conv_offsets on that matrix (K = (c/groups)*kh*kw).  groups == 1 is i8ie_conv2d_u8s8 itself;
 * groups > 1 reads the weights back and packs them for this one call (it waits for the stream): a layer handle
 * (i8ie_conv2d_create_grouped) keeps them packed. */
int i8ie_conv2d_u8s8_grouped(i8ie_ctx* ctx, const uint8_t* in_dev, int n, int c, int h, int w,
                             const int8_t* qw_dev, int kc, int kh, int kw, int stride, int pad, int groups,
                             uint8_t zp_in, const int32_t* oc_dev, float s_in, float s_w, float s_out,
                             uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);

/* i8ie_conv2d_u8s8_grouped with a dilation (see i8ie_conv2d_create_dilated; not in the reference): qw [kc, (c/groups)*kh*kw]
 * and oc [kc] are those of the undilated layer (inflating the kernel by zeros changes neither).  out NCHW [n, kc, oh, ow],
 * oh = (h + 2*pad - dilation*(kh-1) - 1)/stride + 1; acc_dbg_dev NULL or int32 [n, oh*ow, kc].  dilation < 1, or an inflated
 * kernel larger than the padded input: I8IE_ERR_ARG before any device call.  kh == kw == 1 or dilation == 1 is
 * i8ie_conv2d_u8s8_grouped itself; otherwise it reads the weights back and packs them for this one call. */
int i8ie_conv2d_u8s8_dilated(i8ie_ctx* ctx, const uint8_t* in_dev, int n, int c, int h, int w,
                             const int8_t* qw_dev, int kc, int kh, int kw, int stride, int pad, int groups, int dilation,
                             uint8_t zp_in, const int32_t* oc_dev, float s_in, float s_w, float s_out,
                             uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);

/* i8ie_conv2d_u8s8_dilated with the geometry per axis (see i8ie_conv2d_create_rect; not in the reference): qw
 * [kc, (c/groups)*kh*kw] and oc [kc] are those of the compact kernel.  out NCHW [n, kc, oh, ow], acc_dbg_dev NULL or int32
 * [n, oh*ow, kc].  A bad geometry is I8IE_ERR_ARG before any device call.  Equal pairs are i8ie_conv2d_u8s8_dilated itself;
 * otherwise it reads the weights back and packs them for this one call. */
int i8ie_conv2d_u8s8_rect(i8ie_ctx* ctx, const uint8_t* in_dev, int n, int c, int h, int w, const int8_t* qw_dev, int kc,
                          int groups, const i8ie_conv_geom* geom, uint8_t zp_in, const int32_t* oc_dev, float s_in,
                          float s_w, float s_out, uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);

/* ConvTranspose2d in INT8: Conv2d::forward_prop(Tensor<u8>&&), src/conv2d.cc:100-142, of the equivalent problem (see
 * i8ie_conv_transpose2d_create below); the layer itself: not in the reference.  qw_dev is the equivalent matrix
 * [kc, c*k*k], oc_dev [kc] from i8ie_conv_offsets on that matrix (K = c*k*k, src/conv2d.cc:117-124).  out_dev is NCHW
 * [n, kc, oh, ow], acc_dbg_dev NULL or int32 [n, oh*ow, kc]: the full-K sums including the inserted positions.  Reads the
 * weights back and packs them for this one call (it waits for the stream): a layer handle keeps them packed. */
int i8ie_conv_transpose2d_u8s8(i8ie_ctx* ctx, const uint8_t* in_dev, int n, int c, int h, int w,
                               const int8_t* qw_dev, int kc, int k, int stride, int pad, int output_pad,
                               uint8_t zp_in, const int32_t* oc_dev, float s_in, float s_w, float s_out,
                               uint8_t zp_out, uint8_t* out_dev, int32_t* acc_dbg_dev);

/* ---- layer handles: converted layers with device-resident packed weights -
 * What BaseLayer::convert() leaves behind (src/layer.cc:36-54: q_weight_,
 * q_bias_, scale_, zero_point_), kept on the device in MFMA operand order,
 * plus the offset vector cached per (s_in, zp_in) instead of being recomputed
 * on every call (src/conv2d.cc:117-124).                                     */
int i8ie_linear_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k,
                       float s_w, i8ie_layer** out);
int i8ie_conv2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                       int kh, int kw, int stride, int pad, float s_w, i8ie_layer** out);
/* the same with one weight scale per output feature: s_w_host float [n] / [kc], each finite and >= 0
 * (I8IE_ERR_ARG otherwise).  Every forward entry point below then requantises column j with s_w[j]:
 *   deq = ((float)C[., j] * s_in) * s_w[j];  q = deq / s_out + (float)zp_out  (down_scale per column)
 * and takes the same kernels, layouts and fused pools as the per-tensor layer of the same shape. */
int i8ie_linear_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int n, int k,
                                   const float* s_w_host, i8ie_layer** out);
int i8ie_conv2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                                   int kh, int kw, int stride, int pad, const float* s_w_host, i8ie_layer** out);
/* Grouped / depthwise Conv2d: src/conv2d.cc:100-142 applied per group; groups: not in the reference.
 * `groups` divides c and kc; with Cg = c/groups, Ng = kc/groups, output features [g*Ng, (g+1)*Ng) are the reference
 * convolution of input channels [g*Cg, (g+1)*Cg) with weight rows [g*Ng, (g+1)*Ng), all groups sharing the layer's
 * (s_in, zp_in, s_w, s_out, zp_out).  qw_host is [kc][Cg*kh*kw], K ordered (c, kh, kw) inside the group; the offset
 * vector is src/conv2d.cc:117-124 on that matrix as it stands.  groups < 1 or a non-divisor: I8IE_ERR_ARG (checked
 * before any device call).  groups == 1 returns exactly what i8ie_conv2d_create(_per_channel) returns.
 * Kernels (csrc/i8ie_gconv.hip): gconv_mfma when Cg*kh*kw >= 32 and I8IE_OPT_FORCE_FALLBACK is off, gconv_direct
 * otherwise (depthwise, channel multipliers, tiny groups, and every grouped layer under the option).
 * A grouped handle supports i8ie_layer_forward, i8ie_layer_forward_fused and i8ie_layer_forward_pool, in every
 * layout (NCHW, NHWC with any border, NHWC_S8 by converting around the kernel).  It folds nothing:
 * i8ie_layer_fuses_pool answers 0 (the pool runs as the max-pool kernel behind the convolution),
 * i8ie_layer_rebiased_io answers 0 / 0, i8ie_layer_accepts_f32_input answers 0 (i8ie_layer_forward_f32_input*
 * then return I8IE_ERR_STATE), and i8ie_layer_forward_dequant is for Linear layers only. */
int i8ie_conv2d_create_grouped(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                               int kh, int kw, int stride, int pad, int groups, float s_w, i8ie_layer** out);
int i8ie_conv2d_create_grouped_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc,
                                           int c, int kh, int kw, int stride, int pad, int groups,
                                           const float* s_w_host, i8ie_layer** out);
/* Dilated (atrous) Conv2d: torch.nn.Conv2d's dilation=; not in the reference.  Nothing new is defined arithmetically: the
 * layer IS src/conv2d.cc:100-142 (per group, as above) with the kernel
 *   W~  of side k~ = dilation*(k-1)+1, W~[.., ky*dilation, kx*dilation] = W[.., ky, kx] and zero elsewhere.
 * qw_host [kc][(c/groups)*kh*kw] and qb_host are W's own: zeros add nothing to the max-abs, to the weight sums or to the
 * offset vector, so quantising W and inflating commute.  oh = (h + 2*pad - dilation*(kh-1) - 1)/stride + 1.
 * dilation is one integer >= 1 (I8IE_ERR_ARG otherwise, checked before any device call); a forward whose inflated kernel is
 * larger than the padded input returns I8IE_ERR_ARG.  A layer with kh == kw == 1 or dilation == 1 is exactly what
 * i8ie_conv2d_create_grouped(_per_channel) returns (same route, same kernels, same bytes); it only remembers the number
 * for i8ie_layer_dilation.  Kernels (W~ is never built, an NHWC forward is one launch): dconv_mfma (csrc/i8ie_dconv.hip,
 * phase-subsampled input patches resident in LDS) for groups == 1, stride == 1, kh == kw >= 2, c % 16 == 0, 16-byte
 * aligned buffers, an LDS plan of 8*(k+3)^2*min(c, 64) bytes inside 64 KiB and I8IE_OPT_FORCE_FALLBACK off; every other
 * layer in the grouped kernels of csrc/i8ie_gconv.hip with the dilation in the tap offsets (gconv_mfma when
 * (c/groups)*kh*kw >= 32 and the option is off, gconv_direct otherwise).
 * Such a handle answers the layout queries as follows: i8ie_layer_padding 0 (it needs no border and accepts any: taps are
 * bounds-checked against zp_in), i8ie_layer_fuses_pool 0, i8ie_layer_accepts_f32_input 0, i8ie_layer_rebiased_io 0 / 0
 * (pool and re-biased layouts run as passes around the kernel), i8ie_layer_preferred_layout as a grouped handle (NHWC when
 * kc % 16 == 0 and the option is off). */
int i8ie_conv2d_create_dilated(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                               int kh, int kw, int stride, int pad, int groups, int dilation, float s_w,
                               i8ie_layer** out);
int i8ie_conv2d_create_dilated_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc,
                                           int c, int kh, int kw, int stride, int pad, int groups, int dilation,
                                           const float* s_w_host, i8ie_layer** out);
/* *dilation = the number the layer was created with: 1 for Linear, for ConvTranspose2d and for every other create entry.
 * A handle made by i8ie_conv2d_create_rect with dilation_h != dilation_w has no one number: I8IE_ERR_ARG, and the error text
 * names i8ie_layer_geometry. */
int i8ie_layer_dilation(const i8ie_layer* layer, int* dilation);
/* Rectangular / anisotropic Conv2d: torch.nn.Conv2d with pairs for kernel_size, stride, padding and dilation; not in the
 * reference.  The geometry is eight integers: tap (ky, kx) of output pixel (oy, ox) reads input pixel
 *   (oy*stride_h - pad_h + ky*dilation_h, ox*stride_w - pad_w + kx*dilation_w),
 * a tap outside the image is zp_in, oh = (h + 2*pad_h - dilation_h*(kh-1) - 1)/stride_h + 1 and ow likewise on the w axis.
 * Nothing new is defined arithmetically.  As for the dilated layer, the layer IS src/conv2d.cc:100-142 (per group) of a
 * zero-embedded kernel: on the input padded explicitly with zp_in by (pad_h, pad_w), with the kernel W~ of side
 * S = max(dilation_h*(kh-1), dilation_w*(kw-1)) + 1, W~[.., ky*dilation_h, kx*dilation_w] = W[.., ky, kx] (the dilated kernel
 * embedded top-left in a square of zeros), at stride 1 and padding 0, then rows subsampled by stride_h and columns by
 * stride_w.  (Where S exceeds the kernel's extent on an axis, the explicit padding continues by the difference below / to the
 * right: positions that only the zeros of W~ meet.)  Zeros added to a kernel change neither the max-abs (per tensor or per output feature), nor the weight sums, nor
 * the sequential fp32 offset sum (adding fl(zp_in * 0) = 0 to a float leaves it as it is), nor the bias join: so qw_host is
 * the compact [kc][(c/groups)*kh*kw] matrix that convert() quantises, and the offset vector is src/conv2d.cc:117-124 on it.
 * Rules per axis, those of the square entries on their one number: stride > 0, pad >= 0, dilation >= 1 at create time; the
 * dilated kernel no larger than the padded input at forward time.  Each is I8IE_ERR_ARG before any device call.
 * A geometry with all four pairs equal creates exactly what i8ie_conv2d_create_dilated(_per_channel) creates (same route, same
 * kernels, same bytes).  Any other runs in lconv_mfma (csrc/i8ie_lconv.hip: whole lines of pixels resident in LDS) when it is
 * dense, stride (1, 1), dilation (1, 1), 1 x k or k x 1 with k >= 2, c % 16 == 0, the buffers 16-byte aligned, the line's
 * LDS plan inside the kernel's budget and I8IE_OPT_FORCE_FALLBACK off; and otherwise in the grouped kernels of
 * csrc/i8ie_gconv.hip with the pairs in the tap offsets (gconv_mfma when (c/groups)*kh*kw >= 32, the buffers are aligned
 * and the option is off, gconv_direct otherwise).  Such a handle answers the layout queries as a dilated handle does:
 * i8ie_layer_padding 0, i8ie_layer_fuses_pool 0, i8ie_layer_accepts_f32_input 0, i8ie_layer_rebiased_io 0 / 0,
 * i8ie_layer_preferred_layout as a grouped handle. */
typedef struct i8ie_conv_geom {
  int kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w;
} i8ie_conv_geom;
int i8ie_conv2d_create_rect(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int groups,
                            const i8ie_conv_geom* geom, float s_w, i8ie_layer** out);
int i8ie_conv2d_create_rect_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c,
                                        int groups, const i8ie_conv_geom* geom, const float* s_w_host, i8ie_layer** out);
/* the geometry of a conv handle (Conv2d of every create entry, ConvTranspose2d): square handles answer with equal pairs, the
 * dilation pair being the number the layer was created with.  A Linear handle: I8IE_ERR_ARG. */
int i8ie_layer_geometry(const i8ie_layer* layer, i8ie_conv_geom* geom);
/* ConvTranspose2d (torch.nn.ConvTranspose2d with a square kernel, groups = 1, dilation = 1; not in the reference).
 * Nothing new is defined arithmetically: the layer IS src/conv2d.cc:100-142 (stride 1, padding 0) applied to
 *   x~  the input with stride - 1 positions inserted between neighbouring pixels, padded by k - 1 - pad on top / left and
 *       k - 1 - pad + output_pad on bottom / right, every inserted or padded position holding zp_in;
 *   W~  [kc][c][k][k], W~[oc][ic][ky][kx] = W[ic][oc][k-1-ky][k-1-kx] for torch's weight W [c][kc][k][k].
 * qw_host is W~ as the matrix [kc][c*k*k] (K ordered (ic, ky, kx)), qb_host [kc].  The offset vector is
 * src/conv2d.cc:117-124 (i8ie_conv_offsets) on that matrix as it stands, the accumulators (acc_dbg) are the full-K sums
 * including the positions that hold zp_in, the epilogue is down_scale (src/quantize_utils.cc:27-36).
 * oh = (h - 1)*stride - 2*pad + k + output_pad.  stride >= 1, 0 <= pad <= k - 1, 0 <= output_pad < stride
 * (I8IE_ERR_ARG otherwise, checked before any device call).
 * Kernels (csrc/i8ie_deconv.hip; x~ is never built, an NHWC forward is one launch): deconv_mfma when
 * c * ceil(k/stride)^2 >= 32 and I8IE_OPT_FORCE_FALLBACK is off, deconv_direct otherwise.
 * A transposed handle supports i8ie_layer_forward, i8ie_layer_forward_fused and i8ie_layer_forward_pool, in every
 * layout (NCHW, NHWC with any border, NHWC_S8 by converting around the kernel).  It folds nothing and answers as a
 * grouped handle does: i8ie_layer_fuses_pool 0, i8ie_layer_rebiased_io 0 / 0, i8ie_layer_accepts_f32_input 0,
 * i8ie_layer_padding 0 (it reads no border), and i8ie_layer_forward_dequant is for Linear layers only. */
int i8ie_conv_transpose2d_create(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc, int c, int k,
                                 int stride, int pad, int output_pad, float s_w, i8ie_layer** out);
int i8ie_conv_transpose2d_create_per_channel(i8ie_ctx* ctx, const int8_t* qw_host, const int8_t* qb_host, int kc,
                                             int c, int k, int stride, int pad, int output_pad,
                                             const float* s_w_host, i8ie_layer** out);
/* *groups = the layer's groups: 1 for Linear and for a dense Conv2d */
int i8ie_layer_groups(const i8ie_layer* layer, int* groups);
/* the weight scales: out float [n] (n = out features); a per-tensor layer gives n copies of its scale and
 * *per_channel = 0, a per-channel layer its s_w[j] and *per_channel = 1 */
int i8ie_layer_weight_scales(const i8ie_layer* layer, float* out, int n, int* per_channel);
/* the layer's output (scale_, zero_point_): src/layer.cc:44, include/layer.h:46-47 (default 1, 0) */
int i8ie_layer_set_output_qparams(i8ie_layer* layer, float s_out, uint8_t zp_out);
int i8ie_layer_get_output_qparams(const i8ie_layer* layer, float* s_out, uint8_t* zp_out);
/* Linear: in [m,k] -> out [m,n].  Conv2d: in NCHW [m,c,h,w] (m = batch) -> out NCHW.
 * h, w are ignored for Linear.  acc_dbg_dev as in the stateless calls.       */
int i8ie_layer_forward(i8ie_layer* layer, const uint8_t* in_dev, int m, int h, int w, float s_in,
                       uint8_t zp_in, uint8_t* out_dev, int32_t* acc_dbg_dev);
/* dequantize(linear(x)): src/quantize_utils.cc:54-58 applied to the result of Linear::forward_prop(u8)
 * (src/fully_connected.cc:22-52), in one call.  Layers with at most 16 output features (classifier heads)
 * run a fused kernel -- one wavefront per input row, v_dot4_i32_i8 over K, wavefront reduction, the
 * reference's bias/requant epilogue and the dequantize -- and may pass out_u8 = NULL; any other Linear
 * layer runs its ordinary forward into out_u8 (required) followed by the dequantize kernel.
 * in_layout / h / w as for i8ie_layer_forward_fused. */
int i8ie_layer_forward_dequant(i8ie_layer* layer, const uint8_t* in_dev, int in_layout, int m, int h, int w,
                               float s_in, uint8_t zp_in, int relu, uint8_t* out_u8_dev, float* out_f32_dev);

/* Same computation with the layout conversions and the following relu<u8>
 * (src/functional.cc:15-26: out = max(out, zp_out)) folded in.  in/out may each be NCHW or
 * NHWC; an NHWC tensor may carry a physical border of `border` pixels on each side of H and W
 * ([n][h+2b][w+2b][c]) whose bytes hold the tensor's zero point: a conv whose input border
 * covers its padding gathers with no bounds checks (the pad-with-zero-point rule of
 * src/conv2d.cc:24-28 is materialised by the producer).  When out_border > 0 the call writes
 * only the interior of `out`: the border bytes are the caller's (i8ie_fill_border_u8 with
 * zp_out, once per buffer: they stay valid while the buffer is reused for the same tensor).
 * i8ie_layer_preferred_layout tells which output layout avoids a conversion.
 * Linear layers: layouts do not apply to [m][k] rows, with one exception -- in_layout = NHWC together with
 * h, w > 1 declares the rows to be a flattened NHWC activation [m][h][w][c] (c = in_features / (h*w)) rather
 * than the reference's flattened NCHW (`x.reshape(n, -1)` of a Tensor<u8_t>, include/tensor.h:106-133): the
 * layer then walks K in (h, w, c) order with a weight panel permuted once, sparing the transpose. */
int i8ie_layer_forward_fused(i8ie_layer* layer, const uint8_t* in_dev, int in_layout, int in_border, int m,
                             int h, int w, float s_in, uint8_t zp_in, int relu, uint8_t* out_dev,
                             int out_layout, int out_border, int32_t* acc_dbg_dev);
int i8ie_layer_preferred_layout(const i8ie_layer* layer, int* layout);
/* relu(conv(x)) followed by max_pool2d<u8_t>(., kernel_size, stride) (src/functional.cc:36-64; the reference's models
 * call it right behind conv1 / conv2 / conv5, sample/notebooks/AlexNet_cifar10_resize224.ipynb:60-68) as ONE call:
 * out holds the POOLED tensor, [m, kc, (oh - k)/s + 1, (ow - k)/s + 1] in out_layout.  Where a kernel of this library
 * folds the pool into the convolution's epilogue (i8ie_layer_fuses_pool says so: it then pools the INT32
 * accumulators before requantising them -- down_scale and relu are monotone in C, so the bytes are those of
 * pooling afterwards), no unpooled tensor is ever written; otherwise the call runs the convolution into a
 * temporary and the max-pool kernel behind it.  Identical bytes to i8ie_layer_forward_fused followed by
 * i8ie_maxpool2d_u8(_nhwc) either way.  acc_dbg_dev: the convolution's (unpooled) accumulators [m, oh*ow, kc]. */
int i8ie_layer_fuses_pool(const i8ie_layer* layer, int m, int h, int w, int kernel_size, int stride, int* yes);
int i8ie_layer_forward_pool(i8ie_layer* layer, const uint8_t* in_dev, int in_layout, int in_border, int m, int h, int w,
                            float s_in, uint8_t zp_in, int relu, int kernel_size, int stride, uint8_t* out_dev,
                            int out_layout, int out_border, int32_t* acc_dbg_dev);
/* I8IE_LAYOUT_NHWC_S8 between two conv layers: *reads = 1 when this layer's kernel (at batch m, input h x w, with this
 * pool folded in; kernel_size <= 1: none) consumes re-biased input as it is, *stores = 1 when it can store its result
 * re-biased.  The forward calls accept the layout either way (they convert around a kernel that does not); a caller
 * that owns both ends asks here first, so that no conversion launch is ever needed. */
int i8ie_layer_rebiased_io(const i8ie_layer* layer, int m, int h, int w, int kernel_size, int stride, int* reads,
                           int* stores);
/* First layer fused with the input quantisation (Module.__call__ quantises the FP32 input with
 * 0.025 / 127, i8ie/module.py:20, and hands it straight to the first Conv2d): reads FP32 NCHW,
 * computes q = (u8)(x / q_scale + q_zp) exactly as src/quantize_utils.cc:44-52 and the conv of
 * src/conv2d.cc:100-142 on it, writes the interior of an NHWC u8 tensor (+ optional relu).  Only for layers and
 * geometries where i8ie_layer_accepts_f32_input says yes (<= 3 channels, stride % 4 == 0,
 * out features % 32 == 0): AlexNet's 11x11 stride-4 conv1.  Identical bytes to
 * i8ie_quantize_f32_u8 followed by i8ie_layer_forward_fused.  acc_dbg_dev: NULL, or int32 [m, oh*ow, kc] receiving
 * the pre-requant accumulators (the MKL result, src/conv2d.cc:131-133), as in the other forward calls. */
int i8ie_layer_accepts_f32_input(const i8ie_layer* layer, int h, int w, int* yes);
int i8ie_layer_forward_f32_input(i8ie_layer* layer, const float* in_nchw_dev, int m, int h, int w, float q_scale,
                                 uint8_t q_zp, int relu, uint8_t* out_nhwc_dev, int out_border, int32_t* acc_dbg_dev);
/* the same with max_pool2d<u8_t>(kernel_size, stride) behind the (relu'd) convolution, as in i8ie_layer_forward_pool:
 * quantize -> conv1 -> relu -> max-pool of AlexNet in one contraction launch (csrc/i8ie_stem.hip) */
int i8ie_layer_forward_f32_input_pool(i8ie_layer* layer, const float* in_nchw_dev, int m, int h, int w, float q_scale,
                                      uint8_t q_zp, int relu, int kernel_size, int stride, uint8_t* out_nhwc_dev,
                                      int out_layout /* NHWC or NHWC_S8 */, int out_border, int32_t* acc_dbg_dev);
/* padding of a conv layer (0 for Linear): the input border that makes its gather predicate-free */
int i8ie_layer_padding(const i8ie_layer* layer, int* pad);
int i8ie_layer_destroy(i8ie_layer* layer);

/* ---- NHWC companions of the elementwise ops (internal layout between layers) ------------ */
/* NCHW [n,c,h,w] <-> NHWC [n,h+2b,w+2b,c] of a u8 tensor (to_nhwc != 0: NCHW -> NHWC, the border
 * of the destination is filled with border_value) */
int i8ie_layout_convert_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h,
                           int w, int to_nhwc, int border, uint8_t border_value);
/* border bytes of a bordered NHWC u8 tensor [n,h+2b,w+2b,c] := value (interior untouched) */
int i8ie_fill_border_u8(i8ie_ctx* ctx, uint8_t* buf_dev, int n, int c, int h, int w, int border,
                        uint8_t value);
/* max_pool2d<u8_t> (src/functional.cc:36-64) on NHWC data, channels % 16 == 0; h, w are the
 * logical input dims; only the interior of a bordered output is written */
int i8ie_maxpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, uint8_t* out_dev,
                           int out_border, int n, int c, int h, int w, int kernel_size, int stride);

/* ---- quantized residual Add (no counterpart in the reference: it has no op that joins two tensors) ------------
 * Defined as a composition of the reference's own expressions -- dequantize (src/quantize_utils.cc:38-42) of both
 * operands, down_scale's clamp and truncation (src/quantize_utils.cc:27-36), relu<u8> (src/functional.cc:15-26) --
 * in IEEE fp32, one rounding per operation, no contraction:
 *     fa = (float)((int)a - (int)zp_a) * s_a;   fb = (float)((int)b - (int)zp_b) * s_b
 *     t  = (fa + fb) / s_out + (float)zp_out
 *     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)          truncation toward zero
 *     q  = relu ? max(q, zp_out) : q
 * (s_a, zp_a), (s_b, zp_b): the operands' own quantisation parameters; (s_out, zp_out): the result's.  The bytes equal
 * that sequence for every input pair, whichever way the kernel evaluates it (csrc/i8ie_binary.hip).  Scales must be
 * finite and s_out > 0 (I8IE_ERR_ARG otherwise).  Stateless and capturable in a graph.
 * i8ie_add_u8: n bytes in one physical order (NCHW, [m, k] rows, border-free NHWC); 16-byte aligned buffers; out may
 * alias a or b, and a may be b. */
int i8ie_add_u8(i8ie_ctx* ctx, const uint8_t* a_dev, const uint8_t* b_dev, uint8_t* out_dev, int64_t n, float s_a,
                uint8_t zp_a, float s_b, uint8_t zp_b, float s_out, uint8_t zp_out, int relu);
/* The same arithmetic (no reference counterpart) on NHWC buffers [n, h+2b, w+2b, c], each with its own border b and
 * each plain (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  Only the interior of `out` is
 * written: its border bytes are the caller's and must hold zp_out (zp_out ^ 0x80 when out_s8), as i8ie_fill_border_u8
 * leaves them.  Any c; rows of w * c bytes are the contiguous unit (16 / 4 / 1 bytes per lane by c % 16, c % 4).  With
 * all three borders 0 this is the flat form (and out may alias an operand). */
int i8ie_add_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a_dev, int a_border, int a_s8, const uint8_t* b_dev, int b_border,
                     int b_s8, uint8_t* out_dev, int out_border, int out_s8, int n, int c, int h, int w, float s_a,
                     uint8_t zp_a, float s_b, uint8_t zp_b, float s_out, uint8_t zp_out, int relu);
/* out = a + b in fp32, one rounding (no reference counterpart): the Add before convert() and while calibrating.
 * 16-byte aligned buffers; out may alias a or b. */
int i8ie_add_f32(i8ie_ctx* ctx, const float* a_dev, const float* b_dev, float* out_dev, int64_t n);

/* ---- quantized broadcast Mul (no counterpart in the reference: it has no op that joins two tensors) ----------
 * Defined as the Add is, as a composition of the reference's own expressions -- dequantize (src/quantize_utils.cc:38-42)
 * of both operands, down_scale's clamp and truncation (src/quantize_utils.cc:27-36), relu<u8> (src/functional.cc:15-26)
 * -- in IEEE fp32, one rounding per operation, no contraction:
 *     fa = (float)((int)a - (int)zp_a) * s_a;   fb = (float)((int)b - (int)zp_b) * s_b
 *     t  = (fa * fb) / s_out + (float)zp_out
 *     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)          truncation toward zero
 *     q  = relu ? max(q, zp_out) : q
 * b has a's shape, or is a gate: for a of shape [n, c, h, w] one byte per image and channel ([n, c, 1, 1] or [n, c]),
 * multiplied into every pixel of that image (the excitation of a squeeze-and-excitation block).  Only the second operand
 * broadcasts; the result has a's shape and its own (s_out, zp_out).  The bytes equal that sequence for every input
 * pair, whichever way the kernel evaluates it (csrc/i8ie_binary.hip).  Scales must be finite and
 * s_out > 0 (I8IE_ERR_ARG otherwise, like every other argument error before any device call).  Stateless and
 * capturable in a graph.
 * i8ie_mul_u8: n bytes of each operand in one physical order (NCHW, [m, k] rows, border-free NHWC); 16-byte aligned
 * buffers; out may alias a or b, and a may be b. */
int i8ie_mul_u8(i8ie_ctx* ctx, const uint8_t* a_dev, const uint8_t* b_dev, uint8_t* out_dev, int64_t n, float s_a,
                uint8_t zp_a, float s_b, uint8_t zp_b, float s_out, uint8_t zp_out, int relu);
/* The same arithmetic on NHWC buffers: a and out [n, h+2b, w+2b, c], each with its own border b and each plain
 * (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  b_gate = 0: b is a third such buffer.
 * b_gate != 0: b is the gate, c bytes per image, read as its producer left it: [n, 1+2b, 1+2b, c] with its own border
 * and re-bias flag (plain [n, c] rows are b_border = 0, b_s8 = 0).  Only the interior of `out` is written: its border
 * bytes are the caller's and must hold zp_out (zp_out ^ 0x80 when out_s8), as i8ie_fill_border_u8 leaves them.  Any c
 * (16 / 4 / 1 bytes per lane by c % 16, c % 4 and the pointers' alignment).  With equal shapes and all three borders 0
 * this is the flat form (and out may alias an operand); otherwise out must not overlap a or b. */
int i8ie_mul_u8_nhwc(i8ie_ctx* ctx, const uint8_t* a_dev, int a_border, int a_s8, const uint8_t* b_dev, int b_border,
                     int b_s8, int b_gate, uint8_t* out_dev, int out_border, int out_s8, int n, int c, int h, int w,
                     float s_a, uint8_t zp_a, float s_b, uint8_t zp_b, float s_out, uint8_t zp_out, int relu);
/* out = a * b in fp32, one rounding (no reference counterpart): the Mul before convert() and while calibrating.  n
 * elements of a and out.  gate_run = 0: b has n elements too; 16-byte aligned buffers; out may alias a or b.
 * gate_run > 0 (it must divide n): b has n / gate_run elements and out[i] = a[i] * b[i / gate_run] -- NCHW tensors with
 * gate_run = h * w; b 4-byte aligned; out may alias a. */
int i8ie_mul_f32(i8ie_ctx* ctx, const float* a_dev, const float* b_dev, float* out_dev, int64_t n, int64_t gate_run);

/* ---- quantized average pooling (no counterpart in the reference) -----------------------------------------------
 * Everything but the reduction follows max_pool2d<u8_t> (src/functional.cc:36-64): NCHW logical shape, window
 * kernel_h x kernel_w, one stride, floor output size (h - kernel_h) / stride + 1 by (w - kernel_w) / stride + 1, no
 * padding; the result carries the input's (scale, zero_point).  With n = kernel_h * kernel_w and S the exact integer
 * sum of the window's bytes:
 *     q = (S + n / 2) / n        integer floor division: round to nearest, ties up
 * (the value never leaves the integers, so no fp32 step of the reference applies; truncation would bias every pooled
 * tensor by -1/2 LSB).  The global pool is kernel_h = h, kernel_w = w, stride = 1.  n <= 65536.  Null pointers,
 * non-positive sizes, a window larger than the input, n > 65536 and a negative border are I8IE_ERR_ARG, raised before
 * any device call.  Stateless and capturable in a graph (csrc/i8ie_avgpool.hip).
 * i8ie_avgpool2d_u8: NCHW in and out, any shape. */
int i8ie_avgpool2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int kernel_h,
                      int kernel_w, int stride);
/* The same on NHWC buffers [n, h+2b, w+2b, c] / [n, oh+2b', ow+2b', c], each with its own border and each plain
 * (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  relu != 0: q = max(q, zero_point)
 * (relu<u8>, src/functional.cc:15-26, on the result).  Only the interior of `out` is written: its border bytes are
 * the caller's (i8ie_fill_border_u8).  Any c: 16 / 4 / 1 channels per lane by c % 16, c % 4.  h, w: logical input dims. */
int i8ie_avgpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                           int out_border, int out_s8, int n, int c, int h, int w, int kernel_h, int kernel_w,
                           int stride, int relu, uint8_t zero_point);
/* FP32 (before convert(), and while calibrating), NCHW: sum / n, the sum taken in fp32 in window order (rows outer,
 * columns inner), then one division.  NaN and inf propagate as IEEE gives them. */
int i8ie_avgpool2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int kernel_h,
                       int kernel_w, int stride);

/* ---- quantized upsampling by integer factors (no counterpart in the reference: it has no resize op) --------------
 * NCHW logical shape [n, c, h, w]; integer factors fh, fw, each in 1..8; the result is [n, c, h*fh, w*fw] and carries
 * the input's (scale, zero_point), as the pools' results do.
 * I8IE_UPSAMPLE_NEAREST:   out[y, x] = in[y / fh, x / fw] (integer division): a byte copy.
 * I8IE_UPSAMPLE_BILINEAR:  torch's align_corners=False.  Along one axis of length L with factor f, write the output
 * index as o = f*i + r and let t = 2*r + 1 - f:
 *     t >= 0:  i0 = i,      w1 = t
 *     t <  0:  i0 = i - 1,  w1 = 2*f + t
 *     i0 <  0: i0 = 0,      w1 = 0
 *     i1 = min(i0 + 1, L - 1),  w0 = 2*f - w1
 * With (y0, y1, wy0, wy1) and (x0, x1, wx0, wx1) from that rule and D = 4*fh*fw:
 *     S = wx0 * (wy0 * q[y0,x0] + wy1 * q[y1,x0]) + wx1 * (wy0 * q[y0,x1] + wy1 * q[y1,x1])
 *     out = (S + D / 2) / D       integer floor division: round to nearest, ties up (the rule of i8ie_avgpool2d_u8)
 * The value never leaves the integers, so no fp32 step of the reference applies: S / D is the interpolated value
 * exactly, and the only rounding is the one above.  S + D / 2 <= 65408 < 2^16 at fh = fw = 8: the blends fit packed
 * 16-bit lanes, which is the reason for the bound of 8 (compose two calls beyond it).
 *     out = relu ? max(out, zero_point) : out                relu<u8>, src/functional.cc:15-26, on the result
 * FP32 (before convert(), and while calibrating): nearest copies bits; bilinear takes l = (float)w1 / (float)(2*f) per
 * axis, the two row blends a * (1 - lx) + b * lx first, then the column blend of their results with ly; every step in
 * fp32, one rounding per operation, no contraction.
 * Null pointers, non-positive sizes, factors outside 1..8, an unknown mode and negative borders are I8IE_ERR_ARG,
 * raised before any device call.  Stateless and capturable in a graph (csrc/i8ie_upsample.hip).
 * i8ie_upsample2d_u8: NCHW in and out, any shape. */
#define I8IE_UPSAMPLE_NEAREST 0
#define I8IE_UPSAMPLE_BILINEAR 1
int i8ie_upsample2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int fh, int fw,
                       int mode);
/* The same on NHWC buffers [n, h+2b, w+2b, c] -> [n, h*fh+2b', w*fw+2b', c], each with its own border and each plain
 * (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  Edge pixels are replicated by clamping
 * indices: the input's border bytes are never read.  Only the interior of `out` is written: its border bytes are the
 * caller's (i8ie_fill_border_u8).  Any c: 16 / 4 / 1 channels per lane by c % 16, c % 4 and the pointers' alignment.
 * `out` must not overlap `in`.  h, w: logical input dims. */
int i8ie_upsample2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                            int out_border, int out_s8, int n, int c, int h, int w, int fh, int fw, int mode, int relu,
                            uint8_t zero_point);
/* FP32, NCHW (the definition above).  NaN and inf propagate as IEEE gives them. */
int i8ie_upsample2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int fh, int fw,
                        int mode);

/* ---- resize to any size, and adaptive average pooling (no counterpart in the reference) --------------------------
 * NCHW logical shape [n, c, h, w] -> [n, c, oh, ow], any oh, ow >= 1, up or down; the result carries the input's
 * (scale, zero_point), as i8ie_upsample2d_u8's and the pools' results do; nothing is requantised.
 * Resize.  Per axis with input length L and output length O, output index o gets (i0, i1, w0, w1) over `den`:
 *     I8IE_RESIZE_BILINEAR          torch's align_corners=False, src = (o + 0.5) L / O - 0.5, negative clamped to 0:
 *                                   den = 2*O,            num = max((2*o + 1)*L - O, 0)
 *     I8IE_RESIZE_BILINEAR_ALIGNED  torch's align_corners=True, src = o (L - 1) / (O - 1):
 *                                   den = max(O - 1, 1),  num = o*(L - 1), and 0 when O == 1
 *     both:  i0 = num / den (floor),  w1 = num % den,  w0 = den - w1,  i1 = min(i0 + 1, L - 1)
 *     I8IE_RESIZE_NEAREST           i0 = i1 = (o*L) / O (floor), w0 = den = 1, w1 = 0: a byte copy.  (torch's float
 *                                   `scale` lands one index lower at a few places where o*L is a multiple of O; the
 *                                   integer rule is the definition.)
 * Bilinear on uint8, with (y0, y1, wy0, wy1) and (x0, x1, wx0, wx1) from that rule and D = den_y * den_x:
 *     S = wx0 * (wy0 * q[y0,x0] + wy1 * q[y1,x0]) + wx1 * (wy0 * q[y0,x1] + wy1 * q[y1,x1])
 *     out = (S + D / 2) / D       integer floor division: round to nearest, ties up, the rule of i8ie_upsample2d_u8 and
 *                                 i8ie_avgpool2d_u8 (for odd D no tie exists and the floored half gives the same byte)
 *     out = relu ? max(out, zero_point) : out                relu<u8>, src/functional.cc:15-26, on the result
 * S / D is the interpolated value exactly; nothing leaves the integers.  D <= 2^22 (for I8IE_RESIZE_BILINEAR:
 * oh * ow <= 2^20), so that S + D / 2 < 2^31; beyond it the call is I8IE_ERR_ARG.  At O = f*L, f in 1..8, the
 * I8IE_RESIZE_BILINEAR rule is i8ie_upsample2d_u8's: num / den = (2*f*i + t) / (2*f), and S, D and D / 2 all scale by
 * L_h * L_w, so the bytes (and the FP32 bits) are the same.
 * Bilinear on FP32: l = (float)w1 / (float)den per axis, the two row blends a * (1 - lx) + b * lx first, then the
 * column blend of their results with ly; one fp32 rounding per operation, no contraction (the sequence of
 * i8ie_upsample2d_f32).  Nearest copies bits.  NaN and inf propagate as IEEE gives them.
 * Adaptive average pool.  Output i of an axis covers [floor(i*L / O), ceil((i + 1)*L / O)) (torch's windows: they
 * overlap when O does not divide L and are never empty).  uint8: q = (S + n / 2) / n with S the exact window sum and n
 * the window's own element count (i8ie_avgpool2d_u8's rule), then the relu floor as above.  FP32: the fp32 sum of the
 * window, rows outer, columns inner, divided by (float)n.  A window holds at most 65536 elements.  Where O divides L on
 * both axes the result is i8ie_avgpool2d_u8's with kernel_h = L_h / O_h, kernel_w = L_w / O_w and stride = kernel (a
 * square window where that entry takes one stride); (1, 1) is the global pool.
 * Null pointers, non-positive sizes, an unknown mode, negative borders, D > 2^22 and a window of more than 65536
 * elements are I8IE_ERR_ARG, raised before any device call.  Stateless, no allocation, capturable in a graph; `out`
 * must not overlap `in` (csrc/i8ie_resize.hip).
 * i8ie_resize_axis: host only, the rule of one axis: (i0, i1, w0, w1, den) of output index out_index; out_len <= 2^30. */
#define I8IE_RESIZE_NEAREST 0
#define I8IE_RESIZE_BILINEAR 1
#define I8IE_RESIZE_BILINEAR_ALIGNED 2
int i8ie_resize_axis(int in_len, int out_len, int mode, int out_index, int* i0, int* i1, int* w0, int* w1, int* den);
/* NCHW in and out, any shape. */
int i8ie_resize2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int oh, int ow,
                     int mode);
/* The same on NHWC buffers [n, h+2b, w+2b, c] -> [n, oh+2b', ow+2b', c], each with its own border and each plain
 * (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  Taps are read at the clamped indices of the
 * rule: the input's border bytes are never read.  Only the interior of `out` is written: its border bytes are the
 * caller's (i8ie_fill_border_u8).  Any c: 16 / 4 / 1 channels per lane by c % 16, c % 4; a buffer off that alignment
 * takes the one-lane-per-byte kernel (same bytes).  h, w: logical input dims. */
int i8ie_resize2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                          int out_border, int out_s8, int n, int c, int h, int w, int oh, int ow, int mode, int relu,
                          uint8_t zero_point);
/* FP32, NCHW (the definition above). */
int i8ie_resize2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int oh, int ow,
                      int mode);
/* The adaptive average pool: NCHW; NHWC as i8ie_resize2d_u8_nhwc; FP32 NCHW. */
int i8ie_adaptive_avgpool2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int oh,
                               int ow);
int i8ie_adaptive_avgpool2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                                    int out_border, int out_s8, int n, int c, int h, int w, int oh, int ow, int relu,
                                    uint8_t zero_point);
int i8ie_adaptive_avgpool2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int oh,
                                int ow);

/* ---- channel narrow, channel shuffle, pixel shuffle and unshuffle (no counterpart in the reference) ---------------
 * Byte rearrangements of an NCHW logical shape [n, c, h, w]; nothing is requantised: the result carries the input's
 * (scale, zero_point).  `kind` with its parameters p0, p1 (p1 is read by narrow alone):
 *   I8IE_REARRANGE_NARROW           p0 = start, p1 = length, 0 <= start, 1 <= length, start + length <= c:
 *       out[n, k, y, x] = in[n, start + k, y, x]                                    -> [n, length, h, w]
 *   I8IE_REARRANGE_CHANNEL_SHUFFLE  p0 = groups >= 1, c % groups == 0 (torch.nn.ChannelShuffle):
 *       out[n, j*groups + i, y, x] = in[n, i*(c/groups) + j, y, x]                  -> [n, c, h, w]
 *   I8IE_REARRANGE_PIXEL_SHUFFLE    p0 = r in 1..8, c % (r*r) == 0 (torch's pixel_shuffle):
 *       out[n, co, y*r + i, x*r + j] = in[n, co*r*r + i*r + j, y, x]                -> [n, c/(r*r), h*r, w*r]
 *   I8IE_REARRANGE_PIXEL_UNSHUFFLE  p0 = r in 1..8, h % r == 0, w % r == 0 (torch's pixel_unshuffle, the inverse):
 *       out[n, ci*r*r + i*r + j, y, x] = in[n, ci, y*r + i, x*r + j]                -> [n, c*r*r, h/r, w/r]
 *   out = relu ? max(out, zero_point) : out        relu<u8>, src/functional.cc:15-26, on the NHWC entry
 * The three permuting kinds take at most 65535 channels on either side.  Null pointers, non-positive sizes, negative
 * borders, an unknown kind and parameters outside these rules are I8IE_ERR_ARG, raised before any device call; the
 * message begins with the op's name (narrow, channel_shuffle, pixel_shuffle, pixel_unshuffle).  Stateless and capturable
 * in a graph; `out` must not overlap `in` (csrc/i8ie_rearrange.hip).
 * i8ie_rearrange_output_shape (host only): the result's four dims into out_dims, or I8IE_ERR_ARG. */
#define I8IE_REARRANGE_NARROW 0
#define I8IE_REARRANGE_CHANNEL_SHUFFLE 1
#define I8IE_REARRANGE_PIXEL_SHUFFLE 2
#define I8IE_REARRANGE_PIXEL_UNSHUFFLE 3
int i8ie_rearrange_output_shape(int kind, int p0, int p1, int n, int c, int h, int w, int* out_dims);
/* On NHWC buffers [n, h+2b, w+2b, c] -> [n, oh+2b', ow+2b', oc], each with its own border and each plain (x_s8 = 0) or
 * re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  The input's border bytes are never read.  Only the interior
 * of `out` is written: its border bytes are the caller's (i8ie_fill_border_u8).  Any c, any alignment: narrow moves
 * 16 / 8 / 4 / 2 / 1 bytes per lane by start, length, c and the pointers' alignment; the permuting kinds take the
 * 16-byte transposing kernel where c % 16 == 0, oc % 16 == 0 and both pointers are 16-byte aligned, one lane per byte
 * otherwise (and under I8IE_OPT_FORCE_FALLBACK); the bytes are the same.  h, w: logical input dims. */
int i8ie_rearrange_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                           int out_border, int out_s8, int n, int c, int h, int w, int kind, int p0, int p1, int relu,
                           uint8_t zero_point);
/* Plain NCHW in and out, any shape (no relu: a caller applies i8ie_relu_u8).  The rank-2 narrow of [m, f] rows is
 * n = m, c = f, h = w = 1. */
int i8ie_rearrange_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int kind,
                      int p0, int p1);
/* FP32, NCHW: the same index maps, bits copied (before convert(), and while calibrating). */
int i8ie_rearrange_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int kind, int p0,
                       int p1);

/* ---- Spatial padding: constant, reflect, replicate, circular, and cropping (no counterpart in the reference) ------
 * torch.nn.functional.pad on the last two axes of an NCHW logical shape [n, c, h, w] -> [n, c, h + top + bottom,
 * w + left + right]; nothing is requantised: the result carries the input's (scale, zero_point).  Per axis of input
 * length L with amounts (before, after): the output length is O = L + before + after >= 1, output index o reads input
 * index i = o - before, and for i outside [0, L)
 *     I8IE_PAD_CONSTANT   the fill value.  Amounts may be negative: they cut pixels off (a crop to the window
 *                         [top', top' + O_h) x [left', left' + O_w) is the amounts (-left', left' + O_w - w, -top',
 *                         top' + O_h - h)); mixed signs are allowed
 *     I8IE_PAD_REFLECT    i < 0: -i;  i >= L: 2*(L - 1) - i     (the edge pixel is not repeated)   0 <= amount <= L - 1
 *     I8IE_PAD_REPLICATE  i < 0: 0;   i >= L: L - 1                                                0 <= amount
 *     I8IE_PAD_CIRCULAR   i < 0: i + L;  i >= L: i - L                                             0 <= amount <= L
 *     out = relu ? max(out, zero_point) : out       relu<u8>, src/functional.cc:15-26, on the NHWC entry; fill bytes too
 * These are torch's rules and limits.  |amount| <= 65535.  `fill` is the plain byte (not re-biased; the kernel
 * re-biases it with the rest when out_s8) or the float; the three other modes do not read it.  Null pointers,
 * non-positive sizes, negative borders, an unknown mode, an amount beyond its mode's limit, a negative amount outside
 * the constant mode, O < 1 and an `out` that overlaps `in` are I8IE_ERR_ARG, raised before any device call;
 * i8ie_last_error names what is wrong (the shape rules begin with "pad:").  Stateless, nothing is allocated or copied,
 * the geometry travels in the kernel arguments: capturable in a graph (csrc/i8ie_pad.hip).
 * i8ie_pad_output_shape (host only): the result's four dims into out_dims, or I8IE_ERR_ARG. */
#define I8IE_PAD_CONSTANT 0
#define I8IE_PAD_REFLECT 1
#define I8IE_PAD_REPLICATE 2
#define I8IE_PAD_CIRCULAR 3
int i8ie_pad_output_shape(int mode, int left, int right, int top, int bottom, int n, int c, int h, int w, int* out_dims);
/* On NHWC buffers [n, h+2b, w+2b, c] -> [n, oh+2b', ow+2b', c], each with its own border and each plain (x_s8 = 0) or
 * re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  The input's border bytes are never read: they hold the
 * zero point, which is not what reflect, replicate or circular put there.  Only the interior of `out` is written: its
 * border bytes are the caller's (i8ie_fill_border_u8).  Any c: 16 / 4 / 1 bytes per lane by c % 16, c % 4 and the
 * pointers' alignment; one lane per byte under I8IE_OPT_FORCE_FALLBACK; the bytes are the same.  h, w: logical input
 * dims. */
int i8ie_pad2d_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                       int out_s8, int n, int c, int h, int w, int mode, int left, int right, int top, int bottom,
                       uint8_t fill, int relu, uint8_t zero_point);
/* Plain NCHW in and out, any shape (no relu: a caller applies i8ie_relu_u8). */
int i8ie_pad2d_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w, int mode, int left,
                  int right, int top, int bottom, uint8_t fill);
/* FP32, NCHW: the same index rule, bits copied (NaN payloads and -0.0 included, in the data and in `fill`). */
int i8ie_pad2d_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int mode, int left,
                   int right, int top, int bottom, float fill);

/* ---- quantized channel concatenation (no counterpart in the reference: it has no op that joins two tensors) ----
 * cat(x_0 .. x_{k-1}) along axis 1, 1 <= k <= I8IE_CONCAT_MAX_INPUTS; the same buffer may appear more than once.  The
 * result carries its own (s_out, zp_out).  A byte a of input i, with that tensor's (s_i, zp_i), becomes
 *     if (bits(s_i) == bits(s_out) && zp_i == zp_out)  q = a                       the copy rule
 *     else  f = (float)((int)a - (int)zp_i) * s_i                                  dequantize, src/quantize_utils.cc:38-42
 *           t = f / s_out + (float)zp_out                                          IEEE fp32, one rounding per operation
 *           q = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)                               down_scale's clamp + truncation, :27-36
 *     q = relu ? max(q, zp_out) : q                                                relu<u8>, src/functional.cc:15-26
 * The copy rule is part of the definition (the literal sequence is not the identity at equal parameters): a tensor that
 * is already in the result's quantisation is not moved.  The bytes equal that sequence for every input byte, whichever
 * way the kernel evaluates it (csrc/i8ie_concat.hip).  Scales must be finite and s_out > 0; null
 * pointers, k outside [1, 8], non-positive sizes and negative borders are I8IE_ERR_ARG too, all raised before any device
 * call.  `in_dev`, `len`, `s_in`, ... are host arrays of k entries.  One launch for all k inputs; stateless and capturable
 * in a graph.  `out` must not overlap an input.
 * i8ie_concat_u8, the run form: `outer` x (for each input a contiguous run of len[i] bytes), written at
 * outer_index * sum(len) + (len[0] + .. + len[i-1]).  NCHW: outer = n, len[i] = c_i * h * w; [m, f_i] rows: outer = m;
 * border-free plain NHWC: outer = n * h * w, len[i] = c_i.  Any alignment (16 / 4 / 1 bytes per lane, chosen per input). */
#define I8IE_CONCAT_MAX_INPUTS 8
int i8ie_concat_u8(i8ie_ctx* ctx, int k, const uint8_t* const* in_dev, const int64_t* len, const float* s_in,
                   const uint8_t* zp_in, uint8_t* out_dev, int64_t outer, float s_out, uint8_t zp_out, int relu);
/* The same arithmetic on NHWC buffers: out [n, h+2b, w+2b, sum(c_in)], input i [n, h+2b_i, w+2b_i, c_in[i]], every
 * buffer with its own border and plain (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  Only the
 * interior of `out` is written: its border bytes are the caller's and must hold zp_out (zp_out ^ 0x80 when out_s8), as
 * i8ie_fill_border_u8 leaves them.  With every border 0 and nothing re-biased this is the run form. */
int i8ie_concat_u8_nhwc(i8ie_ctx* ctx, int k, const uint8_t* const* in_dev, const int* c_in, const int* border_in,
                        const int* s8_in, const float* s_in, const uint8_t* zp_in, uint8_t* out_dev, int out_border,
                        int out_s8, int n, int h, int w, float s_out, uint8_t zp_out, int relu);
/* The run form on fp32 elements (len[i] counts floats), a copy bit for bit: the Concat before convert() and while
 * calibrating.  4-byte aligned buffers. */
int i8ie_concat_f32(i8ie_ctx* ctx, int k, const float* const* in_dev, const int64_t* len, float* out_dev, int64_t outer);

/* ---- table-driven quantized activations (no counterpart in the reference: its one non-linearity is relu) ----
 * In the quantized domain an activation is a function from one byte to one byte: a 256-entry table applied to a u8
 * tensor.  f(x) on a float x, IEEE fp32, one rounding per operation, no contraction:
 *     I8IE_ACT_RELU6        v = x > 0 ? x : 0;  y = v < 6 ? v : 6                   min(max(x, 0), 6)
 *     I8IE_ACT_LEAKY_RELU   y = x >= 0 ? x : x * param                              param: the slope (finite)
 *     I8IE_ACT_HARDSIGMOID  v = x + 3;  v = v > 0 ? v : 0;  h = v < 6 ? v : 6;  y = h / 6
 *     I8IE_ACT_HARDSWISH    h as above;  y = (x * h) / 6
 *     I8IE_ACT_SIGMOID      y = (float)(1.0 / (1.0 + exp(-(double)x)))              double precision, one rounding to float
 *     I8IE_ACT_TANH         y = (float)tanh((double)x)
 * `param` is read by I8IE_ACT_LEAKY_RELU only.  The table of an activation from (s_in, zp_in) to (s_out, zp_out), for
 * every byte a:
 *     x = (float)((int)a - (int)zp_in) * s_in                                       dequantize, src/quantize_utils.cc:38-42
 *     t = f(x) / s_out + (float)zp_out
 *     table[a] = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)                               down_scale's clamp + truncation, :27-36
 * The scales must be finite, s_out > 0 and 255 * s_in finite in fp32 (no NaN can then arise in any kind); an unknown
 * kind, a non-finite slope and a null table are I8IE_ERR_ARG too.
 * i8ie_activation_table: host only (no ctx, like i8ie_quantize_weight); for sigmoid and tanh it calls the host's
 * double-precision libm.  A following relu folds into a table as max(table[a], zp_out). */
#define I8IE_ACT_RELU6 0
#define I8IE_ACT_LEAKY_RELU 1
#define I8IE_ACT_HARDSIGMOID 2
#define I8IE_ACT_HARDSWISH 3
#define I8IE_ACT_SIGMOID 4
#define I8IE_ACT_TANH 5
int i8ie_activation_table(int kind, float param, float s_in, uint8_t zp_in, float s_out, uint8_t zp_out,
                          uint8_t table_host[256]);
/* out[i] = table[in[i]] over n bytes in one physical order, any n and any alignment (16 / 4 / 1 bytes per lane by the
 * alignment of both pointers); `out` may be `in` itself (no other overlap).  The 256 table bytes are read from the
 * host at the call and travel by value in the kernel arguments: one launch, no device allocation, no copy, no
 * synchronisation; stateless and capturable in a graph.  Every argument error is raised before any device call. */
int i8ie_lut_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t n, const uint8_t* table_host);
/* The same on NHWC buffers [n, h+2b, w+2b, c], each with its own border and plain (x_s8 = 0) or re-biased (x_s8 != 0:
 * I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80); `table_host` maps plain bytes to plain bytes, the re-bias of either side is
 * folded into the table on the host (t'[a ^ 0x80*in_s8] = table[a] ^ 0x80*out_s8).  Only the interior of `out` is
 * written: its border bytes are the caller's.  Any c (16 / 4 / 1 bytes per lane by c % 16, c % 4 and the pointers'
 * alignment).  With both borders 0 this is the flat form. */
int i8ie_lut_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                     int out_s8, int n, int c, int h, int w, const uint8_t* table_host);
/* out[i] = f(in[i]) on n floats (4-byte aligned; in place allowed): the activation before convert() and while
 * calibrating.  relu6, leaky_relu, hardsigmoid and hardswish are the fp32 sequences above bit for bit; sigmoid and
 * tanh go through the device's double-precision exp / tanh (DESIGN.md section 8f states the error bound). */
int i8ie_activation_f32(i8ie_ctx* ctx, int kind, float param, const float* in_dev, float* out_dev, int64_t n);

/* ---- quantized batched MatMul of two activation tensors (no counterpart in the reference: every op of it multiplies
 * by static weights) ------------------------------------------------------------------------------------------------
 * Logical form A [b, m, k] . B [b, k, n] -> [b, m, n]; both operands are u8 tensors with their own (scale, zero_point),
 * the same b on both sides (no broadcast).  The exact int32 sum is
 *     C[b,i,j] = sum_k ((int)a[b,i,k] - zp_a) * ((int)b[b,k,j] - zp_b)
 * k <= 32768 keeps |C| <= 255 * 255 * 32768 < 2^31; a larger k is I8IE_ERR_ARG.  Then
 *     out = down_scale(C, s_a, s_b, s_out, zp_out)        src/quantize_utils.cc:27-36 (csrc/i8ie_requant.h):
 *           deq = ((float)C * s_a) * s_b;  t = deq / s_out + (float)zp_out;  q = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t)
 *     out = relu ? max(q, zp_out) : q                     relu<u8>, src/functional.cc:15-26
 * There is no bias and no alpha: a 1/sqrt(d) factor folds into the weights of the projection that makes the operand.
 * Scales must be finite and s_out > 0.
 * Each operand and the result is described physically (i8ie_bmm_mat): element (batch, row, col) of the logical matrix
 * lies at ptr[batch * batch_stride + row * row_stride + col * col_stride], and one of row_stride, col_stride must be 1.
 * A is [m, k] (rows i, columns k), B is [k, n] (rows k, columns j), the result [m, n]: an operand given transposed
 * ([b, k, m] / [b, n, k]) is the same matrix with its two strides exchanged, so a K-contiguous and a K-strided operand
 * are accepted on either side.  s8 != 0: the bytes are stored re-biased (^0x80, I8IE_LAYOUT_NHWC_S8).
 * The result may instead be the interior of a bordered NHWC feature map [b, h+2B, w+2B, c]: out_pix_axis = 1 (the m
 * rows are the h*w pixels, m == out_h * out_w) or 2 (the n columns are), out_border = B > 0.  `out.ptr` is then the
 * buffer's first byte, out.batch_stride = (h+2B)*(w+2B)*c, the pixel axis' stride is c and the other stride 1; pixel p
 * lies at physical pixel (p / w + B) * (w + 2B) + p % w + B.  Only the interior is written: border bytes are the
 * caller's, as for i8ie_add_u8_nhwc.  out_pix_axis = 0 is the plain strided form.  `out` must not overlap an operand (a
 * and b may be the same buffer).  As in the other stateless entries, extents are the caller's responsibility: neither the
 * overlap nor whether the strides describe disjoint elements inside the caller's allocations is checked.
 * The stride contract (tests/test_gpu_attention.py pins it): any non-negative strides with row_stride == 1 or col_stride == 1
 * are accepted.  A matrix may lie inside a larger allocation -- a row pitch above the row's length, a batch pitch above the
 * matrix' size -- and the bytes between rows and between batch items are never read (operands) or written (result).
 * batch_stride == 0 on an operand is a broadcast: every batch item reads the same matrix, on a, on b or on both.
 * batch_stride == 0 on the result with b > 1 is I8IE_ERR_ARG (the batch items would share their bytes).  No stride needs
 * any alignment for correctness: bmm_mfma stages a K-contiguous operand (unit stride along k) in 16-byte loads where its
 * pointer and every stride other than the unit one (batch_stride included) are multiples of 16, in 4-byte loads where
 * they are multiples of 4, else in bytes; a K-strided operand (unit stride along its rows) in 4-byte loads where they are
 * multiples of 4, else in bytes, never wider; four result columns are one dword store where that address is 4-byte
 * aligned, else bytes.
 * acc_dbg_dev is NULL or int32 [b, m, n] and receives C.  Stateless and capturable in a graph: one launch, no device
 * allocation.  Every argument error (null pointers, non-positive sizes, k > 32768, both strides != 1, negative strides,
 * a result batch_stride of 0 with b > 1, bad scales, a pixel axis that does not match) is I8IE_ERR_ARG before any device call.
 * Two kernels with identical bytes (csrc/i8ie_matmul.hip): bmm_mfma, and bmm_direct for k < 16,
 * for a, b or out not 16-byte aligned, for strides beyond 2^31 and for everything under I8IE_OPT_FORCE_FALLBACK. */
typedef struct i8ie_bmm_mat {
  void* ptr;              /* device pointer (read-only for an operand) */
  int64_t batch_stride;   /* elements between two batch items */
  int64_t row_stride;     /* ... between two rows of the logical matrix */
  int64_t col_stride;     /* ... between two columns; one of row_stride, col_stride is 1 */
  int s8;                 /* != 0: bytes stored re-biased (^0x80) */
} i8ie_bmm_mat;
typedef struct i8ie_bmm_args {
  int b, m, n, k;
  i8ie_bmm_mat a;         /* [m, k] */
  i8ie_bmm_mat bm;        /* [k, n] */
  i8ie_bmm_mat out;       /* [m, n] */
  int out_pix_axis;       /* 0: plain; 1: rows are the pixels of a bordered NHWC map; 2: columns are */
  int out_h, out_w, out_border;
  float s_a, s_b, s_out;
  uint8_t zp_a, zp_b, zp_out;
  int relu;
  int32_t* acc_dbg_dev;   /* NULL or [b, m, n] */
} i8ie_bmm_args;
int i8ie_bmm_u8(i8ie_ctx* ctx, const i8ie_bmm_args* args);
/* FP32 (before convert(), and while calibrating): the same descriptor and stride contract with float elements (s8, the pixel axis, the
 * scales, relu and acc_dbg_dev are ignored and must be 0 / NULL); out[i,j] = sum over k in ascending order of
 * a[i,k] * b[k,j], fp32 products added in fp32 to a sum that starts at 0, one rounding per operation, no contraction. */
int i8ie_bmm_f32(i8ie_ctx* ctx, const i8ie_bmm_args* args);

/* ---- quantized Softmax over the last axis (no counterpart in the reference) ------------------------------------------
 * Input: `rows` rows of L u8 values with (s_in, zero point), 1 <= L <= 65535, in reference order.  The result always
 * carries scale = 1/256, zero_point = 0.  Everything is integer.  Per row:
 *     mx   = max_j x_j
 *     d_j  = mx - x_j                                   0..255; the zero point cancels
 *     E[d] = (uint32) floor(65536 * exp(-(double)s_in * d) + 0.5),  d = 0..255      the host-built table
 *     S    = sum_j E[d_j]                               65536 <= S < 2^32
 *     q_j  = min(255, (E[d_j] * 256 + S / 2) / S)       unsigned 32-bit, floor division
 * E[d] <= 65536, so E * 256 + S / 2 < 2^24 + 2^31 never wraps.  With p the real softmax, the unclamped quotient is within
 * 0.5 + 256 (L + 1) / 131072 of 256 p; the byte clamps at 255, so the bound that holds for q is
 *     |q - min(256 p, 255)| <= 0.5 + 256 (L + 1) / 131072
 * (L = 1 gives q = 255 where 256 p = 256).
 * i8ie_softmax_table: host only (no ctx, like i8ie_activation_table); exp is the host's double-precision libm.  s_in
 * must be finite and >= 0; a null table is I8IE_ERR_ARG too.
 * i8ie_softmax_u8: out may alias in (no other overlap); any alignment.  The table is built at the call and travels by
 * value in the kernel arguments: one launch, no device allocation, no copy; stateless and capturable in a graph.  One
 * wave per row up to L = 1024 (the row stays in registers between the passes), one block per row beyond
 * (csrc/i8ie_softmax.hip). */
int i8ie_softmax_table(float s_in, uint32_t table_host[256]);
int i8ie_softmax_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t rows, int L, float s_in);
/* FP32: per row mx = max_j x_j; e_j = expf(x_j - mx); S = the fp32 sum of e_j in ascending j; out_j = e_j / S (one
 * division per element).  out may alias in. */
int i8ie_softmax_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int64_t rows, int L);

/* ---- fused multi-head attention (no counterpart in the reference) -----------------------------------------------------
 * Scaled-dot-product attention over `heads` heads as one op.  q is [b, tq, c], k and v are [b, tk, c], c = heads * d; each
 * is a u8 tensor with its own (scale, zero_point); head h is columns h*d .. h*d + d - 1.  Nothing new is defined
 * arithmetically: for every (batch item, head) the result is exactly the composition of the three entries above,
 *     S   = bmm_u8(Q_h [tq x d], K_h^T [d x tk]; s_q, zp_q, s_k, zp_k -> s_s, zp_s)    no relu; the u8 scores
 *     P   = softmax_u8(S, s_s) over tk                                                 scale 1/256, zero point 0
 *     O_h = bmm_u8(P [tq x tk], V_h [tk x d]; 1/256, 0, s_v, zp_v -> s_o, zp_o)        then the optional relu
 * byte for byte: down_scale's fp32 steps (the second product's requantiser takes (float)(1.0 / 256) as s_a and s_v as s_b,
 * in this order: its products do not commute), the table E[d] of s_s and min(255, (E * 256 + S / 2) / S).  There is no
 * alpha, no mask, no bias and no dropout: the 1/sqrt(d) factor folds into the weights of the projection that makes q.
 * Conditions: b, heads, d, tq >= 1; 1 <= tk <= 32768 (the second product's k); scales finite, s_s > 0 and s_o > 0.
 * Each operand is described physically (i8ie_attn_mat): element (batch, token, column) lies at
 * ptr[batch * batch_stride + token * token_stride + column], token_stride >= heads * d, columns contiguous; s8 != 0: the
 * bytes are stored re-biased (^0x80).  The strides make a packed QKV operand free: one projection c -> 3c gives
 * [b, t, 3c], and q, k, v are that buffer at byte offsets 0, c, 2c with token stride 3c.  Any two operands may be the
 * same buffer; `out` must not overlap an operand.  The result is plain [b, tq, c] through out.batch_stride and
 * out.token_stride (out_h == 0; out_w and out_border must then be 0 too), or the interior of a bordered NHWC map
 * [b, out_h + 2B, out_w + 2B, .] with B = out_border >= 0 and tq == out_h * out_w: `out.ptr` is then the buffer's first
 * byte, out.token_stride the stride of one physical pixel (>= c), out.batch_stride that of one image, and token p lies at
 * physical pixel (p / out_w + B) * (out_w + 2B) + p % out_w + B (i8ie_bmm_args' pixel rule).  Only the c result bytes of a
 * token are written: border bytes and the gap of a token stride above c are the caller's.  out.s8 != 0 stores re-biased.
 * Debug outputs, each NULL or: scores_dbg_dev u8 [b, heads, tq, tk] (S), probs_dbg_dev u8 [b, heads, tq, tk] (P),
 * acc_dbg_dev int32 [b, tq, c] (the second product's accumulators).  scores_out_dev belongs to the FP32 entry and must be
 * NULL here.  Stateless and capturable in a graph: one launch, no device allocation; the softmax table travels by value in
 * the kernel arguments.  Every argument error is I8IE_ERR_ARG before any device call.  As in the other stateless entries,
 * extents and overlap are the caller's responsibility.
 * Two kernels with identical bytes (csrc/i8ie_attention.hip): attn_mfma (d % 16 == 0, operand
 * pointers and strides 16-byte aligned, tk <= 1024: scores and probabilities stay in LDS) and attn_direct for everything
 * else and for everything under I8IE_OPT_FORCE_FALLBACK. */
typedef struct i8ie_attn_mat {
  void* ptr;              /* device pointer (read-only for an operand) */
  int64_t batch_stride;   /* elements between two batch items */
  int64_t token_stride;   /* ... between two tokens (>= heads * d) */
  int s8;                 /* != 0: bytes stored re-biased (^0x80) */
} i8ie_attn_mat;
typedef struct i8ie_attention_args {
  int b, heads, d, tq, tk;
  i8ie_attn_mat q;        /* [b, tq, heads * d] */
  i8ie_attn_mat k, v;     /* [b, tk, heads * d] */
  i8ie_attn_mat out;      /* [b, tq, heads * d], plain or the interior of a bordered NHWC map */
  int out_h, out_w, out_border;   /* out_h == 0: plain */
  float s_q, s_k, s_v, s_s, s_o;
  uint8_t zp_q, zp_k, zp_v, zp_s, zp_o;
  int relu;
  uint8_t* scores_dbg_dev;   /* NULL or [b, heads, tq, tk] */
  uint8_t* probs_dbg_dev;    /* NULL or [b, heads, tq, tk] */
  int32_t* acc_dbg_dev;      /* NULL or [b, tq, heads * d] */
  float* scores_out_dev;     /* i8ie_attention_f32 only: NULL or float [b, heads, tq, tk] */
} i8ie_attention_args;
int i8ie_attention_u8(i8ie_ctx* ctx, const i8ie_attention_args* args);
/* FP32 (before convert(), and while calibrating): the same descriptor with float elements, strides in floats, a plain
 * result (every s8, out_h, out_w, out_border, the u8 debug pointers and relu must be 0 / NULL; scales and zero points are
 * ignored).  Per head it is i8ie_bmm_f32 (Q_h K_h^T), i8ie_softmax_f32, i8ie_bmm_f32 (P V_h), launched through strides
 * with the scores in the ctx workspace, so it is bit-identical to that composition; scores_out_dev, when given, receives
 * the scores before the softmax (what the calibrator samples).  The calibration path: 3 * heads launches, not tuned. */
int i8ie_attention_f32(i8ie_ctx* ctx, const i8ie_attention_args* args);

/* ---- windowed (local) attention on a map ---------------------------------------------------------
 * Attention inside the non-overlapping win_h x win_w windows of an [n, c, map_h, map_w] map, map_h % win_h == 0 and
 * map_w % win_w == 0.  Nothing new is defined arithmetically.  Let part(x) be
 *     [n, c, h, w] -> [n * (h / win_h) * (w / win_w), win_h * win_w, c]
 * with the window index counted (image, wy, wx) in that order and token j of a window being pixel
 * (wy * win_h + j / win_w, wx * win_w + j % win_w), and unpart its inverse.  Then
 *     out = unpart(attention(part(q), part(k), part(v), heads))
 * and per (window, head) the bytes are exactly those of i8ie_bmm_u8, i8ie_softmax_u8, i8ie_bmm_u8 as i8ie_attention_u8
 * defines them.  There is no shift, no mask and no bias.  A window that is the whole map is the global form, with the same
 * bytes by definition.
 * The i8ie_attention_args are read as follows: b is the image count; tq == tk == win_h * win_w (<= 32768); q, k, v and out
 * describe whole maps, each the interior of a channels-last buffer [b][map_h + 2B][map_w + 2B][.] with a border B of its
 * own (q_border, k_border, v_border here, out_border in the args): ptr is the buffer's first byte (plus the column offset
 * of a packed operand), token_stride the stride of one physical pixel (>= heads * d), batch_stride that of one image, s8
 * the re-bias mark.  Every border is at most 65535 pixels.  An operand's border is never read, the result's never
 * written.  out_h and out_w must equal map_h and map_w, and b * heads * map_h * map_w must fit 31 bits.  The debug outputs count a window as a batch item: scores_dbg_dev and probs_dbg_dev are [b * nW, heads, T, T],
 * acc_dbg_dev is [b * nW, T, c], nW = (map_h / win_h) * (map_w / win_w), T = win_h * win_w.  Everything else (scales, zero
 * points, relu, one launch, no allocation, capturable) is as for i8ie_attention_u8; every argument error is I8IE_ERR_ARG
 * before any device call.  The same two kernels, instantiated with the window's row-to-pixel map
 * (j / win_w) * row pitch + (j % win_w) * pixel stride in place of the single token stride: attn_mfma under the global
 * entry's conditions (d % 16 == 0, 16-byte-aligned pointers and strides, T <= 1024; one window per 64-row tile), attn_direct
 * for everything else and under I8IE_OPT_FORCE_FALLBACK, with identical bytes. */
typedef struct i8ie_attention_window {
  int map_h, map_w;                  /* the map every operand and the result cover */
  int win_h, win_w;                  /* the window; must divide the map */
  int q_border, k_border, v_border;  /* the physical border, in pixels, of each operand's buffer (>= 0) */
} i8ie_attention_window;
int i8ie_attention_window_u8(i8ie_ctx* ctx, const i8ie_attention_args* args, const i8ie_attention_window* win);
/* FP32 (before convert(), and while calibrating): q, k, v and out are NCHW float maps without borders; element
 * (image, column, y, x) lies at ptr[image * batch_stride + column * token_stride + y * map_w + x], so token_stride is here
 * the channel stride (>= map_h * map_w; a packed [n, 3c, h, w] tensor gives q, k, v at offsets 0, c * h * w, 2c * h * w).
 * Every border, s8, relu and u8 debug pointer must be 0 / NULL.  Two small kernels gather the windows of q, k and v into
 * dense [b * nW, T, c] arrays in the ctx workspace and scatter the result back; between them runs i8ie_attention_f32, so
 * the result is bit-identical to that entry on host-partitioned tensors.  scores_out_dev, when given, receives the windowed
 * scores [b * nW, heads, T, T].  The calibration path, not tuned. */
int i8ie_attention_window_f32(i8ie_ctx* ctx, const i8ie_attention_args* args, const i8ie_attention_window* win);

/* ---- quantized LayerNorm over the last axis (no counterpart in the reference: every op of it is a contraction, a pointwise
 * map or a window reduction; none takes a statistic of a row at run time) ----------------------------------------------------
 * A row is C bytes a[0..C) with (s_in, zp_in), 1 <= C <= 16384; eps is finite and > 0; the result carries (s_out, zp_out);
 * gamma[C], beta[C] are fp32.  LayerNorm does not depend on the input zero point and the input scale enters only through
 * eps, so the statistics stay in the integers:
 *     S1 = sum a[c]           S2 = sum a[c]^2        exact; S2 <= 16384 * 65025 < 2^31 (the reason for the bound on C)
 *     V  = C * S2 - S1 * S1   exact in int64, 0 <= V < 2^53          (= C^2 * the variance in byte units)
 *     E  = (double)C * C * (double)eps / ((double)s_in * (double)s_in)                  host, double
 *     r  = (float)(1.0 / sqrt((double)V + E))    IEEE double add, sqrt, divide; one rounding to float
 *     d[c] = C * a[c] - S1                       integer, |d| <= 255 * C < 2^22: exact in fp32
 *     g[c] = gamma[c] / s_out                    fp32 divide                    }  i8ie_layernorm_affine, once per layer
 *     b[c] = (beta[c] / s_out) + (float)zp_out   fp32, two roundings            }
 *     t = (float)d[c] * r;  u = t * g[c];  v = u + b[c]        fp32, three roundings, no contraction
 *     q = v >= 255 ? 255 : (v < 0 ? 0 : (u8)v)   down_scale's clamp + truncation, src/quantize_utils.cc:27-36
 *     q = relu ? max(q, zp_out) : q              relu<u8>, src/functional.cc:15-26
 * A constant row has V = 0, every d = 0, t = 0 and q = clamp(trunc(b[c])).  E must be positive and 1 / sqrt(E) finite in
 * fp32 (so r is finite whatever V is); every g[c] and b[c] must be finite.  No NaN can then arise: t is finite, u may
 * overflow to an infinity, which clamps.
 * The bound against the real numbers.  Let y* = T G + Bt be the real-number LayerNorm of the dequantised row in output
 * units, T = d / sqrt(V + C^2 eps / s_in^2) (= (x - mean) / sqrt(var + eps) exactly: sum d^2 = C V, so |T| <= sqrt(C)),
 * G = gamma / s_out, Bt = beta / s_out + zp_out, all as real numbers of the fp32 inputs.  With u = 2^-24:
 *     r = (1 + e_r) / sqrt(V + E*),  |e_r| <= u + 4 * 2^-53 (three double roundings of E, one each of the add, sqrt, divide)
 *     t u-product: u_fp = T G (1 + th), |th| <= 4.01 u (r, t, g, u: four fp32 roundings)
 *     b = Bt + e_b, |e_b| <= u |beta / s_out| + u (|beta / s_out| (1 + u) + 255)
 *     v = (u_fp + b)(1 + e_3)
 *     |v - y*| <= B(y*) = 1.01 * 2^-24 * (5 |T G| + 2 |beta / s_out| + 255 + |y*|)
 * (5 instead of 4.01 and the factor 1.01 absorb every second-order term; a product below 2^-126 adds at most 2^-149.)
 * Where y* is further than B from an integer, q = clamp(trunc(y*)).
 * i8ie_layernorm_affine: host only (no ctx, like i8ie_activation_table): g_host[c], b_host[c] from gamma, beta.  s_out must
 * be finite and > 0, C in 1..16384, every gamma, beta, g and b finite; null pointers are I8IE_ERR_ARG too. */
int i8ie_layernorm_affine(const float* gamma, const float* beta, int C, float s_out, uint8_t zp_out, float* g_host,
                          float* b_host);
/* `rows` flat rows of C contiguous bytes, any alignment of in and out; out may alias in (no other overlap).  g_dev, b_dev:
 * fp32 [C] on the device (4-byte aligned), as i8ie_layernorm_affine made them.  zp_in is not an argument: it drops out.
 * Stateless: one launch, no device allocation, no host synchronisation, capturable in a graph.  C outside 1..16384, eps
 * or s_in not finite and positive (or an E as excluded above), rows <= 0 or > 2^31 - 1 and null pointers are I8IE_ERR_ARG
 * with a message, before any device call.  Three kernels with identical bytes (csrc/i8ie_layernorm.hip, DESIGN.md section
 * 8l): layernorm_u8_group (a power-of-two group of lanes per row, C <= 4096), layernorm_u8_block (one block per row) and
 * layernorm_u8_direct (one lane per row, the definition verbatim) for in, out, g or b not 16-byte aligned and for
 * everything under I8IE_OPT_FORCE_FALLBACK. */
int i8ie_layernorm_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t rows, int C, const float* g_dev,
                      const float* b_dev, float s_in, float eps, int relu, uint8_t zp_out);
/* The same on NHWC buffers [n, h+2b, w+2b, C] -> [n, h+2b', w+2b', C], each with its own border and plain (x_s8 = 0) or
 * re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80): a pixel is a row.  The input's border bytes are never read.
 * Only the interior of `out` is written: its border bytes are the caller's (i8ie_fill_border_u8), as for i8ie_add_u8_nhwc
 * and i8ie_lut_u8_nhwc.  out may be in itself when both geometries agree.  Negative borders and non-positive sizes are
 * I8IE_ERR_ARG too. */
int i8ie_layernorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                           int out_s8, int n, int C, int h, int w, const float* g_dev, const float* b_dev, float s_in,
                           float eps, int relu, uint8_t zp_out);
/* FP32 (before convert(), and while calibrating): per row of C floats, every step fp32 with one rounding per operation, no
 * contraction: mean = (sum of x[c] in ascending c) / C; var = (sum of (x[c] - mean)^2 in ascending c) / C;
 * out[c] = (x[c] - mean) / sqrtf(var + eps) * gamma[c] + beta[c].  out may alias in.  1 <= C <= 16384, eps finite and > 0.
 * Element c of row r lies at ((r / inner) * C + c) * inner + r % inner: inner = 1 is flat rows of C floats; an NCHW tensor
 * normalised over c per pixel is rows = n * h * w, inner = h * w (one launch, no transposition).  inner must divide rows. */
int i8ie_layernorm_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int64_t rows, int C, const float* gamma_dev,
                       const float* beta_dev, float eps, int64_t inner);

/* ---- quantized GroupNorm over the pixels of an image (no counterpart in the reference) -----------------------------------
 * The input is [n, C, h, w] bytes with (s_in, zp_in); there are G groups, C % G == 0, cg = C / G.  Row (i, g) is the
 * N = cg * h * w bytes of image i whose channel c lies in [g cg, (g + 1) cg); gamma[C], beta[C] are fp32, indexed by the
 * element's channel.  G == C is InstanceNorm, G == 1 a LayerNorm over (c, h, w) of one image.  1 <= N <= 65536:
 *     |N a - S1| <= 255 * 65536 < 2^24, so d is exact in fp32;
 *     S2 <= 65536 * 65025 < 2^32: it is kept in an unsigned 32 (or 64 bits), not in a signed 32;
 *     V = N S2 - S1^2 <= (255 N)^2 / 4 < 2^47 < 2^53, exact in int64 and in a double.
 * eps is finite and > 0.  Per row the arithmetic is the LayerNorm's above with C read as N, line for line:
 *     S1 = sum a     S2 = sum a^2     V = N * S2 - S1 * S1  (int64)
 *     E  = (double)N * N * (double)eps / ((double)s_in * (double)s_in)                  host, double
 *     r  = (float)(1.0 / sqrt((double)V + E))
 *     d = N * a - S1;  t = (float)d * r;  u = t * g[c];  v = u + b[c]     fp32, three roundings, no contraction
 *     q = v >= 255 ? 255 : (v < 0 ? 0 : (u8)v);  q = relu ? max(q, zp_out) : q
 * with g[c], b[c] of the element's channel c from i8ie_layernorm_affine (C values, unchanged).  zp_in drops out.  A constant
 * row has V = 0 and q = clamp(trunc(b[c])).  The exclusions are the LayerNorm's: E positive with 1 / sqrt(E) finite in fp32,
 * every g[c] and b[c] finite; no NaN can then arise.
 * The bound against the real-number GroupNorm y* = T G + Bt (T = d / sqrt(V + N^2 eps / s_in^2) = (x - mean) / sqrt(var +
 * eps), sum d^2 = N V so |T| <= sqrt(N); G = gamma[c] / s_out, Bt = beta[c] / s_out + zp_out) is the LayerNorm's, whose
 * derivation uses the row length in |T| <= sqrt(N) alone:
 *     |v - y*| <= B(y*) = 1.01 * 2^-24 * (5 |T G| + 2 |beta / s_out| + 255 + |y*|)
 * and q = clamp(trunc(y*)) wherever y* is further than B from an integer.
 *
 * i8ie_groupnorm_u8_nhwc: NHWC buffers [n, h+2b, w+2b, C] -> [n, h+2b', w+2b', C], each with its own border and plain or
 * re-biased (x_s8 != 0: bytes ^ 0x80), as for i8ie_layernorm_u8_nhwc.  The input's border bytes are never read; only the
 * interior of `out` is written; out may be in itself when both geometries agree.  A flat [n, C] tensor is h = w = 1, border
 * 0.  g_dev, b_dev: fp32 [C] on the device, 4-byte aligned.  ws_dev: i8ie_groupnorm_workspace_bytes(n, C, G, h, w) bytes
 * of the caller's, 4-byte aligned (may be NULL where that is 0); it need not be zeroed: partial sums are written, then
 * summed, with no atomics on device memory, so the integer statistics are bit-reproducible by construction.  Stateless: no
 * device allocation, no host synchronisation, capturable in a graph.  C % G != 0, N outside 1..65536, C outside 1..16384,
 * eps or s_in not finite and positive (or an E as excluded above), null pointers, negative borders, non-positive sizes and a
 * null ws_dev where the split form runs (the direct form, which unaligned pointers or I8IE_OPT_FORCE_FALLBACK select, takes
 * none) are I8IE_ERR_ARG with a message, before any device call.  Three forms with identical
 * bytes (csrc/i8ie_groupnorm.hip): groupnorm_u8_image (one launch, a block stages one image's interior
 * of at most I8IE_GROUPNORM_IMAGE_BYTES in LDS), groupnorm_u8_stats + groupnorm_u8_apply (two launches, larger images) and
 * groupnorm_u8_direct (the definition verbatim, one wave per row) for C % 16 != 0, C > 4096, in, out, g or b not 16-byte
 * aligned and for everything under I8IE_OPT_FORCE_FALLBACK. */
#define I8IE_GROUPNORM_MAX_N 65536
#define I8IE_GROUPNORM_IMAGE_BYTES 98304 /* h * w * C of the image form */
#define I8IE_GROUPNORM_CHUNK_BYTES 32768 /* the split form's pixel chunk: max(1, this / C) pixels */
int i8ie_groupnorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                           int out_s8, int n, int C, int G, int h, int w, const float* g_dev, const float* b_dev, float s_in,
                           float eps, int relu, uint8_t zp_out, void* ws_dev);
/* Host only, no ctx: the bytes ws_dev must hold for these sizes -- the split form's partial sums, n * chunks * 2 * G
 * unsigned 32-bit values, chunks = ceil(h w / max(1, 32768 / C)) -- or 0 where no form needs any (the image form, and every
 * shape that takes the direct form whatever the pointers are).  -1 with a message for sizes the entry above refuses. */
int64_t i8ie_groupnorm_workspace_bytes(int n, int C, int G, int h, int w);
/* FP32 (before convert(), and while calibrating) on NCHW floats [n, C, hw]: row (i, g) is N = cg * hw contiguous floats.
 * Per row the sequence of i8ie_layernorm_f32 in ascending address order, every step fp32 with one rounding per operation, no
 * contraction: mean = (sum x) / N; var = (sum (x - mean)^2) / N; out = (x - mean) / sqrtf(var + eps) * gamma[c] + beta[c],
 * c the element's channel.  out may alias in.  1 <= N <= 65536, C % G == 0, eps finite and > 0.  Not tuned. */
int i8ie_groupnorm_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int C, int G, int64_t hw,
                       const float* gamma_dev, const float* beta_dev, float eps);

/* ---- max and average pooling with padding and ceil_mode (torch's geometry arguments; no counterpart in the reference) ----
 * One square window k = kernel_size, one stride s, one padding p on every side, 0 <= p <= k / 2 (torch's rule), and
 * k <= h + 2p, k <= w + 2p.  Per axis of length `in` the output size is, in integer division,
 *     o = (in + 2p - k + (ceil_mode ? s - 1 : 0)) / s + 1;     if ceil_mode and (o - 1) * s >= in + p:  o -= 1
 * (a window must start inside the image or its leading padding: (k, s, p, in) = (2, 2, 1, 3) gives 2, not 3).  Output
 * (y, x) sees rows [y*s - p, min(y*s - p + k, h + p)) cut to [0, h), and columns likewise; every window has at least one
 * valid tap (by p <= k / 2 and the drop rule).  The result carries the input's (scale, zero_point).
 * max:  the maximum of the valid taps only -- padding never takes part; relu != 0: q = max(q, zero_point).
 * avg:  with n_valid the number of valid taps and S their exact byte sum,
 *     count_include_pad != 0 (torch's default):  D = (ye - ys) * (xe - xs), ys = y*s - p, ye = min(ys + k, h + p) and
 *         likewise in x: the padding counts, a ceil-mode overhang beyond it does not; S' = S + (D - n_valid) * zero_point,
 *         a padded zero being the byte zero_point
 *     count_include_pad == 0:                    D = n_valid, S' = S
 *     q = (S' + D / 2) / D        integer floor division: round to nearest, ties up (the rule of i8ie_avgpool2d_u8)
 *     q = relu ? max(q, zero_point) : q
 *   k * k <= 65536.
 * FP32 (before convert(), and while calibrating), NCHW: max is i8ie_maxpool2d_f32's running maximum (start -FLT_MAX,
 * mx >= v ? mx : v) over the valid taps in window order; avg sums the valid taps in fp32 in window order (rows outer,
 * columns inner) and divides once by (float)D.
 * With padding = 0 and ceil_mode = 0 every entry computes what its unpadded counterpart does.  Null pointers, non-positive
 * sizes, negative padding or borders, p > k / 2, a window larger than the padded input and k * k > 65536 are I8IE_ERR_ARG,
 * raised before any device call.  Stateless, no scratch, capturable in a graph (csrc/i8ie_padpool.hip, DESIGN.md
 * section 8o).
 * i8ie_pool_output_size: the output size above (host only); I8IE_ERR_ARG (negative) for arguments the entries refuse. */
int i8ie_pool_output_size(int in, int kernel_size, int stride, int padding, int ceil_mode);
/* NCHW in and out, any shape: one lane per output, off the timed path. */
int i8ie_maxpool2d_u8_pad(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w,
                          int kernel_size, int stride, int padding, int ceil_mode);
int i8ie_avgpool2d_u8_pad(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int n, int c, int h, int w,
                          int kernel_size, int stride, int padding, int ceil_mode, int count_include_pad,
                          uint8_t zero_point);
/* The same on NHWC buffers [n, h+2b, w+2b, c] -> [n, oh+2b', ow+2b', c], each with its own border and each plain
 * (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80).  The input's border bytes are not padding:
 * neither kernel ever reads a byte outside the interior.  Only the interior of `out` is written: its border bytes are the
 * caller's (i8ie_fill_border_u8).  Any c: 16 / 4 / 1 channels per lane by c % 16, c % 4 and the pointers' alignment.
 * `out` must not overlap `in`.  h, w: logical input dims. */
int i8ie_maxpool2d_u8_nhwc_pad(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                               int out_border, int out_s8, int n, int c, int h, int w, int kernel_size, int stride,
                               int padding, int ceil_mode, int relu, uint8_t zero_point);
int i8ie_avgpool2d_u8_nhwc_pad(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev,
                               int out_border, int out_s8, int n, int c, int h, int w, int kernel_size, int stride,
                               int padding, int ceil_mode, int count_include_pad, int relu, uint8_t zero_point);
/* FP32, NCHW (above). */
int i8ie_maxpool2d_f32_pad(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w,
                           int kernel_size, int stride, int padding, int ceil_mode);
int i8ie_avgpool2d_f32_pad(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w,
                           int kernel_size, int stride, int padding, int ceil_mode, int count_include_pad);

/* ---- quantized inference BatchNorm (torch.nn.BatchNorm2d in eval mode; no counterpart in the reference) -------------------
 * Inference only: the statistics are the stored running ones; there is no momentum, no training mode and no
 * track_running_stats.  The input is [n, C, h, w] bytes with (s_in, zp_in), 1 <= C <= 16384; gamma, beta, mean, var are fp32
 * [C] with var[c] >= 0; eps is finite and > 0; the result carries (s_out, zp_out):
 *     k[c] = (double)gamma[c] / sqrt((double)var[c] + (double)eps)                          host, double
 *     g[c] = (float)(k[c] / (double)s_out)                                                  } i8ie_batchnorm_affine, once per
 *     b[c] = (float)(((double)beta[c] - (double)mean[c] * k[c]) / (double)s_out + zp_out)   } layer: one rounding to float each
 *     x = (float)((int)a - (int)zp_in) * s_in          dequantize, src/quantize_utils.cc:38-42
 *     t = x * g[c];  v = t + b[c]                      fp32, one rounding per operation, no contraction
 *     q = v >= 255 ? 255 : (v < 0 ? 0 : (u8)v)         down_scale's clamp + truncation, src/quantize_utils.cc:27-36
 *     q = relu ? max(q, zp_out) : q                    relu<u8>, src/functional.cc:15-26
 * (every double operation of k, g, b is IEEE, one rounding each, in the order written, no contraction.)  Every g[c] and b[c]
 * must be finite, else I8IE_ERR_ARG from the host entry; s_in and 255 * s_in must be finite.  No NaN can then arise: x is
 * finite, t may overflow to an infinity, which clamps.  g and b do not depend on the input's quantisation: they are made once
 * per layer, and s_in, zp_in are arguments of the launch.  Per (channel, byte) the op is a fixed function; a kernel may
 * evaluate it any way that gives these bytes.
 * The bound against the real numbers.  With T = (a - zp_in) s_in k / s_out, Bt = (beta - mean k) / s_out + zp_out and
 * y* = T + Bt, all as real numbers of the fp32 inputs:
 *     |v - y*| <= B = 1.01 * 2^-24 * (4 |T| + |Bt| + |y*|)
 * (x, g and t round once each on the T path, b once, v once: 3 |T| + |Bt| + |y*|; 4 and the factor 1.01 absorb the double
 * roundings and every second-order term.)  Where y* lies further than B from an integer, q = clamp(trunc(y*)).
 * i8ie_batchnorm_affine: host only (no ctx, like i8ie_layernorm_affine).  Null pointers, C outside 1..16384, eps or s_out not
 * finite and positive, a gamma, beta, mean or var that is not finite, var[c] < 0 and a g[c] or b[c] that is not finite are
 * I8IE_ERR_ARG; argument errors are reported before anything is written. */
int i8ie_batchnorm_affine(const float* gamma, const float* beta, const float* mean, const float* var, int C, float eps,
                          float s_out, uint8_t zp_out, float* g_host, float* b_host);
/* NHWC buffers [n, h+2b, w+2b, C] -> [n, h+2b', w+2b', C], each with its own border and plain (x_s8 = 0) or re-biased
 * (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80), the rules of i8ie_layernorm_u8_nhwc: the input's border bytes are never
 * read; only the interior of `out` is written; out may be in itself when both geometries agree.  g_dev, b_dev: fp32 [C] on
 * the device (4-byte aligned), as i8ie_batchnorm_affine made them.  Stateless: one launch, no device allocation, no host
 * synchronisation, capturable in a graph.  Null pointers, C outside 1..16384, non-positive sizes, negative borders, more than
 * 2^30 pixels per image and an s_in for which 255 * s_in is not finite are I8IE_ERR_ARG with a message, before any device
 * call.  Two kernels with identical bytes (csrc/i8ie_batchnorm.hip): batchnorm_u8_nhwc (16 / 4 / 1
 * channels per lane by C % 16 and C % 4, g and b in registers over a run of I8IE_BATCHNORM_WALK pixels) and
 * batchnorm_u8_direct (one lane per byte, the definition verbatim) for in, out, g or b not 16-byte aligned and for
 * everything under I8IE_OPT_FORCE_FALLBACK. */
#define I8IE_BATCHNORM_WALK 8
int i8ie_batchnorm_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                           int out_s8, int n, int C, int h, int w, const float* g_dev, const float* b_dev, float s_in,
                           uint8_t zp_in, int relu, uint8_t zp_out);
/* The flat form for reference-order tensors, any alignment of in and out; out may alias in (no other overlap).  Element c of
 * row r lies at ((r / inner) * C + c) * inner + r % inner, the convention of i8ie_layernorm_f32: inner = 1 is rows [m, C],
 * inner = h * w an NCHW tensor in one launch (rows = n * h * w).  inner must divide rows; 1 <= rows <= 2^31 - 1.  Always
 * batchnorm_u8_direct. */
int i8ie_batchnorm_u8(i8ie_ctx* ctx, const uint8_t* in_dev, uint8_t* out_dev, int64_t rows, int C, int64_t inner,
                      const float* g_dev, const float* b_dev, float s_in, uint8_t zp_in, int relu, uint8_t zp_out);
/* FP32 (before convert(), and while calibrating), the same element order: out = (x - mean[c]) / sqrtf(var[c] + eps) *
 * gamma[c] + beta[c], every step fp32 with one rounding per operation, no contraction (torch's eval-mode formula).  out may
 * alias in.  Not tuned. */
int i8ie_batchnorm_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int64_t rows, int C, int64_t inner,
                       const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev, float eps);

/* ---- position embedding with an optional class token (no counterpart in the reference) ----------------------------------
 * The input is [n, c, h, w] bytes with (s_in, zp_in), counted as n sequences of T = h * w tokens of c channels: token j is
 * pixel (j / w, j % w), the order in which i8ie_attention_u8 and i8ie_layernorm_u8_nhwc count a rank-4 tensor.  E is an
 * fp32 table [T', c] shared by every image of the batch; the result carries (s_out, zp_out).
 *     class_token == 0: T' = T, the result is [n, c, h, w], and output token j is input token j.
 *     class_token != 0: T' = T + 1, the result is [n, c, 1, T + 1] (physically [n, T + 1, c]); output token 0 has no input
 *                       byte (its dequantised value is +0) and output token 1 + j is input token j.  This is torchvision's
 *                       cat([class_token.expand(n, -1, -1), tokens], 1) + pos_embedding in the engine's NHWC storage.
 * E = P (the learned table, torch's pos_embedding[0]), except row 0 of the class form: E[0][ch] = cls[ch] + P[0][ch], one
 * fp32 add on the host (i8ie_posembed_table).  Per output element, the composition of the reference's dequantize
 * (src/quantize_utils.cc:38-42) and down_scale's clamp and truncation (:27-36), IEEE fp32, one rounding per operation, no
 * contraction, as for i8ie_add_u8:
 *     fa = (float)((int)a - (int)zp_in) * s_in          (the class column: fa = +0)
 *     t  = (fa + E[tok][ch]) / s_out + (float)zp_out
 *     q  = t >= 255 ? 255 : (t < 0 ? 0 : (u8)t);   q = relu ? max(q, zp_out) : q        (relu<u8>, src/functional.cc:15-26)
 * Every E entry, s_in, 255 * s_in and s_out must be finite and s_out > 0.  No NaN can then arise: fa and E are finite, their
 * sum may overflow to an infinity, which clamps.
 * The bound against the real numbers.  With Fa = (a - zp_in) s_in / s_out, X = ((a - zp_in) s_in + E*) / s_out and
 * y* = X + zp_out as real numbers of the fp32 inputs, E* = P (row 0 of the class form: cls + P[0], the real sum), u = 2^-24:
 *     |t - y*| <= B = 1.01 * u * (|Fa| + 3 |X| + |y*|)
 * (fa rounds once: u |Fa|; E[0] of the class form, the sum fa + E and the quotient once each: 3 u |X|; t once: u |y*|; the
 * factor 1.01 absorbs every second-order term, and a quotient below 2^-126 adds at most 2^-149.)  Where y* lies further than
 * B from an integer, q = clamp(trunc(y*)).
 * i8ie_posembed_table: host only (no ctx, like i8ie_layernorm_affine): E_host[tokens][c] from P[tokens][c] and, where cls is
 * not null, the class token cls[c] added into row 0.  Null P or E_host, c outside 1..16384, tokens < 1 or > 2^30 and a P, cls
 * or E entry that is not finite are I8IE_ERR_ARG; an error is reported before anything is written.  E_host may be P. */
int i8ie_posembed_table(const float* P, const float* cls, int tokens, int c, float* E_host);
/* NHWC buffers [n, h+2b, w+2b, c] -> [n, h+2b', w+2b', c] (class_token: [n, 1+2b', T+1+2b', c]), each with its own border
 * and plain (x_s8 = 0) or re-biased (x_s8 != 0: I8IE_LAYOUT_NHWC_S8, bytes ^ 0x80), the rules of i8ie_layernorm_u8_nhwc: the
 * input's border bytes are never read; only the interior of `out` is written, its border bytes are the caller's
 * (i8ie_fill_border_u8).  out may be in itself in the plain form when both geometries agree; otherwise the buffers must not
 * overlap.  e_dev: fp32 [T'][c] on the device (4-byte aligned), as i8ie_posembed_table made it.  Stateless: one launch, no
 * device allocation, no host synchronisation, capturable in a graph.  Null pointers, c outside 1..16384, non-positive
 * sizes, negative borders, more than 2^30 tokens per image, a scale that is not finite (255 * s_in included) and s_out <= 0
 * are I8IE_ERR_ARG with a message, before any device call; the table's entries are checked where it is made
 * (i8ie_posembed_table).  Two kernels with identical bytes (csrc/i8ie_posembed.hip):
 * posembed_u8_nhwc (16 / 4 / 1 channels of one token per lane by c % 16 and c % 4, the item's E values in registers over
 * up to I8IE_POSEMBED_WALK images, fewer where the batch is too small to fill the grid with that; the guarded estimate of
 * i8ie_add_u8 with its exact replay) and posembed_u8_direct (one lane per output byte, the definition verbatim) for in,
 * out or e_dev not 16-byte aligned and for everything under I8IE_OPT_FORCE_FALLBACK. */
#define I8IE_POSEMBED_WALK 8
int i8ie_posembed_u8_nhwc(i8ie_ctx* ctx, const uint8_t* in_dev, int in_border, int in_s8, uint8_t* out_dev, int out_border,
                          int out_s8, int n, int c, int h, int w, int class_token, const float* e_dev, float s_in,
                          uint8_t zp_in, float s_out, uint8_t zp_out, int relu);
/* FP32 (before convert(), and while calibrating) on NCHW floats: [n, c, h, w] -> [n, c, h, w] or, with class_token,
 * [n, c, 1, T + 1]: out = x + E[tok][ch] in fp32, one rounding; the class column is E[0][ch] itself.  4-byte aligned
 * buffers that do not overlap (the plain form may run in place).  Not tuned. */
int i8ie_posembed_f32(i8ie_ctx* ctx, const float* in_dev, float* out_dev, int n, int c, int h, int w, int class_token,
                      const float* e_dev);

#ifdef __cplusplus
}
#endif
#endif /* I8IE_HIP_H */
