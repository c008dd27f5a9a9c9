/*
 * gemm_provider.c -- the two CBLAS entry points the reference's layer code calls, in plain C.
 *
 * TEST INFRASTRUCTURE ONLY.  Linked into oracle/_ref/_i8ie_ref_layers*.so in place of libmkl_rt (MKL's integer
 * path is exact only on some hosts, see test_contraction_against_live_mkl_when_present), and built on its own as
 * oracle/libgemm_provider.so so that tests can hold it, bit for bit, to the committed MKL results
 * (tests/golden/mkl_gemm_s8u8s32.npz, mkl_gemm_seed9.npz) before anything generated through it is trusted.
 *
 * Only the argument patterns the reference uses are implemented; anything else aborts with a message:
 *   cblas_gemm_s8u8s32(RowMajor, NoTrans, Trans, RowOffset, m, n, k, alpha 1, A u8 lda, ao 0, B s8 ldb, bo 0,
 *                      beta 0, C, ldc, oc):   C[i][j] = sum_k A[i][k] * B[j][k] + oc[j], exact in int32
 *       (src/conv2d.cc:131-133, src/fully_connected.cc:39-41)
 *   cblas_sgemm(RowMajor, NoTrans, Trans, m, n, k, alpha 1, A lda, B ldb, beta 0, C, ldc):
 *       C[i][j] = (float)(sum_k (double)A[i][k] * (double)B[j][k]): each dot product accumulated in double,
 *       rounded once  (src/conv2d.cc:83-84 with A = weights, B = patches; src/fully_connected.cc:10-11 with
 *       A = input rows, B = weights)
 *
 * Hook: gp_set_hook(fn) registers a callback that sees m, n, C, ldc and oc of every integer call after it was
 * computed (the golden generator records the pre-requant accumulators with it).  Calls may come from several
 * OpenMP threads at once; the callback must cope with that.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

enum { ROW_MAJOR = 101, NO_TRANS = 111, TRANS = 112, ROW_OFFSET = 171 };

typedef void (*gp_hook_fn)(int m, int n, int k, const int32_t* c, int ldc, const int32_t* oc, const void* a);
static gp_hook_fn g_hook = 0;
void gp_set_hook(gp_hook_fn fn) { g_hook = fn; }

static void die(const char* what) {
  fprintf(stderr, "gemm_provider: %s: argument pattern the reference does not use\n", what);
  abort();
}

void cblas_gemm_s8u8s32(int layout, int transa, int transb, int offsetc, int m, int n, int k, float alpha,
                        const void* a, int lda, int8_t ao, const void* b, int ldb, int8_t bo, float beta, int32_t* c,
                        int ldc, const int32_t* co) {
  if (layout != ROW_MAJOR || transa != NO_TRANS || transb != TRANS || offsetc != ROW_OFFSET || alpha != 1.0f ||
      beta != 0.0f || ao != 0 || bo != 0 || m < 0 || n < 0 || k < 0 || lda < k || ldb < k || ldc < n)
    die("cblas_gemm_s8u8s32");
  const uint8_t* A = (const uint8_t*)a;
  const int8_t* B = (const int8_t*)b;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      const uint8_t* ar = A + (int64_t)i * lda;
      const int8_t* br = B + (int64_t)j * ldb;
      int32_t s = 0;
      for (int l = 0; l < k; ++l) s += (int32_t)ar[l] * (int32_t)br[l];
      c[(int64_t)i * ldc + j] = s + co[j];
    }
  if (g_hook) g_hook(m, n, k, c, ldc, co, a);
}

void cblas_sgemm(int layout, int transa, int transb, int m, int n, int k, float alpha, const float* a, int lda,
                 const float* b, int ldb, float beta, float* c, int ldc) {
  if (layout != ROW_MAJOR || transa != NO_TRANS || transb != TRANS || alpha != 1.0f || beta != 0.0f || m < 0 ||
      n < 0 || k < 0 || lda < k || ldb < k || ldc < n)
    die("cblas_sgemm");
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      const float* ar = a + (int64_t)i * lda;
      const float* br = b + (int64_t)j * ldb;
      double s = 0;
      for (int l = 0; l < k; ++l) s += (double)ar[l] * (double)br[l];
      c[(int64_t)i * ldc + j] = (float)s;
    }
}
