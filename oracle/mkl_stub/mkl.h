/* mkl.h -- stand-in for Intel MKL's umbrella header, for the oracle/_ref layer build only (oracle/Makefile,
 * target `ref_layers`; this directory is on the include path of that target alone).
 *
 * TEST INFRASTRUCTURE ONLY.  Declarations of the two entry points the reference's layer code calls, written
 * from the public CBLAS / oneMKL interface (enum values are the CBLAS standard's).  They are defined by
 * oracle/gemm_provider.c, not by MKL. */
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef enum { CblasRowMajor = 101, CblasColMajor = 102 } CBLAS_LAYOUT;
typedef enum { CblasNoTrans = 111, CblasTrans = 112, CblasConjTrans = 113 } CBLAS_TRANSPOSE;
typedef enum { CblasRowOffset = 171, CblasColOffset = 172, CblasFixOffset = 173 } CBLAS_OFFSET;
void cblas_sgemm(CBLAS_LAYOUT layout, CBLAS_TRANSPOSE transa, CBLAS_TRANSPOSE transb, int m, int n, int k,
                 float alpha, const float* a, int lda, const float* b, int ldb, float beta, float* c, int ldc);
void cblas_gemm_s8u8s32(CBLAS_LAYOUT layout, CBLAS_TRANSPOSE transa, CBLAS_TRANSPOSE transb, CBLAS_OFFSET offsetc,
                        int m, int n, int k, float alpha, const void* a, int lda, int8_t ao, const void* b, int ldb,
                        int8_t bo, float beta, int32_t* c, int ldc, const int32_t* co);
#ifdef __cplusplus
}
#endif
