/* hlmi_blas.h — apps/linear_algebra's BLAS interface over libhlmi.so, f32 (s*) and f64 (d*): the 2 x twelve pipelines of
 * hlmi_pipelines.h under the call shapes a CBLAS user expects.  A consumer of the reference's halide_blas.h includes this file instead and links
 * libhlmi.so; plain C and C++ both compile it.
 *
 * Three layers, as in the reference:
 *   halide_s*_impl / halide_sdot / ...   the AOT entry points on halide_buffer_t (hlmi_pipelines.h); halide_d* likewise
 *   halide_scopy ... halide_sgemm        inline wrappers that pass the one buffer that is both read and written twice: the output
 *                                        of every pipeline IS its y / C argument
 *   hblas_s*                             raw host pointers: each call wraps them in buffers, runs the pipeline on the GPU, copies the
 *                                        result back and frees the device side
 *
 * Where hblas_s* and hblas_d* depart from the reference, on purpose:
 *   - incX / incY other than 1: one line on stderr, nothing computed (the pipelines take stride 1 only; the reference builds its
 *     pipelines without assertions and would compute garbage);
 *   - HblasRowMajor: one line on stderr, nothing computed (the reference ignores Order and computes column-major);
 *   - hblas_sgemm / hblas_dgemm with a transposed operand that is not square (M != K for TransA, N != K for TransB): one line on stderr, nothing
 *     computed — the generator's own limit, see hlmi_pipelines.h;
 *   - the calls that return a scalar return NaN in those cases, and where the pipeline itself fails.
 * Matrices are column-major with leading dimension lda >= rows. */
#ifndef HLMI_BLAS_H
#define HLMI_BLAS_H

#include "hlmi_pipelines.h"
#include "hlmi_runtime.h"

#ifdef __cplusplus
extern "C" {
#endif

enum HBLAS_ORDER { HblasRowMajor = 101, HblasColMajor = 102 };
enum HBLAS_TRANSPOSE { HblasNoTrans = 111, HblasTrans = 112, HblasConjTrans = 113 };
enum HBLAS_UPLO { HblasUpper = 121, HblasLower = 122 };
enum HBLAS_DIAG { HblasNonUnit = 131, HblasUnit = 132 };
enum HBLAS_SIDE { HblasLeft = 141, HblasRight = 142 };

/* y = x */
static inline int halide_scopy(struct halide_buffer_t *x, struct halide_buffer_t *y) { return halide_scopy_impl(0.0f, x, 0, y); }
/* x = a x */
static inline int halide_sscal(float a, struct halide_buffer_t *x) { return halide_sscal_impl(a, x, 0, x); }
/* y = a x + y */
static inline int halide_saxpy(float a, struct halide_buffer_t *x, struct halide_buffer_t *y) { return halide_saxpy_impl(a, x, y, y); }
/* y = a op(A) x + b y; trans != 0: op(A) is A transposed */
static inline int halide_sgemv(int trans, float a, struct halide_buffer_t *A, struct halide_buffer_t *x, float b, struct halide_buffer_t *y) {
    return trans ? halide_sgemv_trans(a, A, x, b, y, y) : halide_sgemv_notrans(a, A, x, b, y, y);
}
/* A = a x y' + A */
static inline int halide_sger(float a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *A) {
    return halide_sger_impl(a, x, y, A);
}
/* C = a op(A) op(B) + b C */
static inline int halide_sgemm(int transA, int transB, float a, struct halide_buffer_t *A, struct halide_buffer_t *B, float b,
                               struct halide_buffer_t *C) {
    if (transA && transB) return halide_sgemm_transAB(a, A, B, b, C, C);
    if (transA) return halide_sgemm_transA(a, A, B, b, C, C);
    if (transB) return halide_sgemm_transB(a, A, B, b, C, C);
    return halide_sgemm_notrans(a, A, B, b, C, C);
}

/* the same wrappers for the f64 pipelines */
static inline int halide_dcopy(struct halide_buffer_t *x, struct halide_buffer_t *y) { return halide_dcopy_impl(0.0, x, 0, y); }
static inline int halide_dscal(double a, struct halide_buffer_t *x) { return halide_dscal_impl(a, x, 0, x); }
static inline int halide_daxpy(double a, struct halide_buffer_t *x, struct halide_buffer_t *y) { return halide_daxpy_impl(a, x, y, y); }
static inline int halide_dgemv(int trans, double a, struct halide_buffer_t *A, struct halide_buffer_t *x, double b, struct halide_buffer_t *y) {
    return trans ? halide_dgemv_trans(a, A, x, b, y, y) : halide_dgemv_notrans(a, A, x, b, y, y);
}
static inline int halide_dger(double a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *A) {
    return halide_dger_impl(a, x, y, A);
}
static inline int halide_dgemm(int transA, int transB, double a, struct halide_buffer_t *A, struct halide_buffer_t *B, double b,
                               struct halide_buffer_t *C) {
    if (transA && transB) return halide_dgemm_transAB(a, A, B, b, C, C);
    if (transA) return halide_dgemm_transA(a, A, B, b, C, C);
    if (transB) return halide_dgemm_transB(a, A, B, b, C, C);
    return halide_dgemm_notrans(a, A, B, b, C, C);
}

/* level 1 */
void hblas_scopy(const int N, const float *X, const int incX, float *Y, const int incY);
void hblas_sscal(const int N, const float alpha, float *X, const int incX);
void hblas_saxpy(const int N, const float alpha, const float *X, const int incX, float *Y, const int incY);
float hblas_sdot(const int N, const float *X, const int incX, const float *Y, const int incY);
float hblas_snrm2(const int N, const float *X, const int incX); /* sqrtf of hblas_sdot(X, X) */
float hblas_sasum(const int N, const float *X, const int incX);

/* level 2 */
void hblas_sgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const float alpha, const float *A,
                 const int lda, const float *X, const int incX, const float beta, float *Y, const int incY);
void hblas_sger(const enum HBLAS_ORDER order, const int M, const int N, const float alpha, const float *X, const int incX, const float *Y,
                const int incY, float *A, const int lda);

/* level 3 */
void hblas_sgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                 const int K, const float alpha, const float *A, const int lda, const float *B, const int ldb, const float beta, float *C,
                 const int ldc);

/* the f64 calls: the signatures of the reference's halide_blas.h */
void hblas_dcopy(const int N, const double *X, const int incX, double *Y, const int incY);
void hblas_dscal(const int N, const double alpha, double *X, const int incX);
void hblas_daxpy(const int N, const double alpha, const double *X, const int incX, double *Y, const int incY);
double hblas_ddot(const int N, const double *X, const int incX, const double *Y, const int incY);
double hblas_dnrm2(const int N, const double *X, const int incX); /* sqrt of hblas_ddot(X, X) */
double hblas_dasum(const int N, const double *X, const int incX);
void hblas_dgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const double alpha, const double *A,
                 const int lda, const double *X, const int incX, const double beta, double *Y, const int incY);
void hblas_dger(const enum HBLAS_ORDER order, const int M, const int N, const double alpha, const double *X, const int incX, const double *Y,
                const int incY, double *A, const int lda);
void hblas_dgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                 const int K, const double alpha, const double *A, const int lda, const double *B, const int ldb, const double beta, double *C,
                 const int ldc);

#ifdef __cplusplus
}
#endif

#endif /* HLMI_BLAS_H */
