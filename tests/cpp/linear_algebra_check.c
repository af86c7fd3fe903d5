/* linear_algebra_check.c — plain-C checker of the twelve f32 pipelines of apps/linear_algebra: TEST INFRASTRUCTURE ONLY.
 *
 * The contract, verified line by line against the generators (apps/linear_algebra/src/):
 *   - Dimension 0 is innermost.  No generator touches stride.0, so Halide's default constraint stride.0 == 1 holds for every buffer;
 *     every generator pins min to 0.  Matrices are column-major: A(i, k) is A[k * lda + i].
 *   - V = natural_vector_size(float) = 8 on the x86-64 AVX2 target whose numbers SURVEY.md and BASELINE.md take (LA_V below: a choice).
 *   - Float forms (oracle/oracle_common.h): o_mad(a, b, c) = a * b + c, o_mad2(a, b, c, d) = a * b + c * d with the first product
 *     contracted; in form 0 every operator rounds once.  `*` is a rounded multiply.
 *   AXPYGenerator (blas_l1_generators.cpp:34-42): calc = a * x(i) + y(i) | a * x(i) | x(i) by (scale_x, add_to_y); the vectorised
 *     body and the tail evaluate the same expression per element.  scopy/sscal never reference y: the wrappers pass a null pointer.
 *   DotGenerator (:104-116): dot(i) += x(k V + i) * y(k V + i) over k in [0, n / V), from the pure definition's 0 — V lane chains,
 *     k upward; result() = sum(dot(lanes)) — an inline reduction from 0 over lanes 0 .. V - 1 in order; result() += sum(x(tail) *
 *     y(tail)) — a second inline reduction from 0 over the tail upward, added to the first.  AbsSumGenerator (:157-169): the same
 *     with abs(x) (an add, no multiply: one result in both forms).
 *   GEMVGenerator, notrans (blas_l2_generators.cpp:125-136): block(i) = b * y(i); block(i) += a * A(i, k) * x(k) over k in two
 *     RDoms that together run 0 .. N - 1 upward; `a * A * x` parses as (a * A) * x: the rounded a * A has one use and the outer
 *     product is the one contracted with the add.  The schedule (unroll, vectorize over i, reorder) never changes a single output's
 *     order of k.
 *   GEMVGenerator, trans (:45-70): prod(j, i) = A(j, i) * x(j); accum_vecs(j, i) += prod(k V + j, i) over k < M / V; sum_lanes(i) +=
 *     accum_vecs_transpose(i, lanes) from 0 over lanes in order; sum_tail(i) = sum_lanes(i), += prod(tail, i) upward;
 *     result(i) = b * y(i) + a * Ax(i): two products under one add, the first contracted (o_mad2).
 *   GERGenerator (:227-229): result(i, j) += (a * y(j)) * x(i) on the undefined (in-place) output.
 *   GEMMGenerator (blas_l3_generators.cpp:37-96): prod(k, i, j) = A(i, k) * B(k, j); AB(i, j) += prod(rv, i, j), rv = 0 .. sum_size - 1
 *     upward from 0 (unroll(rv, 2) keeps the order); result(i, j) = a * ABt(i, j) + b * C(i, j) — o_mad2, and b * C is evaluated
 *     whatever b is.
 *     Shapes (:37-39, :167-171 with halide_blas.cpp:254-256): num_rows = A_.width(), num_cols = B_.height() and sum_size = A_.height()
 *     come from the STORED matrices whatever the flags; B_.extent.0 is pinned to sum_size; C_ and result are num_rows x num_cols.
 *       notrans  A(i, k) = A_(i, k), B(k, j) = B_(k, j): M, N, K free.
 *       transA   A(i, k) = A_(k, i) (:62-63) with i < A_.width(), k < A_.height(): the reads stay inside A_ (and are not
 *                constant_exterior's zeros) only where A_ is square, M == K; N free.
 *       transB   B(k, j) = B_(j, k) (:71-72) with j < B_.height(), k < sum_size = B_.width(): B_ square, N == K; M free.
 *       transAB  the inputs are swapped (:51-53) and the product transposed (:88-90): ABt(i, j) = sum_k B_(j, k) * A_(k, i) with
 *                i < A_.width(), j < B_.height(), k < A_.height(); A_(k, i) needs A_ square, B_(j, k) with k < B_.width() needs
 *                B_ square: M == N == K.  The swapped operands only commute a product: the value is mad(A_(k, i), B_(j, k), ab).
 *     The checker takes the four as (ta, tb) and leaves the squareness rule to its callers.
 *
 * compareScalars (apps/linear_algebra/tests/test_halide_blas.cpp:150-173) is restated as la_compare. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

#include "oracle_common.h"

enum { LA_V = 8 };

int la_v(void) { return LA_V; }

/* mode 0: copy, 1: scal, 2: axpy; y is read by axpy only */
void la_axpy(int mode, float a, const float *x, const float *y, float *result, long n) {
    for (long i = 0; i < n; i++) result[i] = mode == 0 ? x[i] : mode == 1 ? a * x[i] : o_mad(a, x[i], y[i]);
}

/* the reductions with the vector width as an argument, so that the tests can ask what another width would give; v <= 64 */
float la_dot_v(const float *x, const float *y, long n, int v) {
    float lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0.0f;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = o_mad(x[k * v + i], y[k * v + i], lanes[i]);
    float s = 0.0f;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    float t = 0.0f;
    for (long e = nvec * v; e < n; e++) t = o_mad(x[e], y[e], t);
    return s + t;
}

float la_asum_v(const float *x, long n, int v) {
    float lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0.0f;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = lanes[i] + fabsf(x[k * v + i]);
    float s = 0.0f;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    float t = 0.0f;
    for (long e = nvec * v; e < n; e++) t = t + fabsf(x[e]);
    return s + t;
}

float la_dot(const float *x, const float *y, long n) { return la_dot_v(x, y, n, LA_V); }
float la_asum(const float *x, long n) { return la_asum_v(x, n, LA_V); }

/* A is w x h as stored (A(i, k) = A[k * lda + i]); notrans: x[h], y[w], out[w]; trans: x[w], y[h], out[h], lane width v */
void la_gemv(int trans, float a, const float *A, long lda, int w, int h, const float *x, float b, const float *y, float *out, int v) {
    if (!trans) {
        for (int i = 0; i < w; i++) {
            float acc = b * y[i];
            for (int k = 0; k < h; k++) acc = o_mad(a * A[(long)k * lda + i], x[k], acc);
            out[i] = acc;
        }
        return;
    }
    for (int i = 0; i < h; i++) {
        const float *col = A + (long)i * lda;
        float lanes[64];
        for (int j = 0; j < v; j++) lanes[j] = 0.0f;
        const int nvec = w / v;
        for (int k = 0; k < nvec; k++)
            for (int j = 0; j < v; j++) lanes[j] = o_mad(col[k * v + j], x[k * v + j], lanes[j]);
        float s = 0.0f;
        for (int j = 0; j < v; j++) s = s + lanes[j];
        for (int t = nvec * v; t < w; t++) s = o_mad(col[t], x[t], s);
        out[i] = o_mad2(b, y[i], a, s);
    }
}

/* in place on result[m x n] */
void la_ger(float a, const float *x, int m, const float *y, int n, float *result, long ldr) {
    for (int j = 0; j < n; j++) {
        const float ay = a * y[j];
        for (int i = 0; i < m; i++) result[(long)j * ldr + i] = o_mad(ay, x[i], result[(long)j * ldr + i]);
    }
}

/* result[M x N]; opA(i, k) = ta ? A[i * lda + k] : A[k * lda + i]; opB(k, j) = tb ? B[k * ldb + j] : B[j * ldb + k].  The loops run
 * j, k, i so that a compiler may do several i at once; every output still sees its own k = 0, 1, 2, ... in that order. */
void la_gemm(int ta, int tb, float a, const float *A, long lda, const float *B, long ldb, float b, const float *C, long ldc, float *result, long ldr,
             int M, int N, int K, float *scratch /* M floats */) {
    const int fma = o_canon_fma;
    float *turned = NULL; /* opA with i contiguous: a copy of the values, so that the inner loop reads memory in order */
    if (ta && M > 0 && K > 0) {
        turned = (float *)malloc(sizeof(float) * (size_t)M * (size_t)K);
        for (int i = 0; i < M; i++)
            for (int k = 0; k < K; k++) turned[(size_t)k * M + i] = A[(long)i * lda + k];
    }
    for (int j = 0; j < N; j++) {
        for (int i = 0; i < M; i++) scratch[i] = 0.0f;
        for (int k = 0; k < K; k++) {
            const float bv = tb ? B[(long)k * ldb + j] : B[(long)j * ldb + k];
            const float *col = ta ? turned + (size_t)k * M : A + (long)k * lda;
            if (fma) for (int i = 0; i < M; i++) scratch[i] = fmaf(col[i], bv, scratch[i]);
            else for (int i = 0; i < M; i++) scratch[i] = col[i] * bv + scratch[i];
        }
        for (int i = 0; i < M; i++) result[(long)j * ldr + i] = o_mad2(a, scratch[i], b, C[(long)j * ldc + i]);
    }
    free(turned);
}

/* compareScalars of the reference's tests, instantiated for float as BLASFloatTests does: x the expected value, y the actual one.
 *   x == y: accepted;  x or y zero, or |x - y| below FLT_MIN: accepted if |x - y| < epsilon * FLT_MIN;  else |x - y| / (|x| + |y|) < epsilon
 * every operation in float.  The callers pass 16 FLT_EPSILON for vectors and matrices and 32 FLT_EPSILON for scalars (:150, :176, :189). */
int la_compare(float x, float y, float epsilon) {
    const float min_normal = 1.17549435e-38f; /* std::numeric_limits<float>::min() */
    if (x == y) return 1;
    const float ax = fabsf(x), ay = fabsf(y), diff = fabsf(x - y);
    if (x == 0.0f || y == 0.0f || diff < min_normal) return diff < epsilon * min_normal;
    return diff / (ax + ay) < epsilon;
}

/* the largest |x - y| / (|x| + |y|) / FLT_EPSILON over n pairs (0 for equal pairs), and through *all whether every pair is accepted */
float la_compare_all(const float *expected, const float *actual, long n, float epsilon, int *all) {
    float worst = 0.0f;
    *all = 1;
    for (long i = 0; i < n; i++) {
        if (!la_compare(expected[i], actual[i], epsilon)) *all = 0;
        if (expected[i] != actual[i]) {
            const float r = fabsf(expected[i] - actual[i]) / (fabsf(expected[i]) + fabsf(actual[i])) / 1.1920929e-7f;
            if (r > worst) worst = r;
        }
    }
    return worst;
}
