/* linear_algebra_f64_check.c — plain-C checker of the twelve f64 pipelines of apps/linear_algebra: TEST INFRASTRUCTURE ONLY.
 *
 * The contract, derived from the generators (apps/linear_algebra/src/) instantiated at T = double — the `d*` registrations at the end
 * of each file (blas_l1_generators.cpp:182-186, blas_l2_generators.cpp:248-250, blas_l3_generators.cpp:178) and the twelve halide_d*
 * targets of src/CMakeLists.txt:
 *   - Every Input<Buffer<T>> and the output is a buffer of float64, every Input<T> (a_, b_) a float64 scalar.  Dimension 0 is innermost:
 *     no generator touches stride.0, so Halide's default stride.0 == 1 holds, in ELEMENTS: 8 bytes.  Every generator pins min to 0.
 *     Matrices are column-major: A(i, k) is A[k * lda + i].
 *   - Every RDom below is traversed from its min upward, and an update definition `f += e` over it is a sequential chain per pure
 *     index: every reduction runs its index strictly upward.
 *   - vec_size = natural_vector_size(type_of<T>()) (l1 :47 :98 :151, l2 :38 :224).  On the x86-64 AVX2 target whose numbers SURVEY.md
 *     and BASELINE.md take, a vector register is 32 bytes: 32 / sizeof(double) = 4 (LD_V below; 8 for float).  GEMM's
 *     vec = max(4, natural_vector_size) (:41) only shapes the schedule's tiles, never a single output's order of k.
 *   - Float forms: those of oracle/oracle_common.h in double, defined here (d_mad, d_mad2) and reading the same switch o_canon_fma:
 *     d_mad(a, b, c) = fma(a, b, c) or a * b + c; d_mad2(a, b, c, d) = fma(a, b, c * d) or a * b + c * d, the first product the one
 *     contracted.  `*` alone is a rounded multiply.
 *   AXPYGenerator (l1 :34-42): calc = a * x(i) + y(i) | a * x(i) | x(i) by (scale_x, add_to_y); the vectorised body (RDom vecs) and the
 *     tail evaluate the same expression per element.  dcopy/dscal never reference y.
 *   DotGenerator (l1 :104-116): dot(i) += x(k * 4 + i) * y(k * 4 + i) over k in [0, n / 4) from the pure definition's 0: four lane
 *     chains; result() = sum(dot(lanes)): an inline reduction from 0 over lanes 0 .. 3 in order; result() += sum(x(tail) * y(tail)): a
 *     second inline reduction from 0 over the tail upward, added to the first.  AbsSumGenerator (:157-169): the same with abs(x), adds
 *     only, so one result in both forms.
 *   GEMVGenerator, trans (l2 :45-70): prod(j, i) = A(j, i) * x(j); accum_vecs(j, i) += prod(k * 4 + j, i) over k < M / 4;
 *     sum_lanes(i) += accum_vecs_transpose(i, lanes) from 0 in lane order; sum_tail(i) = sum_lanes(i), += prod(tail, i): the tail goes on
 *     top of the lane sum; result(i) = b * y(i) + a * Ax(i): d_mad2(b, y, a, s).
 *   GEMVGenerator, notrans (l2 :125-136): block(i) = b * y(i); block(i) += a * A(i, k) * x(k) over two RDoms that together run
 *     0 .. N - 1 upward.  `a * A * x` parses as (a * A) * x: the rounded a * A comes first and the outer product is the one contracted.
 *   GERGenerator (l2 :227-229): result(i, j) += (a * y(j)) * x(i) on the undefined (in-place) output.
 *   GEMMGenerator (l3 :37-96): prod(k, i, j) = A(i, k) * B(k, j); AB(i, j) += prod(rv, i, j), rv = 0 .. sum_size - 1 upward from 0;
 *     result(i, j) = a * ABt(i, j) + b * C(i, j): d_mad2(a, ab, b, C), and b * C is evaluated whatever b is.
 *     Shapes (:37-39, :167-171): num_rows = A_.width(), num_cols = B_.height(), sum_size = A_.height() come from the STORED matrices
 *     whatever the flags; B_.extent.0 is pinned to sum_size; C_ and result are num_rows x num_cols.  notrans is fully rectangular;
 *     transA reads A_(k, i), i < A_.width(), k < A_.height(): inside A_ only where A_ is square; transB reads B_(j, k), j < B_.height(),
 *     k < B_.width(): B_ square; transAB both.  The checker takes the four as (ta, tb) and leaves the squareness rule to its callers.
 *
 * compareScalars (apps/linear_algebra/tests/test_halide_blas.cpp:150-173) is restated for double, as BLASDoubleTests instantiates it,
 * as ld_compare. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

extern int o_canon_fma; /* check_canon.c: the form oracle/oracle_common.h's float helpers read too */

static inline double d_mad(double a, double b, double c) { return o_canon_fma ? fma(a, b, c) : a * b + c; }
static inline double d_mad2(double a, double b, double c, double d) { return o_canon_fma ? fma(a, b, c * d) : a * b + c * d; }

enum { LD_V = 4 };

int ld_v(void) { return LD_V; }

/* mode 0: copy, 1: scal, 2: axpy; y is read by axpy only */
void ld_axpy(int mode, double a, const double *x, const double *y, double *result, long n) {
    for (long i = 0; i < n; i++) result[i] = mode == 0 ? x[i] : mode == 1 ? a * x[i] : d_mad(a, x[i], y[i]);
}

/* the reductions with the vector width as an argument, so that the tests can ask what another width would give; v <= 64 */
double ld_dot_v(const double *x, const double *y, long n, int v) {
    double lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0.0;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = d_mad(x[k * v + i], y[k * v + i], lanes[i]);
    double s = 0.0;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    double t = 0.0;
    for (long e = nvec * v; e < n; e++) t = d_mad(x[e], y[e], t);
    return s + t;
}

double ld_asum_v(const double *x, long n, int v) {
    double lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0.0;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = lanes[i] + fabs(x[k * v + i]);
    double s = 0.0;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    double t = 0.0;
    for (long e = nvec * v; e < n; e++) t = t + fabs(x[e]);
    return s + t;
}

/* A is w x h as stored (A(i, k) = A[k * lda + i]); notrans: x[h], y[w], out[w]; trans: x[w], y[h], out[h], lane width v */
void ld_gemv(int trans, double a, const double *A, long lda, int w, int h, const double *x, double b, const double *y, double *out, int v) {
    if (!trans) {
        for (int i = 0; i < w; i++) {
            double acc = b * y[i];
            for (int k = 0; k < h; k++) acc = d_mad(a * A[(long)k * lda + i], x[k], acc);
            out[i] = acc;
        }
        return;
    }
    for (int i = 0; i < h; i++) {
        const double *col = A + (long)i * lda;
        double lanes[64];
        for (int j = 0; j < v; j++) lanes[j] = 0.0;
        const int nvec = w / v;
        for (int k = 0; k < nvec; k++)
            for (int j = 0; j < v; j++) lanes[j] = d_mad(col[k * v + j], x[k * v + j], lanes[j]);
        double s = 0.0;
        for (int j = 0; j < v; j++) s = s + lanes[j];
        for (int t = nvec * v; t < w; t++) s = d_mad(col[t], x[t], s);
        out[i] = d_mad2(b, y[i], a, s);
    }
}

/* in place on result[m x n] */
void ld_ger(double a, const double *x, int m, const double *y, int n, double *result, long ldr) {
    for (int j = 0; j < n; j++) {
        const double ay = a * y[j];
        for (int i = 0; i < m; i++) result[(long)j * ldr + i] = d_mad(ay, x[i], result[(long)j * ldr + i]);
    }
}

/* result[M x N]; opA(i, k) = ta ? A[i * lda + k] : A[k * lda + i]; opB(k, j) = tb ? B[k * ldb + j] : B[j * ldb + k].  The loops run
 * j, k, i so that a compiler may do several i at once; every output still sees its own k = 0, 1, 2, ... in that order. */
void ld_gemm(int ta, int tb, double a, const double *A, long lda, const double *B, long ldb, double b, const double *C, long ldc, double *result,
             long ldr, int M, int N, int K, double *scratch /* M doubles */) {
    const int fused = o_canon_fma;
    double *turned = NULL; /* opA with i contiguous: a copy of the values, so that the inner loop reads memory in order */
    if (ta && M > 0 && K > 0) {
        turned = (double *)malloc(sizeof(double) * (size_t)M * (size_t)K);
        for (int i = 0; i < M; i++)
            for (int k = 0; k < K; k++) turned[(size_t)k * M + i] = A[(long)i * lda + k];
    }
    for (int j = 0; j < N; j++) {
        for (int i = 0; i < M; i++) scratch[i] = 0.0;
        for (int k = 0; k < K; k++) {
            const double bv = tb ? B[(long)k * ldb + j] : B[(long)j * ldb + k];
            const double *col = ta ? turned + (size_t)k * M : A + (long)k * lda;
            if (fused) for (int i = 0; i < M; i++) scratch[i] = fma(col[i], bv, scratch[i]);
            else for (int i = 0; i < M; i++) scratch[i] = col[i] * bv + scratch[i];
        }
        for (int i = 0; i < M; i++) result[(long)j * ldr + i] = d_mad2(a, scratch[i], b, C[(long)j * ldc + i]);
    }
    free(turned);
}

/* compareScalars of the reference's tests, instantiated for double as BLASDoubleTests does: x the expected value, y the actual one.
 *   x == y: accepted;  x or y zero, or |x - y| below DBL_MIN: accepted if |x - y| < epsilon * DBL_MIN;  else |x - y| / (|x| + |y|) < epsilon
 * every operation in double.  The callers pass 16 DBL_EPSILON for vectors and matrices and 32 DBL_EPSILON for scalars (:150, :176, :189). */
int ld_compare(double x, double y, double epsilon) {
    const double min_normal = 2.2250738585072014e-308; /* std::numeric_limits<double>::min() */
    if (x == y) return 1;
    const double ax = fabs(x), ay = fabs(y), diff = fabs(x - y);
    if (x == 0.0 || y == 0.0 || diff < min_normal) return diff < epsilon * min_normal;
    return diff / (ax + ay) < epsilon;
}

/* the largest |x - y| / (|x| + |y|) / DBL_EPSILON over n pairs (0 for equal pairs), and through *all whether every pair is accepted */
double ld_compare_all(const double *expected, const double *actual, long n, double epsilon, int *all) {
    double worst = 0.0;
    *all = 1;
    for (long i = 0; i < n; i++) {
        if (!ld_compare(expected[i], actual[i], epsilon)) *all = 0;
        if (expected[i] != actual[i]) {
            const double r = fabs(expected[i] - actual[i]) / (fabs(expected[i]) + fabs(actual[i])) / 2.220446049250313e-16;
            if (r > worst) worst = r;
        }
    }
    return worst;
}
