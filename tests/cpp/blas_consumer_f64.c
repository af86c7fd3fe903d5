/* blas_consumer_f64.c — a plain C program that uses the f64 half of the library the way a consumer of apps/linear_algebra's
 * halide_blas.h would: it includes hlmi_blas.h and nothing else of ours, calls all nine hblas_d* routines at N = 136 on uniform [0, 1)
 * data and holds each to its own long-double loops with the criterion of the reference's tests (compareScalars in double: 16 epsilon
 * for vectors and matrices, 32 epsilon for scalars).  TEST INFRASTRUCTURE ONLY: tests/test_linear_algebra_f64.py compiles and runs it.
 * Prints one line per routine, returns the number of routines that failed. */
#include "hlmi_blas.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define N 136

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static double uniform(void) { /* a 53-bit fraction in [0, 1) */
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 9007199254740992.0;
}
static void fill(double *p, int n) {
    for (int i = 0; i < n; i++) p[i] = uniform();
}

static int close_enough(double x, double y, double epsilon) {
    if (x == y) return 1;
    const double diff = fabs(x - y);
    if (x == 0.0 || y == 0.0 || diff < DBL_MIN) return diff < epsilon * DBL_MIN;
    return diff / (fabs(x) + fabs(y)) < epsilon;
}

static int fails = 0;
static void report(const char *name, const long double *expected, const double *actual, int n, double epsilon) {
    int bad = 0;
    for (int i = 0; i < n; i++) bad += !close_enough((double)expected[i], actual[i], epsilon);
    printf("%-14s %s\n", name, bad ? "FAIL" : "ok");
    fails += bad != 0;
}

static double x[N], y[N], A[N * N], B[N * N], Cm[N * N], work[N * N];
static long double want[N * N];

/* C = alpha op(A) op(B) + beta C in long double, column-major */
static void gemm_want(int ta, int tb, double alpha, double beta) {
    for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) {
            long double s = 0;
            for (int k = 0; k < N; k++) s += (long double)(ta ? A[i * N + k] : A[k * N + i]) * (long double)(tb ? B[k * N + j] : B[j * N + k]);
            want[j * N + i] = (long double)alpha * s + (long double)beta * (long double)Cm[j * N + i];
        }
}

int main(void) {
    const double vec_eps = 16 * DBL_EPSILON, scalar_eps = 32 * DBL_EPSILON;
    const double alpha = uniform(), beta = uniform();
    fill(x, N), fill(y, N), fill(A, N * N), fill(B, N * N), fill(Cm, N * N);

    for (int i = 0; i < N; i++) work[i] = -1.0, want[i] = x[i];
    hblas_dcopy(N, x, 1, work, 1);
    report("hblas_dcopy", want, work, N, vec_eps);

    for (int i = 0; i < N; i++) work[i] = x[i], want[i] = (long double)alpha * x[i];
    hblas_dscal(N, alpha, work, 1);
    report("hblas_dscal", want, work, N, vec_eps);

    for (int i = 0; i < N; i++) work[i] = y[i], want[i] = (long double)alpha * x[i] + y[i];
    hblas_daxpy(N, alpha, x, 1, work, 1);
    report("hblas_daxpy", want, work, N, vec_eps);

    long double dot = 0, asum = 0, nrm = 0;
    for (int i = 0; i < N; i++) dot += (long double)x[i] * y[i], asum += fabsl((long double)x[i]), nrm += (long double)x[i] * x[i];
    nrm = sqrtl(nrm);
    double got = hblas_ddot(N, x, 1, y, 1);
    report("hblas_ddot", &dot, &got, 1, scalar_eps);
    got = hblas_dasum(N, x, 1);
    report("hblas_dasum", &asum, &got, 1, scalar_eps);
    got = hblas_dnrm2(N, x, 1);
    report("hblas_dnrm2", &nrm, &got, 1, scalar_eps);

    for (int t = 0; t < 2; t++) {
        for (int i = 0; i < N; i++) {
            long double s = 0;
            for (int k = 0; k < N; k++) s += (long double)(t ? A[i * N + k] : A[k * N + i]) * x[k];
            want[i] = (long double)alpha * s + (long double)beta * y[i];
            work[i] = y[i];
        }
        hblas_dgemv(HblasColMajor, t ? HblasTrans : HblasNoTrans, N, N, alpha, A, N, x, 1, beta, work, 1);
        report(t ? "hblas_dgemv T" : "hblas_dgemv N", want, work, N, vec_eps);
    }

    for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) work[j * N + i] = A[j * N + i], want[j * N + i] = (long double)A[j * N + i] + (long double)alpha * x[i] * y[j];
    hblas_dger(HblasColMajor, N, N, alpha, x, 1, y, 1, work, N);
    report("hblas_dger", want, work, N * N, vec_eps);

    for (int v = 0; v < 4; v++) {
        static const char *const names[4] = {"hblas_dgemm NN", "hblas_dgemm TN", "hblas_dgemm NT", "hblas_dgemm TT"};
        const int ta = v & 1, tb = v >> 1;
        gemm_want(ta, tb, alpha, beta);
        for (int i = 0; i < N * N; i++) work[i] = Cm[i];
        hblas_dgemm(HblasColMajor, ta ? HblasTrans : HblasNoTrans, tb ? HblasTrans : HblasNoTrans, N, N, N, alpha, A, N, B, N, beta, work, N);
        report(names[v], want, work, N * N, vec_eps);
    }
    return fails;
}
