/* blas_consumer.c — a plain C program that uses the library the way a consumer of apps/linear_algebra's halide_blas.h would: it
 * includes hlmi_blas.h and nothing else of ours, calls all nine hblas_s* routines at N = 136 on uniform [0, 1) data and holds each to
 * its own double-precision loops with the criterion of the reference's tests (compareScalars: 16 epsilon for vectors and matrices,
 * 32 epsilon for scalars).  TEST INFRASTRUCTURE ONLY: tests/test_linear_algebra.py compiles and runs it.  Prints one line per routine,
 * returns the number of routines that failed. */
#include "hlmi_blas.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define N 136

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static float uniform(void) { /* a 24-bit fraction in [0, 1) */
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(state >> 40) / 16777216.0f;
}
static void fill(float *p, int n) {
    for (int i = 0; i < n; i++) p[i] = uniform();
}

static int close_enough(float x, float y, float epsilon) {
    if (x == y) return 1;
    const float diff = fabsf(x - y);
    if (x == 0.0f || y == 0.0f || diff < FLT_MIN) return diff < epsilon * FLT_MIN;
    return diff / (fabsf(x) + fabsf(y)) < epsilon;
}

static int fails = 0;
static void report(const char *name, const double *expected, const float *actual, int n, float epsilon) {
    int bad = 0;
    for (int i = 0; i < n; i++) bad += !close_enough((float)expected[i], actual[i], epsilon);
    printf("%-14s %s\n", name, bad ? "FAIL" : "ok");
    fails += bad != 0;
}

static float x[N], y[N], A[N * N], B[N * N], Cm[N * N], work[N * N];
static double want[N * N];

/* C = alpha op(A) op(B) + beta C in double, column-major */
static void gemm_want(int ta, int tb, float alpha, float beta) {
    for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) {
            double s = 0;
            for (int k = 0; k < N; k++) s += (double)(ta ? A[i * N + k] : A[k * N + i]) * (double)(tb ? B[k * N + j] : B[j * N + k]);
            want[j * N + i] = (double)alpha * s + (double)beta * (double)Cm[j * N + i];
        }
}

int main(void) {
    const float vec_eps = 16 * FLT_EPSILON, scalar_eps = 32 * FLT_EPSILON;
    const float alpha = uniform(), beta = uniform();
    fill(x, N), fill(y, N), fill(A, N * N), fill(B, N * N), fill(Cm, N * N);

    for (int i = 0; i < N; i++) work[i] = -1.0f, want[i] = x[i];
    hblas_scopy(N, x, 1, work, 1);
    report("hblas_scopy", want, work, N, vec_eps);

    for (int i = 0; i < N; i++) work[i] = x[i], want[i] = (double)alpha * x[i];
    hblas_sscal(N, alpha, work, 1);
    report("hblas_sscal", want, work, N, vec_eps);

    for (int i = 0; i < N; i++) work[i] = y[i], want[i] = (double)alpha * x[i] + y[i];
    hblas_saxpy(N, alpha, x, 1, work, 1);
    report("hblas_saxpy", want, work, N, vec_eps);

    double dot = 0, asum = 0, nrm = 0;
    for (int i = 0; i < N; i++) dot += (double)x[i] * y[i], asum += fabs((double)x[i]), nrm += (double)x[i] * x[i];
    nrm = sqrt(nrm);
    float got = hblas_sdot(N, x, 1, y, 1);
    report("hblas_sdot", &dot, &got, 1, scalar_eps);
    got = hblas_sasum(N, x, 1);
    report("hblas_sasum", &asum, &got, 1, scalar_eps);
    got = hblas_snrm2(N, x, 1);
    report("hblas_snrm2", &nrm, &got, 1, scalar_eps);

    for (int t = 0; t < 2; t++) {
        for (int i = 0; i < N; i++) {
            double s = 0;
            for (int k = 0; k < N; k++) s += (double)(t ? A[i * N + k] : A[k * N + i]) * x[k];
            want[i] = (double)alpha * s + (double)beta * y[i];
            work[i] = y[i];
        }
        hblas_sgemv(HblasColMajor, t ? HblasTrans : HblasNoTrans, N, N, alpha, A, N, x, 1, beta, work, 1);
        report(t ? "hblas_sgemv T" : "hblas_sgemv N", want, work, N, vec_eps);
    }

    for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) work[j * N + i] = A[j * N + i], want[j * N + i] = (double)A[j * N + i] + (double)alpha * x[i] * y[j];
    hblas_sger(HblasColMajor, N, N, alpha, x, 1, y, 1, work, N);
    report("hblas_sger", want, work, N * N, vec_eps);

    for (int v = 0; v < 4; v++) {
        static const char *const names[4] = {"hblas_sgemm NN", "hblas_sgemm TN", "hblas_sgemm NT", "hblas_sgemm TT"};
        const int ta = v & 1, tb = v >> 1;
        gemm_want(ta, tb, alpha, beta);
        for (int i = 0; i < N * N; i++) work[i] = Cm[i];
        hblas_sgemm(HblasColMajor, ta ? HblasTrans : HblasNoTrans, tb ? HblasTrans : HblasNoTrans, N, N, N, alpha, A, N, B, N, beta, work, N);
        report(names[v], want, work, N * N, vec_eps);
    }
    return fails;
}
