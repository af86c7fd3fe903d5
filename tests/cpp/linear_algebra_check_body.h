/* linear_algebra_check_body.h — the body of linear_algebra_check.c, written once in terms of
 *   T            the element type
 *   P(name)      the exported name: la_##name for float, ld_##name for double
 *   MAD, MAD2    o_mad / o_mad2 of oracle/oracle_common.h, or their double forms
 *   FMA, FABS    fmaf / fabsf or fma / fabs
 *   V            the generators' natural vector size for T
 *   T_MIN, T_EPSILON   FLT_MIN / FLT_EPSILON or DBL_MIN / DBL_EPSILON, spelled as literals of T
 * and included once per element type.  No include guard: that is the point.  TEST INFRASTRUCTURE ONLY. */

int P(v)(void) { return V; }

/* mode 0: copy, 1: scal, 2: axpy; y is read by axpy only */
void P(axpy)(int mode, T a, const T *x, const T *y, T *result, long n) {
    for (long i = 0; i < n; i++) result[i] = mode == 0 ? x[i] : mode == 1 ? a * x[i] : MAD(a, x[i], y[i]);
}

/* the reductions with the vector width as an argument, so that the tests can ask what another width would give; v <= 64 */
T P(dot_v)(const T *x, const T *y, long n, int v) {
    T lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = MAD(x[k * v + i], y[k * v + i], lanes[i]);
    T s = 0;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    T t = 0;
    for (long e = nvec * v; e < n; e++) t = MAD(x[e], y[e], t);
    return s + t;
}

T P(asum_v)(const T *x, long n, int v) {
    T lanes[64];
    for (int i = 0; i < v; i++) lanes[i] = 0;
    const long nvec = n / v;
    for (long k = 0; k < nvec; k++)
        for (int i = 0; i < v; i++) lanes[i] = lanes[i] + FABS(x[k * v + i]);
    T s = 0;
    for (int i = 0; i < v; i++) s = s + lanes[i];
    T t = 0;
    for (long e = nvec * v; e < n; e++) t = t + FABS(x[e]);
    return s + t;
}

/* A is w x h as stored (A(i, k) = A[k * lda + i]); notrans: x[h], y[w], out[w]; trans: x[w], y[h], out[h], lane width v */
void P(gemv)(int trans, T a, const T *A, long lda, int w, int h, const T *x, T b, const T *y, T *out, int v) {
    if (!trans) {
        for (int i = 0; i < w; i++) {
            T acc = b * y[i];
            for (int k = 0; k < h; k++) acc = MAD(a * A[(long)k * lda + i], x[k], acc);
            out[i] = acc;
        }
        return;
    }
    for (int i = 0; i < h; i++) {
        const T *col = A + (long)i * lda;
        T lanes[64];
        for (int j = 0; j < v; j++) lanes[j] = 0;
        const int nvec = w / v;
        for (int k = 0; k < nvec; k++)
            for (int j = 0; j < v; j++) lanes[j] = MAD(col[k * v + j], x[k * v + j], lanes[j]);
        T s = 0;
        for (int j = 0; j < v; j++) s = s + lanes[j];
        for (int t = nvec * v; t < w; t++) s = MAD(col[t], x[t], s);
        out[i] = MAD2(b, y[i], a, s);
    }
}

/* in place on result[m x n] */
void P(ger)(T a, const T *x, int m, const T *y, int n, T *result, long ldr) {
    for (int j = 0; j < n; j++) {
        const T ay = a * y[j];
        for (int i = 0; i < m; i++) result[(long)j * ldr + i] = MAD(ay, x[i], result[(long)j * ldr + i]);
    }
}

/* result[M x N]; opA(i, k) = ta ? A[i * lda + k] : A[k * lda + i]; opB(k, j) = tb ? B[k * ldb + j] : B[j * ldb + k].  The loops run
 * j, k, i so that a compiler may do several i at once; every output still sees its own k = 0, 1, 2, ... in that order. */
void P(gemm)(int ta, int tb, T a, const T *A, long lda, const T *B, long ldb, T b, const T *C, long ldc, T *result, long ldr, int M, int N, int K,
             T *scratch /* M elements */) {
    const int fused = o_canon_fma;
    T *turned = NULL; /* opA with i contiguous: a copy of the values, so that the inner loop reads memory in order */
    if (ta && M > 0 && K > 0) {
        turned = (T *)malloc(sizeof(T) * (size_t)M * (size_t)K);
        for (int i = 0; i < M; i++)
            for (int k = 0; k < K; k++) turned[(size_t)k * M + i] = A[(long)i * lda + k];
    }
    for (int j = 0; j < N; j++) {
        for (int i = 0; i < M; i++) scratch[i] = 0;
        for (int k = 0; k < K; k++) {
            const T bv = tb ? B[(long)k * ldb + j] : B[(long)j * ldb + k];
            const T *col = ta ? turned + (size_t)k * M : A + (long)k * lda;
            if (fused) for (int i = 0; i < M; i++) scratch[i] = FMA(col[i], bv, scratch[i]);
            else for (int i = 0; i < M; i++) scratch[i] = col[i] * bv + scratch[i];
        }
        for (int i = 0; i < M; i++) result[(long)j * ldr + i] = MAD2(a, scratch[i], b, C[(long)j * ldc + i]);
    }
    free(turned);
}

/* compareScalars of the reference's tests, instantiated for T as BLASFloatTests / BLASDoubleTests do: x the expected value, y the actual one.
 *   x == y: accepted;  x or y zero, or |x - y| below T_MIN: accepted if |x - y| < epsilon * T_MIN;  else |x - y| / (|x| + |y|) < epsilon
 * every operation in T.  The callers pass 16 T_EPSILON for vectors and matrices and 32 T_EPSILON for scalars (:150, :176, :189). */
int P(compare)(T x, T y, T epsilon) {
    const T min_normal = T_MIN; /* std::numeric_limits<T>::min() */
    if (x == y) return 1;
    const T ax = FABS(x), ay = FABS(y), diff = FABS(x - y);
    if (x == 0 || y == 0 || diff < min_normal) return diff < epsilon * min_normal;
    return diff / (ax + ay) < epsilon;
}

/* the largest |x - y| / (|x| + |y|) / T_EPSILON over n pairs (0 for equal pairs), and through *all whether every pair is accepted */
T P(compare_all)(const T *expected, const T *actual, long n, T epsilon, int *all) {
    T worst = 0;
    *all = 1;
    for (long i = 0; i < n; i++) {
        if (!P(compare)(expected[i], actual[i], epsilon)) *all = 0;
        if (expected[i] != actual[i]) {
            const T r = FABS(expected[i] - actual[i]) / (FABS(expected[i]) + FABS(actual[i])) / T_EPSILON;
            if (r > worst) worst = r;
        }
    }
    return worst;
}
