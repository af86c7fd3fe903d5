/* fft_check.c — the checker of the four 2-D f32 transforms of apps/fft (c2c forward, c2c inverse, r2c, c2r): the arithmetic of
 * fft.cpp, complex.h and fft_generator.cpp restated in plain C, one rounding per operator (no contraction by the compiler), the fused
 * operations written out.  tests/fft_checker.py declares the object: tests/checker_lib.py links this file with check_canon.c into a shared object of
 * its own, and fft_checker.py drives it through ctypes.  The derivation, line by line:
 *
 * complex.h:77-104.  (a + b), (a - b) work per component.  a * b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re): a difference and a
 *   sum of two products.  In form 1 (oracle/oracle_common.h) the first product of each is the one fused: re = mulsub(a.re, b.re,
 *   a.im * b.im), im = mad2(a.re, b.im, a.im, b.re); in form 0 every operator rounds once.  This is `cmul` below and the ONLY place a
 *   multiply feeds an add: every other multiplication (by a real gain, by 0.5f) feeds nothing, and an add whose operand is a cmul
 *   result adds the finished component.  z * real = (re * real, im * real).
 * fft.cpp:295-421, fft_dim1.  A 1-D transform of N = prod R_i points is the sequence of passes i = 0 .. with S = 1, R_0, R_0 R_1, ...
 *   Pass i, for s = 0 .. N/R - 1: v[r] = x[s + r (N/R)], r = 0 .. R - 1 (:335).  For S > 1 (:336-342) v[r] = cmul(v[r], W[r (s mod S)])
 *   for r > 0 and v[0] = v[0] * g, where W is the table of (R S, sign, g) and g is the requested gain in the FIRST pass with S > 1 and
 *   1 in every later one (:342).  V = dftR(v) (:352).  In the last pass (S == N/R) V[r] = V[r] * g (:364-369), g being the requested gain
 *   if no earlier pass took it (a one-pass transform) and 1 otherwise.  y[(s / S) R S + s mod S + r S] = V[r] (:370).
 *   A gain that is the constant 1.0f is simplified away by the reference (x * 1.0f -> x): where g == 1.0f no multiplication is made
 *   and W is the bare (cos, sin).
 * fft.cpp:109-229, the codelets, temporaries and literals as written.  `* j` (complex.h:95 with the integer pair (0, 1), products by
 *   0 and 1 simplified away) is a swap with one negation, (re, im) -> (-im, re); `* sign` is a negation of both components for
 *   sign = -1 and nothing for +1; so `* j * sign` is (-im, re) for +1 and (im, -re) for -1 — the reference compiles with nsz and
 *   defines no more than that.  dft6's W1_3 = (-0.5f, sign * 0.866025404f), W2_3 = (-0.5f, -(sign * 0.866025404f)), W4_3 = W1_3, its
 *   outputs ((T0 + cmul(T2, Wa)) + cmul(T1, Wb)) and ((T3 + cmul(T5, Wa)) - cmul(T4, Wb)), X0 = (T0 + T2) + T1, X3 = (T3 + T5) - T4.
 *   dft8's mul(z, c, d) is cmul(z, (c, d)) with c = +-0.70710678f, d = sign * 0.70710678f.
 * fft.cpp:274-291, twiddle_factors.  W(n) = expj((sign * 2 * kPi * n) / N) * g: sign * 2 is an integer, times kPi = (float)M_PI is
 *   the exact float +-2 kPi, times (float)n rounds once, and the quotient by (float)N is THE CHOICE made here: a true division,
 *   correctly rounded (the reference's simplifier may or may not turn it into a product by 1/N).  cos and sin are libm's cosf and
 *   sinf of that float, on the host; fc_twiddles() below is that function, and the library exports its own copy
 *   (hlmi_fft_twiddles) which fc_set_twiddle_fn() puts in its place, so that GPU parity involves no transcendental.
 * fft.cpp:1066-1097, radix_factor: five special cases (16 -> {4,4}, 32 -> {8,4}, 64 -> {8,8}, 128 -> {8,4,4}, 256 -> {8,8,4}), else
 *   divide out 8, 6, 4, 2 in that order, each as often as it goes, and append what is left if it is not 1 (or if nothing was found).
 *   A size is allowed when 2 <= N <= 4096 and every factor is 8, 6, 4 or 2 (dftN is out of scope).
 * fft.cpp:481-552, fft2d_c2c: dimension 0 first with gain 1, then dimension 1 with the requested gain.
 * fft.cpp:667-883, fft2d_r2c, V = natural_vector_size = FC_V = 8 (x86-64 AVX2), vector_width = 0.
 *   skip_zip = N0 < 2V || (N0 < 4V && N0 % 2V != 0): c2c of (r, +0) with sign -1, rows 0 .. N1/2 kept.
 *   else zw = gcd(V, N0/2); zipped(u, n1) = (r(zx(u), n1), r(zx(u) + zw, n1)), zx(u) = (u / zw) 2 zw + u % zw; dimension 1 of the N0/2
 *   zipped columns, sign -1, gain 1; unzipped(n0, n1) from Z = dft1(ux(n0), n1), Z' = dft1(ux(n0), (N1 - n1) % N1),
 *   ux(n0) = (n0 / 2zw) zw + n0 % zw: X = (Z.re + Z'.re, Z.im - Z'.im) for n0 % 2zw < zw, else D = (Z.re - Z'.re, Z.im + Z'.im) and
 *   Y = -j D = (D.im, -D.re).  Row 0 is zipped again: (re unzipped(n0, 0), re unzipped(n0, N1/2)).  Dimension 0 of rows 0 .. N1/2 - 1,
 *   sign -1, gain g/2 (g * 0.5f).  Then the six updates on row 0 (D) and the new row N1/2 (Q), in this order, each loop upward:
 *     0  Q[0] = (D[0].im, +0)
 *     1  Q[n] = (0.5f E.im, -(0.5f E.re)), E = (D[n].re - D[N0-n].re, D[n].im + D[N0-n].im),  n = 1 .. N0/2
 *     2  Q[n] = conj(Q[N0-n]),  n = N0/2 .. N0 - 1   (n = N0/2 conjugates itself)
 *     3  D[0] = (D[0].re, +0)
 *     4  D[n] = (0.5f (D[n].re + D[N0-n].re), 0.5f (D[n].im - D[N0-n].im)),  n = 1 .. N0/2
 *     5  D[n] = conj(D[N0-n]),  n = N0/2 .. N0 - 1
 *   conj negates the imaginary part (so +0 becomes -0).
 * fft.cpp:886-1061, fft2d_c2r.  skip_zip = N0 < 2V: c2c with sign +1 of c_extended(n0, n1) = c(n0, n1) for n1 <= N1/2, else
 *   conj(c((N0 - n0) % N0, (N1 - n1) % N1)); the real part is kept.
 *   else row 0 is c(n0, 0) + j c(n0, N1/2) = (X.re - Y.im, X.im + Y.re); dimension 0 of rows 0 .. N1/2 - 1, sign +1, gain 1 (dft0);
 *   U(n0, m) = (dft0(n0, 0).re, +0) for m <= 0, (dft0(n0, 0).im, +0) for m >= N1/2, else dft0(n0, m); zw = gcd(gcd(V, N1/2), N0/2)
 *   (the N1 is the reference's); zipped(u, n1) = X + j Y = (X.re - Y.im, X.im + Y.re) with X = U(zx(u), n1) for n1 < N1/2 else
 *   conj(U(zx(u), (N1 - n1) % N1)) and Y the same at zx(u) + zw; dimension 1 of the N0/2 columns, sign +1, the requested gain; the
 *   real part goes to column zx(u), the imaginary part to column zx(u) + zw.  Rows above N1/2 of the input are never read.
 * Subnormals are kept; nothing here depends on the input's values. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "oracle_common.h"

#define FC_V 8          /* natural_vector_size of f32 on the reference's x86-64 AVX2 build */
#define FC_MAX_N 4096
#define FC_MAX_STAGES 4

enum { FC_C2C_FWD = 0, FC_C2C_INV = 1, FC_R2C = 2, FC_C2R = 3 };

typedef struct { float re, im; } cpx;

typedef void (*fc_twiddle_fn)(int n, int sign, float gain, float *out);

/* out[2 k], out[2 k + 1] = W(k), k = 0 .. n - 1, the table of (n = R S, sign, gain) */
void fc_twiddles(int n, int sign, float gain, float *out) {
    const float kPi = (float)3.14159265358979310000;
    const float two_pi = (float)(sign * 2) * kPi;
    for (int k = 0; k < n; k++) {
        const float ang = (two_pi * (float)k) / (float)n;
        float c = cosf(ang), s = sinf(ang);
        if (gain != 1.0f) c = c * gain, s = s * gain;
        out[2 * k] = c, out[2 * k + 1] = s;
    }
}
static fc_twiddle_fn fc_table_fn = fc_twiddles;
void fc_set_twiddle_fn(fc_twiddle_fn fn) { fc_table_fn = fn ? fn : fc_twiddles; }

/* radix_factor: the factors into R (room for 16), their number returned */
int fc_radix_factor(int N, int *R) {
    int n = 0;
    switch (N) {
    case 16: R[0] = 4, R[1] = 4; return 2;
    case 32: R[0] = 8, R[1] = 4; return 2;
    case 64: R[0] = 8, R[1] = 8; return 2;
    case 128: R[0] = 8, R[1] = 4, R[2] = 4; return 3;
    case 256: R[0] = 8, R[1] = 8, R[2] = 4; return 3;
    }
    static const int radices[4] = {8, 6, 4, 2};
    for (int i = 0; i < 4; i++)
        while (N > 0 && N % radices[i] == 0 && n < 15) R[n++] = radices[i], N /= radices[i];
    if (N != 1 || n == 0) R[n++] = N;
    return n;
}

int fc_size_ok(int N) {
    int R[16];
    if (N < 2 || N > FC_MAX_N) return 0;
    const int n = fc_radix_factor(N, R);
    for (int i = 0; i < n; i++)
        if (R[i] != 8 && R[i] != 6 && R[i] != 4 && R[i] != 2) return 0;
    return n <= FC_MAX_STAGES;
}

static int fc_gcd(int x, int y) {
    while (y) { const int r = x % y; x = y, y = r; }
    return x;
}

/* ------------------------------------------------------------------------------------------------------------ complex arithmetic */
static cpx c_add(cpx a, cpx b) { const cpx r = {a.re + b.re, a.im + b.im}; return r; }
static cpx c_sub(cpx a, cpx b) { const cpx r = {a.re - b.re, a.im - b.im}; return r; }
static cpx c_mul(cpx a, cpx b) { const cpx r = {o_mulsub(a.re, b.re, a.im * b.im), o_mad2(a.re, b.im, a.im, b.re)}; return r; }
static cpx c_scale(cpx a, float g) { const cpx r = {a.re * g, a.im * g}; return g == 1.0f ? a : r; }
static cpx c_conj(cpx a) { const cpx r = {a.re, -a.im}; return r; }
static cpx c_jsign(cpx a, int sign) {   /* a * j * sign */
    const cpx p = {-a.im, a.re}, m = {a.im, -a.re};
    return sign > 0 ? p : m;
}
static cpx c_zipj(cpx x, cpx y) { const cpx r = {x.re - y.im, x.im + y.re}; return r; }   /* x + j y */

static void fc_dft2(cpx *x) {
    const cpx a = c_add(x[0], x[1]), b = c_sub(x[0], x[1]);
    x[0] = a, x[1] = b;
}

static void fc_dft4(cpx *x, int sign) {
    const cpx t0 = c_add(x[0], x[2]), t2 = c_add(x[1], x[3]);
    const cpx t1 = c_sub(x[0], x[2]), t3 = c_jsign(c_sub(x[1], x[3]), sign);
    x[0] = c_add(t0, t2), x[2] = c_sub(t0, t2), x[1] = c_add(t1, t3), x[3] = c_sub(t1, t3);
}

static void fc_dft6(cpx *x, int sign) {
    const float wi = (float)sign * 0.866025404f;
    const cpx W1 = {-0.5f, wi}, W2 = {-0.5f, -wi};
    const cpx t0 = c_add(x[0], x[3]), t3 = c_sub(x[0], x[3]), t1 = c_add(x[1], x[4]), t4 = c_sub(x[1], x[4]);
    const cpx t2 = c_add(x[2], x[5]), t5 = c_sub(x[2], x[5]);
    x[0] = c_add(c_add(t0, t2), t1);
    x[4] = c_add(c_add(t0, c_mul(t2, W1)), c_mul(t1, W2));
    x[2] = c_add(c_add(t0, c_mul(t2, W2)), c_mul(t1, W1));
    x[3] = c_sub(c_add(t3, t5), t4);
    x[1] = c_sub(c_add(t3, c_mul(t5, W1)), c_mul(t4, W2));
    x[5] = c_sub(c_add(t3, c_mul(t5, W2)), c_mul(t4, W1));
}

static void fc_dft8(cpx *x, int sign) {
    const float q = 0.70710678f;
    const cpx Wa = {q, (float)sign * q}, Wb = {-q, (float)sign * q};
    cpx X[8], T[8];
    X[0] = c_add(x[0], x[4]), X[2] = c_add(x[2], x[6]);
    T[0] = c_add(X[0], X[2]), T[2] = c_sub(X[0], X[2]);
    X[1] = c_sub(x[0], x[4]), X[3] = c_jsign(c_sub(x[2], x[6]), sign);
    T[1] = c_add(X[1], X[3]), T[3] = c_sub(X[1], X[3]);
    X[4] = c_add(x[1], x[5]), X[6] = c_add(x[3], x[7]);
    T[4] = c_add(X[4], X[6]), T[6] = c_jsign(c_sub(X[4], X[6]), sign);
    X[5] = c_sub(x[1], x[5]), X[7] = c_jsign(c_sub(x[3], x[7]), sign);
    T[5] = c_mul(c_add(X[5], X[7]), Wa), T[7] = c_mul(c_sub(X[5], X[7]), Wb);
    for (int i = 0; i < 4; i++) x[i] = c_add(T[i], T[i + 4]), x[i + 4] = c_sub(T[i], T[i + 4]);
}

/* ------------------------------------------------------------------------------------------------------------------- one 1-D plan */
typedef struct {
    int N, sign, n;
    int R[FC_MAX_STAGES];
    float g_in[FC_MAX_STAGES];    /* pass i, S > 1: the table's gain and the factor of the r = 0 point */
    float g_out[FC_MAX_STAGES];   /* pass i: the factor of its results (the requested gain in a one-pass transform) */
    float *W[FC_MAX_STAGES];      /* the table of (R S, sign, g_in), or null for S = 1 */
} fc_plan;

static int fc_plan_make(fc_plan *p, int N, int sign, float gain) {
    int R[16];
    memset(p, 0, sizeof *p);
    p->N = N, p->sign = sign, p->n = fc_radix_factor(N, R);
    if (p->n > FC_MAX_STAGES) return -1;
    int S = 1;
    for (int i = 0; i < p->n; i++) {
        p->R[i] = R[i];
        p->g_in[i] = i == 1 ? gain : 1.0f;
        p->g_out[i] = p->n == 1 ? gain : 1.0f;
        if (S > 1) {
            p->W[i] = (float *)malloc(sizeof(float) * 2 * (size_t)R[i] * S);
            fc_table_fn(R[i] * S, sign, p->g_in[i], p->W[i]);
        }
        S *= R[i];
    }
    return 0;
}

static void fc_plan_free(fc_plan *p) {
    for (int i = 0; i < FC_MAX_STAGES; i++) free(p->W[i]);
}

/* the passes over one line held in a[0 .. N); tmp has room for N */
static void fc_line(const fc_plan *p, cpx *a, cpx *tmp) {
    const int N = p->N;
    int S = 1;
    for (int i = 0; i < p->n; i++) {
        const int R = p->R[i], M = N / R;
        for (int s = 0; s < M; s++) {
            cpx v[8];
            for (int r = 0; r < R; r++) {
                v[r] = a[s + r * M];
                if (S > 1) {
                    if (r > 0) {
                        const float *w = p->W[i] + 2 * (size_t)(r * (s % S));
                        const cpx W = {w[0], w[1]};
                        v[r] = c_mul(v[r], W);
                    } else {
                        v[r] = c_scale(v[r], p->g_in[i]);
                    }
                }
            }
            switch (R) {
            case 2: fc_dft2(v); break;
            case 4: fc_dft4(v, p->sign); break;
            case 6: fc_dft6(v, p->sign); break;
            default: fc_dft8(v, p->sign); break;
            }
            for (int r = 0; r < R; r++) tmp[(s / S) * R * S + s % S + r * S] = c_scale(v[r], p->g_out[i]);
        }
        memcpy(a, tmp, sizeof(cpx) * (size_t)N);
        S *= R;
    }
}

/* ------------------------------------------------------------------------------------------------------------------ the transforms */
static int fc_skip_r2c(int N0, int V) { return N0 < 2 * V || (N0 < 4 * V && N0 % (2 * V) != 0); }
static int fc_skip_c2r(int N0, int V) { return N0 < 2 * V; }
int fc_zip_width(int kind, int N0, int N1, int V) {   /* 0: skip_zip */
    if (kind == FC_R2C) return fc_skip_r2c(N0, V) ? 0 : fc_gcd(V, N0 / 2);
    if (kind == FC_C2R) return fc_skip_c2r(N0, V) ? 0 : fc_gcd(fc_gcd(V, N1 / 2), N0 / 2);
    return 0;
}
static int fc_zx(int u, int zw) { return (u / zw) * zw * 2 + u % zw; }
static int fc_ux(int n0, int zw) { return (n0 / (2 * zw)) * zw + n0 % zw; }

/* in / out: rows `irs` / `ors` floats apart, a complex element two adjacent floats, a real one one float.  V: the vector width
 * (FC_V is the contract; the tests pass others to show that their inputs tell them apart).  0, or -1 for a size out of scope. */
int fc_fft2d(int kind, int N0, int N1, float gain, int V, const float *in, long irs, float *out, long ors) {
    if (!fc_size_ok(N0) || !fc_size_ok(N1)) return -1;
    if ((kind == FC_R2C || kind == FC_C2R) && ((N0 | N1) & 1)) return -1;
    if (kind < 0 || kind > 3) return -1;
    const int sign = (kind == FC_C2C_INV || kind == FC_C2R) ? 1 : -1;
    const int zw = fc_zip_width(kind, N0, N1, V), H0 = N0 / 2, H1 = N1 / 2;
    const int maxn = N0 > N1 ? N0 : N1;
    cpx *scr = (cpx *)malloc(sizeof(cpx) * (size_t)N0 * N1), *line = (cpx *)malloc(sizeof(cpx) * maxn), *tmp = (cpx *)malloc(sizeof(cpx) * maxn);
    fc_plan pa, pb;
#define IN_C(n0, n1) (*(const cpx *)(in + (size_t)(n1) * irs + 2 * (size_t)(n0)))
#define IN_R(n0, n1) (in[(size_t)(n1) * irs + (n0)])
#define OUT_C(n0, n1) (*(cpx *)(out + (size_t)(n1) * ors + 2 * (size_t)(n0)))
#define OUT_R(n0, n1) (out[(size_t)(n1) * ors + (n0)])
    if (zw == 0) {
        /* c2c, or r2c / c2r through c2c: dimension 0 with gain 1 into scr[n1][n0], then dimension 1 with the gain */
        fc_plan_make(&pa, N0, sign, 1.0f), fc_plan_make(&pb, N1, sign, gain);
        for (int n1 = 0; n1 < N1; n1++) {
            for (int n0 = 0; n0 < N0; n0++) {
                cpx v;
                if (kind == FC_R2C) v.re = IN_R(n0, n1), v.im = 0.0f;
                else if (kind == FC_C2R && n1 > H1) v = c_conj(IN_C((N0 - n0) % N0, (N1 - n1) % N1));
                else v = IN_C(n0, n1);
                line[n0] = v;
            }
            fc_line(&pa, line, tmp);
            memcpy(scr + (size_t)n1 * N0, line, sizeof(cpx) * N0);
        }
        for (int n0 = 0; n0 < N0; n0++) {
            for (int n1 = 0; n1 < N1; n1++) line[n1] = scr[(size_t)n1 * N0 + n0];
            fc_line(&pb, line, tmp);
            for (int n1 = 0; n1 < N1; n1++) {
                if (kind == FC_C2R) OUT_R(n0, n1) = line[n1].re;
                else if (kind != FC_R2C || n1 <= H1) OUT_C(n0, n1) = line[n1];
            }
        }
    } else if (kind == FC_R2C) {
        fc_plan_make(&pa, N1, -1, 1.0f), fc_plan_make(&pb, N0, -1, gain * 0.5f);
        for (int u = 0; u < H0; u++) {   /* scr[n1][u] = dft1 */
            for (int n1 = 0; n1 < N1; n1++) line[n1].re = IN_R(fc_zx(u, zw), n1), line[n1].im = IN_R(fc_zx(u, zw) + zw, n1);
            fc_line(&pa, line, tmp);
            for (int n1 = 0; n1 < N1; n1++) scr[(size_t)n1 * H0 + u] = line[n1];
        }
        cpx *Q = (cpx *)malloc(sizeof(cpx) * N0);
        for (int n1 = 0; n1 < H1; n1++) {
            for (int n0 = 0; n0 < N0; n0++) {
                const int u = fc_ux(n0, zw), isy = n0 % (2 * zw) >= zw;
                cpx un[2];
                for (int k = 0; k < 2; k++) {   /* unzipped(n0, n1) and, for row 0, unzipped(n0, N1/2) */
                    const int m = k ? H1 : n1;
                    const cpx Z = scr[(size_t)m * H0 + u], Zs = scr[(size_t)((N1 - m) % N1) * H0 + u];
                    const cpx X = {Z.re + Zs.re, Z.im - Zs.im}, D = {Z.re - Zs.re, Z.im + Zs.im}, Y = {D.im, -D.re};
                    un[k] = isy ? Y : X;
                }
                if (n1 > 0) line[n0] = un[0];
                else line[n0].re = un[0].re, line[n0].im = un[1].re;
            }
            fc_line(&pb, line, tmp);
            if (n1 > 0) {
                for (int n0 = 0; n0 < N0; n0++) OUT_C(n0, n1) = line[n0];
                continue;
            }
            cpx *D = line;
            Q[0].re = D[0].im, Q[0].im = 0.0f;
            for (int n = 1; n <= H0; n++) {
                const cpx E = {D[n].re - D[N0 - n].re, D[n].im + D[N0 - n].im};
                Q[n].re = 0.5f * E.im, Q[n].im = -(0.5f * E.re);
            }
            for (int n = H0; n < N0; n++) Q[n] = c_conj(Q[N0 - n]);
            D[0].im = 0.0f;
            for (int n = 1; n <= H0; n++) {
                const cpx Sm = {D[n].re + D[N0 - n].re, D[n].im - D[N0 - n].im};
                D[n].re = 0.5f * Sm.re, D[n].im = 0.5f * Sm.im;
            }
            for (int n = H0; n < N0; n++) D[n] = c_conj(D[N0 - n]);
            for (int n0 = 0; n0 < N0; n0++) OUT_C(n0, 0) = D[n0], OUT_C(n0, H1) = Q[n0];
        }
        free(Q);
    } else {   /* c2r, zipped */
        fc_plan_make(&pa, N0, 1, 1.0f), fc_plan_make(&pb, N1, 1, gain);
        for (int n1 = 0; n1 < H1; n1++) {   /* scr[n1][n0] = dft0 */
            for (int n0 = 0; n0 < N0; n0++) line[n0] = n1 > 0 ? IN_C(n0, n1) : c_zipj(IN_C(n0, 0), IN_C(n0, H1));
            fc_line(&pa, line, tmp);
            memcpy(scr + (size_t)n1 * N0, line, sizeof(cpx) * N0);
        }
        for (int u = 0; u < H0; u++) {
            const int x0 = fc_zx(u, zw);
            for (int n1 = 0; n1 < N1; n1++) {
                cpx xy[2];
                for (int k = 0; k < 2; k++) {
                    const int n0 = x0 + k * zw, m = n1 < H1 ? n1 : (N1 - n1) % N1;
                    cpx U;
                    if (m <= 0) U.re = scr[n0].re, U.im = 0.0f;
                    else if (m >= H1) U.re = scr[n0].im, U.im = 0.0f;
                    else U = scr[(size_t)m * N0 + n0];
                    xy[k] = n1 < H1 ? U : c_conj(U);
                }
                line[n1] = c_zipj(xy[0], xy[1]);
            }
            fc_line(&pb, line, tmp);
            for (int n1 = 0; n1 < N1; n1++) OUT_R(x0, n1) = line[n1].re, OUT_R(x0 + zw, n1) = line[n1].im;
        }
    }
    fc_plan_free(&pa), fc_plan_free(&pb);
    free(scr), free(line), free(tmp);
    return 0;
}
