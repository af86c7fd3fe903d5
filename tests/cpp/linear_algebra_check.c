/* linear_algebra_check.c — plain-C checker of the twenty-four pipelines of apps/linear_algebra, twelve f32 (la_*) and twelve f64 (ld_*):
 * TEST INFRASTRUCTURE ONLY.  The routines are written once, in linear_algebra_check_body.h, and instantiated below for float and double.
 *
 * The contract, verified line by line against the generators (apps/linear_algebra/src/), which are templates over T: the `s*` and `d*`
 * registrations at the end of each file (blas_l1_generators.cpp:182-186, blas_l2_generators.cpp:248-250, blas_l3_generators.cpp:178) and
 * the halide_s* / halide_d* targets of src/CMakeLists.txt instantiate them at T = float and T = double.
 *   - Every Input<Buffer<T>> and the output is a buffer of T, every Input<T> (a_, b_) a scalar of T.  Dimension 0 is innermost.  No
 *     generator touches stride.0, so Halide's default constraint stride.0 == 1 holds for every buffer, in ELEMENTS: 4 or 8 bytes; every
 *     generator pins min to 0.  Matrices are column-major: A(i, k) is A[k * lda + i].
 *   - Every RDom below is traversed from its min upward, and an update definition `f += e` over it is a sequential chain per pure
 *     index: every reduction runs its index strictly upward.
 *   - V = vec_size = natural_vector_size(type_of<T>()) (l1 :47 :98 :151, l2 :38 :224).  On the x86-64 AVX2 target whose numbers
 *     SURVEY.md and BASELINE.md take, a vector register is 32 bytes: 32 / sizeof(float) = 8, 32 / sizeof(double) = 4 (V below: a choice).
 *     GEMM's vec = max(4, natural_vector_size) (:41) only shapes the schedule's tiles, never a single output's order of k.
 *   - Float forms (oracle/oracle_common.h): MAD(a, b, c) = a * b + c, MAD2(a, b, c, d) = a * b + c * d with the first product
 *     contracted; in form 0 every operator rounds once.  `*` alone is a rounded multiply.  For float they are o_mad and o_mad2; for
 *     double they are defined here (d_mad = fma(a, b, c) or a * b + c, d_mad2 = fma(a, b, c * d) or a * b + c * d) and read the same
 *     switch o_canon_fma.
 *   AXPYGenerator (blas_l1_generators.cpp:34-42): calc = a * x(i) + y(i) | a * x(i) | x(i) by (scale_x, add_to_y); the vectorised
 *     body (RDom vecs) and the tail evaluate the same expression per element.  copy / scal never reference y: the wrappers pass a null
 *     pointer.
 *   DotGenerator (:104-116): dot(i) += x(k V + i) * y(k V + i) over k in [0, n / V), from the pure definition's 0 — V lane chains,
 *     k upward; result() = sum(dot(lanes)) — an inline reduction from 0 over lanes 0 .. V - 1 in order; result() += sum(x(tail) *
 *     y(tail)) — a second inline reduction from 0 over the tail upward, added to the first.  AbsSumGenerator (:157-169): the same
 *     with abs(x) (an add, no multiply: one result in both forms).
 *   GEMVGenerator, notrans (blas_l2_generators.cpp:125-136): block(i) = b * y(i); block(i) += a * A(i, k) * x(k) over k in two
 *     RDoms that together run 0 .. N - 1 upward; `a * A * x` parses as (a * A) * x: the rounded a * A has one use and the outer
 *     product is the one contracted with the add.  The schedule (unroll, vectorize over i, reorder) never changes a single output's
 *     order of k.
 *   GEMVGenerator, trans (:45-70): prod(j, i) = A(j, i) * x(j); accum_vecs(j, i) += prod(k V + j, i) over k < M / V; sum_lanes(i) +=
 *     accum_vecs_transpose(i, lanes) from 0 over lanes in order; sum_tail(i) = sum_lanes(i), += prod(tail, i) upward: the tail goes on
 *     top of the lane sum; result(i) = b * y(i) + a * Ax(i): two products under one add, the first contracted (MAD2(b, y, a, s)).
 *   GERGenerator (:227-229): result(i, j) += (a * y(j)) * x(i) on the undefined (in-place) output.
 *   GEMMGenerator (blas_l3_generators.cpp:37-96): prod(k, i, j) = A(i, k) * B(k, j); AB(i, j) += prod(rv, i, j), rv = 0 .. sum_size - 1
 *     upward from 0 (unroll(rv, 2) keeps the order); result(i, j) = a * ABt(i, j) + b * C(i, j) — MAD2(a, ab, b, C), and b * C is
 *     evaluated whatever b is.
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
 * compareScalars (apps/linear_algebra/tests/test_halide_blas.cpp:150-173) is restated as la_compare and, as BLASDoubleTests instantiates
 * it, ld_compare. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

#include "oracle_common.h"

static inline double d_mad(double a, double b, double c) { return o_canon_fma ? fma(a, b, c) : a * b + c; }
static inline double d_mad2(double a, double b, double c, double d) { return o_canon_fma ? fma(a, b, c * d) : a * b + c * d; }

#define T float
#define P(name) la_##name
#define MAD o_mad
#define MAD2 o_mad2
#define FMA fmaf
#define FABS fabsf
#define V 8
#define T_MIN 1.17549435e-38f
#define T_EPSILON 1.1920929e-7f
#include "linear_algebra_check_body.h"
#undef T
#undef P
#undef MAD
#undef MAD2
#undef FMA
#undef FABS
#undef V
#undef T_MIN
#undef T_EPSILON

#define T double
#define P(name) ld_##name
#define MAD d_mad
#define MAD2 d_mad2
#define FMA fma
#define FABS fabs
#define V 4
#define T_MIN 2.2250738585072014e-308
#define T_EPSILON 2.220446049250313e-16
#include "linear_algebra_check_body.h"
