/* mat_mul_check.c — plain-C checker of apps/cuda_mat_mul (mat_mul_generator.cpp:27-32): TEST INFRASTRUCTURE ONLY.
 *
 *   out(x, y) = acc_n,  acc_0 = +0.0f,  acc_{r+1} = fmaf(A(x, r), B(r, y), acc_r),  r = 0 .. n - 1
 *
 * Dimension 0 is innermost: A(x, r) is A[r * sa + x], B(r, y) is B[y * sb + r], out(x, y) is out[y * so + x]; strides in elements.
 * Built with -ffp-contract=off: the only fused operation is the fmaf written here.  The loops run y, r, x so that a compiler may
 * do several x at once; every output still sees its own r = 0, 1, 2, ... in that order, which is all the contract says. */
#include <math.h>

void mm_check(const float *A, long sa, const float *B, long sb, float *out, long so, int n) {
    for (int y = 0; y < n; y++) {
        float *row = out + (long)y * so;
        for (int x = 0; x < n; x++) row[x] = 0.0f;
        for (int r = 0; r < n; r++) {
            const float b = B[(long)y * sb + r];
            const float *a = A + (long)r * sa;
            for (int x = 0; x < n; x++) row[x] = fmaf(a[x], b, row[x]);
        }
    }
}
