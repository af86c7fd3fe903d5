// Issue rate and dependent-issue latency of the gfx950 f64 VALU ops: ns per wave-instruction per SIMD for C independent chains of
// v_fma_f64 / v_add_f64 / v_mul_f64 + v_add_f64 pairs at 1, 2, 4 waves per SIMD, beside valu_dep.hip's f32 figures.  One chain at
// one wave per SIMD is the dependent-issue time (what bounds ddot, dasum and dgemv_notrans: DESIGN.md 5.10); eight chains at four
// waves is the issue rate, printed also as lanes per clock per SIMD at the device's reported clock and as the device's FLOP/s.
//   hipcc --offload-arch=gfx950 -O3 valu_f64.hip -o valu_f64
#include <hip/hip_runtime.h>
#include <stdio.h>

template<int OP, int C>
__global__ __launch_bounds__(256) void k(double *out, int iters, double s) {
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = threadIdx.x * 0.001 + i;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int r = 0; r < 64 / C; r++) {
#pragma unroll
            for (int i = 0; i < C; i++) {
                if (OP == 0) asm volatile("v_add_f64 %0, %0, %1" : "+v"(a[i]) : "v"(s));
                if (OP == 1) asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(a[i]) : "v"(s));
                if (OP == 2) asm volatile("v_mul_f64 %0, %0, %1\n\tv_add_f64 %0, %0, %1" : "+v"(a[i]) : "v"(s));
                if (OP == 3) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(*(float *)&a[i]) : "v"((float)s));   // the f32 yardstick of the same run
            }
        }
    }
    double acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc += a[i];
    if (acc == 12345.0) out[0] = acc;
}

static int cus = 256;

template<int OP, int C>
double run(int w, int iters, double *d) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0), hipEventCreate(&e1);
    k<OP, C><<<cus * w, 256>>>(d, 10, 1.0001);
    hipEventRecord(e0);
    k<OP, C><<<cus * w, 256>>>(d, iters, 1.0001);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0), hipEventDestroy(e1);
    return ms * 1e-3 / ((double)iters * 64 * (OP == 2 ? 2 : 1) * w) * 1e9;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    cus = prop.multiProcessorCount;
    const double ghz = prop.clockRate * 1e-6;
    double *d;
    if (hipMalloc(&d, 8) != hipSuccess) return 1;
    const char *names[] = {"v_add_f64", "v_fma_f64", "mul_f64,add_f64", "v_fma_f32"};
    printf("%s, %d CUs, reported clock %.3f GHz\n", prop.name, cus, ghz);
    for (int w : {1, 2, 4}) {
        printf("waves/SIMD=%d  chains:      1      2      4      8   (ns per wave-instruction per SIMD)\n", w);
        printf("  %-16s %6.3f %6.3f %6.3f %6.3f\n", names[0], run<0, 1>(w, 2000, d), run<0, 2>(w, 2000, d), run<0, 4>(w, 2000, d), run<0, 8>(w, 2000, d));
        printf("  %-16s %6.3f %6.3f %6.3f %6.3f\n", names[1], run<1, 1>(w, 2000, d), run<1, 2>(w, 2000, d), run<1, 4>(w, 2000, d), run<1, 8>(w, 2000, d));
        printf("  %-16s %6.3f %6.3f %6.3f %6.3f\n", names[2], run<2, 1>(w, 2000, d), run<2, 2>(w, 2000, d), run<2, 4>(w, 2000, d), run<2, 8>(w, 2000, d));
        printf("  %-16s %6.3f %6.3f %6.3f %6.3f\n", names[3], run<3, 1>(w, 2000, d), run<3, 2>(w, 2000, d), run<3, 4>(w, 2000, d), run<3, 8>(w, 2000, d));
    }
    const double ns = run<1, 8>(4, 2000, d);   // the issue rate: eight chains, four waves per SIMD
    printf("v_fma_f64 issue: %.3f ns per wave-instruction per SIMD = %.2f lanes per clock per SIMD at %.3f GHz = %.1f TFLOP/s over %d CUs x 4 SIMDs\n", ns,
           64.0 / (ns * ghz), ghz, 2.0 * 64.0 * 4.0 * cus / ns * 1e-3, cus);
    hipFree(d);
    return 0;
}
