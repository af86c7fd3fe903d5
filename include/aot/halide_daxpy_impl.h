/* halide_daxpy_impl.h — stands in for the header the reference's generator emits next to halide_daxpy_impl.a
 * (src/CodeGen_C.cpp:1050-1112): code written against apps/linear_algebra's halide_blas.h includes this file unchanged and
 * links libhlmi.so instead of the AOT object.  hlmi_blas.h is the interface over the twelve f32 and the twelve f64. */
#ifndef HLMI_AOT_HALIDE_DAXPY_IMPL_H
#define HLMI_AOT_HALIDE_DAXPY_IMPL_H
/* the generated header includes the runtime header first (src/CodeGen_C.cpp:1066); do the same when the
 * caller has it on the include path, otherwise fall back to the layout-identical re-declaration */
#if defined(__has_include)
#if __has_include("HalideRuntime.h")
#include "HalideRuntime.h"
#endif
#endif
#include "../hlmi_pipelines.h"
#include "../hlmi_runtime.h"
#endif
