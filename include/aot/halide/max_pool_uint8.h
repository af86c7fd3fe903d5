/* max_pool_uint8.h — stands in for the header the reference's generator emits next to max_pool_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/max_pool_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_MAX_POOL_UINT8_H
#define HLMI_AOT_HALIDE_MAX_POOL_UINT8_H
#if defined(__has_include)
#if __has_include("HalideRuntime.h")
#include "HalideRuntime.h"
#endif
#endif
#include <stdint.h>
#include "../../hlmi_abi.h"
#include "hannk_target.h"
#ifndef __cplusplus
#error "the hannk op library is built with C++ name mangling"
#endif
namespace hannk {
/* input u8 [c, x, y, b] -> output u8 [c, x, y, b]: min(max(output_min, the window's taps inside the input), output_max) */
int max_pool_uint8(struct halide_buffer_t *_input_buffer, int32_t _stride_x, int32_t _stride_y, int32_t _filter_width, int32_t _filter_height,
    uint8_t _output_min, uint8_t _output_max, struct halide_buffer_t *_output_buffer);
int max_pool_uint8_argv(void **args);
const struct halide_filter_metadata_t *max_pool_uint8_metadata();
}  // namespace hannk
#endif
