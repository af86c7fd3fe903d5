/* depthwise_conv_shallow_uint8.h — stands in for the header the reference's generator emits next to depthwise_conv_shallow_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/depthwise_conv_shallow_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_DEPTHWISE_CONV_SHALLOW_UINT8_H
#define HLMI_AOT_HALIDE_DEPTHWISE_CONV_SHALLOW_UINT8_H
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
/* the depthwise convolution with c and x fused into dimension 0 (the output's dimension 1 is {0, 1}): input u8 [c, 1, y, b], filter u8 [D, fx, fy] and
 * bias i32 [D] with D a divisor of the channel vector (16) -> output u8 [c, 1, y, b]; the tap rx reads the input at c + rx * dilation_x * input_stride_x */
int depthwise_conv_shallow_uint8(struct halide_buffer_t *_input_buffer, uint8_t _input_zero, struct halide_buffer_t *_filter_buffer, uint8_t _filter_zero,
    struct halide_buffer_t *_bias_buffer, int32_t _stride_x, int32_t _stride_y, int32_t _dilation_x, int32_t _dilation_y,
    int32_t _input_stride_x, int32_t _output_multiplier, int32_t _output_shift, uint8_t _output_zero, uint8_t _output_min, uint8_t _output_max,
    struct halide_buffer_t *_output_buffer);
int depthwise_conv_shallow_uint8_argv(void **args);
const struct halide_filter_metadata_t *depthwise_conv_shallow_uint8_metadata();
}  // namespace hannk
#endif
