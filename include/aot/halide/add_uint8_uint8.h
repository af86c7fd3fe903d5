/* add_uint8_uint8.h — stands in for the header the reference's generator emits next to add_uint8_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/add_uint8_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_ADD_UINT8_UINT8_H
#define HLMI_AOT_HALIDE_ADD_UINT8_UINT8_H
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
/* input1, input2 u8 [x, y] (dimension 0 stride 1, or 0 to broadcast one of them) -> output u8 [x, y] */
int add_uint8_uint8(struct halide_buffer_t *_input1_buffer, uint8_t _input1_zero, int16_t _input1_multiplier, struct halide_buffer_t *_input2_buffer,
    uint8_t _input2_zero, int16_t _input2_multiplier, uint8_t _output_zero, uint8_t _output_min, uint8_t _output_max,
    struct halide_buffer_t *_output_buffer);
int add_uint8_uint8_argv(void **args);
const struct halide_filter_metadata_t *add_uint8_uint8_metadata();
}  // namespace hannk
#endif
