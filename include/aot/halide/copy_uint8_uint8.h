/* copy_uint8_uint8.h — stands in for the header the reference's generator emits next to copy_uint8_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/copy_uint8_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_COPY_UINT8_UINT8_H
#define HLMI_AOT_HALIDE_COPY_UINT8_UINT8_H
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
/* input u8 [c, x, y, b] -> output u8 [c, x, y, b]; channels outside the input's dimension 0 are uint8_t(pad_value) */
int copy_uint8_uint8(struct halide_buffer_t *_input_buffer, int32_t _pad_value, struct halide_buffer_t *_output_buffer);
int copy_uint8_uint8_argv(void **args);
const struct halide_filter_metadata_t *copy_uint8_uint8_metadata();
}  // namespace hannk
#endif
