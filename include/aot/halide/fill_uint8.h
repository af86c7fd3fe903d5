/* fill_uint8.h — stands in for the header the reference's generator emits next to fill_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/fill_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_FILL_UINT8_H
#define HLMI_AOT_HALIDE_FILL_UINT8_H
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
/* output u8 [c, x, y, b] = value */
int fill_uint8(uint8_t _value, struct halide_buffer_t *_output_buffer);
int fill_uint8_argv(void **args);
const struct halide_filter_metadata_t *fill_uint8_metadata();
}  // namespace hannk
#endif
