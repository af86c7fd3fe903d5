/* l2_normalization_uint8.h — stands in for the header the reference's generator emits next to l2_normalization_uint8.a (apps/hannk/halide/CMakeLists.txt builds the op
 * library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/l2_normalization_uint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_L2_NORMALIZATION_UINT8_H
#define HLMI_AOT_HALIDE_L2_NORMALIZATION_UINT8_H
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
/* input u8 [x, y] -> output u8 [x, y]: 128 x / |x| + 128 over the input's dimension 0 */
int l2_normalization_uint8(struct halide_buffer_t *_input_buffer, uint8_t _input_zero, struct halide_buffer_t *_output_buffer);
int l2_normalization_uint8_argv(void **args);
const struct halide_filter_metadata_t *l2_normalization_uint8_metadata();
}  // namespace hannk
#endif
