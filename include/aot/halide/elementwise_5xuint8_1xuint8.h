/* elementwise_5xuint8_1xuint8.h — stands in for the header the reference's generator emits next to elementwise_5xuint8_1xuint8.a (apps/hannk/halide/CMakeLists.txt
 * builds the op library with c_plus_plus_name_mangling: C++ only, every symbol in namespace hannk): code written against the reference
 * (#include "halide/elementwise_5xuint8_1xuint8.h" with -Iinclude/aot) includes this file unchanged and links libhlmi.so instead of the AOT object. */
#ifndef HLMI_AOT_HALIDE_ELEMENTWISE_5XUINT8_1XUINT8_H
#define HLMI_AOT_HALIDE_ELEMENTWISE_5XUINT8_1XUINT8_H
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
/* five inputs u8 [x, y] (dimension 0 stride 1, or 0 to broadcast), program i16 [5, n] (n <= 20 instructions of interpreter/elementwise_program.h)
 * -> output u8 [x, y] = u8_sat(the last slot) */
int elementwise_5xuint8_1xuint8(struct halide_buffer_t *_inputs_0_buffer, struct halide_buffer_t *_inputs_1_buffer, struct halide_buffer_t *_inputs_2_buffer,
    struct halide_buffer_t *_inputs_3_buffer, struct halide_buffer_t *_inputs_4_buffer, struct halide_buffer_t *_program_buffer,
    struct halide_buffer_t *_output_buffer);
int elementwise_5xuint8_1xuint8_argv(void **args);
const struct halide_filter_metadata_t *elementwise_5xuint8_1xuint8_metadata();
}  // namespace hannk
#endif
