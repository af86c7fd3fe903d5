/* hannk_target.h — the layout constants of apps/hannk's convolution ops on this target (gfx950), written down once.
 * The reference derives them from its target (conv_generator.cpp:93-95, depthwise_conv_generator.cpp:60-63) and its interpreter
 * learns them from bounds queries (interpreter/ops.cpp: ConvOp::prepare, DepthwiseConv2DOp::prepare), never from a header: this
 * file is for the library's own sources and for readers.  The filter of conv_* is UInt(8) (the use_8bit_multiply branch). */
#ifndef HLMI_AOT_HANNK_TARGET_H
#define HLMI_AOT_HANNK_TARGET_H
#define HLMI_HANNK_VECTOR_REDUCTION 4     /* filter.dim(0).extent: consecutive input channels in one dword of the tiled filter */
#define HLMI_HANNK_ACCUM_VECTOR_SIZE 16   /* filter.dim(1).extent, the interpreter's vector_tile_: output channels per filter tile */
#define HLMI_HANNK_DEPTHWISE_VECTOR 16    /* depthwise_conv_uint8: the input's channel extent, strides and host pointer are multiples */
#endif
