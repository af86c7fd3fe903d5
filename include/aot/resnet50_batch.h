/* resnet50_batch.h — the header of resnet50_batch, a library extension: the reference's resnet_50 generator has no batch dimension and emits
 * no such object.  It follows the layout of the headers that stand in for generated ones (resnet50.h): the runtime header first, then the
 * declarations. */
#ifndef HLMI_AOT_RESNET50_BATCH_H
#define HLMI_AOT_RESNET50_BATCH_H
#if defined(__has_include)
#if __has_include("HalideRuntime.h")
#include "HalideRuntime.h"
#endif
#endif
#include "../hlmi_pipelines.h"
#include "../hlmi_runtime.h"
#endif
