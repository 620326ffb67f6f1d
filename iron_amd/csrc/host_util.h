// Host-side helpers of the mesh chain (mcubes / texbake / uvunwrap / meshdist / meshrender and bvh_common.h): the 256-byte
// alignment, the ceil-divide grid and the workspace carver (ws_layout.h) and launch-and-check.  Host only: the MLP / tracer /
// shading units do not include it.
#pragma once
#include "iron_common.h"
#include "ws_layout.h"

// launch on `stream`, then the launch's own error -> IRON_ERR_HIP out of the calling entry point
#define IRON_LAUNCH(kernel, grid, block, stream, ...)                                   \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);    \
        IRON_HIP_TRY(hipGetLastError());                                                \
    } while (0)
