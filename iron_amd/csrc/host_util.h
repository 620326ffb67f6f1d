// Host-side helpers of the mesh chain (mcubes / texbake / uvunwrap / meshdist / meshrender and bvh_common.h): the 256-byte
// alignment, the ceil-divide grid, the workspace carver and launch-and-check.  Host only: the MLP / tracer / shading units do not
// include it.
#pragma once
#include "iron_common.h"

namespace iron {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// Carves a workspace into 256-byte aligned regions.  One layout function per workspace runs the carver, for the *_workspace_bytes
// entry and for the entries that use the workspace alike, so a size query and a use cannot disagree; `off` ends as the total.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off = align256(off + bytes);
        return at;
    }
};

template <class T>
inline T* ws_ptr(void* ws, size_t off) { return (T*)((char*)ws + off); }
template <class T>
inline const T* ws_ptr(const void* ws, size_t off) { return (const T*)((const char*)ws + off); }

}  // namespace iron

// launch on `stream`, then the launch's own error -> IRON_ERR_HIP out of the calling entry point
#define IRON_LAUNCH(kernel, grid, block, stream, ...)                                   \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);    \
        IRON_HIP_TRY(hipGetLastError());                                                \
    } while (0)
