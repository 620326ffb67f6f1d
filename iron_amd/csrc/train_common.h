// What the four units of libiron_train.so (train.hip, losses.hip, optim.hip, volume_loss.hip) share on the host: the error word
// behind iron_train_last_hip_error(), check and launch-and-check, the integer helpers, and the host side of the slot pattern of
// fixed_sum.h (one workgroup per `span` items writes one slot of kVals doubles; one workgroup adds the slots).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/iron_train.h"
#include "ws_layout.h"

namespace iron_train {

extern thread_local int g_hip_error;   // defined in train.hip

using iron::align256;
constexpr int kThreads = 256;
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int64_t slot_count(int64_t items, int64_t span) { return cdiv64(items, span); }
inline size_t slot_bytes(int64_t slots, int vals) { return sizeof(double) * vals * (size_t)(slots > 0 ? slots : 1); }
inline bool grid_ok(int64_t blocks) { return blocks <= 0x7fffffff; }   // gridDim.x

}  // namespace iron_train

#define IRON_TRAIN_HIP(expr)                           \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) {                        \
            ::iron_train::g_hip_error = (int)_e;       \
            return IRON_ERR_HIP;                       \
        }                                              \
    } while (0)

// launch on `stream`, then the launch's own error -> IRON_ERR_HIP out of the calling entry point
#define IRON_TRAIN_LAUNCH(kernel, grid, block, stream, ...)                             \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);    \
        IRON_TRAIN_HIP(hipGetLastError());                                              \
    } while (0)
