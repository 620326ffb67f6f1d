// The 256-byte alignment, the ceil-divide grid and the workspace carver: the part of the host helpers that reports no error, so
// that both libraries include it (host_util.h for libiron_hip.so, train_common.h for libiron_train.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iron {

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
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
