// Small helpers every mesh unit needs (texbake / uvunwrap / meshdist / meshrender): the index test of a face, the size check of
// a mesh and the order-preserving uint encoding of fp32.  What a unit treats as an invalid face beyond its indices (a non-finite
// vertex, a non-finite product, a NaN area) stays with that unit's loader.
#pragma once
#include "iron_common.h"

namespace iron {

__device__ __forceinline__ bool face_in_range(int32_t i0, int32_t i1, int32_t i2, int64_t n) {
    return i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < n && i1 < n && i2 < n;
}
__device__ __forceinline__ bool face_in_range(const int32_t* f, int64_t n) { return face_in_range(f[0], f[1], f[2], n); }

// fp32 <-> uint32 whose integer order is the float order (min / max by integer atomics)
__device__ __forceinline__ uint32_t f2ord(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

inline bool mesh_sizes_ok(int64_t n_verts, int64_t n_faces) {
    return n_verts >= 0 && n_faces > 0 && n_faces < 0x7fffffffLL && n_verts <= 0x7fffffffLL;
}

}  // namespace iron
