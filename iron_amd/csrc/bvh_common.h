// The linear BVH of csrc/meshdist.hip as its consumers see it: workspace layout, header, node / triangle records and the small
// vector helpers.  Built by iron_bvh_keys / iron_bvh_hierarchy / iron_bvh_boxes (meshdist.hip), walked by the point query
// (meshdist.hip) and the ray cast (meshrender.hip).
// Node (64 B): float4 {lo0.xyz, child0}, {hi0.xyz, child1}, {lo1.xyz, 0}, {hi1.xyz, 0}; a child >= 0 is an internal node, a child
// < 0 is leaf ~k, whose triangle record (48 B: {A.xyz, face}, {B.xyz, 0}, {C.xyz, 0}) sits at position k of the leaf order.
#pragma once
#include "host_util.h"
#include "mesh_common.h"

namespace iron {

constexpr int kBvBlock = 256;
constexpr int kBvQueryBlock = 64;  // one wave per block: the stack below is 16 KiB per wave
// Along any root-to-leaf path the common-prefix length of the node's key range grows strictly (Karras), and it lies in [0, 63]
// for distinct 64-bit keys: at most 64 internal nodes per path, each pushing at most one sibling, so 64 entries cannot overflow.
constexpr int kBvStack = 64;

struct BvHeader {
    uint32_t lo[3], hi[3];  // centroid box, f2ord of mesh_common.h (min / max by integer atomics)
    int32_t bad;            // a face indexes outside the vertices or has a non-finite coordinate
    int32_t pad;
};

__device__ __forceinline__ bool finite3(float3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

__device__ __forceinline__ float3 ld3(const float* __restrict__ v, int64_t i) { return make_float3(v[3 * i], v[3 * i + 1], v[3 * i + 2]); }

__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// ---- workspace layout ----
struct BvLayout {
    size_t hdr_off, nodes_off, tris_off, pint_off, pleaf_off, cnt_off, bytes;
};

inline BvLayout bv_layout(int64_t nf) {
    BvLayout L{};
    const size_t ni = nf > 1 ? (size_t)(nf - 1) : 1;
    Carver c;
    L.hdr_off = c.take(sizeof(BvHeader));
    L.nodes_off = c.take(64 * ni);
    L.tris_off = c.take(48 * (size_t)nf);
    L.pint_off = c.take(4 * ni);
    L.pleaf_off = c.take(4 * (size_t)nf);
    L.cnt_off = c.take(4 * ni);
    L.bytes = c.off;
    return L;
}

}  // namespace iron
