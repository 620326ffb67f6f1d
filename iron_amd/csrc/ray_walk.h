// The closest-hit walk over the linear BVH of bvh_common.h, shared by the ray cast (meshrender.hip: k_raycast) and the bounce rays of
// the path integrator (envlight.hip: k_shade_env_indirect).  The contract of the walk and of its primitive tests (ray_core.h) is at
// the head of meshrender.hip; `skip` removes one face from the mesh (-1: none), which changes nothing else: t stays a function of
// the set of the remaining faces.
#pragma once
#include "ray_core.h"

namespace iron {

constexpr int32_t kNoFace = 0x7fffffff;

struct RayHit {
    float t, b1, b2;  // distance along d, barycentric weights of the face's second and third vertex
    int32_t face;     // kNoFace: none yet
    int32_t leaf;     // its position in the leaf order
};

// the window's far end is inclusive: any face at t_max beats the sentinel
__device__ __forceinline__ RayHit ray_hit_none(float t_max) {
    RayHit h;
    h.t = t_max; h.face = kNoFace; h.leaf = 0; h.b1 = h.b2 = 0.0f;
    return h;
}

__device__ __forceinline__ void ray_leaf(const float4* __restrict__ tris, int32_t k, const RayPre& r, float t_min, int32_t skip, RayHit& h) {
    TriHit x;
    if (!ray_tri(tris, k, r, t_min, x) || x.face == skip) return;
    if (x.t < h.t || (x.t == h.t && x.face < h.face)) {
        h.t = x.t; h.face = x.face; h.leaf = k; h.b1 = x.V / x.det; h.b2 = x.W / x.det;
    }
}

// The winner's barycentric weights once more, in fp64 from the fp32 inputs (Moeller-Trumbore; the differences are exact there).  The
// ray-space edge functions decide the hit and t; as weights they carry the rounding of the vertices' translation to the ray origin,
// ~2^-24 |A - o| / h (h the face's altitude), which grows with the distance to the camera.  These do not.
__device__ __forceinline__ void refine_bary(const float4* __restrict__ tris, float3 o, float3 d, RayHit& h) {
    const float4 ta = tris[3 * (int64_t)h.leaf], tb = tris[3 * (int64_t)h.leaf + 1], tc = tris[3 * (int64_t)h.leaf + 2];
    const double e1[3] = {(double)tb.x - ta.x, (double)tb.y - ta.y, (double)tb.z - ta.z};
    const double e2[3] = {(double)tc.x - ta.x, (double)tc.y - ta.y, (double)tc.z - ta.z};
    const double s[3] = {(double)o.x - ta.x, (double)o.y - ta.y, (double)o.z - ta.z};
    const double dd[3] = {d.x, d.y, d.z};
    const double p[3] = {dd[1] * e2[2] - dd[2] * e2[1], dd[2] * e2[0] - dd[0] * e2[2], dd[0] * e2[1] - dd[1] * e2[0]};
    const double q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
    const double det = (e1[0] * p[0] + e1[1] * p[1]) + e1[2] * p[2];
    if (det == 0.0) return;  // keeps the fp32 weights
    const double u = ((s[0] * p[0] + s[1] * p[1]) + s[2] * p[2]) / det, v = ((dd[0] * q[0] + dd[1] * q[1]) + dd[2] * q[2]) / det;
    if (!(fabs(u) <= 2.0) || !(fabs(v) <= 2.0)) return;  // a sliver seen edge-on: nothing gained
    h.b1 = (float)fmin(fmax(u, 0.0), 1.0);  // a hit the fp32 test took on an edge may lie a rounding outside
    h.b2 = (float)fmin(fmax(v, 0.0), 1.0);
}

// the closest face other than `skip` with t in (t_min, h.t] (h from ray_hit_none(t_max)); one lane per ray, depth-first, the child
// with the nearer box entry first, the other on the lane's column of `stack` (LDS, [depth][lane]: lane l always on bank l % 32)
__device__ __forceinline__ void bvh_closest_hit(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf, const RayPre& r,
                                                float t_min, int32_t skip, int32_t (*stack)[kBvQueryBlock], int lane, RayHit& h) {
    if (nf == 1) {
        ray_leaf(tris, 0, r, t_min, skip, h);
        return;
    }
    int32_t node = 0, sp = 0;
    for (;;) {
        const float4* nd = nodes + 4 * (int64_t)node;
        const float4 l0 = nd[0], h0 = nd[1], l1 = nd[2], h1 = nd[3];
        const int32_t c0 = __float_as_int(l0.w), c1 = __float_as_int(h0.w);
        float n0, n1;
        const bool v0 = ray_box(r, l0, h0, t_min, h.t, n0);
        if (c0 < 0 && v0) ray_leaf(tris, ~c0, r, t_min, skip, h);
        const bool v1 = ray_box(r, l1, h1, t_min, h.t, n1);
        if (c1 < 0 && v1) ray_leaf(tris, ~c1, r, t_min, skip, h);
        const bool g0 = c0 >= 0 && v0 && n0 <= h.t, g1 = c1 >= 0 && v1 && n1 <= h.t;
        if (g0 && g1) {
            const bool first1 = n1 < n0;
            if (sp < kBvStack) stack[sp++][lane] = first1 ? c0 : c1;  // never full (kBvStack)
            node = first1 ? c1 : c0;
        } else if (g0) {
            node = c0;
        } else if (g1) {
            node = c1;
        } else {
            if (sp == 0) break;
            node = stack[--sp][lane];
        }
    }
}

}  // namespace iron
