// The ray cast's primitive tests, shared by the closest-hit cast (meshrender.hip: k_raycast) and the occlusion query (envlight.hip:
// k_occluded and the environment integrator's shadow rays).  Both walk the linear BVH of bvh_common.h with these, so they accept
// exactly the same faces and visit a box under exactly the same condition; the contract of each is at the head of meshrender.hip.
#pragma once
#include "bvh_common.h"

namespace iron {

constexpr float kInfF = __builtin_huge_valf();

struct RayPre {
    float3 o, inv, pad;   // origin, 1 / d, 2^-21 |1 / d| (0 on an axis whose reciprocal is not finite)
    bool zx, zy, zz;      // that axis: the reciprocal is not finite
    int kx, ky, kz;       // Woop's axis permutation
    float sx, sy, sz;     // shear and scale
};

__device__ __forceinline__ float pick(float3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

__device__ __forceinline__ void ray_setup(float3 o, float3 d, RayPre& r) {
    r.o = o;
    r.inv = make_float3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    r.zx = !(fabsf(r.inv.x) < kInfF); r.zy = !(fabsf(r.inv.y) < kInfF); r.zz = !(fabsf(r.inv.z) < kInfF);
    const float e = 4.76837158203125e-07f;  // 2^-21
    r.pad = make_float3(r.zx ? 0.0f : fabsf(r.inv.x) * e, r.zy ? 0.0f : fabsf(r.inv.y) * e, r.zz ? 0.0f : fabsf(r.inv.z) * e);
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const float dz = pick(d, r.kz);
    if (dz < 0.0f) { const int s = r.kx; r.kx = r.ky; r.ky = s; }  // keeps the winding
    r.sx = pick(d, r.kx) / dz;
    r.sy = pick(d, r.ky) / dz;
    r.sz = 1.0f / dz;
}

// a ray the casts answer at all: finite, with a non-zero direction
__device__ __forceinline__ bool ray_valid(float3 o, float3 d) {
    return finite3(o) && finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
}

// one slab: entry and exit of [lo, hi] on one axis, moved outwards (see the head of meshrender.hip)
__device__ __forceinline__ void slab(float lo, float hi, float o, float inv, float pad, bool zero, float& tn, float& tf) {
    const float t0 = (lo - o) * inv, t1 = (hi - o) * inv;
    const float p = ((fabsf(lo) + fabsf(hi)) + fabsf(o)) * pad;
    const float n = fminf(t0, t1) - p, f = fmaxf(t0, t1) + p;
    tn = fmaxf(tn, zero ? ((o >= lo && o <= hi) ? -kInfF : kInfF) : n);
    tf = fminf(tf, zero ? kInfF : f);
}

// does the ray meet the box within [t_min, best]?  `tn`: the (conservative) entry distance
__device__ __forceinline__ bool ray_box(const RayPre& r, float4 lo, float4 hi, float t_min, float best, float& tn) {
    float tf = kInfF;
    tn = -kInfF;
    slab(lo.x, hi.x, r.o.x, r.inv.x, r.pad.x, r.zx, tn, tf);
    slab(lo.y, hi.y, r.o.y, r.inv.y, r.pad.y, r.zy, tn, tf);
    slab(lo.z, hi.z, r.o.z, r.inv.z, r.pad.z, r.zz, tn, tf);
    return tn <= tf && tn <= best && tf >= t_min;
}

// the ray against the triangle at position k of the leaf order: true when it meets the face at a finite t > t_min
struct TriHit {
    float t, V, W, det;  // distance along d; V / det and W / det are the weights of the face's second and third vertex
    int32_t face;
};

__device__ __forceinline__ bool ray_tri(const float4* __restrict__ tris, int32_t k, const RayPre& r, float t_min, TriHit& x) {
    const float4 ta = tris[3 * (int64_t)k], tb = tris[3 * (int64_t)k + 1], tc = tris[3 * (int64_t)k + 2];
    x.face = __float_as_int(ta.w);
    const float3 A = sub3(make_float3(ta.x, ta.y, ta.z), r.o), B = sub3(make_float3(tb.x, tb.y, tb.z), r.o),
                 C = sub3(make_float3(tc.x, tc.y, tc.z), r.o);
    const float Akz = pick(A, r.kz), Bkz = pick(B, r.kz), Ckz = pick(C, r.kz);
    const float Ax = pick(A, r.kx) - r.sx * Akz, Ay = pick(A, r.ky) - r.sy * Akz;
    const float Bx = pick(B, r.kx) - r.sx * Bkz, By = pick(B, r.ky) - r.sy * Bkz;
    const float Cx = pick(C, r.kx) - r.sx * Ckz, Cy = pick(C, r.ky) - r.sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    bool neg = U < 0.0f || V < 0.0f || W < 0.0f, pos = U > 0.0f || V > 0.0f || W > 0.0f;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {  // on an edge or a vertex (or an underflow): the signs from exact products
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx;
        const double Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
        const double Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        neg = Ud < 0.0 || Vd < 0.0 || Wd < 0.0;
        pos = Ud > 0.0 || Vd > 0.0 || Wd > 0.0;
        U = (float)Ud; V = (float)Vd; W = (float)Wd;
    }
    if (neg && pos) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;  // edge-on or degenerate
    const float T = (U * (r.sz * Akz) + V * (r.sz * Bkz)) + W * (r.sz * Ckz);
    const float t = T / det;
    if (!(t > t_min) || !(t < kInfF)) return false;  // NaN fails too
    x.t = t; x.V = V; x.W = W; x.det = det;
    return true;
}

}  // namespace iron
