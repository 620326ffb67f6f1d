// The per-ray formulas of the reference tracer (models/raytracer.py:45-220), each written once: the callable tracer's bookkeeping
// (trace_any.hip) and the hash-grid field's device tracer (hashgrid_trace.hip) both include this file.  One rounding per product
// and sum (-ffp-contract=off), and the comparisons are the reference's own, not their negations, so that NaN and zero fall where
// torch puts them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iron {
namespace ray {

// p = o + d * t, component by component
__device__ __forceinline__ void ray_point(const float* __restrict__ o, const float* __restrict__ d, int64_t ray, float t, float* __restrict__ out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = o[ray * 3 + c] + d[ray * 3 + c] * t;
}

// raytracer.py:113-117: a ray stays unfinished while it is off the surface and short of its far end
__device__ __forceinline__ bool still_unfinished(bool before, float s, float thr, float t, float far) {
    return before && (fabsf(s) > thr) && (t < far);
}

// raytracer.py:123-130: the step of an unfinished ray, t first, then the point incrementally
__device__ __forceinline__ float advance(float p, float d, float s) { return p + d * s; }

// raytracer.py:132-137
__device__ __forceinline__ bool sphere_converged(bool work, bool unfinished, float s, float thr, float t, float far) {
    return work && !unfinished && (fabsf(s) <= thr) && (t < far);
}

// raytracer.py:56-63: sample behind the last sphere-tracing point when it is outside the surface, in front of it otherwise
__device__ __forceinline__ void sampler_interval(float s, float t, float near, float far, float* lo, float* hi) {
    const float pos = s > 0.0f ? 1.0f : 0.0f;
    const float neg = 1.0f - pos;
    *lo = pos * t + neg * near;
    *hi = pos * far + neg * t;
}

__device__ __forceinline__ float sample_z(float lo, float hi, float lin) { return lo + lin * (hi - lo); }

// raytracer.py:200-203
__device__ __forceinline__ bool bracket_open(float flo, float fhi) { return (flo > 0.0f) && (fhi < 0.0f); }
__device__ __forceinline__ float bracket_mid(float dlo, float dhi) { return (dlo + dhi) / 2.0f; }

// raytracer.py:205-217 for one bracket: a positive mid value moves the low end, a non-positive one the high end, a NaN neither
__device__ __forceinline__ void bracket_update(float fm, float mid, float* dlo, float* dhi, float* flo, float* fhi) {
    if (fm > 0.0f) { *dlo = mid; *flo = fm; }
    if (fm <= 0.0f) { *dhi = mid; *fhi = fm; }
}
__device__ __forceinline__ bool bracket_wide(float dlo, float dhi, float two_thr) { return (dhi - dlo) > two_thr; }

}  // namespace ray
}  // namespace iron
