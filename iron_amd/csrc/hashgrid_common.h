// Multiresolution hash-grid encoding (tiny-cuda-nn's published HashGrid with Linear interpolation; DESIGN.md "Hash-grid
// encoding"): the one definition of the level table and of the corner walk.  The host layout function (iron_hashgrid_layout),
// the forward kernels (hashgrid.hip) and the gradient kernels (hashgrid_train.hip) all include this file.
//
// Level l of (L, F, log2 T, N, b):
//     scale = exp2(l log2 b) N - 1   in double, stored as fp32
//     res   = ceil(scale) + 1
//     size  = min(roundup8(res^3), 2^log2T) entries of F floats;   dense iff res^3 <= size
// A point x (clamped to [0, 1] per axis) sits at pos = x scale + 0.5 in cell floor(pos) with fraction w; corner o in {0,1}^3 has
// integer coordinates cell + o and weight prod_d (o_d ? w_d : 1 - w_d).
//     dense index   (c0 + c1 res + c2 res^2) mod size
//     hashed index  (c0 ^ c1 2654435761 ^ c2 805459861) mod size       (uint32 arithmetic)
// On a dense level the top-face corner (coordinate res, reached by x = 1 when scale is an integer) wraps to another row exactly
// as it does in tiny-cuda-nn; this is kept, not mended.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/iron_hip.h"

namespace iron {
namespace hg {

constexpr int kMaxLevels = IRON_HASHGRID_MAX_LEVELS;
constexpr uint32_t kPrime1 = 2654435761u, kPrime2 = 805459861u;

// what a kernel needs of the level table, passed by value
struct Levels {
    iron_hashgrid_level lv[kMaxLevels];
    int32_t n_levels, n_features;
};

// Validates `d` and fills the level table.  IRON_ERR_BAD_ARG: a parameter outside its range;  IRON_ERR_RANGE: a level's scale
// reaches 2^22 (0.5 - cell must stay exact in fp32, with room to spare).
inline int layout(const iron_hashgrid_desc* d, iron_hashgrid_level* out, int64_t* n_params) {
    if (!d) return IRON_ERR_BAD_ARG;
    const int F = d->n_features_per_level;
    if (d->n_levels < 1 || d->n_levels > kMaxLevels || !(F == 1 || F == 2 || F == 4 || F == 8)) return IRON_ERR_BAD_ARG;
    if (d->log2_hashmap_size < 1 || d->log2_hashmap_size > 24 || d->base_resolution < 1) return IRON_ERR_BAD_ARG;
    if (!(d->per_level_scale >= 1.0) || !(d->per_level_scale < 1e30)) return IRON_ERR_BAD_ARG;
    const double log2b = log2(d->per_level_scale);
    int64_t off = 0;
    for (int l = 0; l < d->n_levels; ++l) {
        const double s = exp2((double)l * log2b) * (double)d->base_resolution - 1.0;
        if (!(s < 4194304.0)) return IRON_ERR_RANGE;
        const float scale = (float)s;
        const uint64_t res = (uint64_t)ceilf(scale) + 1;
        const uint64_t cube = res * res * res;                       // only read when res <= 256: a larger cube exceeds any table
        const uint64_t cap = (uint64_t)1 << d->log2_hashmap_size;
        uint64_t size = cap;
        if (res <= 256 && ((cube + 7) / 8) * 8 < cap) size = ((cube + 7) / 8) * 8;
        if (out) {
            out[l].scale = scale;
            out[l].res = (uint32_t)res;
            out[l].size = (uint32_t)size;
            out[l].dense = (res <= 256 && cube <= size) ? 1u : 0u;
            out[l].offset = off;
        }
        off += (int64_t)size;
    }
    if (n_params) *n_params = off;
    return IRON_OK;
}

inline int make_levels(const iron_hashgrid_desc* d, Levels* L, int64_t* n_params) {
    const int rc = layout(d, L->lv, n_params);
    if (rc != IRON_OK) return rc;
    L->n_levels = d->n_levels;
    L->n_features = d->n_features_per_level;
    return IRON_OK;
}

// One axis: cell, fraction w and complement u = 1 - w of the clamped coordinate, and whether the axis is live (x inside [0, 1]:
// d clamp / dx = 1).  pos = x scale + 0.5 rounded to fp32 only decides the cell; the fraction comes from ONE fused multiply-add,
// w = fma(x, scale, 0.5 - cell), with 0.5 - cell exact below 2^23, so it keeps the bits that pos - floor(pos) loses on the fine
// levels (11 of them at res 2048).  The complement is formed the same way, u = fma(-x, scale, cell + 0.5), not as 1 - w: next to
// a face, where w rounds to within an ulp of 1, 1 - w would carry a relative error of percents into the weights of the far
// corners.  A cell the rounded pos put one too high shows as w < 0 and is stepped down once; the fraction of the lower cell may
// then round to 1.0f, which is accepted: the features are continuous across a face.
__host__ __device__ inline void locate(float x, float scale, uint32_t* cell, float* w, float* u, float* live) {
    *live = (x >= 0.0f && x <= 1.0f) ? 1.0f : 0.0f;
    const float xc = fminf(fmaxf(x, 0.0f), 1.0f);   // NaN -> 0
    float c = floorf(fmaf(xc, scale, 0.5f));
    float f = fmaf(xc, scale, 0.5f - c);
    if (f < 0.0f) {
        c -= 1.0f;
        f = fmaf(xc, scale, 0.5f - c);
    }
    *cell = (uint32_t)c;
    *w = f;
    *u = fmaf(-xc, scale, c + 0.5f);
}

__host__ __device__ inline uint32_t corner_index(const iron_hashgrid_level& lv, uint32_t c0, uint32_t c1, uint32_t c2) {
    const uint32_t i = lv.dense ? c0 + c1 * lv.res + c2 * lv.res * lv.res : c0 ^ (c1 * kPrime1) ^ (c2 * kPrime2);
    return i % lv.size;
}

// The corner walk of one (point, level): the eight entry indices (relative to the level's first entry), their trilinear weights
// and, per axis d, the signed product of the other two axes' weights, dw[o][d] = d weight_o / d w_d.  Corner o = o0 + 2 o1 + 4 o2.
struct Walk {
    uint32_t idx[8];
    float wgt[8];
    float dw[8][3];
    float live[3];
};

__host__ __device__ inline void walk(const iron_hashgrid_level& lv, const float* x, Walk* k) {
    uint32_t c[3];
    float w[3], u[3];
    for (int d = 0; d < 3; ++d) locate(x[d], lv.scale, &c[d], &w[d], &u[d], &k->live[d]);
    for (int o = 0; o < 8; ++o) {
        const int o0 = o & 1, o1 = (o >> 1) & 1, o2 = o >> 2;
        const float a0 = o0 ? w[0] : u[0], a1 = o1 ? w[1] : u[1], a2 = o2 ? w[2] : u[2];
        k->idx[o] = corner_index(lv, c[0] + o0, c[1] + o1, c[2] + o2);
        k->wgt[o] = a0 * a1 * a2;
        k->dw[o][0] = o0 ? a1 * a2 : -(a1 * a2);
        k->dw[o][1] = o1 ? a0 * a2 : -(a0 * a2);
        k->dw[o][2] = o2 ? a0 * a1 : -(a0 * a1);
    }
}

// one entry: F floats in one load (two for F = 8); entries are F-float aligned, levels start on a multiple of 8 entries
template <int F>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float* r) {
    if constexpr (F == 1) {
        r[0] = *p;
    } else if constexpr (F == 2) {
        const float2 v = *(const float2*)p;
        r[0] = v.x; r[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            const float4 v = *(const float4*)(p + 4 * q);
            r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
        }
    }
}

// ---- fixed-point table gradients (hashgrid_train.hip) ----
// A table gradient is a sum of at most 8 n contributions, each bounded by `bound` in magnitude.  Every contribution is rounded to
// a whole number of units 2^e and added as a 64-bit integer: integer sums do not depend on the order the atomics land in.  e is
// the smallest exponent at which 8 n contributions stay below 2^62: with bound < 2^eb (frexp) and 8 n <= 2^k, e = eb + k - 62;
// the rounding adds at most half a unit per contribution, far inside the spare bit.  It depends on bound and n alone.
__host__ __device__ inline int grad_unit_exp(float bound, int64_t n) {
    if (!(bound > 0.0f)) return 0;
    int eb;
    (void)frexpf(bound, &eb);
    int k = 3;
    while (k < 62 && ((int64_t)1 << (k - 3)) < n) ++k;
    return eb + k - 62;
}

}  // namespace hg
}  // namespace iron
