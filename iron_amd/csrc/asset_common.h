// What the flash render (meshrender.hip) and the environment render (envlight.hip) share on a hit of an exported asset: the texture
// fetch in the bake's convention and the surface record (point, shading normal, material) of one ray, primary or bounced.
#pragma once
#include "ray_core.h"

namespace iron {

// ---- texture fetch ----
// The bake's pixel convention (texbake.hip: u = uv_x W, v = H - uv_y H, texel (row, col) covers [col, col + 1) x [row, row + 1)):
// x = uv_x W - 1/2, y = (H - uv_y H) - 1/2 are the coordinates in texel centres.  They are formed in fp64, where they are exact for
// fp32 uv and sizes below 2^24.  Returns true for a hole: no tap with a non-zero bake weight (or a non-finite uv); out is then 0.
template <int MAXC>
__device__ __forceinline__ bool texture_fetch(const float* __restrict__ tex, const float* __restrict__ weight, int H, int W, int C, float u,
                                              float v, int mode, float out[MAXC]) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) out[c] = 0.0f;
    if (!isfinite(u) || !isfinite(v)) return true;
    const double xu = (double)u * (double)W, yv = (double)H - (double)v * (double)H;
    if (mode == IRON_TEX_NEAREST) {
        const int col = (int)fmin(fmax(floor(xu), 0.0), (double)(W - 1)), row = (int)fmin(fmax(floor(yv), 0.0), (double)(H - 1));
        const int64_t t = (int64_t)row * W + col;
        if (weight && !(weight[t] > 0.0f)) return true;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) out[c] = tex[t * C + c];
        return false;
    }
    const double x = fmin(fmax(xu - 0.5, -1.0), (double)W), y = fmin(fmax(yv - 0.5, -1.0), (double)H);  // beyond the edge: the edge texel
    const double x0 = floor(x), y0 = floor(y);
    const float fx = (float)(x - x0), fy = (float)(y - y0);
    const int c0 = min(max((int)x0, 0), W - 1), c1 = min(max((int)x0 + 1, 0), W - 1);
    const int r0 = min(max((int)y0, 0), H - 1), r1 = min(max((int)y0 + 1, 0), H - 1);
    const int64_t tap[4] = {(int64_t)r0 * W + c0, (int64_t)r0 * W + c1, (int64_t)r1 * W + c0, (int64_t)r1 * W + c1};
    float w[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    if (weight) {
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!(weight[tap[k]] > 0.0f)) w[k] = 0.0f;
            sum += w[k];
        }
        if (!(sum > 0.0f)) return true;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = w[k] / sum;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (w[k] != 0.0f) a += w[k] * tex[tap[k] * C + c];  // a dropped tap is not read: an unbaked texel may hold anything
            out[c] = a;
        }
    return false;
}

constexpr int kTexMaxC = 8;

__device__ __forceinline__ float3 unit_or_zero(float3 v) {
    const float l = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    return l > 0.0f && l < kInfF ? make_float3(v.x / l, v.y / l, v.z / l) : make_float3(0.f, 0.f, 0.f);
}

__device__ __forceinline__ void st3(float* __restrict__ p, int64_t i, float x, float y, float z) {
    if (p) { p[3 * i] = x; p[3 * i + 1] = y; p[3 * i + 2] = z; }
}

// ---- the surface under one primary ray ----
// From iron_mesh_raycast's t / face_idx / bary: point = o + t d, distance = |point - o|, uv through the face's own face_uvs, the
// normal = the normalised interpolation of the vertex normals (none, or a zero result: the face's (B-A) x (C-A); never flipped
// towards the viewer), the material = the bilinear fetch with the bake's weight.  A miss (or an index out of range) leaves zeros.
struct SurfHit {
    bool hit, hole;
    int64_t face;
    int32_t iv[3];
    float3 o, d, pt, nrm;
    float dist, uvx, uvy, mat[kTexMaxC];
};

// the unit geometric normal (B - A) x (C - A) of the record's face (zero for a degenerate face)
__device__ __forceinline__ float3 asset_face_normal(const iron_asset_mesh& m, const SurfHit& s) {
    const float3 va = ld3(m.verts, s.iv[0]);
    return unit_or_zero(cross3(sub3(ld3(m.verts, s.iv[1]), va), sub3(ld3(m.verts, s.iv[2]), va)));
}

// one face, t, ray and barycentric pair by value: a primary hit of the array form below, or a vertex of a path
__device__ __forceinline__ void asset_surface_at(const iron_asset_mesh& m, int64_t f, float t, float3 o, float3 d, float b1, float b2,
                                                 SurfHit& s) {
    bool hit = f >= 0 && f < m.n_faces && t < kInfF && t == t;
    int32_t it[3] = {0, 0, 0};
    s.iv[0] = s.iv[1] = s.iv[2] = 0;
    if (hit)
        for (int k = 0; k < 3; ++k) {
            s.iv[k] = m.faces[3 * f + k];
            it[k] = m.face_uvs[3 * f + k];
            if (s.iv[k] < 0 || s.iv[k] >= m.n_verts || it[k] < 0 || it[k] >= m.n_uvs) hit = false;
        }
    s.hit = hit; s.hole = false; s.face = f;
    s.o = s.d = s.pt = s.nrm = make_float3(0.f, 0.f, 0.f);
    s.dist = s.uvx = s.uvy = 0.0f;
#pragma unroll
    for (int c = 0; c < kTexMaxC; ++c) s.mat[c] = 0.0f;
    if (!hit) return;
    const float b0 = (1.0f - b1) - b2;
    s.o = o; s.d = d;
    s.pt = make_float3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
    const float3 rel = sub3(s.pt, o);
    s.dist = sqrtf((rel.x * rel.x + rel.y * rel.y) + rel.z * rel.z);
    s.uvx = (b0 * m.uvs[2 * (int64_t)it[0]] + b1 * m.uvs[2 * (int64_t)it[1]]) + b2 * m.uvs[2 * (int64_t)it[2]];
    s.uvy = (b0 * m.uvs[2 * (int64_t)it[0] + 1] + b1 * m.uvs[2 * (int64_t)it[1] + 1]) + b2 * m.uvs[2 * (int64_t)it[2] + 1];
    if (m.normals) {
        const float3 n0 = ld3(m.normals, s.iv[0]), n1 = ld3(m.normals, s.iv[1]), n2 = ld3(m.normals, s.iv[2]);
        s.nrm = unit_or_zero(make_float3((b0 * n0.x + b1 * n1.x) + b2 * n2.x, (b0 * n0.y + b1 * n1.y) + b2 * n2.y,
                                         (b0 * n0.z + b1 * n1.z) + b2 * n2.z));
    }
    if (s.nrm.x == 0.0f && s.nrm.y == 0.0f && s.nrm.z == 0.0f)  // no vertex normals, or they cancel: the face's own
        s.nrm = asset_face_normal(m, s);
    s.hole = texture_fetch<kTexMaxC>(m.material, m.weight, m.tex_h, m.tex_w, 7, s.uvx, s.uvy, IRON_TEX_BILINEAR, s.mat);
}

// ray i of iron_mesh_raycast's arrays
__device__ __forceinline__ void asset_surface(const iron_asset_mesh& m, const int32_t* __restrict__ face_idx, const float* __restrict__ t_in,
                                              const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                              const float* __restrict__ bary, int64_t i, SurfHit& s) {
    asset_surface_at(m, face_idx[i], t_in[i], ld3(ray_o, i), ld3(ray_d, i), bary[2 * i], bary[2 * i + 1], s);
}

// the geometry and material maps of iron_asset_out (the colours are the caller's)
__device__ __forceinline__ void asset_store_maps(const iron_asset_out& o, int64_t i, const SurfHit& s) {
    st3(o.normal, i, s.nrm.x, s.nrm.y, s.nrm.z);
    st3(o.points, i, s.pt.x, s.pt.y, s.pt.z);
    st3(o.diffuse_albedo, i, s.mat[0], s.mat[1], s.mat[2]);
    st3(o.specular_albedo, i, s.mat[3], s.mat[4], s.mat[5]);
    if (o.distance) o.distance[i] = s.dist;
    if (o.specular_roughness) o.specular_roughness[i] = s.mat[6];
    if (o.uv) { o.uv[2 * i] = s.uvx; o.uv[2 * i + 1] = s.uvy; }
    if (o.hole) o.hole[i] = s.hole ? 1 : 0;
}

}  // namespace iron
