// Flash render of an exported asset (mesh + baked material textures): closest-hit ray cast over the linear
// BVH of meshdist.hip, area-weighted vertex normals, the texture fetch in the bake's pixel convention, and the co-located GGX of
// ggx_core.h on the hits.  Conventions: include/iron_hip.h, iron_mesh_raycast block.
//
// Ray cast (k_raycast; the walk itself is bvh_closest_hit of ray_walk.h, which the path integrator of envlight.hip shares): one lane
// per ray, depth-first, the child with the nearer box entry first, the other on a per-lane stack in LDS (kBvStack entries, see
// bvh_common.h).
//   Triangle test: Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection" (JCGT 2013).  The vertices are translated to the
//   ray origin and sheared into the ray's space (largest direction component = z); the edge functions U, V, W are differences of two
//   products of the sheared x / y of two vertices.  An edge shared by two faces feeds the same two vertices into the same two
//   products, so the two faces compute values that are exact negatives of each other (the library is built with
//   -ffp-contract=off): a ray cannot pass between them.  An exact zero is re-decided in fp64 from the same fp32 operands (the
//   products are then exact), and a zero that remains counts as inside.  Faces are two-sided.
//   Box test: slabs with the reciprocal direction.  Every bound is moved outwards by 2^-21 (|lo| + |hi| + |o|) |1 / d| on its axis,
//   8 ulps of the operands against the ~3 the slab arithmetic and the few the triangle's own t can be off by: the test errs towards
//   visiting.  An axis whose reciprocal is not finite (zero component) passes when lo <= o <= hi, so a ray lying in a box plane
//   visits the box.  A box whose entry equals the best t is visited.
//   A face replaces the best when its t is smaller, or equal with a smaller face index: for a fixed ray, t is a function of the
//   set of faces, not of their order or of the tree.
#include "asset_common.h"
#include "ggx_core.h"
#include "ray_walk.h"

namespace iron {

__global__ __launch_bounds__(kBvQueryBlock) void k_raycast(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf,
                                                            const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t n,
                                                            float t_min, float t_max, float* __restrict__ t_out,
                                                            int32_t* __restrict__ face_idx, float* __restrict__ bary) {
    __shared__ int32_t stack[kBvStack][kBvQueryBlock];  // [depth][lane]: lane l always on bank l % 32
    const int lane = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * kBvQueryBlock + lane;
    if (q >= n) return;
    const float3 o = ld3(ray_o, q), d = ld3(ray_d, q);
    RayHit h = ray_hit_none(t_max);
    const bool valid = finite3(o) && finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f) && t_min <= t_max;  // NaN bounds fail
    if (valid) {
        RayPre r;
        ray_setup(o, d, r);
        bvh_closest_hit(nodes, tris, nf, r, t_min, -1, stack, lane, h);
    }
    const bool hit = h.face != kNoFace;
    if (hit) refine_bary(tris, o, d, h);
    t_out[q] = hit ? h.t : kInfF;
    face_idx[q] = hit ? h.face : -1;
    bary[2 * q] = hit ? h.b1 : 0.0f;
    bary[2 * q + 1] = hit ? h.b2 : 0.0f;
}

// ---- vertex normals ----
// Every face adds its un-normalised cross product (twice its area times its normal) to its three vertices.  The product is formed
// in fp64 (the differences of fp32 coordinates are exact there, so a sliver's product does not cancel).  The sums are int64 in
// units of 2^-40 of the largest cross-product component of the mesh (found first: a max, so order-free), which makes them exact
// integer sums: bitwise the same whatever the order of the atomics and of the faces.
constexpr double kVnScale = 1099511627776.0;  // 2^40: up to 2^22 faces around one vertex fit int64

__device__ __forceinline__ bool vn_face(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t f, int32_t idx[3],
                                        double c[3]) {
    idx[0] = faces[3 * f]; idx[1] = faces[3 * f + 1]; idx[2] = faces[3 * f + 2];
    if (!face_in_range(idx, nv)) return false;
    const float3 a = ld3(v, idx[0]), b = ld3(v, idx[1]), q = ld3(v, idx[2]);
    const double ex = (double)b.x - (double)a.x, ey = (double)b.y - (double)a.y, ez = (double)b.z - (double)a.z;
    const double gx = (double)q.x - (double)a.x, gy = (double)q.y - (double)a.y, gz = (double)q.z - (double)a.z;
    c[0] = ey * gz - ez * gy; c[1] = ez * gx - ex * gz; c[2] = ex * gy - ey * gx;
    return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}

__global__ __launch_bounds__(256) void k_vn_max(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                                                 unsigned long long* __restrict__ vmax) {
    __shared__ unsigned long long s[256];
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long m = 0;
    int32_t idx[3];
    double c[3];
    if (f < nf && vn_face(v, nv, faces, f, idx, c))
        m = (unsigned long long)__double_as_longlong(fmax(fmax(fabs(c[0]), fabs(c[1])), fabs(c[2])));  // >= 0: integer order
    s[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) s[threadIdx.x] = max(s[threadIdx.x], s[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0]) atomicMax(vmax, s[0]);
}

__global__ __launch_bounds__(256) void k_vn_add(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                                                 const unsigned long long* __restrict__ vmax, unsigned long long* __restrict__ acc) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int32_t idx[3];
    double c[3];
    const double m = __longlong_as_double((long long)*vmax);
    if (!(m > 0.0) || !vn_face(v, nv, faces, f, idx, c)) return;
    const double s = kVnScale / m;
    const long long q[3] = {__double2ll_rn(c[0] * s), __double2ll_rn(c[1] * s), __double2ll_rn(c[2] * s)};
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a)
            if (q[a]) atomicAdd(acc + 3 * (int64_t)idx[k] + a, (unsigned long long)q[a]);
}

__global__ void k_vn_finish(const long long* __restrict__ acc, int64_t nv, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const double x = (double)acc[3 * i], y = (double)acc[3 * i + 1], z = (double)acc[3 * i + 2];
    const double l = sqrt(x * x + y * y + z * z);
    const double s = l > 0.0 ? 1.0 / l : 0.0;
    normals[3 * i] = (float)(x * s);
    normals[3 * i + 1] = (float)(y * s);
    normals[3 * i + 2] = (float)(z * s);
}

__global__ void k_texture_fetch(const float* __restrict__ tex, const float* __restrict__ weight, int H, int W, int C,
                                const float* __restrict__ uv, int64_t n, int mode, float* __restrict__ values, uint8_t* __restrict__ hole) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float o[kTexMaxC];
    const bool hl = texture_fetch<kTexMaxC>(tex, weight, H, W, C, uv[2 * i], uv[2 * i + 1], mode, o);
#pragma unroll
    for (int c = 0; c < kTexMaxC; ++c)
        if (c < C) values[i * C + c] = o[c];
    if (hole) hole[i] = hl ? 1 : 0;
}

// ---- shading of the hits ----
struct AssetShadeArgs {
    iron_asset_mesh m;
    iron_asset_out o;
    const float *tab_trans, *tab_diff, *ray_o, *ray_d, *t, *bary;
    const int32_t* face_idx;
    float light;
    int64_t n;
};


__global__ __launch_bounds__(256) void k_asset_shade(AssetShadeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    SurfHit s;
    asset_surface(a.m, a.face_idx, a.t, a.ray_o, a.ray_d, a.bary, i, s);
    GgxOut g;
    for (int c = 0; c < 3; ++c) g.diffuse[c] = g.specular[c] = g.rgb[c] = 0.0f;
    if (s.hit) {
        const float nn[3] = {s.nrm.x, s.nrm.y, s.nrm.z}, vv[3] = {-s.d.x, -s.d.y, -s.d.z};
        ggx_colocated_point(a.light, s.dist, nn, vv, s.mat, s.mat + 3, s.mat[6], a.tab_trans, a.tab_diff, g);
    }
    st3(a.o.color, i, g.rgb[0], g.rgb[1], g.rgb[2]);
    st3(a.o.diffuse_color, i, g.diffuse[0], g.diffuse[1], g.diffuse[2]);
    st3(a.o.specular_color, i, g.specular[0], g.specular[1], g.specular[2]);
    asset_store_maps(a.o, i, s);
}

}  // namespace iron

using namespace iron;

extern "C" int iron_mesh_raycast(const void* workspace, int64_t n_faces, const float* ray_o, const float* ray_d, int64_t n_rays, float t_min,
                                 float t_max, float* t, int32_t* face_idx, float* bary, void* stream) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || n_rays < 0 || !workspace) return IRON_ERR_BAD_ARG;
    if (n_rays == 0) return IRON_OK;
    if (!ray_o || !ray_d || !t || !face_idx || !bary) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(n_faces);
    IRON_LAUNCH(k_raycast, blocks_for(n_rays, kBvQueryBlock), kBvQueryBlock, (hipStream_t)stream, ws_ptr<float4>(workspace, L.nodes_off),
                ws_ptr<float4>(workspace, L.tris_off), n_faces, ray_o, ray_d, n_rays, t_min, t_max, t, face_idx, bary);
    return IRON_OK;
}

extern "C" int iron_mesh_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float* normals,
                                        void* stream) {
    if (n_verts < 0 || n_faces < 0 || n_verts > 0x7fffffffLL || n_faces >= 0x7fffffffLL) return IRON_ERR_BAD_ARG;
    if (n_verts == 0) return IRON_OK;
    if (!verts || !normals || (n_faces > 0 && !faces)) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t acc_bytes = 24 * (size_t)n_verts;
    char* buf = nullptr;
    IRON_HIP_TRY(hipMalloc((void**)&buf, acc_bytes + 256));
    unsigned long long* vmax = (unsigned long long*)(buf + acc_bytes);
    hipError_t e = hipMemsetAsync(buf, 0, acc_bytes + 256, st);
    if (e == hipSuccess && n_faces > 0) {
        hipLaunchKernelGGL(k_vn_max, dim3(blocks_for(n_faces, 256)), dim3(256), 0, st, verts, n_verts, faces, n_faces, vmax);
        hipLaunchKernelGGL(k_vn_add, dim3(blocks_for(n_faces, 256)), dim3(256), 0, st, verts, n_verts, faces, n_faces, (const unsigned long long*)vmax,
                           (unsigned long long*)buf);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_vn_finish, dim3(blocks_for(n_verts, 256)), dim3(256), 0, st, (const long long*)buf, n_verts, normals);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(st);  // the accumulator is released below
    (void)hipFree(buf);
    if (e != hipSuccess) return hip_fail(e);
    if (e2 != hipSuccess) return hip_fail(e2);
    return IRON_OK;
}

extern "C" int iron_texture_fetch(const float* tex, const float* weight, int32_t H, int32_t W, int32_t C, const float* uv, int64_t n,
                                  int32_t mode, float* values, uint8_t* hole, void* stream) {
    if (H <= 0 || W <= 0 || C <= 0 || C > kTexMaxC || (int64_t)H * W > (1 << 24) || n < 0) return IRON_ERR_BAD_ARG;
    if (mode != IRON_TEX_BILINEAR && mode != IRON_TEX_NEAREST) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!tex || !uv || !values) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_texture_fetch, blocks_for(n, 256), 256, (hipStream_t)stream, tex, weight, H, W, C, uv, n, mode, values, hole);
    return IRON_OK;
}

extern "C" int iron_asset_shade_ggx(const iron_asset_mesh* mesh, float light, const float* tab_trans, const float* tab_diff_trans,
                                    const float* ray_o, const float* ray_d, const float* t, const int32_t* face_idx, const float* bary,
                                    int64_t n_rays, const iron_asset_out* out, void* stream) {
    if (!mesh || !out || n_rays < 0) return IRON_ERR_BAD_ARG;
    if (mesh->n_faces <= 0 || mesh->n_verts <= 0 || mesh->n_uvs <= 0 || mesh->tex_h <= 0 || mesh->tex_w <= 0 ||
        (int64_t)mesh->tex_h * mesh->tex_w > (1 << 24))
        return IRON_ERR_BAD_ARG;
    if (!mesh->verts || !mesh->faces || !mesh->uvs || !mesh->face_uvs || !mesh->material || !tab_trans || !tab_diff_trans) return IRON_ERR_BAD_ARG;
    if (n_rays == 0) return IRON_OK;
    if (!ray_o || !ray_d || !t || !face_idx || !bary) return IRON_ERR_BAD_ARG;
    AssetShadeArgs a;
    a.m = *mesh; a.o = *out;
    a.tab_trans = tab_trans; a.tab_diff = tab_diff_trans; a.ray_o = ray_o; a.ray_d = ray_d; a.t = t; a.bary = bary; a.face_idx = face_idx;
    a.light = light; a.n = n_rays;
    IRON_LAUNCH(k_asset_shade, blocks_for(n_rays, 256), 256, (hipStream_t)stream, a);
    return IRON_OK;
}
