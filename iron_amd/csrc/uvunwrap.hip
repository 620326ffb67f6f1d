// Face connectivity, Smart UV project and the export chain's component step (models/export_uv.py's Blender smart_project and the
// largest-component split of models/export_mesh.py).  Conventions: include/iron_hip.h, iron_mesh_* / iron_uv_* block.
//
// Connectivity (shared by UV islands and export_mesh's largest component):
//   iron_mesh_edge_keys   k_cc_keys   one thread per face: three records, key min(v) << 32 | max(v) of each edge whose two indices
//                                     differ (kNoEdge otherwise); record r belongs to face r / 3.  Checks the face (indices in
//                                     [0, n_verts), nine finite coordinates; else state->bad).
//   (caller)              sorts the keys ascending, keeping the permutation.
//   iron_mesh_components  rounds of  k_cc_hook  one thread per sorted record: every later record of its run of equal keys whose face
//                                                carries the same group is united with it: both roots are found by following parent
//                                                links (which only ever point to smaller indices), the larger root is hooked onto the
//                                                smaller by an integer atomicMin; any pair with two roots raises state->changed
//                                    k_cc_jump  one thread per face: parent = root
//                         one host wait per round reads state; the rounds stop at the first that changed nothing.  No workgroup
//                         waits on another: visibility across workgroups comes from the kernel boundaries and the integer atomics
//                         (a stale parent read inside a round is an older ancestor, still inside the component).  The root of each
//                         component is its smallest face index, so the result does not depend on the schedule.
// Smart UV project (iron_uv_projections; the rest of the algorithm is in iron_amd/uv_unwrap.py):
//   k_uv_geometry  one thread per face: n = cross(v1 - v0, v2 - v0) / |.|, a = |.| (fp32); the largest-area face (ties: smallest
//                  index) by a block min of (ord(-a), f) and one 64-bit atomicMin per block
//   per projection normal k:  k_uv_cone     tags the untagged non-degenerate faces with n.seed > cos(limit / 2); per-block sums of
//                                           their normals in a fixed tree order (no float atomics)
//                             k_uv_cone_sum one block: the partials in a fixed order -> P[k] = normalize(sum)
//                             k_uv_farthest the running max of n.p per untagged face, argmin of (ord(max), f) per block, one 64-bit
//                                           atomicMin per block; the host reads it (one wait per normal) and stops when no face is
//                                           untagged or the minimum is >= cos(limit)
//   k_uv_assign    g(f) = argmax_p n.p (ties: the smallest p); degenerate faces (a == 0) take 0.
//   iron_uv_project  k_uv_project  one thread per vt: (x.t, x.b) in the basis of its island's normal
//   iron_uv_rotation_search  k_uv_rot_boxes  one thread per vt, per candidate angle the rotated point; min / max per (island, angle)
//                                            by integer atomics on order-preserving bits, pre-reduced across the wave when the
//                                            wave's vts all lie in one island (vts are sorted by island)
//   iron_uv_apply  k_uv_apply  one thread per vt: rotate, subtract the box minimum, offset, scale, clamp to [0, 1].
#include <cstring>

#include "host_util.h"
#include "mesh_common.h"

namespace iron {

constexpr int kUvBlock = 256;
constexpr uint64_t kNoEdge = 0x7fffffffffffffffull;  // the largest signed int64: a device sort of int64 keys puts it last
constexpr uint64_t kNoFace = 0xffffffffffffffffull;

struct UvState {
    uint64_t best;    // argmin word (ord(value) << 32 | face)
    int32_t bad;      // a face indexes outside the vertices or references a non-finite coordinate
    int32_t changed;  // a hook round found two roots
};

__device__ __forceinline__ float uv_dot(float ax, float ay, float az, const float* __restrict__ p) {
    return ax * p[0] + ay * p[1] + az * p[2];
}

// the face's indices and three vertices; false when an index is out of range or a coordinate is not finite
__device__ __forceinline__ bool uv_face(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t f, int32_t* idx,
                                        float* p) {
    idx[0] = faces[3 * f]; idx[1] = faces[3 * f + 1]; idx[2] = faces[3 * f + 2];
    if (!face_in_range(idx, nv)) return false;
    bool ok = true;
    for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d) {
            p[3 * c + d] = v[3 * (int64_t)idx[c] + d];
            ok = ok && isfinite(p[3 * c + d]);
        }
    return ok;
}

__device__ __forceinline__ void block_min_u64(uint64_t x, uint64_t* dst) {
    __shared__ uint64_t s[kUvBlock];
    s[threadIdx.x] = x;
    __syncthreads();
    for (int h = kUvBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) s[threadIdx.x] = min(s[threadIdx.x], s[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0] != kNoFace) atomicMin((unsigned long long*)dst, (unsigned long long)s[0]);
}

// ---- connectivity ----
__global__ __launch_bounds__(kUvBlock) void k_cc_keys(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                                                       uint64_t* __restrict__ keys, UvState* st) {
    const int64_t f = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    if (f >= nf) return;
    int32_t i[3];
    float p[9];
    const bool ok = uv_face(v, nv, faces, f, i, p);
    if (!ok) atomicOr(&st->bad, 1);
    for (int e = 0; e < 3; ++e) {
        const int32_t a = i[e], b = i[(e + 1) % 3];
        uint64_t k = kNoEdge;
        if (ok && a != b) k = ((uint64_t)(uint32_t)min(a, b) << 32) | (uint64_t)(uint32_t)max(a, b);
        keys[3 * f + e] = k;
    }
}

__global__ void k_cc_init(int32_t* __restrict__ parent, int64_t nf) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nf) parent[f] = (int32_t)f;
}

__device__ __forceinline__ int32_t cc_root(const int32_t* parent, int32_t x) {
    for (;;) {  // parent[x] <= x always, and strictly smaller off a root: the walk ends
        const int32_t p = parent[x];
        if (p == x) return x;
        x = p;
    }
}

__global__ __launch_bounds__(kUvBlock) void k_cc_hook(const uint64_t* __restrict__ keys, const int64_t* __restrict__ perm, int64_t n,
                                                       const int32_t* __restrict__ group, int32_t* parent, UvState* st) {
    const int64_t r = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    if (r >= n) return;
    const uint64_t k = keys[r];
    if (k == kNoEdge) return;
    const int32_t fa = (int32_t)(perm[r] / 3);
    const int32_t ga = group ? group[fa] : 0;
    bool changed = false;
    for (int64_t j = r + 1; j < n && keys[j] == k; ++j) {  // every later member of the run (a non-manifold edge has more than two)
        const int32_t fb = (int32_t)(perm[j] / 3);
        if (fb == fa || (group && group[fb] != ga)) continue;
        const int32_t ra = cc_root(parent, fa), rb = cc_root(parent, fb);
        if (ra == rb) continue;
        atomicMin(parent + max(ra, rb), min(ra, rb));
        changed = true;
    }
    if (changed) atomicOr(&st->changed, 1);
}

__global__ void k_cc_jump(int32_t* parent, int64_t nf) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    parent[f] = cc_root(parent, (int32_t)f);
}

// ---- smart UV project: projection normals ----
__global__ __launch_bounds__(kUvBlock) void k_uv_geometry(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces,
                                                           int64_t nf, float* __restrict__ normals, float* __restrict__ area, UvState* st) {
    const int64_t f = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    uint64_t key = kNoFace;
    if (f < nf) {
        int32_t i[3];
        float p[9];
        float nx = 0.f, ny = 0.f, nz = 0.f, a = 0.f;
        if (uv_face(v, nv, faces, f, i, p)) {
            const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
            const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
            const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
            a = sqrtf(cx * cx + cy * cy + cz * cz);
            if (a > 0.f) { nx = cx / a; ny = cy / a; nz = cz / a; }
        } else {
            atomicOr(&st->bad, 1);
        }
        normals[3 * f] = nx; normals[3 * f + 1] = ny; normals[3 * f + 2] = nz;
        area[f] = a;
        key = ((uint64_t)f2ord(-a) << 32) | (uint64_t)f;
    }
    block_min_u64(key, &st->best);
}

__global__ __launch_bounds__(kUvBlock) void k_uv_cone(const float* __restrict__ normals, const float* __restrict__ area, int64_t nf,
                                                       const UvState* st, float cos_half, int32_t k, int32_t* __restrict__ tag,
                                                       float* __restrict__ partial) {
    __shared__ float s[3][kUvBlock];
    const int64_t f = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    const int64_t seed = (int64_t)(uint32_t)st->best;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (f < nf && tag[f] < 0 && area[f] > 0.f && area[seed] > 0.f) {
        const float x = normals[3 * f], y = normals[3 * f + 1], z = normals[3 * f + 2];
        if (uv_dot(x, y, z, normals + 3 * seed) > cos_half) { tag[f] = k; nx = x; ny = y; nz = z; }
    }
    s[0][threadIdx.x] = nx; s[1][threadIdx.x] = ny; s[2][threadIdx.x] = nz;
    __syncthreads();
    for (int h = kUvBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h)
            for (int c = 0; c < 3; ++c) s[c][threadIdx.x] = s[c][threadIdx.x] + s[c][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[3 * (int64_t)blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kUvBlock) void k_uv_cone_sum(const float* __restrict__ partial, int64_t nblk, int32_t k, float* __restrict__ P) {
    __shared__ float s[3][kUvBlock];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int64_t b = threadIdx.x; b < nblk; b += kUvBlock)
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + partial[3 * b + c];
    for (int c = 0; c < 3; ++c) s[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int h = kUvBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h)
            for (int c = 0; c < 3; ++c) s[c][threadIdx.x] = s[c][threadIdx.x] + s[c][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float x = s[0][0], y = s[1][0], z = s[2][0];
        const float l = sqrtf(x * x + y * y + z * z);
        float* p = P + 3 * k;
        if (l > 0.f) { p[0] = x / l; p[1] = y / l; p[2] = z / l; }
        else { p[0] = 0.f; p[1] = 0.f; p[2] = 1.f; }  // no non-degenerate face at all
    }
}

__global__ __launch_bounds__(kUvBlock) void k_uv_farthest(const float* __restrict__ normals, const float* __restrict__ area, int64_t nf,
                                                           const float* __restrict__ P, int32_t k, const int32_t* __restrict__ tag,
                                                           float* __restrict__ runmax, UvState* st) {
    const int64_t f = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    uint64_t key = kNoFace;
    if (f < nf && tag[f] < 0 && area[f] > 0.f) {
        const float d = uv_dot(normals[3 * f], normals[3 * f + 1], normals[3 * f + 2], P + 3 * k);
        const float m = k == 0 ? d : fmaxf(runmax[f], d);
        runmax[f] = m;
        key = ((uint64_t)f2ord(m) << 32) | (uint64_t)f;
    }
    block_min_u64(key, &st->best);
}

__global__ void k_uv_assign(const float* __restrict__ normals, const float* __restrict__ area, int64_t nf, const float* __restrict__ P,
                            int32_t np, int32_t* __restrict__ group) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    int32_t g = 0;
    if (area[f] > 0.f) {
        const float x = normals[3 * f], y = normals[3 * f + 1], z = normals[3 * f + 2];
        float bd = uv_dot(x, y, z, P);
        for (int32_t p = 1; p < np; ++p) {
            const float d = uv_dot(x, y, z, P + 3 * p);
            if (d > bd) { bd = d; g = p; }
        }
    }
    group[f] = g;
}

// ---- smart UV project: charts ----
// right-handed basis (t, b, p): t = normalize(e x p), e the axis of the smallest |p_i| (ties: the lowest i), b = p x t
__device__ __forceinline__ void uv_basis(const float* __restrict__ p, float* t, float* b) {
    const float ax = fabsf(p[0]), ay = fabsf(p[1]), az = fabsf(p[2]);
    const int e = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
    float cx, cy, cz;  // e x p with e a unit axis
    if (e == 0) { cx = 0.f; cy = -p[2]; cz = p[1]; }
    else if (e == 1) { cx = p[2]; cy = 0.f; cz = -p[0]; }
    else { cx = -p[1]; cy = p[0]; cz = 0.f; }
    const float l = sqrtf(cx * cx + cy * cy + cz * cz);
    t[0] = cx / l; t[1] = cy / l; t[2] = cz / l;
    b[0] = p[1] * t[2] - p[2] * t[1];
    b[1] = p[2] * t[0] - p[0] * t[2];
    b[2] = p[0] * t[1] - p[1] * t[0];
}

__global__ void k_uv_project(const float* __restrict__ v, const int32_t* __restrict__ vt_vertex, const int32_t* __restrict__ vt_island,
                             int64_t n, const int32_t* __restrict__ island_group, const float* __restrict__ P, float* __restrict__ xy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = P + 3 * (int64_t)island_group[vt_island[i]];
    float t[3], b[3];
    uv_basis(p, t, b);
    const int64_t w = vt_vertex[i];
    const float x = v[3 * w], y = v[3 * w + 1], z = v[3 * w + 2];
    xy[2 * i] = uv_dot(x, y, z, t);
    xy[2 * i + 1] = uv_dot(x, y, z, b);
}

// boxes [n_islands][n_angles][4] = ord(-min x), ord(-min y), ord(max x), ord(max y): all four by atomicMax from zero (negation is
// exact, so -ord2f(ord(-min)) is the minimum bitwise)
__global__ __launch_bounds__(kUvBlock) void k_uv_rot_boxes(const float* __restrict__ xy, const int32_t* __restrict__ island, int64_t n,
                                                            const float* __restrict__ cs, int32_t n_angles, int32_t per_island,
                                                            uint32_t* __restrict__ boxes) {
    const int64_t i = (int64_t)blockIdx.x * kUvBlock + threadIdx.x;
    const bool valid = i < n;
    const int32_t isl = valid ? island[i] : -1;
    const int32_t isl0 = __shfl(isl, 0);
    if (isl0 < 0) return;  // lane 0 is the wave's first vt: the whole wave lies past the end
    const bool uniform = __all(!valid || isl == isl0);
    const int32_t me = valid ? isl : isl0;
    const float x = valid ? xy[2 * i] : 0.f, y = valid ? xy[2 * i + 1] : 0.f;
    const float* tab = cs + (per_island ? 2 * (int64_t)me * n_angles : 0);
    for (int32_t a = 0; a < n_angles; ++a) {
        const float c = tab[2 * a], s = tab[2 * a + 1];
        const float xr = x * c - y * s, yr = x * s + y * c;
        uint32_t w[4] = {f2ord(-xr), f2ord(-yr), f2ord(xr), f2ord(yr)};
        uint32_t* dst = boxes + 4 * ((int64_t)me * n_angles + a);
        if (uniform) {
            if (!valid) { w[0] = w[1] = w[2] = w[3] = 0u; }
            for (int o = 32; o > 0; o >>= 1)
                for (int c4 = 0; c4 < 4; ++c4) w[c4] = max(w[c4], (uint32_t)__shfl_xor((int)w[c4], o));
            if ((threadIdx.x & 63) == 0)
                for (int c4 = 0; c4 < 4; ++c4) atomicMax(dst + c4, w[c4]);
        } else if (valid) {
            for (int c4 = 0; c4 < 4; ++c4) atomicMax(dst + c4, w[c4]);
        }
    }
}

// params [n_islands][8]: cos, sin, min x, min y, max x, max y (the rotated box), offset u, offset v; swap[k] != 0 turns the island
// by +90 degrees after the rotation ((x, y) -> (-y, x)) so that its box is at least as wide as high
__global__ void k_uv_apply(const float* __restrict__ xy, const int32_t* __restrict__ island, int64_t n, const float* __restrict__ params,
                           const int32_t* __restrict__ swap, float scale, float* __restrict__ uv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t k = island[i];
    const float* q = params + 8 * k;
    const float x = xy[2 * i], y = xy[2 * i + 1];
    const float xr = x * q[0] - y * q[1], yr = x * q[1] + y * q[0];
    float u, w;
    if (swap[k]) { u = q[5] - yr; w = xr - q[2]; }
    else { u = xr - q[2]; w = yr - q[3]; }
    u = (u + q[6]) * scale;
    w = (w + q[7]) * scale;
    uv[2 * i] = fminf(fmaxf(u, 0.f), 1.f);
    uv[2 * i + 1] = fminf(fmaxf(w, 0.f), 1.f);
}

// ---- workspace of iron_uv_projections ----
struct UvLayout {
    size_t normals_off, area_off, tag_off, runmax_off, partial_off, bytes;
};

static UvLayout uv_layout(int64_t nf) {
    UvLayout L{};
    Carver c;
    L.normals_off = c.take(12 * (size_t)nf);
    L.area_off = c.take(4 * (size_t)nf);
    L.tag_off = c.take(4 * (size_t)nf);
    L.runmax_off = c.take(4 * (size_t)nf);
    L.partial_off = c.take(12 * (size_t)blocks_for(nf, kUvBlock));
    L.bytes = c.off;
    return L;
}

static int uv_read_state(UvState* st, UvState* host, hipStream_t s) {
    IRON_HIP_TRY(hipMemcpyAsync(host, st, sizeof(UvState), hipMemcpyDeviceToHost, s));
    IRON_HIP_TRY(hipStreamSynchronize(s));
    return IRON_OK;
}

}  // namespace iron

using namespace iron;

extern "C" int iron_mesh_edge_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, uint64_t* keys, void* state,
                                   void* stream) {
    if (!mesh_sizes_ok(n_verts, n_faces) || !verts || !faces || !keys || !state) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_cc_keys, blocks_for(n_faces, kUvBlock), kUvBlock, (hipStream_t)stream, verts, n_verts, faces, n_faces, keys,
                (UvState*)state);
    return IRON_OK;
}

extern "C" int iron_mesh_components(const uint64_t* sorted_keys, const int64_t* perm, int64_t n_records, const int32_t* group,
                                    int64_t n_faces, int32_t* parent, void* state, int32_t max_rounds, int32_t* rounds, void* stream) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || n_records != 3 * n_faces || !sorted_keys || !perm || !parent || !state || !rounds ||
        max_rounds < 1)
        return IRON_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    UvState* st = (UvState*)state;
    IRON_LAUNCH(k_cc_init, blocks_for(n_faces, 256), 256, s, parent, n_faces);
    *rounds = 0;
    for (int32_t r = 0; r < max_rounds; ++r) {
        IRON_HIP_TRY(hipMemsetAsync(&st->changed, 0, sizeof(int32_t), s));
        IRON_LAUNCH(k_cc_hook, blocks_for(n_records, kUvBlock), kUvBlock, s, sorted_keys, perm, n_records, group, parent, st);
        IRON_LAUNCH(k_cc_jump, blocks_for(n_faces, 256), 256, s, parent, n_faces);
        UvState h;
        const int e = uv_read_state(st, &h, s);
        if (e != IRON_OK) return e;
        *rounds = r + 1;
        if (h.bad) return IRON_ERR_BAD_ARG;
        if (!h.changed) return IRON_OK;
    }
    return IRON_ERR_RANGE;  // never a partial labelling
}

extern "C" int iron_uv_workspace_bytes(int64_t n_faces, size_t* bytes) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = uv_layout(n_faces).bytes;
    return IRON_OK;
}

extern "C" int iron_uv_projections(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float cos_half,
                                   float cos_limit, int32_t max_normals, void* workspace, void* state, float* normals_out, float* P,
                                   int32_t* group, int32_t* n_normals, int32_t* n_waits, void* stream) {
    if (!mesh_sizes_ok(n_verts, n_faces) || !verts || !faces || !workspace || !state || !P || !group || !n_normals || !n_waits ||
        max_normals < 1)
        return IRON_ERR_BAD_ARG;
    const UvLayout L = uv_layout(n_faces);
    hipStream_t s = (hipStream_t)stream;
    void* ws = workspace;
    UvState* st = (UvState*)state;
    float* nrm = ws_ptr<float>(ws, L.normals_off);
    float* area = ws_ptr<float>(ws, L.area_off);
    int32_t* tag = ws_ptr<int32_t>(ws, L.tag_off);
    float* runmax = ws_ptr<float>(ws, L.runmax_off);
    float* partial = ws_ptr<float>(ws, L.partial_off);
    const int64_t nblk = blocks_for(n_faces, kUvBlock);
    *n_normals = 0;
    *n_waits = 0;
    IRON_HIP_TRY(hipMemsetAsync(tag, 0xff, 4 * (size_t)n_faces, s));  // -1: untagged
    IRON_HIP_TRY(hipMemsetAsync(&st->best, 0xff, sizeof(uint64_t), s));
    IRON_LAUNCH(k_uv_geometry, nblk, kUvBlock, s, verts, n_verts, faces, n_faces, nrm, area, st);
    for (int32_t k = 0;; ++k) {
        if (k == max_normals) return IRON_ERR_RANGE;
        // st->best holds the seed: the largest face for k = 0, the farthest untagged face afterwards
        IRON_LAUNCH(k_uv_cone, nblk, kUvBlock, s, (const float*)nrm, (const float*)area, n_faces, (const UvState*)st, cos_half, k, tag,
                    partial);
        IRON_LAUNCH(k_uv_cone_sum, 1, kUvBlock, s, (const float*)partial, nblk, k, P);
        IRON_HIP_TRY(hipMemsetAsync(&st->best, 0xff, sizeof(uint64_t), s));
        IRON_LAUNCH(k_uv_farthest, nblk, kUvBlock, s, (const float*)nrm, (const float*)area, n_faces, (const float*)P, k,
                    (const int32_t*)tag, runmax, st);
        UvState h;
        const int e = uv_read_state(st, &h, s);
        if (e != IRON_OK) return e;
        *n_waits += 1;
        *n_normals = k + 1;
        if (h.bad) return IRON_ERR_BAD_ARG;
        if (h.best == kNoFace) break;
        uint32_t u = (uint32_t)(h.best >> 32);
        float m;
        u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        memcpy(&m, &u, sizeof(m));
        if (m >= cos_limit) break;
    }
    IRON_LAUNCH(k_uv_assign, blocks_for(n_faces, 256), 256, s, (const float*)nrm, (const float*)area, n_faces, (const float*)P, *n_normals,
                group);
    if (normals_out) IRON_HIP_TRY(hipMemcpyAsync(normals_out, nrm, 12 * (size_t)n_faces, hipMemcpyDeviceToDevice, s));
    return IRON_OK;
}

extern "C" int iron_uv_project(const float* verts, const int32_t* vt_vertex, const int32_t* vt_island, int64_t n_vt,
                               const int32_t* island_group, const float* P, float* xy, void* stream) {
    if (n_vt < 0) return IRON_ERR_BAD_ARG;
    if (n_vt == 0) return IRON_OK;
    if (!verts || !vt_vertex || !vt_island || !island_group || !P || !xy) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_uv_project, blocks_for(n_vt, 256), 256, (hipStream_t)stream, verts, vt_vertex, vt_island, n_vt, island_group, P, xy);
    return IRON_OK;
}

extern "C" int iron_uv_rotation_search(const float* xy, const int32_t* vt_island, int64_t n_vt, int64_t n_islands, const float* cs,
                                       int32_t n_angles, int32_t per_island, uint32_t* boxes, void* stream) {
    if (n_vt <= 0 || n_islands <= 0 || n_angles < 1 || !xy || !vt_island || !cs || !boxes) return IRON_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    IRON_HIP_TRY(hipMemsetAsync(boxes, 0, 16 * (size_t)n_islands * (size_t)n_angles, s));
    IRON_LAUNCH(k_uv_rot_boxes, blocks_for(n_vt, kUvBlock), kUvBlock, s, xy, vt_island, n_vt, cs, n_angles, per_island, boxes);
    return IRON_OK;
}

extern "C" int iron_uv_apply(const float* xy, const int32_t* vt_island, int64_t n_vt, const float* params, const int32_t* swap, float scale,
                             float* uv, void* stream) {
    if (n_vt < 0) return IRON_ERR_BAD_ARG;
    if (n_vt == 0) return IRON_OK;
    if (!xy || !vt_island || !params || !swap || !uv) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_uv_apply, blocks_for(n_vt, 256), 256, (hipStream_t)stream, xy, vt_island, n_vt, params, swap, scale, uv);
    return IRON_OK;
}
