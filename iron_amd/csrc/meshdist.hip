// Point-to-mesh distance over a linear BVH (evaluation/eval_mesh.py's igl.point_mesh_squared_distance).
// Conventions: include/iron_hip.h, iron_bvh_* block.
//
// Build, four steps on one stream (only the last waits on the device):
//   iron_bvh_keys   k_bvh_bounds  one thread per face: checks the face (indices in [0, n_verts), nine finite coordinates; else the
//                                 device flag), box of the face centroids by block min/max + one ordered-uint atomic per block
//                   k_bvh_keys    key = (30-bit Morton code of the centroid in that box) << 32 | face index; unique keys
//   (caller)        sort the keys ascending (not part of this file)
//   iron_bvh_hierarchy  k_bvh_karras  Karras (HPG 2012): internal node i of n-1 covers a key range, children and parent links
//   iron_bvh_boxes  k_bvh_refit   one thread per leaf: copies its triangle in leaf order, then climbs; at each internal node the
//                                 first of the two arrivals leaves (its child box published by an agent-scope release), the
//                                 second acquires, unions the two child boxes (min/max: the tree is bitwise reproducible whatever
//                                 the arrival order) and goes on to the parent
//                   then one host wait: the device flag -> IRON_ERR_BAD_ARG.
// Node and triangle records, the workspace layout and the vector helpers: bvh_common.h (shared with the ray cast of meshrender.hip).
// Query (iron_point_mesh_distance): one lane per point, depth-first; a child box whose squared-distance lower bound is <= the best
// so far is visited (so ties are visited), the nearer internal child first, the other pushed on a per-lane stack in LDS.  A face
// replaces the best when its fp32 distance is smaller, or equal with a smaller face index: the answer does not depend on the tree.
#include "bvh_common.h"

namespace iron {

// the face's three vertices; false (and zeros) when an index is out of range or a coordinate is not finite
__device__ __forceinline__ bool load_face(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t f, float3& a,
                                          float3& b, float3& c) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    a = b = c = make_float3(0.f, 0.f, 0.f);
    if (!face_in_range(i0, i1, i2, nv)) return false;
    a = ld3(v, i0); b = ld3(v, i1); c = ld3(v, i2);
    if (finite3(a) && finite3(b) && finite3(c)) return true;
    a = b = c = make_float3(0.f, 0.f, 0.f);
    return false;
}

__device__ __forceinline__ float3 centroid(float3 a, float3 b, float3 c) {
    return make_float3((a.x + b.x + c.x) * (1.0f / 3.0f), (a.y + b.y + c.y) * (1.0f / 3.0f), (a.z + b.z + c.z) * (1.0f / 3.0f));
}

__global__ __launch_bounds__(kBvBlock) void k_bvh_bounds(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                                                          BvHeader* __restrict__ hdr) {
    __shared__ uint32_t s[6][kBvBlock];
    const int64_t f = (int64_t)blockIdx.x * kBvBlock + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (f < nf) {
        float3 a, b, c;
        if (load_face(v, nv, faces, f, a, b, c)) {
            const float3 m = centroid(a, b, c);
            lo[0] = hi[0] = f2ord(m.x); lo[1] = hi[1] = f2ord(m.y); lo[2] = hi[2] = f2ord(m.z);
        } else {
            hdr->bad = 1;
        }
    }
    for (int k = 0; k < 3; ++k) { s[k][threadIdx.x] = lo[k]; s[3 + k][threadIdx.x] = hi[k]; }
    __syncthreads();
    for (int h = kBvBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h)
            for (int k = 0; k < 3; ++k) {
                s[k][threadIdx.x] = min(s[k][threadIdx.x], s[k][threadIdx.x + h]);
                s[3 + k][threadIdx.x] = max(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + h]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) atomicMin(&hdr->lo[threadIdx.x], s[threadIdx.x][0]);
    else if (threadIdx.x < 6) atomicMax(&hdr->hi[threadIdx.x - 3], s[threadIdx.x][0]);
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {  // 10 bits -> every third bit of 30
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ uint32_t cell10(float x, float lo, float hi) {
    const float e = hi - lo;
    float t = e > 0.0f ? (x - lo) / e : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);  // also maps NaN (an invalid face, flagged already) to 0
    return min((uint32_t)(t * 1024.0f), 1023u);
}

__global__ void k_bvh_keys(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                           const BvHeader* __restrict__ hdr, uint64_t* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    float3 a, b, c;
    uint32_t code = 0;
    if (load_face(v, nv, faces, f, a, b, c)) {
        const float3 m = centroid(a, b, c);
        const float lx = ord2f(hdr->lo[0]), ly = ord2f(hdr->lo[1]), lz = ord2f(hdr->lo[2]);
        const float hx = ord2f(hdr->hi[0]), hy = ord2f(hdr->hi[1]), hz = ord2f(hdr->hi[2]);
        code = (spread10(cell10(m.x, lx, hx)) << 2) | (spread10(cell10(m.y, ly, hy)) << 1) | spread10(cell10(m.z, lz, hz));
    }
    keys[f] = ((uint64_t)code << 32) | (uint64_t)(uint32_t)f;
}

// common-prefix length of keys i and j; -1 outside [0, n)
__device__ __forceinline__ int delta(const uint64_t* __restrict__ k, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(k[i] ^ k[j]));
}

__global__ void k_bvh_karras(const uint64_t* __restrict__ k, int64_t n, float4* __restrict__ nodes, int32_t* __restrict__ parent_int,
                             int32_t* __restrict__ parent_leaf) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const int d = delta(k, n, i, i + 1) > delta(k, n, i, i - 1) ? 1 : -1;
    const int dmin = delta(k, n, i, i - d);
    int64_t lmax = 2;
    while (delta(k, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(k, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(k, n, i, j);
    int64_t s = 0, t = l;
    do {  // steps ceil(l / 2), ceil(l / 4), ..., 1
        t = (t + 1) >> 1;
        if (s + t < l && delta(k, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t lo = d > 0 ? i : j, hi = d > 0 ? j : i;
    const int32_t c0 = lo == g ? ~(int32_t)g : (int32_t)g;
    const int32_t c1 = hi == g + 1 ? ~(int32_t)(g + 1) : (int32_t)(g + 1);
    float4* nd = nodes + 4 * i;
    nd[0] = make_float4(0.f, 0.f, 0.f, __int_as_float(c0));
    nd[1] = make_float4(0.f, 0.f, 0.f, __int_as_float(c1));
    nd[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    nd[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < 0) parent_leaf[g] = (int32_t)(i << 1); else parent_int[g] = (int32_t)(i << 1);
    if (c1 < 0) parent_leaf[g + 1] = (int32_t)(i << 1) | 1; else parent_int[g + 1] = (int32_t)(i << 1) | 1;
    if (i == 0) parent_int[0] = -1;
}

__global__ __launch_bounds__(kBvBlock) void k_bvh_refit(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces,
                                                         const uint64_t* __restrict__ keys, int64_t n, float4* nodes,
                                                         const int32_t* __restrict__ parent_int, const int32_t* __restrict__ parent_leaf,
                                                         int32_t* cnt, float4* __restrict__ tris) {
    const int64_t k = (int64_t)blockIdx.x * kBvBlock + threadIdx.x;
    if (k >= n) return;
    const int32_t f = (int32_t)(uint32_t)keys[k];
    float3 a, b, c;
    load_face(v, nv, faces, f, a, b, c);  // a bad face was flagged by k_bvh_bounds; zeros keep the tree well formed
    tris[3 * k] = make_float4(a.x, a.y, a.z, __int_as_float(f));
    tris[3 * k + 1] = make_float4(b.x, b.y, b.z, 0.f);
    tris[3 * k + 2] = make_float4(c.x, c.y, c.z, 0.f);
    float3 lo = make_float3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z));
    float3 hi = make_float3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z));
    int32_t pl = n > 1 ? parent_leaf[k] : -1;
    while (pl >= 0) {
        const int32_t p = pl >> 1, side = pl & 1;
        float* slot = (float*)(nodes + 4 * (int64_t)p + 2 * side);
        slot[0] = lo.x; slot[1] = lo.y; slot[2] = lo.z;
        slot[4] = hi.x; slot[5] = hi.y; slot[6] = hi.z;
        // publish the child box: agent-scope release, its stores drained, then the ticket (cdna_hip_programming.md §6 G16)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int32_t old = __hip_atomic_fetch_add(cnt + p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) return;  // the sibling's box is not there yet: its thread builds the parent
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const float4* nd = nodes + 4 * (int64_t)p;
        const float4 l0 = nd[0], h0 = nd[1], l1 = nd[2], h1 = nd[3];
        lo = make_float3(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z));
        hi = make_float3(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z));
        pl = parent_int[p];
    }
}

// ---- query ----
// closest point of segment [a, b] to p, relative to a; the end points themselves when the parameter leaves (0, 1)
__device__ __forceinline__ float3 seg_closest(float3 p, float3 a, float3 b) {
    const float3 ab = sub3(b, a);
    const float l2 = dot3(ab, ab);
    const float t = l2 > 0.0f ? dot3(sub3(p, a), ab) / l2 : 0.0f;
    if (!(t > 0.0f)) return a;
    if (t >= 1.0f) return b;
    return make_float3(a.x + t * ab.x, a.y + t * ab.y, a.z + t * ab.z);
}

__device__ __forceinline__ float dist2(float3 p, float3 c) {
    const float3 d = sub3(p, c);
    return dot3(d, d);
}

// Closest point of triangle (a, b, c) to p by Voronoi region, relative to vertex a.  Face region: the three edge functions
// (e x (p - start)) . n with n = ab x ac are all > 0 (strictly: a point on an edge or vertex goes to the boundary); then p minus its
// offset along n.  Otherwise the closest point is on the boundary: the nearest of the three segments (first on ties), which covers
// the edge and vertex regions and is also the whole rule for a degenerate triangle (n = 0: coincident or collinear vertices).
__device__ __forceinline__ float3 tri_closest(float3 p, float3 a, float3 b, float3 c, float& d2) {
    const float3 ab = sub3(b, a), ac = sub3(c, a), ap = sub3(p, a);
    const float3 n = cross3(ab, ac);
    const float nn = dot3(n, n);
    if (nn > 0.0f) {
        const float3 bc = sub3(c, b), bp = sub3(p, b), cp = sub3(p, c);
        const float ea = dot3(cross3(ab, ap), n), eb = dot3(cross3(bc, bp), n), ec = dot3(cross3(sub3(a, c), cp), n);
        if (ea > 0.0f && eb > 0.0f && ec > 0.0f) {
            const float t = dot3(ap, n) / nn;
            const float3 q = make_float3(a.x + (ap.x - t * n.x), a.y + (ap.y - t * n.y), a.z + (ap.z - t * n.z));
            d2 = dist2(p, q);
            return q;
        }
    }
    float3 q = seg_closest(p, a, b);
    d2 = dist2(p, q);
    const float3 q1 = seg_closest(p, b, c);
    const float d1 = dist2(p, q1);
    if (d1 < d2) { d2 = d1; q = q1; }
    const float3 q2 = seg_closest(p, c, a);
    const float dd = dist2(p, q2);
    if (dd < d2) { d2 = dd; q = q2; }
    return q;
}

__device__ __forceinline__ float box_d2(float3 p, float4 lo, float4 hi) {
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ void leaf_test(const float4* __restrict__ tris, int32_t k, float3 p, float& best, int32_t& bf, float3& bc) {
    const float4 ta = tris[3 * k], tb = tris[3 * k + 1], tc = tris[3 * k + 2];
    const int32_t f = __float_as_int(ta.w);
    float d2;
    const float3 q = tri_closest(p, make_float3(ta.x, ta.y, ta.z), make_float3(tb.x, tb.y, tb.z), make_float3(tc.x, tc.y, tc.z), d2);
    if (d2 < best || (d2 == best && f < bf)) { best = d2; bf = f; bc = q; }
}

__global__ __launch_bounds__(kBvQueryBlock) void k_bvh_query(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf,
                                                              const float* __restrict__ pts, int64_t np, float* __restrict__ sqr_dist,
                                                              int32_t* __restrict__ face_idx, float* __restrict__ closest) {
    __shared__ int32_t stack[kBvStack][kBvQueryBlock];  // [depth][lane]: lane l always on bank l % 32
    const int lane = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * kBvQueryBlock + lane;
    if (q >= np) return;
    const float3 p = ld3(pts, q);
    float best = __builtin_huge_valf();
    int32_t bf = -1;
    float3 bc = make_float3(0.f, 0.f, 0.f);
    if (!finite3(p)) {
        best = bc.x = bc.y = bc.z = __builtin_nanf("");
    } else if (nf == 1) {
        leaf_test(tris, 0, p, best, bf, bc);
    } else {
        int32_t node = 0, sp = 0;
        for (;;) {
            const float4* nd = nodes + 4 * (int64_t)node;
            const float4 l0 = nd[0], h0 = nd[1], l1 = nd[2], h1 = nd[3];
            const int32_t c0 = __float_as_int(l0.w), c1 = __float_as_int(h0.w);
            const float b0 = box_d2(p, l0, h0), b1 = box_d2(p, l1, h1);
            if (c0 < 0 && b0 <= best) leaf_test(tris, ~c0, p, best, bf, bc);
            if (c1 < 0 && b1 <= best) leaf_test(tris, ~c1, p, best, bf, bc);
            const bool t0 = c0 >= 0 && b0 <= best, t1 = c1 >= 0 && b1 <= best;
            if (t0 && t1) {
                const bool first1 = b1 < b0;
                if (sp < kBvStack) stack[sp++][lane] = first1 ? c0 : c1;  // never full (kBvStack above)
                node = first1 ? c1 : c0;
            } else if (t0) {
                node = c0;
            } else if (t1) {
                node = c1;
            } else {
                if (sp == 0) break;
                node = stack[--sp][lane];
            }
        }
    }
    sqr_dist[q] = best;
    face_idx[q] = bf;
    closest[3 * q] = bc.x;
    closest[3 * q + 1] = bc.y;
    closest[3 * q + 2] = bc.z;
}

}  // namespace iron

using namespace iron;

extern "C" int iron_bvh_workspace_bytes(int64_t n_faces, size_t* bytes) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = bv_layout(n_faces).bytes;
    return IRON_OK;
}

extern "C" int iron_bvh_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* workspace, uint64_t* keys,
                             void* stream) {
    if (!mesh_sizes_ok(n_verts, n_faces) || !verts || !faces || !workspace || !keys) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(n_faces);
    hipStream_t st = (hipStream_t)stream;
    BvHeader* hdr = ws_ptr<BvHeader>(workspace, L.hdr_off);
    IRON_HIP_TRY(hipMemsetAsync(workspace, 0, L.bytes, st));     // padding included: the workspace is a function of the mesh
    IRON_HIP_TRY(hipMemsetAsync(hdr->lo, 0xff, sizeof(hdr->lo), st));  // min identity of the ordered encoding
    IRON_LAUNCH(k_bvh_bounds, blocks_for(n_faces, kBvBlock), kBvBlock, st, verts, n_verts, faces, n_faces, hdr);
    IRON_LAUNCH(k_bvh_keys, blocks_for(n_faces, 256), 256, st, verts, n_verts, faces, n_faces, (const BvHeader*)hdr, keys);
    return IRON_OK;
}

extern "C" int iron_bvh_hierarchy(const uint64_t* sorted_keys, int64_t n_faces, void* workspace, void* stream) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || !sorted_keys || !workspace) return IRON_ERR_BAD_ARG;
    if (n_faces == 1) return IRON_OK;  // the root is the one leaf
    const BvLayout L = bv_layout(n_faces);
    IRON_LAUNCH(k_bvh_karras, blocks_for(n_faces - 1, 256), 256, (hipStream_t)stream, sorted_keys, n_faces,
                ws_ptr<float4>(workspace, L.nodes_off), ws_ptr<int32_t>(workspace, L.pint_off), ws_ptr<int32_t>(workspace, L.pleaf_off));
    return IRON_OK;
}

extern "C" int iron_bvh_boxes(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const uint64_t* sorted_keys,
                              void* workspace, void* stream) {
    if (!mesh_sizes_ok(n_verts, n_faces) || !verts || !faces || !workspace || !sorted_keys) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(n_faces);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    int32_t* cnt = ws_ptr<int32_t>(ws, L.cnt_off);
    IRON_HIP_TRY(hipMemsetAsync(cnt, 0, 4 * (size_t)(n_faces > 1 ? n_faces - 1 : 1), st));  // the arrival counters
    IRON_LAUNCH(k_bvh_refit, blocks_for(n_faces, kBvBlock), kBvBlock, st, verts, n_verts, faces, sorted_keys, n_faces,
                ws_ptr<float4>(ws, L.nodes_off), ws_ptr<int32_t>(ws, L.pint_off), ws_ptr<int32_t>(ws, L.pleaf_off), cnt,
                ws_ptr<float4>(ws, L.tris_off));
    int32_t bad = 0;
    IRON_HIP_TRY(hipMemcpyAsync(&bad, &ws_ptr<BvHeader>(ws, L.hdr_off)->bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    return bad ? IRON_ERR_BAD_ARG : IRON_OK;
}

extern "C" int iron_point_mesh_distance(const void* workspace, int64_t n_faces, const float* points, int64_t n_points, float* sqr_dist,
                                        int32_t* face_idx, float* closest, void* stream) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || n_points < 0 || !workspace) return IRON_ERR_BAD_ARG;
    if (n_points == 0) return IRON_OK;
    if (!points || !sqr_dist || !face_idx || !closest) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(n_faces);
    IRON_LAUNCH(k_bvh_query, blocks_for(n_points, kBvQueryBlock), kBvQueryBlock, (hipStream_t)stream,
                ws_ptr<float4>(workspace, L.nodes_off), ws_ptr<float4>(workspace, L.tris_off), n_faces, points, n_points, sqr_dist,
                face_idx, closest);
    return IRON_OK;
}
