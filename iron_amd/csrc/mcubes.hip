// Marching cubes over a device-resident scalar field (models/renderer.py:34-42's mcubes.marching_cubes).
// Conventions (include/iron_hip.h, iron_amd/mc_table.py): u [nx][ny][nz] fp32, z fastest; a corner is above when u > threshold
// (NaN: below); one welded vertex per crossed lattice edge, owned by its lower lattice point, ordered by (point, axis x<y<z);
// triangles ordered by (cell = its min lattice point, table order).  All orders come from prefix sums, so the output is
// bitwise deterministic.
//
// One thread per lattice point p, 256-point blocks over the linear index (z fastest: a wave reads 64 consecutive floats):
//   k_mc_count     cube index of the cell at p (0 when p is on a max face) -> cube[p]; crossed owned edges -> emask[p];
//                  per-block (vertices, triangles) -> sums[block]
//   pair_scan      exclusive scan of the block sums over all blocks, the totals on the top level (pair_scan.h)
//   k_mc_verts     in-block scan of popc(emask) -> vbase[p] and the vertex positions
//   k_mc_tris      in-block scan of the triangle counts; each active cell looks its edges' vertices up in vbase / emask
// emit reads only the crossing pattern the count left in the workspace, so every index it writes is below the counted totals.
#include "mc_table.h"
#include "pair_scan.h"

namespace iron {

constexpr int kMcBlock = 256;
static_assert(sizeof(kMcTriEdges[0]) == 3 * kMcMaxTris, "table rows are sized to the generator's maximum");

// block sums and their prefixes are Pair64 (pair_scan.h): a = vertices, b = triangles

__device__ __forceinline__ int wave_incl_scan(int x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// exclusive prefix of (a, b) over the kMcBlock threads of the block; totals of the block in *ta, *tb
__device__ __forceinline__ void block_excl_scan2(int& a, int& b, int* ta, int* tb) {
    __shared__ int sa[kMcBlock / 64], sb[kMcBlock / 64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ia = wave_incl_scan(a), ib = wave_incl_scan(b);
    if (lane == 63) { sa[w] = ia; sb[w] = ib; }
    __syncthreads();
    int oa = 0, ob = 0, suma = 0, sumb = 0;
#pragma unroll
    for (int i = 0; i < kMcBlock / 64; ++i) {
        if (i < w) { oa += sa[i]; ob += sb[i]; }
        suma += sa[i]; sumb += sb[i];
    }
    a = oa + ia - a;
    b = ob + ib - b;
    *ta = suma;
    *tb = sumb;
}

__device__ __forceinline__ bool above(float x, float thr) { return x > thr; }  // NaN: false

__global__ __launch_bounds__(kMcBlock) void k_mc_count(const float* __restrict__ u, int nx, int ny, int nz, float thr,
                                                       uint8_t* __restrict__ cube, uint8_t* __restrict__ emask, Pair64* __restrict__ sums,
                                                       int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const int64_t sy = nz, sx = (int64_t)ny * nz;
    int nv = 0, nt = 0;
    if (p < n) {
        const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / sx);
        const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
        const bool a0 = above(u[p], thr);
        const bool ax = hx && above(u[p + sx], thr), ay = hy && above(u[p + sy], thr), az = hz && above(u[p + 1], thr);
        const int m = (hx && ax != a0 ? 1 : 0) | (hy && ay != a0 ? 2 : 0) | (hz && az != a0 ? 4 : 0);
        int c = 0;
        if (hx && hy && hz) {
            c = (a0 ? 1 : 0) | (ax ? 2 : 0) | (ay ? 4 : 0) | (az ? 16 : 0);
            c |= above(u[p + sx + sy], thr) ? 8 : 0;
            c |= above(u[p + sx + 1], thr) ? 32 : 0;
            c |= above(u[p + sy + 1], thr) ? 64 : 0;
            c |= above(u[p + sx + sy + 1], thr) ? 128 : 0;
        }
        cube[p] = (uint8_t)c;
        emask[p] = (uint8_t)m;
        nv = __popc(m);
        nt = kMcTriCount[c];
    }
    int tv, tt;
    block_excl_scan2(nv, nt, &tv, &tt);
    if (threadIdx.x == 0) sums[blockIdx.x] = Pair64{tv, tt};
}

__device__ __forceinline__ float edge_t(float u0, float u1, float thr) {
    float t = (thr - u0) / (u1 - u0);
    t = t >= 0.0f ? t : 0.0f;  // NaN -> 0
    return t > 1.0f ? 1.0f : t;
}

__global__ __launch_bounds__(kMcBlock) void k_mc_verts(const float* __restrict__ u, int ny, int nz, float thr,
                                                       const uint8_t* __restrict__ emask, const Pair64* __restrict__ offs,
                                                       int32_t* __restrict__ vbase, float* __restrict__ verts, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const int m = p < n ? emask[p] : 0;
    int nv = __popc(m), dummy = 0, tv, tt;
    block_excl_scan2(nv, dummy, &tv, &tt);
    if (p >= n) return;
    const int64_t base = offs[blockIdx.x].a + nv;
    vbase[p] = (int32_t)base;
    if (!m) return;
    const int64_t sy = nz, sx = (int64_t)ny * nz;
    const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / sx);
    const float u0 = u[p];
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    int64_t v = base;
    if (m & 1) {
        float* o = verts + 3 * v++;
        o[0] = fi + edge_t(u0, u[p + sx], thr); o[1] = fj; o[2] = fk;
    }
    if (m & 2) {
        float* o = verts + 3 * v++;
        o[0] = fi; o[1] = fj + edge_t(u0, u[p + sy], thr); o[2] = fk;
    }
    if (m & 4) {
        float* o = verts + 3 * v;
        o[0] = fi; o[1] = fj; o[2] = fk + edge_t(u0, u[p + 1], thr);
    }
}

__global__ __launch_bounds__(kMcBlock) void k_mc_tris(int ny, int nz, const uint8_t* __restrict__ cube, const uint8_t* __restrict__ emask,
                                                      const int32_t* __restrict__ vbase, const Pair64* __restrict__ offs,
                                                      int32_t* __restrict__ tris, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const int c = p < n ? cube[p] : 0;
    int nt = kMcTriCount[c], dummy = 0, tv, tt;
    const int cnt = nt;
    block_excl_scan2(nt, dummy, &tv, &tt);
    if (p >= n || cnt == 0) return;
    const int64_t sy = nz, sx = (int64_t)ny * nz;
    int32_t* o = tris + 3 * (offs[blockIdx.x].b + nt);
    for (int s = 0; s < 3 * cnt; ++s) {
        const int e = kMcTriEdges[c][s], axis = e >> 2;
        const int64_t q = p + kMcEdgeOrigin[e][0] * sx + kMcEdgeOrigin[e][1] * sy + kMcEdgeOrigin[e][2];
        o[s] = vbase[q] + __popc(emask[q] & ((1u << axis) - 1u));
    }
}

// ---- workspace layout ----
struct McLayout {
    int64_t n, blocks;
    size_t cube_off, emask_off, vbase_off, bytes;
    ScanLevels scan;  // over the block sums
};

static McLayout mc_layout(int32_t nx, int32_t ny, int32_t nz) {
    McLayout L{};
    L.n = (int64_t)nx * ny * nz;
    L.blocks = (L.n + kMcBlock - 1) / kMcBlock;
    Carver c;
    L.cube_off = c.take((size_t)L.n);
    L.emask_off = c.take((size_t)L.n);
    L.vbase_off = c.take(4 * (size_t)L.n);
    L.scan = scan_levels(L.blocks, c);
    L.bytes = c.off;
    return L;
}

static inline bool mc_empty(int32_t nx, int32_t ny, int32_t nz) { return nx < 2 || ny < 2 || nz < 2; }

}  // namespace iron

using namespace iron;

extern "C" int iron_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes) {
    if (nx < 0 || ny < 0 || nz < 0 || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = mc_empty(nx, ny, nz) ? 0 : mc_layout(nx, ny, nz).bytes;
    return IRON_OK;
}

extern "C" int iron_mc_count(const float* u, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, int64_t* n_verts,
                             int64_t* n_tris, void* stream) {
    if (nx < 0 || ny < 0 || nz < 0 || !n_verts || !n_tris) return IRON_ERR_BAD_ARG;
    *n_verts = 0;
    *n_tris = 0;
    if (mc_empty(nx, ny, nz)) return IRON_OK;
    if (!u || !workspace) return IRON_ERR_BAD_ARG;
    const McLayout L = mc_layout(nx, ny, nz);
    if (L.blocks > 0x7fffffffLL) return IRON_ERR_RANGE;
    hipStream_t st = (hipStream_t)stream;
    IRON_LAUNCH(k_mc_count, (unsigned)L.blocks, kMcBlock, st, u, nx, ny, nz, threshold, ws_ptr<uint8_t>(workspace, L.cube_off),
                ws_ptr<uint8_t>(workspace, L.emask_off), L.scan.level(workspace, 0), L.n);
    const int rc = pair_scan(L.scan, workspace, st);
    if (rc != IRON_OK) return rc;
    Pair64 total{0, 0};
    IRON_HIP_TRY(hipMemcpyAsync(&total, L.scan.level(workspace, L.scan.levels), sizeof(total), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    // vbase and the triangle indices are int32; kernel-side offsets fit int64 either way
    if (total.a >= 0x7fffffffLL || total.b >= 0x7fffffffLL) return IRON_ERR_RANGE;
    *n_verts = total.a;
    *n_tris = total.b;
    return IRON_OK;
}

extern "C" int iron_mc_emit(const float* u, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, float* verts, int32_t* tris,
                            void* stream) {
    if (nx < 0 || ny < 0 || nz < 0) return IRON_ERR_BAD_ARG;
    if (mc_empty(nx, ny, nz)) return IRON_OK;
    if (!u || !workspace || !verts || !tris) return IRON_ERR_BAD_ARG;
    const McLayout L = mc_layout(nx, ny, nz);
    if (L.blocks > 0x7fffffffLL) return IRON_ERR_RANGE;
    hipStream_t st = (hipStream_t)stream;
    const Pair64* offs = L.scan.level(workspace, 0);
    const uint8_t* cube = ws_ptr<uint8_t>(workspace, L.cube_off);
    const uint8_t* emask = ws_ptr<uint8_t>(workspace, L.emask_off);
    int32_t* vbase = ws_ptr<int32_t>(workspace, L.vbase_off);
    IRON_LAUNCH(k_mc_verts, (unsigned)L.blocks, kMcBlock, st, u, ny, nz, threshold, emask, offs, vbase, verts, L.n);
    IRON_LAUNCH(k_mc_tris, (unsigned)L.blocks, kMcBlock, st, ny, nz, cube, emask, (const int32_t*)vbase, offs, tris, L.n);
    return IRON_OK;
}
