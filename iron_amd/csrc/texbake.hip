// Material texture baking (models/export_materials.py's sample_surface + accumulate_splat_material + the final normalisation;
// DESIGN.md row f-5).  Conventions: include/iron_hip.h, iron_bake_* block.
//
// Counts (iron_bake_count), one thread per face, 256-face blocks:
//   k_bake_area     fp32 area |cross(v0 - v2, v1 - v2)| -> area[f]; fp64 partial sums per block -> part[b]
//   k_bake_sum      one block sums the partials (fixed_sum.h) -> the normaliser (rounded to fp32 like the reference's sum)
//   k_bake_count    cnt[f] = ceil(n * (area / sum)) in fp32; pair[f] = (cnt, cnt > 0)
//   pair_scan       exclusive scan of the pairs (pair_scan.h); the top level holds the totals: sum(cnt) and the number of faces
//                   with a sample
//   k_bake_compact  list of the faces with cnt > 0 (the reference's np.where(cnt > 0))
//   k_bake_draw     floor_num = sum(cnt) - n draws with replacement among them (Philox, stream 0), each setting an idempotent flag
//                   on its face: a face drawn twice loses one sample, like numpy's `cnt[idx] -= 1`
//   k_bake_sub      cnt -= flag; pair[f] = (cnt, 0); scan again -> per-face sample offsets, total on top
// Sampling (iron_bake_sample): one thread per sample; its face is the last face whose offset is <= the sample index (binary
// search); r1, r2 from Philox stream 1; the point and uv in fp64 in the reference's operation order, then rounded to fp32.
// Splat (iron_bake_splat): 16 lanes per sample, one per accumulator channel, so one atomic wave-instruction adds 4 rows of
// (C + 1) int64.  The taps follow the reference's fp32 arithmetic; every term is w * value in fp64, rounded to an integer number
// of 2^-24 units; integer adds are associative, so the accumulator is the same whatever order the atomics land in.
// Resolve (iron_bake_resolve): fp32 texel values and acc / (w + 1e-10) in fp32, like the reference's float32 images.
#include "fixed_sum.h"
#include "mesh_common.h"
#include "pair_scan.h"

namespace iron {

constexpr int kBkBlock = 256;
constexpr double kBkScale = 16777216.0;  // 2^24 fixed-point units per 1.0
constexpr int kBkLanes = 16;             // lanes per sample in the splat

// ---- Philox4x32-10 (Salmon et al., SC'11), counter (index lo, index hi, round, stream), key = seed ----
__device__ __forceinline__ uint4 philox(uint64_t seed, uint64_t index, uint32_t round, uint32_t stream) {
    uint32_t c0 = (uint32_t)index, c1 = (uint32_t)(index >> 32), c2 = round, c3 = stream;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ double unit53(uint32_t lo, uint32_t hi) {  // [0, 1) with 53 random bits
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return (double)(x >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(kBkBlock) void k_bake_area(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces,
                                                        const int32_t* __restrict__ fuv, int64_t nuv, int64_t nf,
                                                        float* __restrict__ area, double* __restrict__ part, int32_t* __restrict__ bad) {
    __shared__ double s[kBkBlock];
    const int64_t f = (int64_t)blockIdx.x * kBkBlock + threadIdx.x;
    float a = 0.0f;
    if (f < nf) {
        const int32_t* t = faces + 3 * f;
        if (face_in_range(t, nv) && face_in_range(fuv + 3 * f, nuv)) {
            const float* p0 = v + 3 * (int64_t)t[0];
            const float* p1 = v + 3 * (int64_t)t[1];
            const float* p2 = v + 3 * (int64_t)t[2];
            const float ax = p0[0] - p2[0], ay = p0[1] - p2[1], az = p0[2] - p2[2];
            const float bx = p1[0] - p2[0], by = p1[1] - p2[1], bz = p1[2] - p2[2];
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;  // np.cross, no contraction
            a = sqrtf(cx * cx + cy * cy + cz * cz);
            a = a == a ? a : 0.0f;
        } else {
            *bad = 1;
        }
        area[f] = a;
    }
    const double r = fixed_sum::block_sum<kBkBlock>((double)a, s);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(1024) void k_bake_sum(const double* __restrict__ part, int64_t n, float* __restrict__ sum) {
    __shared__ double s[1024];
    const double r = fixed_sum::slot_sum<1024>(part, n, 1, s);
    if (threadIdx.x == 0) *sum = (float)r;
}

__global__ void k_bake_count(const float* __restrict__ area, const float* __restrict__ sum, int64_t nf, float n_samples,
                             int32_t* __restrict__ cnt, Pair64* __restrict__ pair) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const float s = *sum;
    int32_t c = 0;
    if (s > 0.0f) {
        const float x = ceilf(n_samples * (area[f] / s));
        c = x > 0.0f ? (int32_t)x : 0;
    }
    cnt[f] = c;
    pair[f] = Pair64{c, c > 0 ? 1 : 0};
}

__global__ void k_bake_compact(const int32_t* __restrict__ cnt, const Pair64* __restrict__ pair, int64_t nf, int32_t* __restrict__ pos,
                               uint8_t* __restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    flag[f] = 0;
    if (cnt[f] > 0) pos[pair[f].b] = (int32_t)f;
}

__global__ void k_bake_draw(const int32_t* __restrict__ pos, const Pair64* __restrict__ tot, int64_t n_samples, uint64_t seed,
                            uint32_t round, uint8_t* __restrict__ flag) {
    const int64_t floor_num = tot->a - n_samples, n_pos = tot->b;
    if (n_pos <= 0) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < floor_num; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 r = philox(seed, (uint64_t)i, round, 0u);
        const uint64_t x = ((uint64_t)r.y << 32) | r.x;
        const int64_t j = (int64_t)__umul64hi(x, (uint64_t)n_pos);  // uniform in [0, n_pos)
        flag[pos[j]] = 1;
    }
}

__global__ void k_bake_sub(int32_t* __restrict__ cnt, const uint8_t* __restrict__ flag, int64_t nf, Pair64* __restrict__ pair) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int32_t c = cnt[f] - (int32_t)flag[f];
    cnt[f] = c;
    pair[f] = Pair64{c, 0};
}

// P = (1 - sqrt(r1)) A + sqrt(r1) (1 - r2) B + sqrt(r1) r2 C in the reference's fp64 order, rounded to fp32
__device__ __forceinline__ void bary_point(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int d,
                                           double r1, double r2, float* __restrict__ out) {
    const double sq = sqrt(r1);
    const double wa = 1.0 - sq, wb = sq * (1.0 - r2), wc = sq * r2;
    for (int k = 0; k < d; ++k) out[k] = (float)(wa * (double)a[k] + wb * (double)b[k] + wc * (double)c[k]);
}

__device__ __forceinline__ void emit_sample(const float* __restrict__ v, const int32_t* __restrict__ faces, const float* __restrict__ uvs,
                                            const int32_t* __restrict__ fuv, int64_t f, double r1, double r2, int64_t s,
                                            float* __restrict__ pts, float* __restrict__ uv) {
    const int32_t* t = faces + 3 * f;
    const int32_t* tu = fuv + 3 * f;
    bary_point(v + 3 * (int64_t)t[0], v + 3 * (int64_t)t[1], v + 3 * (int64_t)t[2], 3, r1, r2, pts + 3 * s);
    bary_point(uvs + 2 * (int64_t)tu[0], uvs + 2 * (int64_t)tu[1], uvs + 2 * (int64_t)tu[2], 2, r1, r2, uv + 2 * s);
}

__global__ void k_bake_sample(const float* __restrict__ v, const int32_t* __restrict__ faces, const float* __restrict__ uvs,
                              const int32_t* __restrict__ fuv, const Pair64* __restrict__ offs, int64_t nf, int64_t total, uint64_t seed,
                              uint32_t round, float* __restrict__ pts, float* __restrict__ uv, int32_t* __restrict__ face_out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= total) return;
    int64_t lo = 0, hi = nf;  // first face whose offset is > s, minus one
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid].a <= s) lo = mid + 1; else hi = mid;
    }
    const int64_t f = lo - 1;  // >= 0: offs[0] = 0 <= s
    const uint4 r = philox(seed, (uint64_t)s, round, 1u);
    emit_sample(v, faces, uvs, fuv, f, unit53(r.x, r.y), unit53(r.z, r.w), s, pts, uv);
    if (face_out) face_out[s] = (int32_t)f;
}

__global__ void k_bake_sample_explicit(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ faces, const float* __restrict__ uvs,
                                       int64_t nuv, const int32_t* __restrict__ fuv, int64_t nf, const int32_t* __restrict__ face_idx,
                                       const double* __restrict__ r1, const double* __restrict__ r2, int64_t n, float* __restrict__ pts,
                                       float* __restrict__ uv) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t f = face_idx[s];
    if (f < 0 || f >= nf || !face_in_range(faces + 3 * f, nv) || !face_in_range(fuv + 3 * f, nuv)) {
        const float q = __builtin_nanf("");
        pts[3 * s] = pts[3 * s + 1] = pts[3 * s + 2] = q;
        uv[2 * s] = uv[2 * s + 1] = q;
        return;
    }
    emit_sample(v, faces, uvs, fuv, f, r1[s], r2[s], s, pts, uv);
}

// ---- splat ----
// One tap of accumulate_splat_material: label (or -1 when the flat label leaves [0, H*W)) and weight, in the reference's fp32
// arithmetic: u = uv_x * W, v = H - uv_y * H, shifted by the tap, floor, label = row * W + col (fp32), weight
// exp(-((u - col - 0.5)^2 + (v - row - 0.5)^2) / 2).
__device__ __forceinline__ int64_t splat_tap(float u, float v, int tap, int H, int W, float* w) {
    if (tap == 1) v = v - 1.0f;
    else if (tap == 2) u = u + 1.0f;
    else if (tap == 3) v = v + 1.0f;
    else if (tap == 4) u = u - 1.0f;
    const float col = floorf(u), row = floorf(v);
    const float lab = row * (float)W + col;
    if (!(lab >= 0.0f && lab < (float)H * (float)W)) return -1;  // NaN / inf drop too
    const float du = (u - col) - 0.5f, dv = (v - row) - 0.5f;
    *w = expf(-(du * du + dv * dv) / 2.0f);
    return (int64_t)lab;
}

__global__ __launch_bounds__(256) void k_bake_splat(const float* __restrict__ uv, const float* __restrict__ va, int32_t ca,
                                                    const float* __restrict__ vb, int32_t cb, int64_t n, int32_t H, int32_t W,
                                                    double bound, unsigned long long* __restrict__ acc, int32_t* __restrict__ flag) {
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kBkLanes;
    const int ch0 = threadIdx.x % kBkLanes;
    if (s >= n) return;
    const int c = ca + cb, stride = c + 1;
    const float u = uv[2 * s] * (float)W;
    const float v = (float)H - uv[2 * s + 1] * (float)H;
    for (int ch = ch0; ch < stride; ch += kBkLanes) {
        const float x = ch < ca ? va[s * ca + ch] : (ch < c ? vb[s * cb + (ch - ca)] : 1.0f);
        bool bad = false;
        for (int tap = 0; tap < 5; ++tap) {
            float w;
            const int64_t lab = splat_tap(u, v, tap, H, W, &w);
            if (lab < 0) continue;
            const double t = (double)w * (double)x * kBkScale;
            if (!(fabs(t) <= bound)) { bad = true; continue; }  // NaN fails too
            atomicAdd(acc + lab * stride + ch, (unsigned long long)__double2ll_rn(t));
        }
        if (bad) *flag = 1;
    }
}

__global__ void k_bake_resolve(const long long* __restrict__ acc, int32_t c, int64_t n_texels, float* __restrict__ out,
                               float* __restrict__ weight) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_texels) return;
    const long long* a = acc + t * (c + 1);
    const float w = (float)((double)a[c] * (1.0 / kBkScale));
    const float d = w + 1e-10f;
    for (int k = 0; k < c; ++k) out[t * c + k] = (float)((double)a[k] * (1.0 / kBkScale)) / d;
    weight[t] = w;
}

// ---- workspace layout ----
struct BkLayout {
    int64_t nf, blocks;
    size_t area_off, cnt_off, pos_off, flag_off, part_off, sum_off, bad_off, bytes;
    ScanLevels scan;  // over the per-face pairs
};

static BkLayout bk_layout(int64_t nf) {
    BkLayout L{};
    L.nf = nf;
    L.blocks = (nf + kBkBlock - 1) / kBkBlock;
    Carver c;
    L.area_off = c.take(4 * (size_t)nf);
    L.cnt_off = c.take(4 * (size_t)nf);
    L.pos_off = c.take(4 * (size_t)nf);
    L.flag_off = c.take((size_t)nf);
    L.part_off = c.take(8 * (size_t)L.blocks);
    L.sum_off = c.take(8);
    L.bad_off = c.take(8);
    L.scan = scan_levels(nf, c);
    L.bytes = c.off;
    return L;
}

}  // namespace iron

using namespace iron;

extern "C" int iron_bake_workspace_bytes(int64_t n_faces, size_t* bytes) {
    if (n_faces < 0 || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = n_faces == 0 ? 0 : bk_layout(n_faces).bytes;
    return IRON_OK;
}

extern "C" int iron_bake_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_uvs,
                               const int32_t* face_uvs, int64_t n_faces, int64_t n_samples, uint64_t seed, uint32_t round, void* workspace,
                               int32_t* ceil_counts, int32_t* counts, int64_t* n_total, void* stream) {
    if (n_verts < 0 || n_uvs < 0 || n_faces < 0 || n_samples < 0 || !n_total) return IRON_ERR_BAD_ARG;
    *n_total = 0;
    if (n_faces == 0) return IRON_OK;
    if (!verts || !faces || !face_uvs || !workspace) return IRON_ERR_BAD_ARG;
    // counts are fp32 products like the reference's: n must be exact in fp32, and the per-face offsets fit int32 face indices
    if (n_samples > (1LL << 24) || n_faces >= 0x7fffffffLL) return IRON_ERR_RANGE;
    const BkLayout L = bk_layout(n_faces);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    float* area = ws_ptr<float>(ws, L.area_off);
    int32_t* cnt = ws_ptr<int32_t>(ws, L.cnt_off);
    int32_t* pos = ws_ptr<int32_t>(ws, L.pos_off);
    uint8_t* flag = ws_ptr<uint8_t>(ws, L.flag_off);
    double* part = ws_ptr<double>(ws, L.part_off);
    float* sum = ws_ptr<float>(ws, L.sum_off);
    int32_t* bad = ws_ptr<int32_t>(ws, L.bad_off);
    Pair64* pair = L.scan.level(ws, 0);
    const Pair64* tot = L.scan.level(ws, L.scan.levels);
    const unsigned grid = blocks_for(n_faces, 256);
    IRON_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    IRON_LAUNCH(k_bake_area, (unsigned)L.blocks, kBkBlock, st, verts, n_verts, faces, face_uvs, n_uvs, n_faces, area, part, bad);
    IRON_LAUNCH(k_bake_sum, 1, 1024, st, (const double*)part, L.blocks, sum);
    IRON_LAUNCH(k_bake_count, grid, 256, st, (const float*)area, (const float*)sum, n_faces, (float)n_samples, cnt, pair);
    if (ceil_counts) IRON_HIP_TRY(hipMemcpyAsync(ceil_counts, cnt, 4 * (size_t)n_faces, hipMemcpyDeviceToDevice, st));
    int rc = pair_scan(L.scan, ws, st);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_bake_compact, grid, 256, st, (const int32_t*)cnt, (const Pair64*)pair, n_faces, pos, flag);
    IRON_LAUNCH(k_bake_draw, grid, 256, st, (const int32_t*)pos, tot, n_samples, seed, round, flag);
    IRON_LAUNCH(k_bake_sub, grid, 256, st, cnt, (const uint8_t*)flag, n_faces, pair);
    rc = pair_scan(L.scan, ws, st);
    if (rc != IRON_OK) return rc;
    if (counts) IRON_HIP_TRY(hipMemcpyAsync(counts, cnt, 4 * (size_t)n_faces, hipMemcpyDeviceToDevice, st));
    struct { Pair64 t; int32_t bad; } host{};
    IRON_HIP_TRY(hipMemcpyAsync(&host.t, tot, sizeof(Pair64), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipMemcpyAsync(&host.bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    if (host.bad) return IRON_ERR_BAD_ARG;
    *n_total = host.t.a;
    return IRON_OK;
}

extern "C" int iron_bake_sample(const float* verts, const int32_t* faces, const float* uvs, const int32_t* face_uvs, int64_t n_faces,
                                uint64_t seed, uint32_t round, const void* workspace, int64_t n_total, float* points, float* uv,
                                int32_t* face_idx, void* stream) {
    if (n_faces < 0 || n_total < 0) return IRON_ERR_BAD_ARG;
    if (n_total == 0) return IRON_OK;
    if (!verts || !faces || !uvs || !face_uvs || !workspace || !points || !uv || n_faces == 0) return IRON_ERR_BAD_ARG;
    const BkLayout L = bk_layout(n_faces);
    hipStream_t st = (hipStream_t)stream;
    IRON_LAUNCH(k_bake_sample, blocks_for(n_total, 256), 256, st, verts, faces, uvs, face_uvs, L.scan.level(workspace, 0), n_faces, n_total,
                seed, round, points, uv, face_idx);
    return IRON_OK;
}

extern "C" int iron_bake_sample_explicit(const float* verts, int64_t n_verts, const int32_t* faces, const float* uvs, int64_t n_uvs,
                                         const int32_t* face_uvs, int64_t n_faces, const int32_t* face_idx, const double* r1, const double* r2,
                                         int64_t n, float* points, float* uv, void* stream) {
    if (n_verts < 0 || n_uvs < 0 || n_faces < 0 || n < 0) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!verts || !faces || !uvs || !face_uvs || !face_idx || !r1 || !r2 || !points || !uv) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    IRON_LAUNCH(k_bake_sample_explicit, blocks_for(n, 256), 256, st, verts, n_verts, faces, uvs, n_uvs, face_uvs, n_faces, face_idx, r1, r2,
                n, points, uv);
    return IRON_OK;
}

extern "C" int iron_bake_splat(const float* uv, const float* values_a, int32_t c_a, const float* values_b, int32_t c_b, int64_t n,
                               int32_t H, int32_t W, int64_t term_bound, int64_t* acc, int32_t* flag, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || c_a < 0 || c_b < 0 || c_a + c_b > 16 || term_bound <= 0) return IRON_ERR_BAD_ARG;
    if ((int64_t)H * W > (1LL << 24)) return IRON_ERR_RANGE;  // the fp32 label of the reference is exact below 2^24
    if (n == 0) return IRON_OK;
    if (!uv || !acc || !flag || (c_a && !values_a) || (c_b && !values_b)) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * 256 / kBkLanes) return IRON_ERR_RANGE;
    hipStream_t st = (hipStream_t)stream;
    IRON_LAUNCH(k_bake_splat, blocks_for(n * kBkLanes, 256), 256, st, uv, values_a, c_a, values_b, c_b, n, H, W, (double)term_bound,
                (unsigned long long*)acc, flag);
    return IRON_OK;
}

extern "C" int iron_bake_resolve(const int64_t* acc, int32_t c, int32_t H, int32_t W, const int32_t* flag, float* out, float* weight,
                                 void* stream) {
    if (H <= 0 || W <= 0 || c < 0 || c > 16 || !acc || !flag || !weight || (c && !out)) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nt = (int64_t)H * W;
    IRON_LAUNCH(k_bake_resolve, blocks_for(nt, 256), 256, st, (const long long*)acc, c, nt, out, weight);
    int32_t f = 0;
    IRON_HIP_TRY(hipMemcpyAsync(&f, flag, sizeof(f), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    return f ? IRON_ERR_RANGE : IRON_OK;
}
