// Gradients of the hash-grid encoding (include/iron_train.h, iron_hashgrid_* block; definition and corner walk: hashgrid_common.h).
//
// Table gradients are scatters: up to 8 n contributions land on one entry, in whatever order the hardware serves them.  They are
// therefore summed as 64-bit integers (texbake.hip's scheme): every contribution is rounded ONCE, in fp64, to a whole number of
// units 2^e and added with an integer atomic; the integers are converted to fp32 once at the end.  Integer addition is
// associative and commutative, so the result is the same bit pattern from run to run and under any permutation of the points.
// The unit is chosen per call and per level from order-independent quantities only (hg::grad_unit_exp): max |dy| (an exact
// maximum, found by k_hg_absmax), n, and for the second-order pass max |g| and the level's scale.
//
//   k_hg_absmax       max |v| as its bit pattern (atomicMax on uint32: non-negative floats order like their bits; NaN sorts on top)
//   k_hg_scatter<F,SECOND>
//                     one thread per (point, level), blockIdx.y = level.
//                     first order:   acc[idx_o][f] += round(wgt_o dy[f] / unit)
//                     second order:  c_o = sum_d (g_d live_d scale) dw[o][d];  acc[idx_o][f] += round(c_o dy[f] / unit);
//                                    d_dy[f] = sum_o c_o table[idx_o][f]   (= sum_d J[f][d] g_d)
//   k_hg_scatter_pair<F>
//                     both orders in one pass: acc[idx_o][f] += round((wgt_o dy1[f] + c_o dy2[f]) / unit), c_o from (g, dy2's
//                     level) as above; one rounding and one atomic per (corner, feature) where the two calls spend two
//   k_hg_dx<F>        one thread per point, levels in order: d_x[d] = sum_l sum_f dy[l,f] J[l,f,d], one fp32 chain per axis
//   k_hg_convert<F>   acc -> fp32, every entry of d_table written (+0.0 where nothing landed); NaN everywhere when max |dy| (or
//                     max |g|) is not finite
#include "hashgrid_common.h"
#include "train_common.h"

namespace iron_train {

using namespace iron;

constexpr int kHgBlock = 256;

struct HgHead {            // first 256 bytes of the workspace
    uint32_t max_dy, max_g;
};

struct HgLayout {
    size_t head_off, acc_off, bytes;
};

static HgLayout hg_ws_layout(int64_t n_params, int F) {
    HgLayout w{};
    Carver c;
    w.head_off = c.take(sizeof(HgHead));
    w.acc_off = c.take(sizeof(int64_t) * (size_t)n_params * (size_t)F);
    w.bytes = c.off;
    return w;
}

__global__ __launch_bounds__(kHgBlock) void k_hg_absmax(const float* __restrict__ v, int64_t count, uint32_t* __restrict__ out) {
    __shared__ uint32_t s[kHgBlock];
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * kHgBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kHgBlock) {
        const uint32_t b = __float_as_uint(v[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    s[threadIdx.x] = m;
    __syncthreads();
    for (int k = kHgBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s[threadIdx.x] = s[threadIdx.x + k] > s[threadIdx.x] ? s[threadIdx.x + k] : s[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, s[0]);
}

__device__ __forceinline__ bool hg_finite_bits(uint32_t b) { return b < 0x7f800000u; }

// the bound of one contribution to level `lv` and the unit exponent that follows from it
template <bool SECOND>
__device__ __forceinline__ int hg_unit_exp(const HgHead& h, const iron_hashgrid_level& lv, int64_t n) {
    const float mdy = __uint_as_float(h.max_dy);
    const float bound = SECOND ? ((3.0f * __uint_as_float(h.max_g)) * lv.scale) * mdy : mdy;
    return hg::grad_unit_exp(bound, n);
}

template <int F, bool SECOND>
__global__ __launch_bounds__(kHgBlock) void k_hg_scatter(hg::Levels L, const float* __restrict__ x, int64_t n,
                                                         const float* __restrict__ dy, const float* __restrict__ g,
                                                         const float* __restrict__ table, const HgHead* __restrict__ head,
                                                         unsigned long long* __restrict__ acc, float* __restrict__ d_dy) {
    const int64_t p = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (p >= n) return;
    const int l = blockIdx.y;
    const iron_hashgrid_level lv = L.lv[l];
    HgHead h{};
    if (acc) h = *head;   // without a table gradient the maxima are not taken and the workspace may be absent
    const bool finite = hg_finite_bits(h.max_dy) && (!SECOND || hg_finite_bits(h.max_g));
    const double inv_unit = ldexp(1.0, -hg_unit_exp<SECOND>(h, lv, n));
    const float xs[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
    hg::Walk k;
    hg::walk(lv, xs, &k);
    const int64_t width = (int64_t)L.n_levels * F;
    const int64_t col = p * width + (int64_t)l * F;
    float v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = dy[col + f];
    float coef[8];
    if constexpr (SECOND) {
        float gs[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) gs[d] = (g[3 * p + d] * k.live[d]) * lv.scale;
#pragma unroll
        for (int o = 0; o < 8; ++o) coef[o] = fmaf(gs[2], k.dw[o][2], fmaf(gs[1], k.dw[o][1], gs[0] * k.dw[o][0]));
        if (d_dy) {
            const float* base = table + lv.offset * F;
            float row[8][F];
#pragma unroll
            for (int o = 0; o < 8; ++o) hg::load_row<F>(base + (int64_t)k.idx[o] * F, row[o]);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) s = fmaf(coef[o], row[o][f], s);
                d_dy[col + f] = s;
            }
        }
    } else {
#pragma unroll
        for (int o = 0; o < 8; ++o) coef[o] = k.wgt[o];
    }
    if (!acc || !finite) return;
    unsigned long long* a = acc + lv.offset * F;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long long q = __double2ll_rn(((double)coef[o] * (double)v[f]) * inv_unit);
            if (q != 0) atomicAdd(a + (int64_t)k.idx[o] * F + f, (unsigned long long)q);
        }
    }
}

template <int F>
__global__ __launch_bounds__(kHgBlock) void k_hg_dx(hg::Levels L, const float* __restrict__ x, int64_t n, const float* __restrict__ dy,
                                                    const float* __restrict__ table, float* __restrict__ d_x) {
    const int64_t p = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (p >= n) return;
    const float xs[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
    const int64_t width = (int64_t)L.n_levels * F;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < L.n_levels; ++l) {
        const iron_hashgrid_level lv = L.lv[l];
        hg::Walk k;
        hg::walk(lv, xs, &k);
        const float* base = table + lv.offset * F;
        float row[8][F];
#pragma unroll
        for (int o = 0; o < 8; ++o) hg::load_row<F>(base + (int64_t)k.idx[o] * F, row[o]);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float v = dy[p * width + (int64_t)l * F + f] * lv.scale;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float vd = v * k.live[d];
#pragma unroll
                for (int o = 0; o < 8; ++o) s[d] = fmaf(vd * k.dw[o][d], row[o][f], s[d]);
            }
        }
    }
    d_x[3 * p] = s[0];
    d_x[3 * p + 1] = s[1];
    d_x[3 * p + 2] = s[2];
}

template <int F, bool SECOND>
__global__ __launch_bounds__(kHgBlock) void k_hg_convert(hg::Levels L, const HgHead* __restrict__ head, int64_t n,
                                                         const long long* __restrict__ acc, float* __restrict__ d_table) {
    const int l = blockIdx.y;
    const iron_hashgrid_level lv = L.lv[l];
    const int64_t i = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (i >= (int64_t)lv.size * F) return;
    const HgHead h = *head;
    const bool finite = hg_finite_bits(h.max_dy) && (!SECOND || hg_finite_bits(h.max_g));
    const int64_t at = lv.offset * F + i;
    d_table[at] = finite ? (float)ldexp((double)acc[at], hg_unit_exp<SECOND>(h, lv, n)) : __builtin_nanf("");
}

static unsigned hg_max_blocks(int64_t count) {
    const int64_t b = cdiv64(count, kHgBlock);
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

template <int F, bool SECOND>
static int hg_table_grad(const hg::Levels& L, int64_t n_params, const float* x, int64_t n, const float* table, const float* dy,
                         const float* g, float* d_dy, float* d_table, void* ws, hipStream_t st) {
    const HgLayout w = hg_ws_layout(n_params, F);
    HgHead* head = ws_ptr<HgHead>(ws, w.head_off);
    long long* acc = d_table ? ws_ptr<long long>(ws, w.acc_off) : nullptr;
    const int64_t width = (int64_t)L.n_levels * F;
    if (d_table) {
        IRON_TRAIN_HIP(hipMemsetAsync(head, 0, sizeof(HgHead), st));
        IRON_TRAIN_HIP(hipMemsetAsync(acc, 0, sizeof(int64_t) * (size_t)n_params * F, st));
        IRON_TRAIN_LAUNCH(k_hg_absmax, hg_max_blocks(n * width), kHgBlock, st, dy, n * width, &head->max_dy);
        if (SECOND) IRON_TRAIN_LAUNCH(k_hg_absmax, hg_max_blocks(n * 3), kHgBlock, st, g, n * 3, &head->max_g);
    }
    if (d_table || (SECOND && d_dy)) {
        const dim3 grid(blocks_for(n, kHgBlock), (unsigned)L.n_levels);
        IRON_TRAIN_LAUNCH((k_hg_scatter<F, SECOND>), grid, kHgBlock, st, L, x, n, dy, g, table, (const HgHead*)head,
                          (unsigned long long*)acc, d_dy);
    }
    if (d_table) {
        uint32_t top = 0;
        for (int l = 0; l < L.n_levels; ++l) top = L.lv[l].size > top ? L.lv[l].size : top;
        const dim3 grid(blocks_for((int64_t)top * F, kHgBlock), (unsigned)L.n_levels);
        IRON_TRAIN_LAUNCH((k_hg_convert<F, SECOND>), grid, kHgBlock, st, L, (const HgHead*)head, n, (const long long*)acc, d_table);
    }
    return IRON_OK;
}

template <int F>
static int hg_backward(const hg::Levels& L, int64_t n_params, const float* x, int64_t n, const float* table, const float* dy,
                       float* d_table, float* d_x, void* ws, hipStream_t st) {
    if (d_table) {
        const int rc = hg_table_grad<F, false>(L, n_params, x, n, table, dy, nullptr, nullptr, d_table, ws, st);
        if (rc != IRON_OK) return rc;
    }
    if (d_x) IRON_TRAIN_LAUNCH(k_hg_dx<F>, blocks_for(n, kHgBlock), kHgBlock, st, L, x, n, dy, table, d_x);
    return IRON_OK;
}

// ---- both orders in one pass (iron_hashgrid_backward_pair): one rounding and one atomic per (corner, feature) ----
struct HgPairHead {        // first 256 bytes of the workspace
    uint32_t max_dy1, max_dy2, max_g;
};

__device__ __forceinline__ bool hg_pair_finite(const HgPairHead& h) {
    return hg_finite_bits(h.max_dy1) && hg_finite_bits(h.max_dy2) && hg_finite_bits(h.max_g);
}

// one contribution is wgt_o dy1 + c_o dy2: the first-order bound plus the second-order bound of the level
__device__ __forceinline__ int hg_pair_unit_exp(const HgPairHead& h, const iron_hashgrid_level& lv, int64_t n) {
    const float first = __uint_as_float(h.max_dy1);
    const float second = ((3.0f * __uint_as_float(h.max_g)) * lv.scale) * __uint_as_float(h.max_dy2);
    return hg::grad_unit_exp(first + second, n);
}

template <int F>
__global__ __launch_bounds__(kHgBlock) void k_hg_scatter_pair(hg::Levels L, const float* __restrict__ x, int64_t n,
                                                              const float* __restrict__ dy1, const float* __restrict__ dy2,
                                                              const float* __restrict__ g, const HgPairHead* __restrict__ head,
                                                              unsigned long long* __restrict__ acc) {
    const int64_t p = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (p >= n) return;
    const iron_hashgrid_level lv = L.lv[blockIdx.y];
    const HgPairHead h = *head;
    if (!hg_pair_finite(h)) return;
    const double inv_unit = ldexp(1.0, -hg_pair_unit_exp(h, lv, n));
    const float xs[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
    hg::Walk k;
    hg::walk(lv, xs, &k);
    const int64_t col = p * ((int64_t)L.n_levels * F) + (int64_t)blockIdx.y * F;
    float v1[F], v2[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        v1[f] = dy1[col + f];
        v2[f] = dy2[col + f];
    }
    float gs[3];                                  // the coefficient of k_hg_scatter<F, true>, bit for bit
#pragma unroll
    for (int d = 0; d < 3; ++d) gs[d] = (g[3 * p + d] * k.live[d]) * lv.scale;
    unsigned long long* a = acc + lv.offset * F;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const float coef = fmaf(gs[2], k.dw[o][2], fmaf(gs[1], k.dw[o][1], gs[0] * k.dw[o][0]));
#pragma unroll
        for (int f = 0; f < F; ++f) {
            // both products are exact in fp64; their sum is rounded there once (2^-53) and then to the unit
            const double t = fma((double)k.wgt[o], (double)v1[f], (double)coef * (double)v2[f]);
            const long long q = __double2ll_rn(t * inv_unit);
            if (q != 0) atomicAdd(a + (int64_t)k.idx[o] * F + f, (unsigned long long)q);
        }
    }
}

template <int F>
__global__ __launch_bounds__(kHgBlock) void k_hg_convert_pair(hg::Levels L, const HgPairHead* __restrict__ head, int64_t n,
                                                              const long long* __restrict__ acc, float* __restrict__ d_table) {
    const iron_hashgrid_level lv = L.lv[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (i >= (int64_t)lv.size * F) return;
    const HgPairHead h = *head;
    const int64_t at = lv.offset * F + i;
    d_table[at] = hg_pair_finite(h) ? (float)ldexp((double)acc[at], hg_pair_unit_exp(h, lv, n)) : __builtin_nanf("");
}

template <int F>
static int hg_table_grad_pair(const hg::Levels& L, int64_t n_params, const float* x, int64_t n, const float* dy1, const float* dy2,
                              const float* g, float* d_table, void* ws, hipStream_t st) {
    const HgLayout w = hg_ws_layout(n_params, F);
    HgPairHead* head = ws_ptr<HgPairHead>(ws, w.head_off);
    long long* acc = ws_ptr<long long>(ws, w.acc_off);
    const int64_t width = (int64_t)L.n_levels * F;
    IRON_TRAIN_HIP(hipMemsetAsync(head, 0, sizeof(HgPairHead), st));
    IRON_TRAIN_HIP(hipMemsetAsync(acc, 0, sizeof(int64_t) * (size_t)n_params * F, st));
    IRON_TRAIN_LAUNCH(k_hg_absmax, hg_max_blocks(n * width), kHgBlock, st, dy1, n * width, &head->max_dy1);
    IRON_TRAIN_LAUNCH(k_hg_absmax, hg_max_blocks(n * width), kHgBlock, st, dy2, n * width, &head->max_dy2);
    IRON_TRAIN_LAUNCH(k_hg_absmax, hg_max_blocks(n * 3), kHgBlock, st, g, n * 3, &head->max_g);
    const dim3 grid(blocks_for(n, kHgBlock), (unsigned)L.n_levels);
    IRON_TRAIN_LAUNCH(k_hg_scatter_pair<F>, grid, kHgBlock, st, L, x, n, dy1, dy2, g, (const HgPairHead*)head, (unsigned long long*)acc);
    uint32_t top = 0;
    for (int l = 0; l < L.n_levels; ++l) top = L.lv[l].size > top ? L.lv[l].size : top;
    const dim3 cgrid(blocks_for((int64_t)top * F, kHgBlock), (unsigned)L.n_levels);
    IRON_TRAIN_LAUNCH(k_hg_convert_pair<F>, cgrid, kHgBlock, st, L, (const HgPairHead*)head, n, (const long long*)acc, d_table);
    return IRON_OK;
}

static size_t hg_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n) {
    hg::Levels L;
    int64_t n_params = 0;
    if (n < 0 || hg::make_levels(desc, &L, &n_params) != IRON_OK) return 0;
    return hg_ws_layout(n_params, L.n_features).bytes;
}

}  // namespace iron_train

using namespace iron_train;

extern "C" int iron_hashgrid_grad_unit_exp(float bound, int64_t n) { return hg::grad_unit_exp(bound, n); }

extern "C" size_t iron_hashgrid_backward_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n) { return hg_workspace_bytes(desc, n); }

extern "C" size_t iron_hashgrid_backward_backward_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n) {
    return hg_workspace_bytes(desc, n);
}

extern "C" int iron_hashgrid_backward(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table_or_null,
                                      const float* dy, float* d_table_or_null, float* d_x_or_null, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    hg::Levels L;
    int64_t n_params = 0;
    const int rc = hg::make_levels(desc, &L, &n_params);
    if (rc != IRON_OK) return rc;
    if (n < 0) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * kHgBlock / (3 * L.n_levels * L.n_features)) return IRON_ERR_RANGE;
    const int F = L.n_features;
    hipStream_t st = (hipStream_t)stream;
    if (d_table_or_null) {
        if (!workspace) return IRON_ERR_BAD_ARG;
        if (workspace_bytes < hg_ws_layout(n_params, F).bytes) return IRON_ERR_WORKSPACE;
    }
    if (n == 0) {
        if (d_table_or_null) IRON_TRAIN_HIP(hipMemsetAsync(d_table_or_null, 0, sizeof(float) * (size_t)n_params * F, st));
        return IRON_OK;
    }
    if (!x || !dy || (d_x_or_null && !table_or_null)) return IRON_ERR_BAD_ARG;
    switch (F) {
        case 1: return hg_backward<1>(L, n_params, x, n, table_or_null, dy, d_table_or_null, d_x_or_null, workspace, st);
        case 2: return hg_backward<2>(L, n_params, x, n, table_or_null, dy, d_table_or_null, d_x_or_null, workspace, st);
        case 4: return hg_backward<4>(L, n_params, x, n, table_or_null, dy, d_table_or_null, d_x_or_null, workspace, st);
        default: return hg_backward<8>(L, n_params, x, n, table_or_null, dy, d_table_or_null, d_x_or_null, workspace, st);
    }
}

extern "C" size_t iron_hashgrid_backward_pair_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n) {
    return hg_workspace_bytes(desc, n);
}

extern "C" int iron_hashgrid_backward_pair(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table_or_null,
                                           const float* dy1, const float* dy2, const float* g, float* d_table, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    (void)table_or_null;   // the table term of either order does not read the table
    hg::Levels L;
    int64_t n_params = 0;
    const int rc = hg::make_levels(desc, &L, &n_params);
    if (rc != IRON_OK) return rc;
    if (n < 0 || !d_table || !workspace) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * kHgBlock / (3 * L.n_levels * L.n_features)) return IRON_ERR_RANGE;
    const int F = L.n_features;
    hipStream_t st = (hipStream_t)stream;
    if (workspace_bytes < hg_ws_layout(n_params, F).bytes) return IRON_ERR_WORKSPACE;
    if (n == 0) {
        IRON_TRAIN_HIP(hipMemsetAsync(d_table, 0, sizeof(float) * (size_t)n_params * F, st));
        return IRON_OK;
    }
    if (!x || !dy1 || !dy2 || !g) return IRON_ERR_BAD_ARG;
    switch (F) {
        case 1: return hg_table_grad_pair<1>(L, n_params, x, n, dy1, dy2, g, d_table, workspace, st);
        case 2: return hg_table_grad_pair<2>(L, n_params, x, n, dy1, dy2, g, d_table, workspace, st);
        case 4: return hg_table_grad_pair<4>(L, n_params, x, n, dy1, dy2, g, d_table, workspace, st);
        default: return hg_table_grad_pair<8>(L, n_params, x, n, dy1, dy2, g, d_table, workspace, st);
    }
}

extern "C" int iron_hashgrid_backward_backward(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table,
                                               const float* dy, const float* g, float* d_dy_or_null, float* d_table_or_null,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    hg::Levels L;
    int64_t n_params = 0;
    const int rc = hg::make_levels(desc, &L, &n_params);
    if (rc != IRON_OK) return rc;
    if (n < 0) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * kHgBlock / (3 * L.n_levels * L.n_features)) return IRON_ERR_RANGE;
    const int F = L.n_features;
    hipStream_t st = (hipStream_t)stream;
    if (d_table_or_null) {
        if (!workspace) return IRON_ERR_BAD_ARG;
        if (workspace_bytes < hg_ws_layout(n_params, F).bytes) return IRON_ERR_WORKSPACE;
    }
    if (n == 0) {
        if (d_table_or_null) IRON_TRAIN_HIP(hipMemsetAsync(d_table_or_null, 0, sizeof(float) * (size_t)n_params * F, st));
        return IRON_OK;
    }
    if (!x || !dy || !g || (d_dy_or_null && !table)) return IRON_ERR_BAD_ARG;
    switch (F) {
        case 1: return hg_table_grad<1, true>(L, n_params, x, n, table, dy, g, d_dy_or_null, d_table_or_null, workspace, st);
        case 2: return hg_table_grad<2, true>(L, n_params, x, n, table, dy, g, d_dy_or_null, d_table_or_null, workspace, st);
        case 4: return hg_table_grad<4, true>(L, n_params, x, n, table, dy, g, d_dy_or_null, d_table_or_null, workspace, st);
        default: return hg_table_grad<8, true>(L, n_params, x, n, table, dy, g, d_dy_or_null, d_table_or_null, workspace, st);
    }
}
