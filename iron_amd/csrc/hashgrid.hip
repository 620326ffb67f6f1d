// Multiresolution hash-grid encoding, forward and input Jacobian (include/iron_hip.h, iron_hashgrid_* block; the definition and
// the corner walk are hashgrid_common.h).
//
//   k_hg_encode<F, JAC>   one thread per (point, level): blockIdx.y is the level, so the gathers of a workgroup stay inside one
//                         level's table (at most 2^24 entries; 4 MiB at the usual 2^19 x 2 floats).  The eight corner rows are
//                         loaded first (eight independent loads of F floats in flight), then summed in corner order:
//                             y[f]    = sum_o wgt[o] row_o[f]
//                             J[f][d] = live[d] scale sum_o dw[o][d] row_o[f]
//                         Stores are point-major: F floats at a stride of L F floats for y, 3 F floats at 3 L F for J.
#include "hashgrid_common.h"
#include "host_util.h"

namespace iron {

constexpr int kHgBlock = 256;

template <int F, bool JAC>
__global__ __launch_bounds__(kHgBlock) void k_hg_encode(hg::Levels L, const float* __restrict__ x, int64_t n,
                                                        const float* __restrict__ table, float* __restrict__ y,
                                                        float* __restrict__ jac) {
    const int64_t p = (int64_t)blockIdx.x * kHgBlock + threadIdx.x;
    if (p >= n) return;
    const int l = blockIdx.y;
    const iron_hashgrid_level lv = L.lv[l];
    const float xs[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
    hg::Walk k;
    hg::walk(lv, xs, &k);
    const float* base = table + lv.offset * F;
    float row[8][F];
#pragma unroll
    for (int o = 0; o < 8; ++o) hg::load_row<F>(base + (int64_t)k.idx[o] * F, row[o]);
    const int64_t col = (int64_t)l * F;
    const int64_t width = (int64_t)L.n_levels * F;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float s = 0.0f;
#pragma unroll
        for (int o = 0; o < 8; ++o) s = fmaf(k.wgt[o], row[o][f], s);
        y[p * width + col + f] = s;
    }
    if constexpr (JAC) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) s = fmaf(k.dw[o][d], row[o][f], s);
                jac[(p * width + col + f) * 3 + d] = k.live[d] * (lv.scale * s);
            }
        }
    }
}

template <int F>
static int hg_encode(const hg::Levels& L, const float* x, int64_t n, const float* table, float* y, float* jac, hipStream_t st) {
    const dim3 grid(blocks_for(n, kHgBlock), (unsigned)L.n_levels);
    if (jac) IRON_LAUNCH((k_hg_encode<F, true>), grid, kHgBlock, st, L, x, n, table, y, jac);
    else IRON_LAUNCH((k_hg_encode<F, false>), grid, kHgBlock, st, L, x, n, table, y, jac);
    return IRON_OK;
}

}  // namespace iron

using namespace iron;

extern "C" int iron_hashgrid_layout(const iron_hashgrid_desc* desc, iron_hashgrid_level* levels_out, int64_t* n_params_out) {
    return hg::layout(desc, levels_out, n_params_out);
}

extern "C" int iron_hashgrid_encode(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table, float* y,
                                    float* jac_or_null, void* stream) {
    hg::Levels L;
    int64_t n_params = 0;
    const int rc = hg::make_levels(desc, &L, &n_params);
    if (rc != IRON_OK) return rc;
    if (n < 0) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!x || !table || !y) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * kHgBlock) return IRON_ERR_RANGE;
    hipStream_t st = (hipStream_t)stream;
    switch (L.n_features) {
        case 1: return hg_encode<1>(L, x, n, table, y, jac_or_null, st);
        case 2: return hg_encode<2>(L, x, n, table, y, jac_or_null, st);
        case 4: return hg_encode<4>(L, x, n, table, y, jac_or_null, st);
        default: return hg_encode<8>(L, x, n, table, y, jac_or_null, st);
    }
}
