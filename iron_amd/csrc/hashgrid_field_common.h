// What the fused hash-grid field kernels share: the plan of a validated descriptor, the LDS stage layout of the
// inference kernel, the activation and its derivative, the per-lane encode and input-gradient loops and the MFMA tile product.
// hashgrid_field.hip (inference, libiron_hip) and hashgrid_field_train.hip (backward, libiron_train) both include this file, so the
// training backward recomputes the forward with the very instructions the forward ran.
#pragma once
#include "hashgrid_common.h"
#include "mlp_core.h"

#include <type_traits>

namespace iron {

constexpr int kFieldMaxLayers = 5;    // 4 hidden + the output layer
constexpr int kFieldMaxWidth = 128;   // L F and n_neurons
constexpr int kFieldLdsTwoTiles = 64 * 1024;   // up to here a wave takes 64 points (two MFMA column tiles), above it 32
constexpr int kFieldFragAhead = 4;             // weight fragments (16 bytes per lane each) in flight ahead of the MFMAs

// What the kernels need of a validated descriptor.  Offsets into the packed blob count float4s.
struct FieldPlan {
    int32_t m, lf, neurons, n_out, act;
    int32_t in[kFieldMaxLayers], out[kFieldMaxLayers], w_off[kFieldMaxLayers];      // layer j: dims and first weight in the flat array
    int32_t kq[kFieldMaxLayers], tiles[kFieldMaxLayers], fwd_off[kFieldMaxLayers];   // forward: k quads (8 inputs each), output tiles
    int32_t tq[kFieldMaxLayers], ttiles[kFieldMaxLayers], tr_off[kFieldMaxLayers];   // transposed (layers 0 .. m-1)
    int32_t row0_off, total_f4;
    int32_t n_weights;
};

static inline int round_up(int v, int q) { return (v + q - 1) / q * q; }

static inline int make_plan(const iron_hashgrid_field_desc* d, FieldPlan* pl) {
    if (!d) return IRON_ERR_BAD_ARG;
    const int rc = hg::layout(&d->encoding, nullptr, nullptr);
    if (rc != IRON_OK) return rc;
    if (d->activation < IRON_FIELD_ACT_NONE || d->activation > IRON_FIELD_ACT_SOFTPLUS) return IRON_ERR_BAD_ARG;
    const int lf = d->encoding.n_levels * d->encoding.n_features_per_level, N = d->n_neurons;
    if (lf > kFieldMaxWidth) return IRON_ERR_RANGE;
    if (!(N == 16 || N == 32 || N == 64 || N == 128)) return IRON_ERR_RANGE;
    if (d->n_hidden_layers < 1 || d->n_hidden_layers > kFieldMaxLayers - 1) return IRON_ERR_RANGE;
    if (d->n_out < 1 || d->n_out > 16) return IRON_ERR_RANGE;
    FieldPlan p = {};
    p.m = d->n_hidden_layers; p.lf = lf; p.neurons = N; p.n_out = d->n_out; p.act = d->activation;
    int off = 0, w = 0;
    for (int j = 0; j <= p.m; ++j) {
        p.in[j] = j == 0 ? lf : N;
        p.out[j] = j == p.m ? d->n_out : N;
        p.w_off[j] = w;
        w += p.in[j] * p.out[j];
        p.kq[j] = round_up(p.in[j], 8) / 8;
        p.tiles[j] = round_up(p.out[j], 32) / 32;
        p.fwd_off[j] = off;
        off += p.tiles[j] * p.kq[j] * 64;
    }
    for (int j = 0; j < p.m; ++j) {
        p.tq[j] = round_up(p.out[j], 8) / 8;
        p.ttiles[j] = round_up(p.in[j], 32) / 32;
        p.tr_off[j] = off;
        off += p.ttiles[j] * p.tq[j] * 64;
    }
    p.row0_off = off;
    off += round_up(N, 32) / 4;
    p.total_f4 = off;
    p.n_weights = w;
    *pl = p;
    return IRON_OK;
}

// stage buffers in LDS (float offsets for P points): value only, one buffer serves every stage in place; with the gradient every
// stage 0 .. m keeps its own (the backward chain walks them in place)
struct FieldLds {
    int32_t buf[kFieldMaxLayers + 1];
};
static inline size_t lds_layout(const FieldPlan& p, bool grad, int P, FieldLds* out) {
    const int r0 = round_up(p.lf, 32), rn = round_up(p.neurons, 32);
    FieldLds L = {};
    size_t rows;
    if (grad) {
        int o = 0;
        for (int s = 0; s <= p.m; ++s) {
            L.buf[s] = o * P;
            o += s == 0 ? r0 : rn;
        }
        rows = (size_t)o;
    } else {
        rows = (size_t)(r0 > rn ? r0 : rn);          // every stage in the one buffer (offset 0)
    }
    if (out) *out = L;
    return rows * P * sizeof(float);
}

// x -> a x + b per axis, from the caller's coordinates into the unit cube of the encoding
struct FieldMap {
    float a[3], b[3];
};

// What a launch needs of a field: the levels and the plan of its descriptor, the map, the table and the packed head.  The entries
// of hashgrid_field.hip, hashgrid_field_train.hip and hashgrid_trace.hip fill one with the two helpers below; the tracer's kernels
// take it as their first argument.
struct FieldBinding {
    hg::Levels L;
    FieldPlan pl;
    FieldMap map;
    const float* table;
    const float4* packed;
};

// levels and plan of a descriptor: BAD_ARG for a null or malformed one, RANGE for a shape the kernels are not built for
static inline int field_open(const iron_hashgrid_field_desc* d, FieldBinding* F, int64_t* n_params = nullptr) {
    const int rc = make_plan(d, &F->pl);
    if (rc != IRON_OK) return rc;
    return hg::make_levels(&d->encoding, &F->L, n_params);
}

// map (a null half is the identity's), table and packed head: BAD_ARG unless both are there and the head is 16-byte aligned
static inline int field_bind(FieldBinding* F, const float* map_a3_or_null, const float* map_b3_or_null, const float* table, const void* packed) {
    if (!table || !packed || ((uintptr_t)packed & 15)) return IRON_ERR_BAD_ARG;
    for (int d = 0; d < 3; ++d) {
        F->map.a[d] = map_a3_or_null ? map_a3_or_null[d] : 1.0f;
        F->map.b[d] = map_b3_or_null ? map_b3_or_null[d] : 0.0f;
    }
    F->table = table;
    F->packed = (const float4*)packed;
    return IRON_OK;
}

// fn(integral_constant<int, ACT>) for the activation of a validated plan
template <class Fn>
static inline int with_act(const FieldPlan& pl, Fn&& fn) {
    switch (pl.act) {
        case IRON_FIELD_ACT_RELU: return fn(std::integral_constant<int, IRON_FIELD_ACT_RELU>{});
        case IRON_FIELD_ACT_SOFTPLUS: return fn(std::integral_constant<int, IRON_FIELD_ACT_SOFTPLUS>{});
        default: return fn(std::integral_constant<int, IRON_FIELD_ACT_NONE>{});
    }
}

// fn(integral_constant ACT, integral_constant NT) for the <ACT, NT> instance of the value path (field_value_acc) that serves a
// plan: NT is the number of 32-row output tiles of a hidden layer, 1, 2 or 4 for the 16 / 32, 64 and 128 neurons make_plan accepts
template <class Fn>
static inline int with_value_path(const FieldPlan& pl, Fn&& fn) {
    return with_act(pl, [&](auto act) {
        switch (pl.tiles[0]) {
            case 1: return fn(act, std::integral_constant<int, 1>{});
            case 2: return fn(act, std::integral_constant<int, 2>{});
            default: return fn(act, std::integral_constant<int, 4>{});
        }
    });
}

template <int ACT>
__device__ __forceinline__ float field_act(float z) {
    if constexpr (ACT == IRON_FIELD_ACT_RELU) return fmaxf(z, 0.0f);
    else if constexpr (ACT == IRON_FIELD_ACT_SOFTPLUS) return z > 20.0f ? z : log1pf(expf(z));   // nn.Softplus(): beta 1, threshold 20
    else return z;
}
// act'(z) from h = act(z)
template <int ACT>
__device__ __forceinline__ float field_act_grad(float h) {
    if constexpr (ACT == IRON_FIELD_ACT_RELU) return h > 0.0f ? 1.0f : 0.0f;
    else if constexpr (ACT == IRON_FIELD_ACT_SOFTPLUS) return -expm1f(-h);
    else return 1.0f;
}

// the row of accumulator register r in lane half h (C/D map of the 32x32 MFMAs)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The level loop of a wave, G levels at a time: the corner walks and the 8 G gathers of a group are issued first, then every level
// is summed, in level order.  A wave has few other waves to hide its latency behind (LDS holds the stages of a handful), so the
// gathers in flight have to come from the wave itself.  Per level the arithmetic is k_hg_encode's: y[f] = sum_o wgt[o] row_o[f]
// in corner order -> rows l F .. l F + F - 1 of the stage, this lane's column.  P is the row pitch of the stage in floats.
template <int F>
__device__ __forceinline__ void field_encode(const hg::Levels& L, const float* xs, const float* __restrict__ table,
                                             float* __restrict__ dst, int P) {
    constexpr int G = F <= 2 ? 4 : 2;
    for (int l0 = 0; l0 < L.n_levels; l0 += G) {
        hg::Walk k[G];
        float row[G][8][F];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (l0 + g < L.n_levels) {
                const iron_hashgrid_level lv = L.lv[l0 + g];
                hg::walk(lv, xs, &k[g]);
                const float* base = table + lv.offset * F;
#pragma unroll
                for (int o = 0; o < 8; ++o) hg::load_row<F>(base + (int64_t)k[g].idx[o] * F, row[g][o]);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (l0 + g < L.n_levels) {
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    float s = 0.0f;
#pragma unroll
                    for (int o = 0; o < 8; ++o) s = fmaf(k[g].wgt[o], row[g][o][f], s);
                    dst[((l0 + g) * F + f) * P] = s;
                }
            }
        }
    }
}

// g[d] = fma(e[l,f], J[l,f,d], g[d]) in ascending (l, f), J as k_hg_encode forms it; the gathers grouped as above
template <int F>
__device__ __forceinline__ void field_grad(const hg::Levels& L, const float* xs, const float* __restrict__ table,
                                           const float* __restrict__ e, int P, float* gr) {
    constexpr int G = F <= 2 ? 4 : 2;
    for (int l0 = 0; l0 < L.n_levels; l0 += G) {
        hg::Walk k[G];
        float row[G][8][F];
        float scale[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (l0 + g < L.n_levels) {
                const iron_hashgrid_level lv = L.lv[l0 + g];
                hg::walk(lv, xs, &k[g]);
                scale[g] = lv.scale;
                const float* base = table + lv.offset * F;
#pragma unroll
                for (int o = 0; o < 8; ++o) hg::load_row<F>(base + (int64_t)k[g].idx[o] * F, row[g][o]);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (l0 + g < L.n_levels) {
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const float ef = e[((l0 + g) * F + f) * P];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        float s = 0.0f;
#pragma unroll
                        for (int o = 0; o < 8; ++o) s = fmaf(k[g].dw[o][d], row[g][o][f], s);
                        gr[d] = fmaf(ef, k[g].live[d] * (scale[g] * s), gr[d]);
                    }
                }
            }
        }
    }
}

// acc[ct] = sum over k of frag[k][row of this lane] * in[k][point], k ascending: nq quads of four k-steps.  PITCH is the row pitch
// of `in` in floats: the 32 CT points of the inference stages, padded in the training kernel.
template <int CT, int PITCH = 32 * CT>
__device__ __forceinline__ void field_tile(const float4* __restrict__ frag, int nq, const float* __restrict__ in, int lane,
                                           f32x16 (&acc)[CT]) {
    constexpr int P = PITCH;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    const float* bp = in + (lane >> 5) * P + (lane & 31);
    // the fragments come from L2: kFieldFragAhead of them are fetched while the previous ones feed the MFMAs (the order of the
    // k-steps, and so every bit of the result, is that of the plain loop)
    float4 ahead[kFieldFragAhead];
#pragma unroll
    for (int i = 0; i < kFieldFragAhead; ++i) ahead[i] = i < nq ? frag[i * 64 + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int q0 = 0; q0 < nq; q0 += kFieldFragAhead) {
        float4 a[kFieldFragAhead];
#pragma unroll
        for (int i = 0; i < kFieldFragAhead; ++i) {
            a[i] = ahead[i];
            if (q0 + kFieldFragAhead + i < nq) ahead[i] = frag[(q0 + kFieldFragAhead + i) * 64 + lane];
        }
#pragma unroll
        for (int i = 0; i < kFieldFragAhead; ++i) {
            if (q0 + i < nq) {
                const float* b = bp + (q0 + i) * 8 * P;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma32(a[i].x, b[32 * ct], acc[ct]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma32(a[i].y, b[2 * P + 32 * ct], acc[ct]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma32(a[i].z, b[4 * P + 32 * ct], acc[ct]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma32(a[i].w, b[6 * P + 32 * ct], acc[ct]);
            }
        }
    }
}

// The value path of one wave64 on P = 32 CT points: lane `lane` < P encodes the point xs (already mapped into the
// unit cube) into stage 0, the hidden layers run in the one LDS buffer `lds` (lds_layout(pl, false, P) bytes) with their NT output
// tiles waiting in registers until the layer's last k-step has read its input, and the last layer's accumulator comes back in
// `acc`: row acc_row(r, lane >> 5) of point 32 ct + (lane & 31) in acc[ct][r].  Every lane of the wave must call it (MFMAs and
// barriers).  k_hg_field's value form and the device tracer (hashgrid_trace.hip) are both this function, so they agree bit for bit.
template <int ACT, int CT, int NT>
__device__ __forceinline__ void field_value_acc(const hg::Levels& L, const FieldPlan& pl, float* __restrict__ lds, const float* xs, bool owner,
                                                const float* __restrict__ table, const float4* __restrict__ packed, int lane,
                                                f32x16 (&acc)[CT]) {
    constexpr int P = 32 * CT;
    const int half = lane >> 5, col = lane & 31;
    // ---- encode: stage 0, rows l F + f; the rows between L F and the next multiple of 8 are zero (k-step padding) ----
    if (owner) {
        for (int k = pl.lf; k < pl.kq[0] * 8; ++k) lds[k * P + lane] = 0.0f;
        switch (L.n_features) {
            case 1: field_encode<1>(L, xs, table, lds + lane, P); break;
            case 2: field_encode<2>(L, xs, table, lds + lane, P); break;
            case 4: field_encode<4>(L, xs, table, lds + lane, P); break;
            default: field_encode<8>(L, xs, table, lds + lane, P); break;
        }
    }
    // ---- head ----
    for (int j = 0; j < pl.m; ++j) {
        __syncthreads();
        const float4* w = packed + pl.fwd_off[j];
        const int nq = pl.kq[j];
        f32x16 hid[NT][CT];
#pragma unroll
        for (int t = 0; t < NT; ++t) field_tile<CT>(w + (size_t)t * nq * 64, nq, lds, lane, hid[t]);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) lds[(32 * t + acc_row(r, half)) * P + 32 * ct + col] = field_act<ACT>(hid[t][ct][r]);
    }
    __syncthreads();
    field_tile<CT>(packed + pl.fwd_off[pl.m], pl.kq[pl.m], lds, lane, acc);   // n_out <= 16: one tile
}

// Output 0 of the 64 points of a wave (CT = 2), handed back to the point's own lane: row 0 sits in accumulator register 0 of the
// lower lane half, point 32 ct + col in acc[ct] of lane col.
template <int ACT, int NT>
__device__ __forceinline__ float field_value(const hg::Levels& L, const FieldPlan& pl, float* __restrict__ lds, const float* xs,
                                             const float* __restrict__ table, const float4* __restrict__ packed, int lane) {
    f32x16 acc[2];
    field_value_acc<ACT, 2, NT>(L, pl, lds, xs, true, table, packed, lane, acc);
    const float upper = __shfl(acc[1][0], lane & 31, 64);
    return lane < 32 ? acc[0][0] : upper;
}

}  // namespace iron
