// Fused training backward of the hash-grid SDF field (include/iron_train.h, iron_hashgrid_field_* block): for the
// adjoints d_out [n, n_out] and d_g [n, 3] of iron_hashgrid_field_eval's two results, the gradient of the head's weights and, through
// iron_hashgrid_backward_pair, of the table -- the first-order path and the second-order (eikonal) path in one kernel.
//
//   k_hg_field_bwd<ACT, CT>   one wave64 per workgroup owns one SLOT of C(n) consecutive points and walks its tiles of P = 32 CT
//                             points in order.  Per tile, every stage in LDS as [row][PT floats], PT = P + 1 (an odd pitch: a read
//                             with the row on the lane meets 32 distinct banks per half wave; a read along a row stays contiguous):
//       forward   y = enc(x) and h_0 .. h_{m-1} with hashgrid_field_common.h's encode and tile product: the bits of k_hg_field
//       d chain   d_{m-1} = act'(h_{m-1}) W_m[0,:];  G_l = W_l^T d_l;  d_{l-1} = act'(h_{l-1}) G_l  (the bits of k_hg_field's gradient);
//                 Softplus also keeps c_l = act''(h_l) G_l;  e = G_0 goes to memory
//       tangent   v'_d = a_d d_g[d] on live axes;  ydot_k = fma chain over d of J[k,d] v'_d;  zdot_l = W_l hdot_{l-1};
//                 hdot_l = act'(h_l) zdot_l;  Softplus: s_l = c_l zdot_l in place of c_l
//       adjoint   delta_m = d_out;  for l = m .. 0:  Wbar_l += delta_l h_{l-1}^T + d_l hdot_{l-1}^T  (below), then
//                 delta_{l-1} = act'(h_{l-1}) (W_l^T delta_l) [fma with s_{l-1} for Softplus] in place of h_{l-1};  ybar = W_0^T delta_0
//                 goes to memory
//       Wbar      one 32x32 accumulator tile per (32 outputs, 32 inputs) on v_mfma_f32_32x32x2_f32 with the POINT as the k index:
//                 per pair of points first delta h^T, then d hdot^T, points ascending.  The tiles of a slot are carried from one
//                 point tile to the next in LDS where they fit beside the stages (7 tiles, 28 KiB, at the check head), otherwise in
//                 the slot's own row of the workspace (read and written by this wave alone); fp32 either way, the values an
//                 accumulator register would hold.  They leave the kernel as fp64 partials [weight][slot].
//   k_hg_field_wsum           one workgroup per weight: fixed_sum::slot_sum over the slots in fp64, rounded to fp32 once.
//   k_hg_field_train_pack     W_m^T in fragment order (the inference blob lacks it: its gradient needs row 0 of W_m only).
//
// A column past the slot's end evaluates at the origin with zero adjoints: every product it adds to Wbar is an exact zero.
#include "hashgrid_field_common.h"
#include "fixed_sum.h"
#include "train_common.h"

namespace iron_train {

using namespace iron;

constexpr int kTrainLdsMax = 160 * 1024;    // the LDS of a CU
constexpr int kTrainSlotQuantum = 64;       // a slot is a whole number of point tiles at either CT
constexpr int kTrainMaxSlots = 1024;

// C(n): points per slot.  A function of n alone; the order of every weight-gradient sum follows from it.
static int64_t train_slot_points(int64_t n) {
    const int64_t q = cdiv64(n, (int64_t)kTrainSlotQuantum * kTrainMaxSlots);
    return kTrainSlotQuantum * (q < 1 ? 1 : q);
}

struct TrainPlan {
    int32_t itiles[kFieldMaxLayers], wt_off[kFieldMaxLayers];   // layer j: 32-input tiles, first accumulator tile
    int32_t n_tiles;
    int32_t trm_tq, trm_tiles, total_f4;                        // the training blob: W_m^T, k = output index
};

static TrainPlan make_train_plan(const FieldPlan& p) {
    TrainPlan t = {};
    int o = 0;
    for (int j = 0; j <= p.m; ++j) {
        t.itiles[j] = round_up(p.in[j], 32) / 32;
        t.wt_off[j] = o;
        o += p.tiles[j] * t.itiles[j];
    }
    t.n_tiles = o;
    t.trm_tq = round_up(p.n_out, 8) / 8;
    t.trm_tiles = round_up(p.neurons, 32) / 32;
    t.total_f4 = t.trm_tiles * t.trm_tq * 64;
    return t;
}

// stage buffers (float offsets at pitch PT)
struct TrainLds {
    int32_t y, yt, dm;
    int32_t tiles;            // >= 0: the slot's accumulator tiles live in LDS at this offset; -1: in the slot's workspace row
    int32_t h[kFieldMaxLayers - 1], d[kFieldMaxLayers - 1], t[kFieldMaxLayers - 1], c[kFieldMaxLayers - 1];
};
static size_t train_lds_layout(const FieldPlan& p, int P, TrainLds* out, int acc_tiles = 0) {
    const int PT = P + 1, r0 = round_up(p.lf, 32), rn = round_up(p.neurons, 32);
    TrainLds L = {};
    int rows = 0;
    auto take = [&](int r) { const int at = rows * PT; rows += r; return at; };
    L.y = take(r0);
    L.yt = take(r0);
    L.dm = take(32);
    for (int l = 0; l < p.m; ++l) {
        L.h[l] = take(rn);
        L.d[l] = take(rn);
        L.t[l] = take(rn);
        L.c[l] = p.act == IRON_FIELD_ACT_SOFTPLUS ? take(rn) : 0;
    }
    L.tiles = acc_tiles > 0 ? rows * PT : -1;
    if (out) *out = L;
    return ((size_t)rows * PT + (size_t)acc_tiles * 1024) * sizeof(float);
}

// act''(z) from h = act(z): sigma (1 - sigma) for Softplus, zero otherwise
__device__ __forceinline__ float field_act_curv(float h) {
    const float s = -expm1f(-h);
    return s * (1.0f - s);
}

// ydot[l F + f] = fma chain over d = 0, 1, 2 from zero of J[l,f,d] v'_d, J as field_grad forms it
template <int F>
__device__ __forceinline__ void field_tangent(const hg::Levels& L, const float* xs, const float* __restrict__ table, const float* vp,
                                              float* __restrict__ dst, int PT) {
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
            float t = 0.0f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) s = fmaf(k.dw[o][d], row[o][f], s);
                t = fmaf(k.live[d] * (lv.scale * s), vp[d], t);
            }
            dst[(l * F + f) * PT] = t;
        }
    }
}

struct TrainArgs {
    const float* p;
    const float* table;
    const float4* packed;
    const float4* tpacked;
    const float* d_out;      // may be null
    const float* d_g;        // may be null
    float* ybar;             // [n, L F]
    float* e;                // [n, L F]
    float* xmap;             // [n, 3]: the mapped points, for the table scatter
    float* vp;               // [n, 3]: a_d d_g[d]
    float* tiles;            // [slots][n_tiles][16][64] fp32
    double* part;            // [n_weights][slots]
    int64_t n, slot_points;
    int32_t slots;
};

template <int ACT, int CT>
__global__ __launch_bounds__(64) void k_hg_field_bwd(hg::Levels L, FieldPlan pl, TrainPlan tp, TrainLds lo, FieldMap map, TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = 32 * CT, PT = P + 1;
    constexpr bool SP = ACT == IRON_FIELD_ACT_SOFTPLUS;
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const bool owner = lane < P;
    const int F = L.n_features, m = pl.m;
    const int64_t s_first = (int64_t)blockIdx.x * a.slot_points;
    const int64_t s_end = s_first + a.slot_points < a.n ? s_first + a.slot_points : a.n;
    float* my_tiles = lo.tiles >= 0 ? lds + lo.tiles : a.tiles + (size_t)blockIdx.x * tp.n_tiles * 1024;
    float* Y = lds + lo.y;
    float* YT = lds + lo.yt;
    float* DM = lds + lo.dm;
    const float* w0 = (const float*)(a.packed + pl.row0_off);

    for (int64_t first = s_first; first < s_end; first += P) {
        const int64_t pt = first + lane;
        const bool have = owner && pt < s_end;
        float xs[3] = {0.0f, 0.0f, 0.0f}, vp[3] = {0.0f, 0.0f, 0.0f};
        if (have) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                xs[d] = fmaf(a.p[3 * pt + d], map.a[d], map.b[d]);
                const bool live = xs[d] >= 0.0f && xs[d] <= 1.0f;
                if (a.d_g && live) vp[d] = map.a[d] * a.d_g[3 * pt + d];
                a.xmap[3 * pt + d] = xs[d];
                a.vp[3 * pt + d] = vp[d];
            }
        }
        __syncthreads();   // the previous tile's reads are done

        // ---- encode, and the tangent of the features ----
        if (owner) {
            for (int k = pl.lf; k < pl.kq[0] * 8; ++k) {
                Y[k * PT + lane] = 0.0f;
                YT[k * PT + lane] = 0.0f;
            }
            switch (F) {
                case 1: field_encode<1>(L, xs, a.table, Y + lane, PT); field_tangent<1>(L, xs, a.table, vp, YT + lane, PT); break;
                case 2: field_encode<2>(L, xs, a.table, Y + lane, PT); field_tangent<2>(L, xs, a.table, vp, YT + lane, PT); break;
                case 4: field_encode<4>(L, xs, a.table, Y + lane, PT); field_tangent<4>(L, xs, a.table, vp, YT + lane, PT); break;
                default: field_encode<8>(L, xs, a.table, Y + lane, PT); field_tangent<8>(L, xs, a.table, vp, YT + lane, PT); break;
            }
            for (int o = 0; o < 32; ++o) DM[o * PT + lane] = (have && a.d_out && o < pl.n_out) ? a.d_out[pt * pl.n_out + o] : 0.0f;
        }

        // ---- forward: h_l = act(W_l h_{l-1}) ----
        for (int l = 0; l < m; ++l) {
            __syncthreads();
            const float* in = l == 0 ? Y : lds + lo.h[l - 1];
            float* o = lds + lo.h[l];
            const float4* w = a.packed + pl.fwd_off[l];
            const int nq = pl.kq[l];
            for (int t = 0; t < pl.tiles[l]; ++t) {
                f32x16 acc[CT];
                field_tile<CT, PT>(w + (size_t)t * nq * 64, nq, in, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[(32 * t + acc_row(r, half)) * PT + 32 * ct + col] = field_act<ACT>(acc[ct][r]);
            }
        }

        // ---- d chain: d_{m-1} = act'(h_{m-1}) W_m[0,:], then G_l = W_l^T d_l ----
        __syncthreads();
        if (owner) {
            const float* hb = lds + lo.h[m - 1];
            float* db = lds + lo.d[m - 1];
            float* cb = lds + lo.c[m - 1];
            for (int k = 0; k < pl.tq[m - 1] * 8; ++k) {
                const float h = hb[k * PT + lane];
                db[k * PT + lane] = field_act_grad<ACT>(h) * w0[k];
                if constexpr (SP) cb[k * PT + lane] = field_act_curv(h) * w0[k];
            }
        }
        for (int l = m - 1; l >= 0; --l) {
            __syncthreads();
            const float* din = lds + lo.d[l];
            const float4* w = a.packed + pl.tr_off[l];
            const int nq = pl.tq[l];
            for (int t = 0; t < pl.ttiles[l]; ++t) {
                f32x16 acc[CT];
                field_tile<CT, PT>(w + (size_t)t * nq * 64, nq, din, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 32 * t + acc_row(r, half);
                        if (l > 0) {
                            const int at = row * PT + 32 * ct + col;
                            const float h = lds[lo.h[l - 1] + at];
                            lds[lo.d[l - 1] + at] = field_act_grad<ACT>(h) * acc[ct][r];
                            if constexpr (SP) lds[lo.c[l - 1] + at] = field_act_curv(h) * acc[ct][r];
                        } else {
                            const int64_t q = first + 32 * ct + col;
                            if (q < s_end && row < pl.lf) a.e[q * pl.lf + row] = acc[ct][r];
                        }
                    }
            }
        }

        // ---- tangent chain: zdot_l = W_l hdot_{l-1}; hdot_l = act'(h_l) zdot_l; Softplus: s_l = c_l zdot_l ----
        for (int l = 0; l < m; ++l) {
            __syncthreads();
            const float* in = l == 0 ? YT : lds + lo.t[l - 1];
            const float4* w = a.packed + pl.fwd_off[l];
            const int nq = pl.kq[l];
            for (int t = 0; t < pl.tiles[l]; ++t) {
                f32x16 acc[CT];
                field_tile<CT, PT>(w + (size_t)t * nq * 64, nq, in, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int at = (32 * t + acc_row(r, half)) * PT + 32 * ct + col;
                        lds[lo.t[l] + at] = field_act_grad<ACT>(lds[lo.h[l] + at]) * acc[ct][r];
                        if constexpr (SP) lds[lo.c[l] + at] = lds[lo.c[l] + at] * acc[ct][r];
                    }
            }
        }

        // ---- adjoint chain and the weight gradients, l = m .. 0 ----
        for (int l = m; l >= 0; --l) {
            __syncthreads();
            const float* A1 = l == m ? DM : lds + lo.h[l];                       // delta_l
            const float* B1 = l == 0 ? Y : lds + lo.h[l - 1];                    // h_{l-1}
            const float* A2 = l == m ? DM : lds + lo.d[l];                       // d_l (l = m: the unit vector of row 0, formed below)
            const float* B2 = l == 0 ? YT : lds + lo.t[l - 1];                   // hdot_{l-1}
            for (int ot = 0; ot < pl.tiles[l]; ++ot)
                for (int it = 0; it < tp.itiles[l]; ++it) {
                    float* tile = my_tiles + (size_t)(tp.wt_off[l] + ot * tp.itiles[l] + it) * 1024 + lane;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = first == s_first ? 0.0f : tile[r * 64];
                    const float* a1 = A1 + (32 * ot + col) * PT + half;
                    const float* b1 = B1 + (32 * it + col) * PT + half;
                    const float* a2 = A2 + (32 * ot + col) * PT + half;
                    const float* b2 = B2 + (32 * it + col) * PT + half;
                    const float unit = (ot == 0 && col == 0) ? 1.0f : 0.0f;
#pragma unroll 4
                    for (int s = 0; s < P / 2; ++s) {
                        acc = mfma32(a1[2 * s], b1[2 * s], acc);
                        acc = mfma32(l == m ? unit : a2[2 * s], b2[2 * s], acc);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) tile[r * 64] = acc[r];
                }
            __syncthreads();
            const float4* w = l == m ? a.tpacked : a.packed + pl.tr_off[l];
            const int nq = l == m ? tp.trm_tq : pl.tq[l];
            const int nt = l == m ? tp.trm_tiles : pl.ttiles[l];
            for (int t = 0; t < nt; ++t) {
                f32x16 acc[CT];
                field_tile<CT, PT>(w + (size_t)t * nq * 64, nq, A1, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 32 * t + acc_row(r, half);
                        if (l > 0) {
                            const int at = row * PT + 32 * ct + col;
                            float* hq = lds + lo.h[l - 1] + at;
                            if constexpr (SP) *hq = fmaf(field_act_grad<ACT>(*hq), acc[ct][r], lds[lo.c[l - 1] + at]);
                            else *hq = field_act_grad<ACT>(*hq) * acc[ct][r];
                        } else {
                            const int64_t q = first + 32 * ct + col;
                            if (q < s_end && row < pl.lf) a.ybar[q * pl.lf + row] = acc[ct][r];
                        }
                    }
            }
        }
    }

    // ---- the slot's partials, fp64, [weight][slot] ----
    for (int l = 0; l <= m; ++l)
        for (int ot = 0; ot < pl.tiles[l]; ++ot)
            for (int it = 0; it < tp.itiles[l]; ++it) {
                const float* tile = my_tiles + (size_t)(tp.wt_off[l] + ot * tp.itiles[l] + it) * 1024 + lane;
                const int in = 32 * it + col;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int out = 32 * ot + acc_row(r, half);
                    if (out < pl.out[l] && in < pl.in[l])
                        a.part[(size_t)(pl.w_off[l] + out * pl.in[l] + in) * a.slots + blockIdx.x] = (double)tile[r * 64];
                }
            }
}

__global__ __launch_bounds__(64) void k_hg_field_wsum(const double* __restrict__ part, int64_t slots, float* __restrict__ d_weights) {
    __shared__ double red[64];
    const double s = fixed_sum::slot_sum<64>(part + (size_t)blockIdx.x * slots, slots, 1, red);
    if (threadIdx.x == 0) d_weights[blockIdx.x] = (float)s;
}

// one thread per float4: lane row i = input of W_m, k = its output
__global__ __launch_bounds__(256) void k_hg_field_train_pack(FieldPlan pl, TrainPlan tp, const float* __restrict__ w, float4* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= tp.total_f4) return;
    const int lane = e & 63, q = (e >> 6) % tp.trm_tq, t = (e >> 6) / tp.trm_tq;
    const int i = 32 * t + (lane & 31), h = lane >> 5;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < 4; ++c) {
        const int k = 8 * q + 2 * c + h;
        if (i < pl.neurons && k < pl.n_out) v[c] = w[pl.w_off[pl.m] + k * pl.neurons + i];
    }
    dst[e] = make_float4(v[0], v[1], v[2], v[3]);
}

struct TrainWs {
    size_t ybar, e, xmap, vp, tiles, part, pair, bytes;
    size_t pair_bytes;
};

static TrainWs train_ws_layout(const iron_hashgrid_field_desc* d, const FieldPlan& pl, const TrainPlan& tp, int64_t n) {
    TrainWs w{};
    Carver c;
    const int64_t slots = n > 0 ? cdiv64(n, train_slot_points(n)) : 0;
    const size_t rows = (size_t)(n > 0 ? n : 1);
    w.ybar = c.take(rows * pl.lf * sizeof(float));
    w.e = c.take(rows * pl.lf * sizeof(float));
    w.xmap = c.take(rows * 3 * sizeof(float));
    w.vp = c.take(rows * 3 * sizeof(float));
    w.tiles = c.take((size_t)(slots > 0 ? slots : 1) * tp.n_tiles * 1024 * sizeof(float));
    w.part = c.take(slot_bytes(slots, pl.n_weights));
    w.pair_bytes = iron_hashgrid_backward_pair_workspace_bytes(&d->encoding, n);
    w.pair = c.take(w.pair_bytes);
    w.bytes = c.off;
    return w;
}

// the training plan of a shape the backward is built for: IRON_ERR_RANGE for 128 neurons and for stages that do not fit the LDS of a CU
static int train_plan(const FieldPlan& pl, TrainPlan* tp) {
    if (pl.neurons > 64) return IRON_ERR_RANGE;
    if (train_lds_layout(pl, 32, nullptr) > (size_t)kTrainLdsMax) return IRON_ERR_RANGE;
    *tp = make_train_plan(pl);
    return IRON_OK;
}

static int make_train(const iron_hashgrid_field_desc* d, FieldPlan* pl, TrainPlan* tp) {
    const int rc = make_plan(d, pl);
    return rc != IRON_OK ? rc : train_plan(*pl, tp);
}

template <int ACT, int CT>
static int train_launch(const FieldBinding& F, const TrainPlan& tp, const TrainLds& lo, size_t lds_bytes, const TrainArgs& a, hipStream_t st) {
    if (lds_bytes > 64 * 1024)
        IRON_TRAIN_HIP(hipFuncSetAttribute((const void*)k_hg_field_bwd<ACT, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL((k_hg_field_bwd<ACT, CT>), dim3((unsigned)a.slots), dim3(64), lds_bytes, st, F.L, F.pl, tp, lo, F.map, a);
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}

template <int ACT>
static int train_dispatch(const FieldBinding& F, const TrainPlan& tp, const TrainArgs& a, hipStream_t st) {
    // 64 points per tile where their stages fit; the accumulator tiles beside them in LDS where those fit too
    TrainLds lo;
    const int P = train_lds_layout(F.pl, 64, nullptr) <= (size_t)kTrainLdsMax ? 64 : 32;
    size_t bytes = train_lds_layout(F.pl, P, &lo, tp.n_tiles);
    if (bytes > (size_t)kTrainLdsMax) bytes = train_lds_layout(F.pl, P, &lo);
    if (P == 64) return train_launch<ACT, 2>(F, tp, lo, bytes, a, st);
    return train_launch<ACT, 1>(F, tp, lo, bytes, a, st);
}

}  // namespace iron_train

using namespace iron_train;

extern "C" int iron_hashgrid_field_train_check(const iron_hashgrid_field_desc* desc) {
    FieldPlan pl;
    TrainPlan tp;
    return make_train(desc, &pl, &tp);
}

extern "C" int64_t iron_hashgrid_field_train_slot(int64_t n) { return n < 0 ? 0 : train_slot_points(n); }

extern "C" size_t iron_hashgrid_field_train_pack_bytes(const iron_hashgrid_field_desc* desc) {
    FieldPlan pl;
    TrainPlan tp;
    if (make_train(desc, &pl, &tp) != IRON_OK) return 0;
    return (size_t)tp.total_f4 * sizeof(float4);
}

extern "C" int iron_hashgrid_field_train_pack(const iron_hashgrid_field_desc* desc, const float* weights, void* train_packed, void* stream) {
    FieldPlan pl;
    TrainPlan tp;
    const int rc = make_train(desc, &pl, &tp);
    if (rc != IRON_OK) return rc;
    if (!weights || !train_packed || ((uintptr_t)train_packed & 15)) return IRON_ERR_BAD_ARG;
    IRON_TRAIN_LAUNCH(k_hg_field_train_pack, blocks_for(tp.total_f4, 256), 256, (hipStream_t)stream, pl, tp, weights, (float4*)train_packed);
    return IRON_OK;
}

extern "C" size_t iron_hashgrid_field_backward_workspace_bytes(const iron_hashgrid_field_desc* desc, int64_t n) {
    FieldPlan pl;
    TrainPlan tp;
    if (n < 0 || make_train(desc, &pl, &tp) != IRON_OK) return 0;
    return train_ws_layout(desc, pl, tp, n).bytes;
}

extern "C" int iron_hashgrid_field_backward(const iron_hashgrid_field_desc* desc, const float* p, int64_t n, const float* map_a3_or_null,
                                            const float* map_b3_or_null, const float* table, const void* packed,
                                            const void* train_packed, const float* d_out_or_null, const float* d_g_or_null,
                                            float* d_weights, float* d_table_or_null, float* ybar_out_or_null, float* e_out_or_null,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    FieldBinding F;
    TrainPlan tp;
    int64_t n_params = 0;
    int rc = field_open(desc, &F, &n_params);
    if (rc == IRON_OK) rc = train_plan(F.pl, &tp);
    if (rc != IRON_OK) return rc;
    const FieldPlan& pl = F.pl;
    if (n < 0 || !d_weights) return IRON_ERR_BAD_ARG;
    if (n > (int64_t)0x7fffffff * 32) return IRON_ERR_RANGE;   // iron_hashgrid_field_eval's limit; the scatter checks its own
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        IRON_TRAIN_HIP(hipMemsetAsync(d_weights, 0, sizeof(float) * (size_t)pl.n_weights, st));
        if (d_table_or_null) IRON_TRAIN_HIP(hipMemsetAsync(d_table_or_null, 0, sizeof(float) * (size_t)n_params * F.L.n_features, st));
        return IRON_OK;
    }
    if (!p || !train_packed || !workspace) return IRON_ERR_BAD_ARG;
    rc = field_bind(&F, map_a3_or_null, map_b3_or_null, table, packed);
    if (rc != IRON_OK) return rc;
    if (((uintptr_t)train_packed & 15) || ((uintptr_t)workspace & 255)) return IRON_ERR_BAD_ARG;
    const TrainWs w = train_ws_layout(desc, pl, tp, n);
    if (workspace_bytes < w.bytes) return IRON_ERR_WORKSPACE;
    TrainArgs a{};
    a.p = p; a.table = F.table; a.packed = F.packed; a.tpacked = (const float4*)train_packed;
    a.d_out = d_out_or_null; a.d_g = d_g_or_null;
    a.ybar = ybar_out_or_null ? ybar_out_or_null : ws_ptr<float>(workspace, w.ybar);
    a.e = e_out_or_null ? e_out_or_null : ws_ptr<float>(workspace, w.e);
    a.xmap = ws_ptr<float>(workspace, w.xmap);
    a.vp = ws_ptr<float>(workspace, w.vp);
    a.tiles = ws_ptr<float>(workspace, w.tiles);
    a.part = ws_ptr<double>(workspace, w.part);
    a.n = n; a.slot_points = train_slot_points(n);
    a.slots = (int32_t)cdiv64(n, a.slot_points);
    rc = with_act(pl, [&](auto act) { return train_dispatch<act()>(F, tp, a, st); });
    if (rc != IRON_OK) return rc;
    IRON_TRAIN_LAUNCH(k_hg_field_wsum, (unsigned)pl.n_weights, 64, st, (const double*)a.part, (int64_t)a.slots, d_weights);
    if (!d_table_or_null) return IRON_OK;
    return iron_hashgrid_backward_pair(&desc->encoding, a.xmap, n, table, a.ybar, a.e, a.vp, d_table_or_null,
                                       ws_ptr<void>(workspace, w.pair), w.pair_bytes, stream);
}
