// Fused inference evaluation of the hash-grid SDF field (include/iron_hip.h, iron_hashgrid_field_* block): the
// encoding of hashgrid_common.h and the bias-free MLP head behind it in ONE launch, the value and on request d out[0] / dp.
//
//   k_hg_field<ACT, GRAD, CT, NT>   one wave64 per workgroup owns P = 32 CT points.  Every stage of the head lives in LDS as
//                               [row k][P points] floats, so a k-step's B operand (rows 2s, 2s+1) is one ds_read per lane.
//       encode    lane = point, the level loop inside the wave (its gathers stay within four neighbouring levels, two for
//                 F >= 4); hg::walk, the rows loaded first, then y[f] = sum_o wgt[o] row_o[f] in corner order: the bits of
//                 iron_hashgrid_encode.
//       head      Z^T[out, point] = W[out, in] H^T[in, point] on v_mfma_f32_32x32x2_f32, A = a packed weight fragment (one
//                 16-byte load per lane feeds 4 CT MFMAs), accumulator from zero: per output one fp32 fma chain over the input
//                 index in ascending order.  The activation is applied on the accumulator, which is then written to the next
//                 stage's rows.  The last layer's accumulator goes straight to `out`.
//       gradient  (GRAD) the derivative of the activation is recovered from the stored activation itself (ReLU: h > 0;
//                 Softplus: sigmoid(z) = -expm1(-h)), so the forward keeps nothing but the stages.  d_{m-1} = act'(h_{m-1}) W_m[0,:],
//                 then per layer G = W_l^T d_l with the transposed fragments (a chain over the OUTPUT index, ascending),
//                 d_{l-1} = act'(h_{l-1}) G in place, e = W_0^T d_0 into the feature rows.  The corner rows are gathered again,
//                 J[l,f,d] is formed as k_hg_encode forms it and grad_d = fma(e[l,f], J[l,f,d], grad_d) in ascending (l, f).
//   k_hg_field_pack             W (flat [out, in] row-major, layer after layer) -> fragment order, both orientations.
//
// Rows are independent: a point only ever touches its own LDS column, and padded rows / k-steps multiply exact zeros.
#include "hashgrid_field_common.h"
#include "host_util.h"

namespace iron {

// NT > 0 (value only): one LDS buffer serves every stage in place -- the NT output tiles of a hidden layer wait in registers until
// the layer's last k-step has read its input -- which halves the LDS of a wave and doubles the waves a CU holds.  That form is
// field_value_acc (hashgrid_field_common.h), which the device tracer (hashgrid_trace.hip) calls too.
template <int ACT, bool GRAD, int CT, int NT>
__global__ __launch_bounds__(64) void k_hg_field(hg::Levels L, FieldPlan pl, FieldLds lo, const float* __restrict__ p, int64_t n,
                                                 FieldMap map, const float* __restrict__ table, const float4* __restrict__ packed,
                                                 float* __restrict__ out, float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = 32 * CT;
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const int64_t first = (int64_t)blockIdx.x * P;
    const int64_t pt = first + lane;
    const bool owner = lane < P;               // this lane encodes a point
    const bool have = owner && pt < n;
    float xs[3] = {0.0f, 0.0f, 0.0f};          // a column past n evaluates at the origin; nothing of it is written
    if (have) {
#pragma unroll
        for (int d = 0; d < 3; ++d) xs[d] = fmaf(p[3 * pt + d], map.a[d], map.b[d]);
    }
    if constexpr (NT > 0) {   // value only: the shared value path (field_value_acc), then every output row of the last accumulator
        f32x16 acc[CT];
        field_value_acc<ACT, CT, NT>(L, pl, lds, xs, owner, table, packed, lane, acc);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int64_t q = first + 32 * ct + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = acc_row(r, half);
                if (q < n && o < pl.n_out) out[q * pl.n_out + o] = acc[ct][r];
            }
        }
        return;
    }
    const int F = L.n_features;

    // ---- encode: stage 0, rows l F + f; the rows between L F and the next multiple of 8 are zero (k-step padding) ----
    float* s0 = lds + lo.buf[0];
    if (owner) {
        for (int k = pl.lf; k < pl.kq[0] * 8; ++k) s0[k * P + lane] = 0.0f;
        switch (F) {
            case 1: field_encode<1>(L, xs, table, s0 + lane, P); break;
            case 2: field_encode<2>(L, xs, table, s0 + lane, P); break;
            case 4: field_encode<4>(L, xs, table, s0 + lane, P); break;
            default: field_encode<8>(L, xs, table, s0 + lane, P); break;
        }
    }

    // ---- head ----
    for (int j = 0; j <= pl.m; ++j) {
        __syncthreads();
        const float* in = lds + lo.buf[j];
        const float4* w = packed + pl.fwd_off[j];
        const int nq = pl.kq[j];
        if (j < pl.m) {
            float* o = lds + lo.buf[j + 1];
            for (int t = 0; t < pl.tiles[j]; ++t) {
                f32x16 acc[CT];
                field_tile<CT>(w + (size_t)t * nq * 64, nq, in, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[(32 * t + acc_row(r, half)) * P + 32 * ct + col] = field_act<ACT>(acc[ct][r]);
            }
        } else {
            f32x16 acc[CT];
            field_tile<CT>(w, nq, in, lane, acc);   // n_out <= 16: one tile
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int64_t q = first + 32 * ct + col;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = acc_row(r, half);
                    if (q < n && o < pl.n_out) out[q * pl.n_out + o] = acc[ct][r];
                }
            }
        }
    }

    if constexpr (GRAD) {
        // ---- d_{m-1} = act'(h_{m-1}) W_m[0, :] ----
        __syncthreads();
        {
            const float* w0 = (const float*)(packed + pl.row0_off);
            float* hb = lds + lo.buf[pl.m];
            const int rows = pl.tq[pl.m - 1] * 8;
            if (owner)
                for (int k = 0; k < rows; ++k) hb[k * P + lane] = field_act_grad<ACT>(hb[k * P + lane]) * w0[k];
        }
        // ---- G = W_l^T d_l;  d_{l-1} = act'(h_{l-1}) G in place, e = G at l = 0 ----
        for (int l = pl.m - 1; l >= 0; --l) {
            __syncthreads();
            const float* din = lds + lo.buf[l + 1];
            float* o = lds + lo.buf[l];
            const float4* w = packed + pl.tr_off[l];
            const int nq = pl.tq[l];
            for (int t = 0; t < pl.ttiles[l]; ++t) {
                f32x16 acc[CT];
                field_tile<CT>(w + (size_t)t * nq * 64, nq, din, lane, acc);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* q = o + (32 * t + acc_row(r, half)) * P + 32 * ct + col;
                        *q = l > 0 ? field_act_grad<ACT>(*q) * acc[ct][r] : acc[ct][r];
                    }
            }
        }
        // ---- grad_d = sum_{l,f} e[l,f] J[l,f,d], the corner rows gathered again ----
        __syncthreads();
        if (owner) {
            float g[3] = {0.0f, 0.0f, 0.0f};
            switch (F) {
                case 1: field_grad<1>(L, xs, table, s0 + lane, P, g); break;
                case 2: field_grad<2>(L, xs, table, s0 + lane, P, g); break;
                case 4: field_grad<4>(L, xs, table, s0 + lane, P, g); break;
                default: field_grad<8>(L, xs, table, s0 + lane, P, g); break;
            }
            if (have) {
#pragma unroll
                for (int d = 0; d < 3; ++d) grad[3 * pt + d] = map.a[d] * g[d];
            }
        }
    }
}

// one thread per float4 of the blob
__global__ __launch_bounds__(256) void k_hg_field_pack(FieldPlan pl, const float* __restrict__ w, float4* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= pl.total_f4) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e >= pl.row0_off) {                       // W_m[0, k], zero past n_neurons
        const int k0 = (e - pl.row0_off) * 4;
        for (int c = 0; c < 4; ++c)
            if (k0 + c < pl.in[pl.m]) v[c] = w[pl.w_off[pl.m] + k0 + c];
    } else {
        int j = 0;
        bool tr = false;
        if (e >= pl.tr_off[0]) {
            tr = true;
            while (j + 1 < pl.m && e >= pl.tr_off[j + 1]) ++j;
        } else {
            while (j < pl.m && e >= pl.fwd_off[j + 1]) ++j;
        }
        const int r = e - (tr ? pl.tr_off[j] : pl.fwd_off[j]);
        const int nq = tr ? pl.tq[j] : pl.kq[j];
        const int lane = r & 63, q = (r >> 6) % nq, t = (r >> 6) / nq;
        const int i = 32 * t + (lane & 31), h = lane >> 5;
        const float* wj = w + pl.w_off[j];
        for (int c = 0; c < 4; ++c) {
            const int k = 8 * q + 2 * c + h;
            if (!tr) {
                if (i < pl.out[j] && k < pl.in[j]) v[c] = wj[(size_t)i * pl.in[j] + k];       // lane row i = output, k = input
            } else {
                if (i < pl.in[j] && k < pl.out[j]) v[c] = wj[(size_t)k * pl.in[j] + i];       // lane row i = input, k = output
            }
        }
    }
    dst[e] = make_float4(v[0], v[1], v[2], v[3]);
}

template <int ACT, bool GRAD, int CT, int NT>
static int field_launch(const FieldBinding& F, const FieldLds& lo, size_t lds_bytes, const float* p, int64_t n, float* out, float* grad,
                        hipStream_t st) {
    if (lds_bytes > 64 * 1024)
        IRON_HIP_TRY(hipFuncSetAttribute((const void*)k_hg_field<ACT, GRAD, CT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const int64_t blocks = (n + 32 * CT - 1) / (32 * CT);
    hipLaunchKernelGGL((k_hg_field<ACT, GRAD, CT, NT>), dim3((unsigned)blocks), dim3(64), lds_bytes, st, F.L, F.pl, lo, p, n, F.map, F.table,
                       F.packed, out, grad);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

static int field_dispatch(const FieldBinding& F, const float* p, int64_t n, float* out, float* grad, hipStream_t st) {
    FieldLds lo;
    if (!grad) {   // value: 64 points per wave always fit (at most 128 rows of 256 bytes); the hidden layers' tiles in registers
        const size_t bytes = lds_layout(F.pl, false, 64, &lo);
        return with_value_path(F.pl, [&](auto act, auto nt) { return field_launch<act(), false, 2, nt()>(F, lo, bytes, p, n, out, grad, st); });
    }
    return with_act(F.pl, [&](auto act) {
        size_t bytes = lds_layout(F.pl, true, 64, &lo);
        if (bytes <= (size_t)kFieldLdsTwoTiles) return field_launch<act(), true, 2, 0>(F, lo, bytes, p, n, out, grad, st);
        bytes = lds_layout(F.pl, true, 32, &lo);
        return field_launch<act(), true, 1, 0>(F, lo, bytes, p, n, out, grad, st);
    });
}

}  // namespace iron

using namespace iron;

extern "C" int iron_hashgrid_field_check(const iron_hashgrid_field_desc* desc, int64_t* n_weights_out) {
    FieldPlan pl;
    const int rc = make_plan(desc, &pl);
    if (rc != IRON_OK) return rc;
    if (n_weights_out) *n_weights_out = pl.n_weights;
    return IRON_OK;
}

extern "C" size_t iron_hashgrid_field_pack_bytes(const iron_hashgrid_field_desc* desc) {
    FieldPlan pl;
    if (make_plan(desc, &pl) != IRON_OK) return 0;
    return (size_t)pl.total_f4 * sizeof(float4);
}

extern "C" int iron_hashgrid_field_pack(const iron_hashgrid_field_desc* desc, const float* weights, void* packed, void* stream) {
    FieldPlan pl;
    const int rc = make_plan(desc, &pl);
    if (rc != IRON_OK) return rc;
    if (!weights || !packed || ((uintptr_t)packed & 15)) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_hg_field_pack, blocks_for(pl.total_f4, 256), 256, (hipStream_t)stream, pl, weights, (float4*)packed);
    return IRON_OK;
}

extern "C" int iron_hashgrid_field_eval(const iron_hashgrid_field_desc* desc, const float* p, int64_t n, const float* map_a3_or_null,
                                        const float* map_b3_or_null, const float* table, const void* packed, float* out,
                                        float* grad_or_null, void* stream) {
    FieldBinding F;
    int rc = field_open(desc, &F);
    if (rc != IRON_OK) return rc;
    if (n < 0) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!p || !out) return IRON_ERR_BAD_ARG;
    rc = field_bind(&F, map_a3_or_null, map_b3_or_null, table, packed);
    if (rc != IRON_OK) return rc;
    if (n > (int64_t)0x7fffffff * 32) return IRON_ERR_RANGE;   // behind the pointers: a null one is a bad argument whatever n is
    return field_dispatch(F, p, n, out, grad_or_null, (hipStream_t)stream);
}
