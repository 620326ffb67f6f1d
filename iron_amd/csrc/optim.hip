// The tail of the stage-2 training step (render_surface.py:533-653) that is neither rendering nor an image loss: the optimiser
// and the regularisers.  C ABI in include/iron_train.h; Python side in iron_amd/optim.py (FusedAdam) and
// iron_amd/image_losses.py (surface_regularisers).
//
// iron_adam_multi: torch.optim.Adam (no weight decay, no amsgrad) over a HOST table of tensors in as few launches as the table
// allows.  The table is copied into the kernel's argument block (AdamLaunch, under 4 KiB: kAdamMaxTensors slots), so a step
// uploads nothing, allocates nothing and never waits for the device.  Every tensor is cut into chunks of IRON_ADAM_CHUNK
// elements; workgroup b finds its slot by a binary search over the slots' first-chunk numbers.  A chunk whose four pointers are
// all 16-byte aligned moves float4s and finishes its last 1..3 elements one by one; any other chunk (the ABI promises 4-byte
// alignment only) takes the scalar path throughout.  The arithmetic is torch's, operation by operation, with the last multiply-add
// of each of its three kernels (lerp, addcmul, addcdiv) fused, one rounding less each -- written as fmaf, because this
// translation unit is built with -ffp-contract=off; sqrtf and / are correctly rounded:
//     m = fma(1 - b1, g - m, m);  v = fma((1 - b2) g, g, v b2);  p = fma(-lr / (1 - b1^t), m / (sqrt(v) / sqrt(1 - b2^t) + eps), p)
// with both bias corrections formed in fp64 on the host and rounded once.
//
// iron_surface_reg: the eikonal and roughness-range terms of render_surface.py:580-613, 639 over three sets of 3-vectors (the
// uniform eikonal gradients, the frame's normals under the mask, the edge normals) and the masked roughness map.
//   k_reg_partial   one workgroup per kRegSpan items of the concatenated index space: six block sums -> one slot (fixed_sum.h)
//   k_reg_final     one workgroup: the slots' totals (fixed_sum.h), then the two losses, the counts and the backward's scales
//   k_reg_backward  one thread per item: 2 (|g| - 1) g / |g| w / cnt (0 for a zero vector), w / n on the selected roughness
// No atomics anywhere: forward and backward are bitwise reproducible.
#include <cmath>

#include "fixed_sum.h"
#include "train_common.h"

using namespace iron_train;

namespace {

// ================================================= multi-tensor Adam ==========================================================

constexpr int kAdamChunk = IRON_ADAM_CHUNK;
constexpr int kAdamMaxTensors = IRON_ADAM_MAX_TENSORS;
constexpr int64_t kAdamPiece = (int64_t)1 << 30;       // a longer tensor takes several slots (numel is 32-bit in a slot)
constexpr uint32_t kAdamMaxChunks = 1u << 22;          // chunks (= workgroups) per launch

struct AdamSlot {
    float* p;
    float* g;
    float* m;
    float* v;
    float neg_step;      // -lr / (1 - b1^t)
    float bc2_sqrt;      // sqrt(1 - b2^t)
    uint32_t numel;
    uint32_t first_chunk;
};

struct AdamLaunch {
    AdamSlot slot[kAdamMaxTensors];
    int32_t n;
    int32_t zero_grad;
    float w1, b2, w2, eps;   // 1 - b1, b2, 1 - b2
};
static_assert(sizeof(AdamLaunch) <= 4096, "the table travels in the kernel's argument block");
static_assert(kAdamChunk % (4 * kThreads) == 0, "a chunk is a whole number of float4 rounds");

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamLaunch& L, float neg_step, float bc2_sqrt) {
    m = fmaf(L.w1, g - m, m);
    v = fmaf(L.w2 * g, g, v * L.b2);
    const float denom = sqrtf(v) / bc2_sqrt + L.eps;
    p = fmaf(neg_step, m / denom, p);
}

__global__ __launch_bounds__(kThreads) void k_adam(const AdamLaunch L) {
    const uint32_t chunk = blockIdx.x;
    int lo = 0, hi = L.n;   // the last slot whose first chunk is <= chunk
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (L.slot[mid].first_chunk <= chunk) lo = mid;
        else hi = mid;
    }
    const AdamSlot s = L.slot[lo];
    const uint32_t off = (chunk - s.first_chunk) * (uint32_t)kAdamChunk;
    if (off >= s.numel) return;
    const uint32_t len = min((uint32_t)kAdamChunk, s.numel - off);
    float* __restrict__ P = s.p + off;
    float* __restrict__ G = s.g + off;
    float* __restrict__ M = s.m + off;
    float* __restrict__ V = s.v + off;
    const bool zero = L.zero_grad != 0;
    const bool aligned = ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0;
    uint32_t done = 0;
    if (aligned) {
        const uint32_t quads = len >> 2;
        for (uint32_t q = threadIdx.x; q < quads; q += kThreads) {
            float4 p = reinterpret_cast<float4*>(P)[q];
            const float4 g = reinterpret_cast<const float4*>(G)[q];
            float4 m = reinterpret_cast<float4*>(M)[q];
            float4 v = reinterpret_cast<float4*>(V)[q];
            adam_one(p.x, g.x, m.x, v.x, L, s.neg_step, s.bc2_sqrt);
            adam_one(p.y, g.y, m.y, v.y, L, s.neg_step, s.bc2_sqrt);
            adam_one(p.z, g.z, m.z, v.z, L, s.neg_step, s.bc2_sqrt);
            adam_one(p.w, g.w, m.w, v.w, L, s.neg_step, s.bc2_sqrt);
            reinterpret_cast<float4*>(P)[q] = p;
            reinterpret_cast<float4*>(M)[q] = m;
            reinterpret_cast<float4*>(V)[q] = v;
            if (zero) reinterpret_cast<float4*>(G)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        done = quads << 2;
    }
    for (uint32_t i = done + threadIdx.x; i < len; i += kThreads) {
        float p = P[i], m = M[i], v = V[i];
        adam_one(p, G[i], m, v, L, s.neg_step, s.bc2_sqrt);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (zero) G[i] = 0.f;
    }
}

// ================================================= surface regularisers =======================================================

constexpr int kRegPerThread = 8;
constexpr int kRegSpan = kThreads * kRegPerThread;   // items of the concatenated index space per workgroup
constexpr int kRegVals = 6;                          // sum_uniform, sum_masked, sum_edge, sum_rough, n_mask, n_sel

__device__ __forceinline__ float vec_norm(const float* __restrict__ g) {
    return sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
}

__global__ __launch_bounds__(kThreads) void k_reg_partial(iron_surface_reg_args a, double* __restrict__ part) {
    __shared__ double red[kThreads];
    const int64_t total = a.m + a.n_pix + a.e;
    const int64_t base = (int64_t)blockIdx.x * kRegSpan;
    double acc[kRegVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < kRegPerThread; ++k) {
        const int64_t i = base + (int64_t)k * kThreads + threadIdx.x;
        if (i >= total) break;
        if (i < a.m) {
            const float d = vec_norm(a.eik_grad + 3 * i) - 1.f;
            acc[0] += (double)(d * d);
        } else if (i < a.m + a.n_pix) {
            const int64_t px = i - a.m;
            if (a.mask[px]) {
                const float d = vec_norm(a.normal + 3 * px) - 1.f;
                acc[1] += (double)(d * d);
                acc[4] += 1.0;
                const float r = a.roughness[px];
                if (r > 0.5f) {
                    acc[3] += (double)(r - 0.5f);
                    acc[5] += 1.0;
                }
            }
        } else {
            const float d = vec_norm(a.edge_normal + 3 * (i - a.m - a.n_pix)) - 1.f;
            acc[2] += (double)(d * d);
        }
    }
    fixed_sum::store_slot<kThreads>(acc, part, red);
}

// state: [0] eik_weight / cnt, [1] roughrange_weight / n_sel (0: none selected), [2] 1 when the masked and edge sets count
__global__ __launch_bounds__(kThreads) void k_reg_final(iron_surface_reg_args a, const double* __restrict__ part, int64_t nb,
                                                       float* __restrict__ eik_loss, float* __restrict__ rr_loss,
                                                       int64_t* __restrict__ counts, double* __restrict__ state) {
    __shared__ double red[kThreads];
    double tot[kRegVals];
    fixed_sum::load_slots<kThreads>(part, nb, tot, red);
    if (threadIdx.x != 0) return;
    const int64_t n_mask = (int64_t)tot[4], n_sel = (int64_t)tot[5];
    const bool on = n_mask > 0;   // render_surface.py:591: the masked and the edge set enter only under mask.any()
    const int64_t cnt = a.m + (on ? n_mask + a.e : 0);
    const double sum = tot[0] + (on ? tot[1] + tot[2] : 0.0);
    const double ws = cnt > 0 ? (double)a.eik_weight / (double)cnt : 0.0;
    const double wr = n_sel > 0 ? (double)a.roughrange_weight / (double)n_sel : 0.0;
    *eik_loss = (float)(sum * ws);
    *rr_loss = (float)(tot[3] * wr);
    counts[0] = cnt;
    counts[1] = n_mask;
    counts[2] = n_sel;
    state[0] = ws;
    state[1] = wr;
    state[2] = on ? 1.0 : 0.0;
    state[3] = 0.0;
}

__device__ __forceinline__ void eik_seed(const float* __restrict__ g, float scale, float* __restrict__ out) {
    const float n = vec_norm(g);
    const float f = n > 0.f ? (2.f * (n - 1.f) * scale) / n : 0.f;   // torch's norm backward: a zero vector gets zero
    out[0] = g[0] * f;
    out[1] = g[1] * f;
    out[2] = g[2] * f;
}

__global__ __launch_bounds__(kThreads) void k_reg_backward(iron_surface_reg_args a, const double* __restrict__ state,
                                                          const float* __restrict__ d_eik, const float* __restrict__ d_rr,
                                                          float* __restrict__ d_eik_grad, float* __restrict__ d_normal,
                                                          float* __restrict__ d_rough, float* __restrict__ d_edge) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.m + a.n_pix + a.e) return;
    const float se = (float)((d_eik ? (double)*d_eik : 0.0) * state[0]);
    const float sr = (float)((d_rr ? (double)*d_rr : 0.0) * state[1]);
    const bool on = state[2] != 0.0;
    if (i < a.m) {
        if (d_eik_grad) eik_seed(a.eik_grad + 3 * i, se, d_eik_grad + 3 * i);
    } else if (i < a.m + a.n_pix) {
        const int64_t px = i - a.m;
        const bool in = a.mask[px] != 0;
        if (d_normal) {
            if (in) eik_seed(a.normal + 3 * px, se, d_normal + 3 * px);
            else d_normal[3 * px] = d_normal[3 * px + 1] = d_normal[3 * px + 2] = 0.f;
        }
        if (d_rough) d_rough[px] = in && a.roughness[px] > 0.5f ? sr : 0.f;
    } else if (d_edge) {
        const int64_t k = i - a.m - a.n_pix;
        if (on) eik_seed(a.edge_normal + 3 * k, se, d_edge + 3 * k);
        else d_edge[3 * k] = d_edge[3 * k + 1] = d_edge[3 * k + 2] = 0.f;
    }
}

int reg_args_ok(const iron_surface_reg_args* a) {
    if (!a || a->m < 0 || a->n_pix < 0 || a->e < 0) return 0;
    if (a->m > 0 && !a->eik_grad) return 0;
    if (a->n_pix > 0 && (!a->normal || !a->mask || !a->roughness)) return 0;
    if (a->e > 0 && !a->edge_normal) return 0;
    return 1;
}

}  // namespace

extern "C" {

int iron_adam_multi(const iron_adam_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps, int32_t zero_grad,
                    void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return IRON_ERR_BAD_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return IRON_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_tensors; ++i) {   // the whole table is checked before anything is enqueued
        const iron_adam_tensor& t = tensors[i];
        if (t.numel < 0 || t.step < 1) return IRON_ERR_BAD_ARG;
        if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return IRON_ERR_BAD_ARG;
    }
    AdamLaunch L;
    L.n = 0;
    L.zero_grad = zero_grad;
    L.w1 = (float)(1.0 - beta1);
    L.b2 = (float)beta2;
    L.w2 = (float)(1.0 - beta2);
    L.eps = (float)eps;
    uint32_t chunks = 0;
    auto flush = [&]() -> int {
        if (L.n == 0) return IRON_OK;
        IRON_TRAIN_LAUNCH(k_adam, chunks, kThreads, (hipStream_t)stream, L);
        L.n = 0;
        chunks = 0;
        return IRON_OK;
    };
    for (int64_t i = 0; i < n_tensors; ++i) {
        const iron_adam_tensor& t = tensors[i];
        const double bc1 = 1.0 - std::pow(beta1, (double)t.step);
        const double bc2 = 1.0 - std::pow(beta2, (double)t.step);
        for (int64_t off = 0; off < t.numel; off += kAdamPiece) {
            const int64_t len = t.numel - off < kAdamPiece ? t.numel - off : kAdamPiece;
            const uint32_t nc = (uint32_t)cdiv64(len, kAdamChunk);
            if (L.n == kAdamMaxTensors || chunks + nc > kAdamMaxChunks) {
                const int st = flush();
                if (st != IRON_OK) return st;
            }
            AdamSlot& s = L.slot[L.n++];
            s.p = t.param + off;
            s.g = t.grad + off;
            s.m = t.exp_avg + off;
            s.v = t.exp_avg_sq + off;
            s.neg_step = (float)(-(t.lr / bc1));
            s.bc2_sqrt = (float)std::sqrt(bc2);
            s.numel = (uint32_t)len;
            s.first_chunk = chunks;
            chunks += nc;
        }
    }
    return flush();
}

size_t iron_surface_reg_workspace_bytes(int64_t m, int64_t n_pix, int64_t e) {
    if (m < 0 || n_pix < 0 || e < 0) return 0;
    return slot_bytes(slot_count(m + n_pix + e, kRegSpan), kRegVals);
}

int iron_surface_reg(const iron_surface_reg_args* a, float* eik_loss, float* roughrange_loss, int64_t* counts, double* state,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (!reg_args_ok(a) || !eik_loss || !roughrange_loss || !counts || !state || !workspace) return IRON_ERR_BAD_ARG;
    if (workspace_bytes < iron_surface_reg_workspace_bytes(a->m, a->n_pix, a->e)) return IRON_ERR_WORKSPACE;
    const int64_t nb = slot_count(a->m + a->n_pix + a->e, kRegSpan);
    if (!grid_ok(nb)) return IRON_ERR_UNSUPPORTED;
    double* part = (double*)workspace;
    if (nb > 0) IRON_TRAIN_LAUNCH(k_reg_partial, (unsigned)nb, kThreads, (hipStream_t)stream, *a, part);
    IRON_TRAIN_LAUNCH(k_reg_final, 1, kThreads, (hipStream_t)stream, *a, part, nb, eik_loss, roughrange_loss, counts, state);
    return IRON_OK;
}

int iron_surface_reg_backward(const iron_surface_reg_args* a, const double* state, const float* d_eik, const float* d_roughrange,
                              float* d_eik_grad, float* d_normal, float* d_roughness, float* d_edge_normal, void* stream) {
    if (!reg_args_ok(a) || !state) return IRON_ERR_BAD_ARG;
    const int64_t nb = cdiv64(a->m + a->n_pix + a->e, kThreads);
    if (!grid_ok(nb)) return IRON_ERR_UNSUPPORTED;
    if (nb == 0) return IRON_OK;
    IRON_TRAIN_LAUNCH(k_reg_backward, (unsigned)nb, kThreads, (hipStream_t)stream, *a, state, d_eik, d_roughrange, d_eik_grad, d_normal,
                      d_roughness, d_edge_normal);
    return IRON_OK;
}

}  // extern "C"
