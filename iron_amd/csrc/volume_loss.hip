// The loss of the stage-1 training step (render_volume.py:458-496, and the statistics of :507-510) in one launch chain.  C ABI
// in include/iron_train.h; Python side in iron_amd/image_losses.py (volume_losses) over iron_amd.autograd.VolumeLossFn.
//
//   k_vloss_partial   one workgroup per kVlSpan rays: per-ray values in fp32 as torch forms them, six block sums in fp64 -> one
//                     slot of the workspace (fixed_sum.h)
//   k_vloss_final     one workgroup: the slots' totals (fixed_sum.h), then the scalars of the record and the backward's scales
//   k_vloss_backward  one thread per ray: d color_fine, d weight_sum (and thread 0: d gradient_error)
// No atomics anywhere, and the cut into workgroups is fixed by the batch size alone: forward and backward are bitwise reproducible.
//
// Per ray (fp32):  m = raw > 0.5 (mask_weight > 0) or 1;  e = (c - t) m;  |e|;  (c - t)^2 m;  w = clip(weight_sum, 1e-3, 1 - 1e-3);
// bce = (m - 1) max(log(1 - w), -100) - m max(log(w), -100) (torch's binary_cross_entropy);  cdf m;  weight_max m.
// Scalars (fp64 from the fp64 sums, rounded once to fp32):  mask_sum = sum m + 1e-5;  color = sum |e| / mask_sum;
// psnr = 20 log10(1 / sqrt(sum (c - t)^2 m / (3 mask_sum)));  mask_loss = sum bce / B;  loss = color + igr_weight gradient_error +
// mask_weight mask_loss.
#include <cmath>

#include "fixed_sum.h"
#include "train_common.h"

using namespace iron_train;

namespace {

constexpr int kVlPerThread = 8;
constexpr int kVlSpan = kThreads * kVlPerThread;   // rays per workgroup
constexpr int kVlVals = 6;                         // sum |e|, sum sq, sum bce, sum cdf m, sum weight_max m, sum m
constexpr float kClipLo = 1e-3f;                   // torch clamps a float tensor at the bounds rounded to float
constexpr float kClipHi = (float)(1.0 - 1e-3);

__device__ __forceinline__ float ray_mask(const iron_volume_loss_args& a, int64_t i) {
    if (!(a.mask_weight > 0.f)) return 1.f;
    return a.mask[i * a.mask_stride] > 0.5f ? 1.f : 0.f;
}

__global__ __launch_bounds__(kThreads) void k_vloss_partial(iron_volume_loss_args a, double* __restrict__ part) {
    __shared__ double red[kThreads];
    const int64_t base = (int64_t)blockIdx.x * kVlSpan;
    double acc[kVlVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < kVlPerThread; ++k) {
        const int64_t i = base + (int64_t)k * kThreads + threadIdx.x;
        if (i >= a.b) break;
        const float m = ray_mask(a, i);
        const float* __restrict__ c = a.color_fine + 3 * i;
        const float* __restrict__ t = a.true_rgb + i * a.rgb_stride;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float d = c[ch] - t[ch];
            acc[0] += (double)fabsf(d * m);
            acc[1] += (double)((d * d) * m);
        }
        const float w = fminf(fmaxf(a.weight_sum[i], kClipLo), kClipHi);
        const float bce = (m - 1.f) * fmaxf(logf(1.f - w), -100.f) - m * fmaxf(logf(w), -100.f);
        acc[2] += (double)bce;
        acc[3] += (double)(a.cdf_fine[i * a.cdf_stride] * m);
        acc[4] += (double)(a.weight_max[i] * m);
        acc[5] += (double)m;
    }
    fixed_sum::store_slot<kThreads>(acc, part, red);
}

// state: [0] 1 / mask_sum, [1] mask_weight / B, [2] igr_weight
__global__ __launch_bounds__(kThreads) void k_vloss_final(iron_volume_loss_args a, const double* __restrict__ part, int64_t nb,
                                                         float* __restrict__ loss, float* __restrict__ record,
                                                         double* __restrict__ state) {
    __shared__ double red[kThreads];
    double tot[kVlVals];
    fixed_sum::load_slots<kThreads>(part, nb, tot, red);
    if (threadIdx.x != 0) return;
    const double mask_sum = tot[5] + 1e-5;
    const double color = tot[0] / mask_sum;
    const double eik = (double)*a.gradient_error;
    const double mask_loss = tot[2] / (double)a.b;
    const double psnr = 20.0 * log10(1.0 / sqrt(tot[1] / (mask_sum * 3.0)));   // +inf when prediction equals target
    const double total = color + eik * (double)a.igr_weight + mask_loss * (double)a.mask_weight;
    *loss = (float)total;
    record[IRON_VL_LOSS] = (float)total;
    record[IRON_VL_COLOR] = (float)color;
    record[IRON_VL_EIKONAL] = (float)eik;
    record[IRON_VL_MASK] = (float)mask_loss;
    record[IRON_VL_PSNR] = (float)psnr;
    record[IRON_VL_CDF] = (float)(tot[3] / mask_sum);
    record[IRON_VL_WEIGHT_MAX] = (float)(tot[4] / mask_sum);
    record[IRON_VL_MASK_SUM] = (float)mask_sum;
    state[0] = 1.0 / mask_sum;
    state[1] = (double)a.mask_weight / (double)a.b;
    state[2] = (double)a.igr_weight;
    state[3] = 0.0;
}

__global__ __launch_bounds__(kThreads) void k_vloss_backward(iron_volume_loss_args a, const double* __restrict__ state,
                                                            const float* __restrict__ d_loss, float* __restrict__ d_color,
                                                            float* __restrict__ d_weight_sum, float* __restrict__ d_gradient_error) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const double up = d_loss ? (double)*d_loss : 1.0;
    if (i == 0 && d_gradient_error) *d_gradient_error = (float)(state[2] * up);
    if (i >= a.b) return;
    const float m = ray_mask(a, i);
    if (d_color) {
        const float sc = (float)(state[0] * up);
        const float* __restrict__ c = a.color_fine + 3 * i;
        const float* __restrict__ t = a.true_rgb + i * a.rgb_stride;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float e = (c[ch] - t[ch]) * m;
            const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);   // torch's L1 backward: sign(0) = 0
            d_color[3 * i + ch] = (sg * m) * sc;
        }
    }
    if (d_weight_sum) {
        const float w = a.weight_sum[i];
        float g = 0.f;
        if (w >= kClipLo && w <= kClipHi)   // torch's clamp passes the gradient on the closed interval
            g = (-m / w + (1.f - m) / (1.f - w)) * (float)(state[1] * up);
        d_weight_sum[i] = g;
    }
}

int vloss_args_ok(const iron_volume_loss_args* a) {
    if (!a || a->b < 1 || a->rgb_stride < 3 || a->mask_stride < 1 || a->cdf_stride < 1) return 0;
    if (!a->color_fine || !a->true_rgb || !a->weight_sum || !a->weight_max || !a->cdf_fine || !a->gradient_error) return 0;
    if (a->mask_weight > 0.f && !a->mask) return 0;
    return 1;
}

}  // namespace

extern "C" {

size_t iron_volume_loss_workspace_bytes(int64_t b) {
    if (b < 0) return 0;
    return slot_bytes(slot_count(b, kVlSpan), kVlVals);
}

int iron_volume_loss(const iron_volume_loss_args* a, float* loss, float* record, double* state, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!vloss_args_ok(a) || !loss || !record || !state || !workspace) return IRON_ERR_BAD_ARG;
    if (workspace_bytes < iron_volume_loss_workspace_bytes(a->b)) return IRON_ERR_WORKSPACE;
    const int64_t nb = slot_count(a->b, kVlSpan);
    if (!grid_ok(nb)) return IRON_ERR_UNSUPPORTED;
    double* part = (double*)workspace;
    IRON_TRAIN_LAUNCH(k_vloss_partial, (unsigned)nb, kThreads, (hipStream_t)stream, *a, part);
    IRON_TRAIN_LAUNCH(k_vloss_final, 1, kThreads, (hipStream_t)stream, *a, part, nb, loss, record, state);
    return IRON_OK;
}

int iron_volume_loss_backward(const iron_volume_loss_args* a, const double* state, const float* d_loss, float* d_color,
                              float* d_weight_sum, float* d_gradient_error, void* stream) {
    if (!vloss_args_ok(a) || !state) return IRON_ERR_BAD_ARG;
    const int64_t nb = cdiv64(a->b, kThreads);
    if (!grid_ok(nb)) return IRON_ERR_UNSUPPORTED;
    IRON_TRAIN_LAUNCH(k_vloss_backward, (unsigned)nb, kThreads, (hipStream_t)stream, *a, state, d_loss, d_color, d_weight_sum,
                      d_gradient_error);
    return IRON_OK;
}

}  // extern "C"
