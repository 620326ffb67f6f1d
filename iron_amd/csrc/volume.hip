// Stage-1 (render_volume.py) batch generation and validation tail.  C ABI in include/iron_hip.h; Python side in
// iron_amd/dataset.py (VolumeDataset) and iron_amd/train_volume.py (validate_image).
//
// iron_volume_rays / iron_volume_rays_grid: models/dataset.py:271-300, 335-361 for one view, one thread per ray.  The arithmetic
// is the reference's in its order (this library is built with -ffp-contract=off: every product and sum rounds on its own):
//     p = Kinv (x, y, 1);  v = p / |p|;  d = R v;  o = t;  a = sum d^2;  b = 2 sum o d;  mid = 0.5 (-b) / a;  near, far = mid -+ 1
// The random mode takes the pixel columns and rows as device int64 (torch.randint draws them; no random numbers are made here) and
// gathers colour and mask from the uint8 pictures as v / 255; the grid mode takes the two fp32 coordinate rows torch.linspace
// made and writes the rays in [rows, columns] order.  The matrices are read from device memory: nothing waits for the host.
//
// iron_volume_frame_u8: the tail of validate_image (render_volume.py:696-729) for one batch of rays, one thread per ray walking
// its samples in order.
#include "iron_common.h"

namespace iron {

struct RayOut {
    float o[3], d[3], near, far;
};

__device__ __forceinline__ RayOut volume_ray(const float* __restrict__ kinv, const float* __restrict__ pose, float x, float y) {
    float p[3], v[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = kinv[4 * r] * x + kinv[4 * r + 1] * y + kinv[4 * r + 2] * 1.0f;
    const float len = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = p[r] / len;
    RayOut out;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out.d[r] = pose[4 * r] * v[0] + pose[4 * r + 1] * v[1] + pose[4 * r + 2] * v[2];
        out.o[r] = pose[4 * r + 3];
    }
    const float a = out.d[0] * out.d[0] + out.d[1] * out.d[1] + out.d[2] * out.d[2];
    const float b = 2.0f * (out.o[0] * out.d[0] + out.o[1] * out.d[1] + out.o[2] * out.d[2]);
    const float mid = (0.5f * (-b)) / a;
    out.near = mid - 1.0f;
    out.far = mid + 1.0f;
    return out;
}

__global__ __launch_bounds__(256) void k_volume_rays(const uint8_t* __restrict__ image, int H, int W, int C,
                                                     const uint8_t* __restrict__ mask, int Cm, const float* __restrict__ kinv,
                                                     const float* __restrict__ pose, const int64_t* __restrict__ px,
                                                     const int64_t* __restrict__ py, int64_t n, float* __restrict__ data,
                                                     float* __restrict__ near, float* __restrict__ far) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t x = px[i], y = py[i];
    const RayOut r = volume_ray(kinv, pose, (float)x, (float)y);
    float* __restrict__ row = data + 10 * i;
    row[0] = r.o[0], row[1] = r.o[1], row[2] = r.o[2];
    row[3] = r.d[0], row[4] = r.d[1], row[5] = r.d[2];
    const bool in = x >= 0 && x < W && y >= 0 && y < H;   // torch.randint(0, W) never leaves the picture; a caller's own list may
    const int64_t pix = in ? y * W + x : 0;
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int c = 0; c < 3; ++c) row[6 + c] = in ? (float)image[pix * C + c] / 255.0f : nan;
    row[9] = !in ? nan : (mask ? (float)mask[pix * Cm] / 255.0f : 1.0f);
    near[i] = r.near;
    far[i] = r.far;
}

__global__ __launch_bounds__(256) void k_volume_rays_grid(const float* __restrict__ kinv, const float* __restrict__ pose,
                                                          const float* __restrict__ tx, const float* __restrict__ ty, int rows, int cols,
                                                          float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    const int row = (int)(i / cols), col = (int)(i % cols);
    const RayOut r = volume_ray(kinv, pose, tx[col], ty[row]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rays_o[3 * i + c] = r.o[c];
        rays_d[3 * i + c] = r.d[c];
    }
}

__device__ __forceinline__ uint8_t clip_u8(float v) {
    v = fminf(fmaxf(v, 0.0f), 255.0f);   // numpy's clip(0, 255), then astype(uint8): truncation
    return (uint8_t)(int)v;
}

__global__ __launch_bounds__(256) void k_volume_frame_u8(const float* __restrict__ color, const float* __restrict__ gradients,
                                                         const float* __restrict__ weights, const float* __restrict__ inside,
                                                         const float* __restrict__ rot, int64_t n, int m, int mw, int64_t offset,
                                                         uint8_t* __restrict__ rgb_frame, uint8_t* __restrict__ normal_frame) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t at = 3 * (offset + i);
    if (rgb_frame) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb_frame[at + c] = clip_u8(color[3 * i + c] * 256.0f);
    }
    if (!normal_frame) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    const float* __restrict__ g = gradients + (size_t)i * m * 3;
    const float* __restrict__ w = weights + (size_t)i * mw;
    const float* __restrict__ in = inside ? inside + (size_t)i * m : nullptr;
    for (int j = 0; j < m; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = g[3 * j + c] * wj;
            if (in) t = t * in[j];
            acc[c] += t;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v = rot[3 * r] * acc[0] + rot[3 * r + 1] * acc[1] + rot[3 * r + 2] * acc[2];
        normal_frame[at + r] = clip_u8(v * 128.0f + 128.0f);
    }
}

static inline int64_t vol_blocks(int64_t n) { return (n + 255) / 256; }

}  // namespace iron

using namespace iron;

extern "C" int iron_volume_rays(const uint8_t* image, int32_t h, int32_t w, int32_t c, const uint8_t* mask, int32_t cm,
                                const float* kinv44, const float* pose44, const int64_t* px, const int64_t* py, int64_t n, float* data,
                                float* near, float* far, void* stream) {
    if (n < 0 || h < 1 || w < 1 || c < 3 || (mask && cm < 1) || !image || !kinv44 || !pose44) return IRON_ERR_BAD_ARG;
    if (n > 0 && (!px || !py || !data || !near || !far)) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (vol_blocks(n) > 0x7fffffff) return IRON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_volume_rays, dim3((unsigned)vol_blocks(n)), dim3(256), 0, (hipStream_t)stream, image, h, w, c, mask, cm, kinv44,
                       pose44, px, py, n, data, near, far);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_volume_rays_grid(const float* kinv44, const float* pose44, const float* tx, const float* ty, int32_t rows,
                                     int32_t cols, float* rays_o, float* rays_d, void* stream) {
    if (rows < 0 || cols < 0 || !kinv44 || !pose44) return IRON_ERR_BAD_ARG;
    const int64_t n = (int64_t)rows * cols;
    if (n > 0 && (!tx || !ty || !rays_o || !rays_d)) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (vol_blocks(n) > 0x7fffffff) return IRON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_volume_rays_grid, dim3((unsigned)vol_blocks(n)), dim3(256), 0, (hipStream_t)stream, kinv44, pose44, tx, ty, rows,
                       cols, rays_o, rays_d);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_volume_frame_u8(const float* color, const float* gradients, const float* weights, const float* inside_sphere,
                                    const float* rot33, int64_t n, int32_t m, int32_t mw, int64_t offset, int64_t frame_rays,
                                    uint8_t* rgb_frame, uint8_t* normal_frame, void* stream) {
    if (n < 0 || m < 0 || mw < m || offset < 0 || frame_rays < 0 || offset + n > frame_rays) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!rgb_frame && !normal_frame) return IRON_ERR_BAD_ARG;
    if (rgb_frame && !color) return IRON_ERR_BAD_ARG;
    if (normal_frame && (!rot33 || (m > 0 && (!gradients || !weights)))) return IRON_ERR_BAD_ARG;
    if (vol_blocks(n) > 0x7fffffff) return IRON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_volume_frame_u8, dim3((unsigned)vol_blocks(n)), dim3(256), 0, (hipStream_t)stream, color, gradients, weights,
                       inside_sphere, rot33, n, m, mw, offset, rgb_frame, normal_frame);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}
