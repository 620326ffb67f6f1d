// Image evaluation metrics (evaluation/eval_image_folder.py: PSNR, skimage's uniform-window SSIM, LPIPS-AlexNet).
// Conventions: include/iron_hip.h, iron_img_* / iron_lpips_* block.
//
// Every reduction here is a fixed-order sum (fixed_sum.h): a kernel leaves one fp64 partial per workgroup (or per wave) in the
// caller's workspace and k_reduce_f64 / k_lpips_final add them -- no float atomics, so every output is bitwise reproducible.
//
//   iron_img_sqerr   k_sqerr<T>      uint8: integer differences, exact uint64 sums; fp32: difference and square in fp32, fp64 sums
//   iron_img_ssim    k_ssim<T, Acc>  one workgroup = a 16 x 32 tile of S of one channel: the (16+10) x (32+10) input tile in LDS, the
//                                    five 11-wide row sums of every tile row (Acc = int32 for uint8: exact; fp64 for fp32 input,
//                                    products included), then the 11-high column sums, S in fp64, tile sum
//   LPIPS            k_lpips_prepare image pair -> [2, H, W, 3] fp32, (2 x - 1 - shift) / scale
//                    k_conv_h2       convolution + bias + ReLU as an implicit GEMM over NHWC activations: rows = output pixels of
//                                    both images, columns = output channels, k = (ky, kx, c); the patch rows are gathered straight
//                                    from the activation (no im2col buffer), both operands split into fp16 hi / lo pieces on the way
//                                    into LDS (fragment order of gemm_h2.h), three v_mfma_f32_32x32x16_f16 per fragment pair
//                    k_maxpool3s2    3 x 3 / 2 max-pool, NHWC
//                    k_lpips_tap     one wave per pixel: both channel norms, the squared difference of the unit vectors, the lin
//                                    dot product (fp64), per-wave spatial sums
//                    k_lpips_final   the five layer means added in order; NaN and a raised flag word if an operand left fp16 range
#include "fixed_sum.h"
#include "host_util.h"

namespace iron {

using fixed_sum::block_sum;
using fixed_sum::slot_sum;

typedef _Float16 im_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 im_half2 __attribute__((ext_vector_type(2)));
typedef float im_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int im_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kImBlock = 256;
constexpr int kImSqerrBlocks = 1024;   // partials of iron_img_sqerr
constexpr int kImTapBlocks = 256;      // k_lpips_tap: 4 waves each, one partial per wave
constexpr int kImTapPartials = kImTapBlocks * 4;

// out[g] = scale * (the fixed-order sum of partials[g * n .. g * n + n))
__global__ __launch_bounds__(kImBlock) void k_reduce_f64(const double* __restrict__ partials, int n, double scale, double* __restrict__ out) {
    __shared__ double s[kImBlock];
    const double r = slot_sum<kImBlock>(partials + (size_t)blockIdx.x * n, n, 1, s);
    if (threadIdx.x == 0) out[blockIdx.x] = r * scale;
}

// ------------------------------------------------------------------------------------------------------------ squared error
template <typename T>
__global__ __launch_bounds__(kImBlock) void k_sqerr(const T* __restrict__ a, const T* __restrict__ b, int64_t count, double* __restrict__ partials) {
    __shared__ double s[kImBlock];
    const int64_t stride = (int64_t)gridDim.x * kImBlock;
    double acc = 0.0;
    if constexpr (sizeof(T) == 1) {
        unsigned long long ia = 0;  // exact: at most 2^31 terms of at most 255^2
        for (int64_t i = (int64_t)blockIdx.x * kImBlock + threadIdx.x; i < count; i += stride) {
            const int d = (int)a[i] - (int)b[i];
            ia += (unsigned)(d * d);
        }
        acc = (double)ia;           // < 2^53: still exact, and so is every partial sum of the tree below
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kImBlock + threadIdx.x; i < count; i += stride) {
            const float d = a[i] - b[i];
            acc += (double)(d * d);  // the square rounded to fp32 as numpy's (pred - trgt) ** 2 on float32 arrays
        }
    }
    const double r = block_sum<kImBlock>(acc, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

__global__ void k_set_f64(double* p, double v) { *p = v; }

// ---------------------------------------------------------------------------------------------------------------------- SSIM
constexpr int kSsTW = 32, kSsTH = 16, kSsWin = 11, kSsIW = kSsTW + kSsWin - 1, kSsIH = kSsTH + kSsWin - 1;

// x, y: [H, W, 3]; blockIdx = (tile x, tile y, channel).  S exists for (oy, ox) in [0, H - 10) x [0, W - 10): the window of S(oy, ox)
// is rows oy .. oy + 10, columns ox .. ox + 10 (skimage's crop of 5 pixels on every side).  Tile pixels beyond the image are read as
// 0 and only reach outputs that are discarded.
template <typename T, typename Acc>
__global__ __launch_bounds__(kImBlock) void k_ssim(const T* __restrict__ x, const T* __restrict__ y, int H, int W, double* __restrict__ partials,
                                                  double* __restrict__ smap) {
    __shared__ T sx[kSsIH][kSsIW], sy[kSsIH][kSsIW];
    __shared__ Acc hs[5][kSsIH][kSsTW];
    __shared__ double red[kImBlock];
    const int tid = threadIdx.x, ch = blockIdx.z;
    const int tx0 = blockIdx.x * kSsTW, ty0 = blockIdx.y * kSsTH;
    const int OW = W - (kSsWin - 1), OH = H - (kSsWin - 1);
    for (int i = tid; i < kSsIH * kSsIW; i += kImBlock) {
        const int r = i / kSsIW, c = i - r * kSsIW;
        const int gy = ty0 + r, gx = tx0 + c;
        T a = 0, b = 0;
        if (gy < H && gx < W) {
            const size_t o = ((size_t)gy * W + gx) * 3 + ch;
            a = x[o];
            b = y[o];
        }
        sx[r][c] = a;
        sy[r][c] = b;
    }
    __syncthreads();
    for (int i = tid; i < kSsIH * kSsTW; i += kImBlock) {   // row sums, left to right
        const int r = i / kSsTW, c = i - r * kSsTW;
        Acc s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int j = 0; j < kSsWin; ++j) {
            const T a = sx[r][c + j], b = sy[r][c + j];
            if constexpr (sizeof(T) == 1) {
                const int ia = a, ib = b;
                s0 += ia; s1 += ib; s2 += ia * ia; s3 += ib * ib; s4 += ia * ib;
            } else {
                const Acc da = a, db = b;   // fp32 input: products and sums in fp64 (a product of two fp32 values is exact there)
                s0 += da; s1 += db; s2 += da * da; s3 += db * db; s4 += da * db;
            }
        }
        hs[0][r][c] = s0; hs[1][r][c] = s1; hs[2][r][c] = s2; hs[3][r][c] = s3; hs[4][r][c] = s4;
    }
    __syncthreads();
    double local = 0.0;
    for (int i = tid; i < kSsTH * kSsTW; i += kImBlock) {   // column sums, top to bottom; two outputs per thread
        const int r = i / kSsTW, c = i - r * kSsTW;
        Acc s[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kSsWin; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) s[q] += hs[q][r + j][c];
        // uint8: the means of k / 255; 121 * 255 and 121 * 255^2 divide the exact integer sums once
        const double n1 = sizeof(T) == 1 ? 121.0 * 255.0 : 121.0, n2 = sizeof(T) == 1 ? 121.0 * 65025.0 : 121.0;
        const double ux = (double)s[0] / n1, uy = (double)s[1] / n1;
        const double vx = (double)s[2] / n2 - ux * ux, vy = (double)s[3] / n2 - uy * uy, vxy = (double)s[4] / n2 - ux * uy;
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
        const int oy = ty0 + r, ox = tx0 + c;
        if (oy < OH && ox < OW) {
            local += S;
            if (smap) smap[((size_t)ch * OH + oy) * OW + ox] = S;
        }
    }
    const double rsum = block_sum<kImBlock>(local, red);
    if (tid == 0) partials[(size_t)ch * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = rsum;
}

// --------------------------------------------------------------------------------------------------------------------- LPIPS
__constant__ float kLpShift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float kLpScale[3] = {0.458f, 0.448f, 0.450f};

// out [2, H, W, 3]: image 0 = pred, 1 = trgt; uint8 k -> float(k) / 255 as the reference's reader; then 2 x - 1 and the scaling layer
template <typename T>
__global__ __launch_bounds__(kImBlock) void k_lpips_prepare(const T* __restrict__ pred, const T* __restrict__ trgt, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kImBlock + threadIdx.x;
    if (i >= 2 * n) return;
    const int64_t j = i < n ? i : i - n;
    const T raw = i < n ? pred[j] : trgt[j];
    float v;
    if constexpr (sizeof(T) == 1) v = (float)raw / 255.0f; else v = raw;
    const int c = (int)(j % 3);
    out[i] = ((v * 2.0f - 1.0f) - kLpShift[c]) / kLpScale[c];
}

struct ConvArgs {
    const float* in;    // [B, H, W, Cin]
    const float* w;     // [Cout, ks, ks, Cin] = [Cout, K]
    const float* bias;  // [Cout]
    float* out;         // [B, Ho, Wo, Cout] = [M, Cout]
    int* flag;          // raised when an operand element has no fp16 high piece
    int B, H, W, Cin, Cout, ks, stride, pad, Ho, Wo, M, K;
};

// Workgroup tile 128 output pixels x 64 output channels, K 32 at a time through a double-buffered LDS stage; four waves, each a
// 64 x 32 quadrant (two A fragments against one B fragment: six ds_read_b128 feed six MFMAs per k-step).  LDS image of a stage, as
// in gemm_h2.h: fragment = 32 rows x 16 k x fp16 = 1 KiB, lane (k-half, row % 32) x 16 B; operand image = [row tile][k-step][hi, lo].
constexpr int kCvTM = 128, kCvTN = 64, kCvTK = 32;
constexpr int kCvABytes = 4 * 2 * 2 * 1024, kCvBBytes = 2 * 2 * 2 * 1024, kCvStageBytes = kCvABytes + kCvBBytes;
constexpr float kCvLoScale = 2048.0f, kCvLoInv = 1.0f / 2048.0f;

// 8 fp32 -> 8 fp16 high pieces + 8 low pieces (x = hi + lo / 2048; both round to nearest, x - f32(hi) is exact)
// (gemm_split8 of gemm_h2.h restated: that header belongs to libiron_train.so and brings its own device flag word and kernels)
__device__ __forceinline__ void cv_split8(const float* v, im_u32x4& hi, im_u32x4& lo, unsigned& bad) {
#pragma unroll
    for (int i = 0; i < 8; ++i) bad |= !(fabsf(v[i]) <= 65504.0f) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        im_half2 h, l;
        h[0] = (_Float16)v[2 * i];
        h[1] = (_Float16)v[2 * i + 1];
        l[0] = (_Float16)((v[2 * i] - (float)h[0]) * kCvLoScale);
        l[1] = (_Float16)((v[2 * i + 1] - (float)h[1]) * kCvLoScale);
        hi[i] = __builtin_bit_cast(unsigned, h);
        lo[i] = __builtin_bit_cast(unsigned, l);
    }
}

// FAST: Cin % 32 == 0, so a K tile is 32 consecutive channels of one tap (ky, kx): 64 contiguous bytes per thread.  Otherwise
// (conv1: Cin = 3, K = 363) every element finds its own (ky, kx, c).
template <bool FAST>
__global__ __launch_bounds__(kImBlock) void k_conv_h2(ConvArgs g) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kCvStageBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * kCvTM, n0 = blockIdx.y * kCvTN;

    // operand A: thread -> patch row tid % 128, k-chunks ac, ac + 1 (16 consecutive k)
    const int ar = tid & 127, ac = (tid >> 7) * 2;
    const int m = m0 + ar;
    const bool mvalid = m < g.M;
    int img = 0, iy0 = 0, ix0 = 0;
    if (mvalid) {
        img = m / (g.Ho * g.Wo);
        const int rem = m - img * (g.Ho * g.Wo);
        const int oy = rem / g.Wo;
        iy0 = oy * g.stride - g.pad;
        ix0 = (rem - oy * g.Wo) * g.stride - g.pad;
    }
    // operand B: thread -> output channel tid % 64, k-chunk bc (8 consecutive k)
    const int br = tid & 63, bc = tid >> 6;
    const int n = n0 + br;
    const bool nvalid = n < g.Cout;
    const bool b_vec = (g.K & 3) == 0;

    float va[16], vb[8];
    unsigned bad = 0;
    auto fetch = [&](int kb) {
        if (FAST) {
            const int tap = kb / g.Cin, c0 = kb - tap * g.Cin + 8 * ac;
            const int ky = tap / g.ks, kx = tap - ky * g.ks;
            const int iy = iy0 + ky, ix = ix0 + kx;
            if (mvalid && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                const float4* p = reinterpret_cast<const float4*>(g.in + (((size_t)img * g.H + iy) * g.W + ix) * g.Cin + c0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 t = p[q];
                    va[4 * q] = t.x; va[4 * q + 1] = t.y; va[4 * q + 2] = t.z; va[4 * q + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) va[i] = 0.0f;
            }
        } else {
            const int kwc = g.ks * g.Cin;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = kb + 8 * ac + i;
                float t = 0.0f;
                if (mvalid && k < g.K) {
                    const int ky = k / kwc, r = k - ky * kwc;
                    const int kx = r / g.Cin, c = r - kx * g.Cin;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) t = g.in[(((size_t)img * g.H + iy) * g.W + ix) * g.Cin + c];
                }
                va[i] = t;
            }
        }
        const int k0 = kb + 8 * bc;
        if (nvalid && b_vec && k0 + 8 <= g.K) {
            const float4* p = reinterpret_cast<const float4*>(g.w + (size_t)n * g.K + k0);
            const float4 a = p[0], b = p[1];
            vb[0] = a.x; vb[1] = a.y; vb[2] = a.z; vb[3] = a.w; vb[4] = b.x; vb[5] = b.y; vb[6] = b.z; vb[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) vb[i] = (nvalid && k0 + i < g.K) ? g.w[(size_t)n * g.K + k0 + i] : 0.0f;
        }
    };
    const int a_off = ((ar >> 5) * 2 + (ac >> 1)) * 2048 + (ar & 31) * 16;                           // chunk ac (even): k-half 0
    const int b_off = kCvABytes + ((br >> 5) * 2 + (bc >> 1)) * 2048 + ((bc & 1) * 32 + (br & 31)) * 16;
    auto stage = [&](char* buf) {
        im_u32x4 hi, lo;
        cv_split8(va, hi, lo, bad);
        *reinterpret_cast<im_u32x4*>(buf + a_off) = hi;
        *reinterpret_cast<im_u32x4*>(buf + a_off + 1024) = lo;
        cv_split8(va + 8, hi, lo, bad);
        *reinterpret_cast<im_u32x4*>(buf + a_off + 512) = hi;                                      // chunk ac + 1: k-half 1
        *reinterpret_cast<im_u32x4*>(buf + a_off + 512 + 1024) = lo;
        cv_split8(vb, hi, lo, bad);
        *reinterpret_cast<im_u32x4*>(buf + b_off) = hi;
        *reinterpret_cast<im_u32x4*>(buf + b_off + 1024) = lo;
    };

    im_f32x16 acc_hi[2], acc_lo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_hi[i][r] = 0.0f; acc_lo[i][r] = 0.0f; }

    int cur = 0;
    fetch(0);
    stage(lds);
    __syncthreads();
    for (int kb = 0; kb < g.K; kb += kCvTK) {
        const bool more = kb + kCvTK < g.K;
        if (more) fetch(kb + kCvTK);   // the next slice's global loads fly under this slice's MFMAs
        const char* buf = lds + cur * kCvStageBytes;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            im_half8 ah[2], al[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int fa = ((wm * 2 + i) * 2 + ks) * 2048 + lane * 16;
                ah[i] = *reinterpret_cast<const im_half8*>(buf + fa);
                al[i] = *reinterpret_cast<const im_half8*>(buf + fa + 1024);
            }
            const int fb = kCvABytes + (wn * 2 + ks) * 2048 + lane * 16;
            const im_half8 bh = *reinterpret_cast<const im_half8*>(buf + fb);
            const im_half8 bl = *reinterpret_cast<const im_half8*>(buf + fb + 1024);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc_lo[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl, acc_lo[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc_hi[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh, acc_hi[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc_lo[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh, acc_lo[i], 0, 0, 0);
        }
        if (more) stage(lds + (cur ^ 1) * kCvStageBytes);   // the other buffer: nobody reads it during this slice
        __syncthreads();
        cur ^= 1;
    }
    if (bad) atomicOr(g.flag, 1);

    // C/D layout of the 32x32 MFMA: lane l holds column l % 32, rows (r % 4) + 8 (r / 4) + 4 (l / 32); bias + ReLU on the way out
    const int on = n0 + wn * 32 + (lane & 31);
    if (on < g.Cout) {
        const float bias = g.bias[on];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int om = m0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (om < g.M) g.out[(size_t)om * g.Cout + on] = fmaxf(fmaf(acc_lo[i][r], kCvLoInv, acc_hi[i][r]) + bias, 0.0f);
            }
    }
}

// in [B, H, W, C] -> out [B, Ho, Wo, C], Ho = (H - 3) / 2 + 1: every window lies inside the input
__global__ __launch_bounds__(kImBlock) void k_maxpool3s2(const float* __restrict__ in, int H, int W, int C, int Ho, int Wo, int64_t total,
                                                        float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kImBlock + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    int64_t t = i / C;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int64_t b = t / Ho;
    const float* p = in + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
    float v = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, p[((size_t)dy * W + dx) * C]);
    out[i] = v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// feat [2, HW, C], C a multiple of 64 and <= 384.  Wave w of the grid takes pixels w, w + n_waves, ...; partials[w] = its sum of
// sum_c lin[c] (f0[c] / (|f0| + 1e-10) - f1[c] / (|f1| + 1e-10))^2, all in fp64.
__global__ __launch_bounds__(kImBlock) void k_lpips_tap(const float* __restrict__ feat, int HW, int C, const float* __restrict__ lin,
                                                       double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int per = C >> 6;
    double l[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) l[q] = q < per ? (double)lin[q * 64 + lane] : 0.0;
    double acc = 0.0;
    for (int p = gw; p < HW; p += nw) {
        const float* f0 = feat + (size_t)p * C;
        const float* f1 = feat + ((size_t)HW + p) * C;
        double a[6], b[6], na = 0.0, nb = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            a[q] = q < per ? (double)f0[q * 64 + lane] : 0.0;
            b[q] = q < per ? (double)f1[q * 64 + lane] : 0.0;
            na += a[q] * a[q];
            nb += b[q] * b[q];
        }
        na = sqrt(wave_sum_f64(na)) + 1e-10;
        nb = sqrt(wave_sum_f64(nb)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double t = a[q] / na - b[q] / nb;
            d += l[q] * (t * t);
        }
        acc += wave_sum_f64(d);
    }
    if (lane == 0) partials[gw] = acc;
}

// partials [5][kImTapPartials]; out[0] = sum_l (sum of layer l's partials) / hw[l], out[1] = 1 if the range flag is up (out[0] NaN)
struct LpFinalArgs { double inv_hw[5]; };
__global__ __launch_bounds__(kImBlock) void k_lpips_final(const double* __restrict__ partials, LpFinalArgs a, const int* __restrict__ flag,
                                                         double* __restrict__ out) {
    __shared__ double s[kImBlock];
    double total = 0.0;
    for (int l = 0; l < 5; ++l) total += slot_sum<kImBlock>(partials + (size_t)l * kImTapPartials, kImTapPartials, 1, s) * a.inv_hw[l];
    if (threadIdx.x == 0) {
        const bool bad = *flag != 0;
        out[0] = bad ? __longlong_as_double(0x7ff8000000000000LL) : total;
        out[1] = bad ? 1.0 : 0.0;
    }
}

// ---- host side ----
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int kImMaxSide = 16384;

static int launch_conv(const float* in, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int ks, int stride,
                       int pad, float* out, int* flag, hipStream_t st) {
    if (!in || !weight || !bias || !out || !flag || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ks <= 0 || stride <= 0 || pad < 0 ||
        H > kImMaxSide || W > kImMaxSide || Cin > 4096 || Cout > 4096 || ks > 31 || pad >= ks)
        return IRON_ERR_BAD_ARG;
    if (H + 2 * pad < ks || W + 2 * pad < ks) return IRON_ERR_BAD_ARG;
    if (!aligned16(in) || !aligned16(weight) || !aligned16(out)) return IRON_ERR_BAD_ARG;
    ConvArgs g;
    g.in = in; g.w = weight; g.bias = bias; g.out = out; g.flag = flag;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.ks = ks; g.stride = stride; g.pad = pad;
    g.Ho = (H + 2 * pad - ks) / stride + 1;
    g.Wo = (W + 2 * pad - ks) / stride + 1;
    const int64_t M = (int64_t)B * g.Ho * g.Wo;
    if (M >= (1LL << 30)) return IRON_ERR_BAD_ARG;
    g.M = (int)M;
    g.K = ks * ks * Cin;
    const dim3 grid((g.M + kCvTM - 1) / kCvTM, (Cout + kCvTN - 1) / kCvTN);
    if (Cin % 32 == 0) hipLaunchKernelGGL(k_conv_h2<true>, grid, dim3(kImBlock), 0, st, g);
    else hipLaunchKernelGGL(k_conv_h2<false>, grid, dim3(kImBlock), 0, st, g);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

static int launch_pool(const float* in, int B, int H, int W, int C, float* out, hipStream_t st) {
    if (!in || !out || B <= 0 || H < 3 || W < 3 || C <= 0 || H > kImMaxSide || W > kImMaxSide || C > 4096) return IRON_ERR_BAD_ARG;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int64_t total = (int64_t)B * Ho * Wo * C;
    if (total >= (1LL << 40)) return IRON_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_maxpool3s2, dim3(blocks_for(total, kImBlock)), dim3(kImBlock), 0, st, in, H, W, C, Ho, Wo, total, out);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

static int launch_tap(const float* feat, int H, int W, int C, const float* lin, double* partials, hipStream_t st) {
    if (!feat || !lin || !partials || H <= 0 || W <= 0 || H > kImMaxSide || W > kImMaxSide || C <= 0 || C % 64 != 0 || C > 384) return IRON_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_lpips_tap, dim3(kImTapBlocks), dim3(kImBlock), 0, st, feat, H * W, C, lin, partials);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

static int launch_prepare(const void* pred, const void* trgt, int H, int W, int is_f32, float* out, hipStream_t st) {
    if (!pred || !trgt || !out || H <= 0 || W <= 0 || H > kImMaxSide || W > kImMaxSide) return IRON_ERR_BAD_ARG;
    const int64_t n = (int64_t)H * W * 3;
    if (is_f32) hipLaunchKernelGGL(k_lpips_prepare<float>, dim3(blocks_for(2 * n, kImBlock)), dim3(kImBlock), 0, st, (const float*)pred, (const float*)trgt, n, out);
    else hipLaunchKernelGGL(k_lpips_prepare<uint8_t>, dim3(blocks_for(2 * n, kImBlock)), dim3(kImBlock), 0, st, (const uint8_t*)pred, (const uint8_t*)trgt, n, out);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

// AlexNet's feature stack as LPIPS taps it: {Cin, Cout, kernel, stride, pad, pool after the tap}
struct LpLayer { int cin, cout, ks, stride, pad, pool; };
static const LpLayer kLpLayers[5] = {{3, 64, 11, 4, 2, 1}, {64, 192, 5, 1, 2, 1}, {192, 384, 3, 1, 1, 0}, {384, 256, 3, 1, 1, 0}, {256, 256, 3, 1, 1, 0}};

struct LpLayout {
    bool ok;
    int th[5], tw[5];          // the tap maps' sizes
    int ph[2], pw[2];          // the pooled maps' sizes
    size_t in_off, tap_off[5], pool_off[2], part_off, flag_off, bytes;
};

static LpLayout lp_layout(int H, int W) {
    LpLayout L{};
    if (H <= 0 || W <= 0 || H > kImMaxSide || W > kImMaxSide) return L;
    size_t off = 0;
    L.in_off = off;
    off += align256((size_t)2 * H * W * 3 * 4);
    int h = H, w = W, np = 0;
    for (int l = 0; l < 5; ++l) {
        const LpLayer& y = kLpLayers[l];
        if (h + 2 * y.pad < y.ks || w + 2 * y.pad < y.ks) return L;
        h = (h + 2 * y.pad - y.ks) / y.stride + 1;
        w = (w + 2 * y.pad - y.ks) / y.stride + 1;
        L.th[l] = h; L.tw[l] = w;
        L.tap_off[l] = off;
        off += align256((size_t)2 * h * w * y.cout * 4);
        if (y.pool) {
            if (h < 3 || w < 3) return L;
            h = (h - 3) / 2 + 1;
            w = (w - 3) / 2 + 1;
            L.ph[np] = h; L.pw[np] = w;
            L.pool_off[np] = off;
            off += align256((size_t)2 * h * w * y.cout * 4);
            ++np;
        }
    }
    L.part_off = off;
    off += align256((size_t)5 * kImTapPartials * 8);
    L.flag_off = off;
    off += 256;
    L.bytes = off;
    L.ok = true;
    return L;
}

}  // namespace iron

using namespace iron;

extern "C" int iron_img_sqerr_workspace_bytes(int64_t count, size_t* bytes) {
    if (count <= 0 || count >= (1LL << 31) || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = (size_t)kImSqerrBlocks * 8;
    return IRON_OK;
}

extern "C" int iron_img_sqerr(const void* a, const void* b, int64_t count, int32_t is_f32, void* workspace, double* out, void* stream) {
    if (count <= 0 || count >= (1LL << 31) || !a || !b || !workspace || !out) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* partials = (double*)workspace;
    if (is_f32) hipLaunchKernelGGL(k_sqerr<float>, dim3(kImSqerrBlocks), dim3(kImBlock), 0, st, (const float*)a, (const float*)b, count, partials);
    else hipLaunchKernelGGL(k_sqerr<uint8_t>, dim3(kImSqerrBlocks), dim3(kImBlock), 0, st, (const uint8_t*)a, (const uint8_t*)b, count, partials);
    IRON_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_reduce_f64, dim3(1), dim3(kImBlock), 0, st, (const double*)partials, kImSqerrBlocks, is_f32 ? 1.0 : 1.0 / 65025.0, out);
    IRON_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_set_f64, dim3(1), dim3(1), 0, st, out + 1, (double)count);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

static bool ssim_shape_ok(int H, int W) { return H >= kSsWin && W >= kSsWin && H <= kImMaxSide && W <= kImMaxSide; }

extern "C" int iron_img_ssim_workspace_bytes(int32_t H, int32_t W, size_t* bytes) {
    if (!ssim_shape_ok(H, W) || !bytes) return IRON_ERR_BAD_ARG;
    const size_t tiles = (size_t)((W - 10 + kSsTW - 1) / kSsTW) * ((H - 10 + kSsTH - 1) / kSsTH);
    *bytes = 3 * tiles * 8;
    return IRON_OK;
}

extern "C" int iron_img_ssim(const void* x, const void* y, int32_t H, int32_t W, int32_t is_f32, void* workspace, double* sums, double* s_map,
                             void* stream) {
    if (!ssim_shape_ok(H, W) || !x || !y || !workspace || !sums) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((W - 10 + kSsTW - 1) / kSsTW, (H - 10 + kSsTH - 1) / kSsTH, 3);
    double* partials = (double*)workspace;
    if (is_f32) hipLaunchKernelGGL((k_ssim<float, double>), grid, dim3(kImBlock), 0, st, (const float*)x, (const float*)y, H, W, partials, s_map);
    else hipLaunchKernelGGL((k_ssim<uint8_t, int>), grid, dim3(kImBlock), 0, st, (const uint8_t*)x, (const uint8_t*)y, H, W, partials, s_map);
    IRON_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_reduce_f64, dim3(3), dim3(kImBlock), 0, st, (const double*)partials, (int)(grid.x * grid.y), 1.0, sums);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_lpips_prepare(const void* pred, const void* trgt, int32_t H, int32_t W, int32_t is_f32, float* out, void* stream) {
    return launch_prepare(pred, trgt, H, W, is_f32, out, (hipStream_t)stream);
}

extern "C" int iron_conv2d_relu(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* weight, const float* bias,
                                int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float* out, int32_t* range_flag, void* stream) {
    return launch_conv(in, B, H, W, Cin, weight, bias, Cout, ksize, stride, pad, out, range_flag, (hipStream_t)stream);
}

extern "C" int iron_maxpool3s2(const float* in, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream) {
    return launch_pool(in, B, H, W, C, out, (hipStream_t)stream);
}

extern "C" int iron_lpips_tap(const float* feat, int32_t H, int32_t W, int32_t C, const float* lin, double* partials, void* stream) {
    return launch_tap(feat, H, W, C, lin, partials, (hipStream_t)stream);
}

extern "C" int iron_lpips_workspace_bytes(int32_t H, int32_t W, size_t* bytes) {
    const LpLayout L = lp_layout(H, W);
    if (!L.ok || !bytes) return IRON_ERR_BAD_ARG;
    *bytes = L.bytes;
    return IRON_OK;
}

extern "C" int iron_lpips_forward(const void* pred, const void* trgt, int32_t H, int32_t W, int32_t is_f32, const iron_lpips_weights* w,
                                  void* workspace, double* out, void* stream) {
    const LpLayout L = lp_layout(H, W);
    if (!L.ok || !pred || !trgt || !w || !workspace || !out || !aligned16(workspace)) return IRON_ERR_BAD_ARG;
    for (int l = 0; l < 5; ++l)
        if (!w->conv_weight[l] || !w->conv_bias[l] || !w->lin[l]) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* flag = (int*)(ws + L.flag_off);
    double* partials = (double*)(ws + L.part_off);
    IRON_HIP_TRY(hipMemsetAsync(flag, 0, 256, st));
    float* cur = (float*)(ws + L.in_off);
    int rc = launch_prepare(pred, trgt, H, W, is_f32, cur, st);
    if (rc != IRON_OK) return rc;
    int h = H, wd = W, np = 0;
    LpFinalArgs fa;
    for (int l = 0; l < 5; ++l) {
        const LpLayer& y = kLpLayers[l];
        float* tap = (float*)(ws + L.tap_off[l]);
        rc = launch_conv(cur, 2, h, wd, y.cin, w->conv_weight[l], w->conv_bias[l], y.cout, y.ks, y.stride, y.pad, tap, flag, st);
        if (rc != IRON_OK) return rc;
        h = L.th[l]; wd = L.tw[l];
        rc = launch_tap(tap, h, wd, y.cout, w->lin[l], partials + (size_t)l * kImTapPartials, st);
        if (rc != IRON_OK) return rc;
        fa.inv_hw[l] = 1.0 / ((double)h * wd);
        cur = tap;
        if (y.pool) {
            float* pooled = (float*)(ws + L.pool_off[np]);
            rc = launch_pool(tap, 2, h, wd, y.cout, pooled, st);
            if (rc != IRON_OK) return rc;
            h = L.ph[np]; wd = L.pw[np];
            cur = pooled;
            ++np;
        }
    }
    hipLaunchKernelGGL(k_lpips_final, dim3(1), dim3(kImBlock), 0, st, (const double*)partials, fa, (const int*)flag, out);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}
