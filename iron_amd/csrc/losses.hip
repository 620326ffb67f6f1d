// Stage-2 image losses of the reference's training drivers (models/image_losses.py; render_surface.py:597-598): the pyramid L2
// loss and the (masked) SSIM loss, forward and closed-form backward.  C ABI in include/iron_train.h; Python side in
// iron_amd/image_losses.py + iron_amd/autograd.py (PyramidL2Fn, SSIMFn).
//
// Conventions: images are [B, C, H, W] fp32 contiguous, processed as B*C independent planes (the pyramid filter is diagonal in
// the channels).  Every reduction goes through per-workgroup partials written to fixed slots and one single-workgroup reduce
// in the fixed order of fixed_sum.h, in fp64; there are no atomics, so the loss and both gradients are bitwise reproducible.
// The upstream gradient is read on the device; nothing here synchronises the host.
//
// Pyramid L2 (PyramidL2Loss.forward): d0 = X - Y, d_{k+1} = avgpool2(conv7x7(d_k)) (zero padding 3, floor pooling), loss =
// sum_k |d_k|^2 / ((h/2^k)(w/2^k)), k = 0..4.
//   k_pyr_down   one launch per level k = 0..3: a 32x32 tile of level k plus a 3-px halo in LDS; every thread makes one pooled
//                output from the 2x2 conv outputs under it (an 8x8 LDS window); partials: sum d_k^2 over the tile, and sum
//                d_{k+1}^2 over its outputs (used for the last level).  d_1..d_4 stay in the workspace for the backward.
//   k_pyr_reduce one workgroup: the five level sums over their partials, weighted.
//   k_pyr_up     one launch per level k = 3..0: g_k = 2 w_k s d_k + conv^T(pool^T(g_{k+1})), g_4 = 2 w_4 s d_4 made on the fly.
//                pool^T spreads 1/4 over each 2x2 block and gives 0 to rows / columns the floor dropped; the taps are point
//                symmetric (f[6-i][6-j] == f[i][j] bit for bit), so conv^T is the same zero-padded correlation.
//
// SSIM (ssim_loss_fn): five "valid" separable Gaussian blurs (X, Y, X^2, Y^2, XY), the per-pixel SSIM, mean over channels,
// optionally masked by the 11x11 erosion of the mask over the map padded with 1.0, then 1 - mean.  The blurs and the SSIM
// formula run in fp64 (the variances are differences of nearly equal blurred moments).
//   k_erode         (mask only) E = min over the in-image part of the win x win window of mask > 0.5 -> uint8 map; partial
//                   counts of E and of E on the border band outside the valid map (which counts with value 1.0)
//   k_ssim_tile     mode 0: partial sums of e(q) * ssim(q) over a 16x32 tile of the valid map; mode 1 (backward): the
//                   adjoints of the five blurred maps (four distinct: d sigma11 == d sigma22), written per channel
//   k_ssim_reduce   one workgroup: N = |E| (or B*H'*W'), loss = 1 - (sum + band) / N
//   k_ssim_adjoint  dX = G^T(dmu1) + 2X G^T(dsig) + Y G^T(dm12), dY the same with X, Y swapped; G^T is the "full" correlation
//   k_blur_valid    gaussian_filter(): the valid separable blur alone (inference)
#include "fixed_sum.h"
#include "train_common.h"

using namespace iron_train;
using fixed_sum::block_sum;
using fixed_sum::slot_sum;

namespace {

constexpr int kLevels = 5;
constexpr int kPyrTile = 32;              // level-k pixels per tile side
constexpr int kPyrSpan = kPyrTile + 6;    // with the 3-px halo
constexpr int kMaxWin = 21;               // largest SSIM / gaussian_filter window
constexpr int kTy = 16, kTx = 32;         // SSIM tile (valid-map pixels)
constexpr int kErodeTile = 32;

struct Taps49 {
    float f[49];
};
struct Win {
    float w[kMaxWin];
};

// ================================================= pyramid L2 =================================================================

struct PyrLayout {
    int h[kLevels], w[kLevels];
    int64_t n;                // planes
    size_t d_off[kLevels];    // d_1..d_4 (index 0 unused)
    size_t g_off[kLevels];    // g_1..g_3
    size_t part_off[4];       // per launch: nb WGs x (in, out) doubles
    int nbx[4], nby[4];
    size_t bytes;
};

PyrLayout pyr_layout(int64_t n, int h, int w) {
    PyrLayout L{};
    L.n = n;
    L.h[0] = h;
    L.w[0] = w;
    for (int k = 1; k < kLevels; ++k) {
        L.h[k] = L.h[k - 1] / 2;
        L.w[k] = L.w[k - 1] / 2;
    }
    size_t off = 0;
    for (int k = 1; k < kLevels; ++k) {
        L.d_off[k] = off;
        off += align256(sizeof(float) * (size_t)n * L.h[k] * L.w[k]);
    }
    for (int k = 1; k < kLevels - 1; ++k) {
        L.g_off[k] = off;
        off += align256(sizeof(float) * (size_t)n * L.h[k] * L.w[k]);
    }
    for (int k = 0; k < 4; ++k) {
        L.nbx[k] = cdiv64(L.w[k], kPyrTile);
        L.nby[k] = cdiv64(L.h[k], kPyrTile);
        L.part_off[k] = off;
        off += align256(sizeof(double) * 2 * (size_t)L.nbx[k] * L.nby[k] * n);
    }
    L.bytes = off;
    return L;
}

// one level down: src = d_k (or X - Y when src == nullptr), dst = d_{k+1}
__global__ __launch_bounds__(kThreads) void k_pyr_down(const float* __restrict__ src, const float* __restrict__ x,
                                                      const float* __restrict__ y, int hk, int wk, float* __restrict__ dst, int hn,
                                                      int wn, Taps49 taps, double* __restrict__ part) {
    __shared__ float s[kPyrSpan][kPyrSpan + 1];
    __shared__ double red[kThreads];
    const int tx = threadIdx.x, ty = threadIdx.y, t = tx + ty * 16;
    const int x0 = blockIdx.x * kPyrTile, y0 = blockIdx.y * kPyrTile;
    const int64_t plane = blockIdx.z;
    const size_t base = (size_t)plane * hk * wk;
    double in_sq = 0.0;
    for (int i = t; i < kPyrSpan * kPyrSpan; i += kThreads) {
        const int ly = i / kPyrSpan, lx = i % kPyrSpan;
        const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
        float v = 0.f;
        if (gy >= 0 && gy < hk && gx >= 0 && gx < wk) {
            const size_t p = base + (size_t)gy * wk + gx;
            v = src ? src[p] : x[p] - y[p];
            if (ly >= 3 && ly < 3 + kPyrTile && lx >= 3 && lx < 3 + kPyrTile) in_sq += (double)v * v;
        }
        s[ly][lx] = v;
    }
    __syncthreads();
    const int py = blockIdx.y * (kPyrTile / 2) + ty, px = blockIdx.x * (kPyrTile / 2) + tx;
    double out_sq = 0.0;
    if (py < hn && px < wn) {
        float c00 = 0.f, c01 = 0.f, c10 = 0.f, c11 = 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float f = taps.f[i * 7 + j];
                c00 = fmaf(f, s[2 * ty + i][2 * tx + j], c00);
                c01 = fmaf(f, s[2 * ty + i][2 * tx + j + 1], c01);
                c10 = fmaf(f, s[2 * ty + i + 1][2 * tx + j], c10);
                c11 = fmaf(f, s[2 * ty + i + 1][2 * tx + j + 1], c11);
            }
        }
        const float v = ((c00 + c01) + (c10 + c11)) * 0.25f;
        dst[(size_t)plane * hn * wn + (size_t)py * wn + px] = v;
        out_sq = (double)v * v;
    }
    const size_t slot = ((size_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double a = block_sum<kThreads>(in_sq, red);
    const double b = block_sum<kThreads>(out_sq, red);
    if (t == 0) {
        part[2 * slot] = a;
        part[2 * slot + 1] = b;
    }
}

struct PyrSums {
    const double* part[4];
    int count[4];
    double inv[kLevels];  // 1 / ((h/2^k)(w/2^k))
};

__global__ __launch_bounds__(kThreads) void k_pyr_reduce(PyrSums P, float* __restrict__ loss) {
    __shared__ double red[kThreads];
    double total = 0.0;
    for (int k = 0; k < kLevels; ++k) {
        const int launch = k < 4 ? k : 3, comp = k < 4 ? 0 : 1;
        total += slot_sum<kThreads>(P.part[launch] + comp, P.count[launch], 2, red) * P.inv[k];
    }
    if (threadIdx.x == 0) loss[0] = (float)total;
}

// one level up: g_k from g_{k+1} (or, for k = 3, from coef_next * s * d_4); d_k = src (or X - Y when src == nullptr).
// Level 0 writes dX = g_0 and dY = -g_0 (dy nullable).
__global__ __launch_bounds__(kThreads) void k_pyr_up(const float* __restrict__ src, const float* __restrict__ x,
                                                    const float* __restrict__ y, int hk, int wk, const float* __restrict__ gnext,
                                                    int next_is_d, int hn, int wn, Taps49 taps, float coef, float coef_next,
                                                    const float* __restrict__ d_loss, float* __restrict__ gk, float* __restrict__ dy) {
    __shared__ float u[kPyrSpan][kPyrSpan + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, t = tx + ty * 16;
    const int x0 = blockIdx.x * kPyrTile, y0 = blockIdx.y * kPyrTile;
    const int64_t plane = blockIdx.z;
    const float s = d_loss[0];
    const float scale_next = next_is_d ? 0.25f * (coef_next * s) : 0.25f;
    for (int i = t; i < kPyrSpan * kPyrSpan; i += kThreads) {
        const int ly = i / kPyrSpan, lx = i % kPyrSpan;
        const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
        float v = 0.f;
        if (gy >= 0 && gy < hk && gx >= 0 && gx < wk && (gy >> 1) < hn && (gx >> 1) < wn)
            v = scale_next * gnext[(size_t)plane * hn * wn + (size_t)(gy >> 1) * wn + (gx >> 1)];
        u[ly][lx] = v;
    }
    __syncthreads();
    const float cs = coef * s;
    const size_t base = (size_t)plane * hk * wk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        // 16x16 threads cover the 32x32 tile as 2x2 pixel quads, one quad row per r (rows ty*2 + (r>>1), cols tx*2 + (r&1))
        const int ly = ty * 2 + (r >> 1), lx = tx * 2 + (r & 1);
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= hk || gx >= wk) continue;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 7; ++j) acc = fmaf(taps.f[i * 7 + j], u[ly + i][lx + j], acc);
        const size_t p = base + (size_t)gy * wk + gx;
        const float d = src ? src[p] : x[p] - y[p];
        const float g = cs * d + acc;
        gk[p] = g;
        if (dy) dy[p] = -g;
    }
}

// ================================================= SSIM =======================================================================

struct SsimGeom {
    int b, c, h, w;
    int wy, wx;     // window taps per axis (1: the axis is not smoothed)
    int hv, wv;     // valid map
    int r;          // win // 2 (mask offset)
    int masked;
};

struct SsimLayout {
    size_t e_off, epart_off, spart_off, stats_off, bytes;
    int ebx, eby, sbx, sby;
};

SsimLayout ssim_layout(const SsimGeom& g) {
    SsimLayout L{};
    size_t off = 0;
    L.ebx = cdiv64(g.w, kErodeTile);
    L.eby = cdiv64(g.h, kErodeTile);
    L.sbx = cdiv64(g.wv, kTx);
    L.sby = cdiv64(g.hv, kTy);
    L.stats_off = off;
    off += 256;
    L.e_off = off;
    if (g.masked) off += align256((size_t)g.b * g.h * g.w);
    L.epart_off = off;
    if (g.masked) off += align256(sizeof(double) * 2 * (size_t)L.ebx * L.eby * g.b);
    L.spart_off = off;
    off += align256(sizeof(double) * (size_t)L.sbx * L.sby * g.b);
    L.bytes = off;
    return L;
}

int ssim_geom(int32_t b, int32_t c, int32_t h, int32_t w, int32_t win, int32_t masked, SsimGeom* g) {
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || win <= 0 || !(win & 1)) return IRON_ERR_BAD_ARG;
    if (win > kMaxWin) return IRON_ERR_UNSUPPORTED;
    g->b = b; g->c = c; g->h = h; g->w = w;
    g->wy = h >= win ? win : 1;
    g->wx = w >= win ? win : 1;
    g->hv = h - g->wy + 1;
    g->wv = w - g->wx + 1;
    g->r = win / 2;
    g->masked = masked ? 1 : 0;
    if (masked && (g->wy != win || g->wx != win)) return IRON_ERR_UNSUPPORTED;  // the reference fails there (shape mismatch)
    return IRON_OK;
}

void ssim_windows(const float* win, int32_t ws, const SsimGeom& g, Win* wy, Win* wx) {
    *wy = Win{};
    *wx = Win{};
    for (int i = 0; i < g.wy; ++i) wy->w[i] = g.wy == 1 ? 1.f : win[i];
    for (int i = 0; i < g.wx; ++i) wx->w[i] = g.wx == 1 ? 1.f : win[i];
    (void)ws;
}

// E = (erosion of mask.float() by a win x win window, geodesic border) > 0.5  ==  every in-image pixel of the window > 0.5
__global__ __launch_bounds__(kThreads) void k_erode(const void* __restrict__ mask, int mask_kind, int h, int w, int win, int r, int hv,
                                                   int wv, uint8_t* __restrict__ e, double* __restrict__ part) {
    constexpr int kSpan = kErodeTile + kMaxWin - 1;
    __shared__ uint8_t bad[kSpan][kSpan];
    __shared__ uint8_t rowbad[kSpan][kErodeTile];
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * kErodeTile, y0 = blockIdx.y * kErodeTile, img = blockIdx.z;
    const int span = kErodeTile + win - 1;
    const size_t base = (size_t)img * h * w;
    for (int i = t; i < span * span; i += kThreads) {
        const int ly = i / span, lx = i % span;
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        uint8_t b = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const size_t p = base + (size_t)gy * w + gx;
            b = mask_kind == 1 ? (((const uint8_t*)mask)[p] == 0) : !(((const float*)mask)[p] > 0.5f);
        }
        bad[ly][lx] = b;
    }
    __syncthreads();
    for (int i = t; i < span * kErodeTile; i += kThreads) {
        const int ly = i / kErodeTile, lx = i % kErodeTile;
        uint8_t b = 0;
        for (int j = 0; j < win; ++j) b |= bad[ly][lx + j];
        rowbad[ly][lx] = b;
    }
    __syncthreads();
    double n_all = 0.0, n_band = 0.0;
    for (int i = t; i < kErodeTile * kErodeTile; i += kThreads) {
        const int ly = i / kErodeTile, lx = i % kErodeTile;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= h || gx >= w) continue;
        uint8_t b = 0;
        for (int j = 0; j < win; ++j) b |= rowbad[ly + j][lx];
        const uint8_t keep = !b;
        e[base + (size_t)gy * w + gx] = keep;
        if (keep) {
            n_all += 1.0;
            if (gy < r || gy >= r + hv || gx < r || gx >= r + wv) n_band += 1.0;
        }
    }
    const size_t slot = ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double a = block_sum<kThreads>(n_all, red);
    const double bsum = block_sum<kThreads>(n_band, red);
    if (t == 0) {
        part[2 * slot] = a;
        part[2 * slot + 1] = bsum;
    }
}

struct SsimArgs {
    const float* x;
    const float* y;
    const uint8_t* e;       // eroded mask [B,H,W] or nullptr
    double c1, c2;
    const double* stats;    // backward: N
    const float* d_loss;    // backward
    double* part;           // forward
    float* adj;             // backward: [4][B][C][hv][wv]
};

// dynamic LDS: sX, sY [(kTy + wy - 1) x (kTx + wx - 1)] floats, then hmap[5][(kTy + wy - 1)][kTx] doubles
size_t ssim_tile_lds(const SsimGeom& g) {
    const size_t ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    return align256(2 * ry * rx * sizeof(float)) + 5 * ry * kTx * sizeof(double);
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void k_ssim_tile(SsimGeom g, Win wy, Win wx, SsimArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    const int ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    float* sX = (float*)lds;
    float* sY = sX + ry * rx;
    double* hm = (double*)(lds + align256(2 * (size_t)ry * rx * sizeof(float)));
    const int ox0 = blockIdx.x * kTx, oy0 = blockIdx.y * kTy, img = blockIdx.z;
    const int cx = t % kTx, cy = t / kTx;   // this thread's outputs: (cy, cx) and (cy + 8, cx)
    const size_t hw = (size_t)g.h * g.w, hvwv = (size_t)g.hv * g.wv;

    double acc[2] = {0.0, 0.0};
    double gq[2] = {0.0, 0.0};
    bool valid[2];
    for (int k = 0; k < 2; ++k) {
        const int oy = oy0 + cy + 8 * k, ox = ox0 + cx;
        valid[k] = oy < g.hv && ox < g.wv;
        if (kMode == 1 && valid[k]) {
            const bool keep = !a.e || a.e[(size_t)img * hw + (size_t)(oy + g.r) * g.w + (ox + g.r)];
            gq[k] = keep ? -(double)a.d_loss[0] / (a.stats[0] * g.c) : 0.0;
        }
    }
    for (int c = 0; c < g.c; ++c) {
        const size_t pb = ((size_t)img * g.c + c) * hw;
        for (int i = t; i < ry * rx; i += kThreads) {
            const int ly = i / rx, lx = i % rx;
            const int gy = oy0 + ly, gx = ox0 + lx;
            float vx = 0.f, vy = 0.f;
            if (gy < g.h && gx < g.w) {
                vx = a.x[pb + (size_t)gy * g.w + gx];
                vy = a.y[pb + (size_t)gy * g.w + gx];
            }
            sX[i] = vx;
            sY[i] = vy;
        }
        __syncthreads();
        const size_t plane5 = (size_t)ry * kTx;
        for (int i = t; i < ry * kTx; i += kThreads) {
            const int ly = i / kTx, lx = i % kTx;
            double m1 = 0, m2 = 0, m11 = 0, m22 = 0, m12 = 0;
            for (int j = 0; j < g.wx; ++j) {
                const double w = wx.w[j];
                const double vx = sX[ly * rx + lx + j], vy = sY[ly * rx + lx + j];
                const double px = vx * vx, py = vy * vy, pxy = vx * vy;  // exact: products of two floats
                m1 += w * vx;
                m2 += w * vy;
                m11 += w * px;
                m22 += w * py;
                m12 += w * pxy;
            }
            hm[0 * plane5 + i] = m1;
            hm[1 * plane5 + i] = m2;
            hm[2 * plane5 + i] = m11;
            hm[3 * plane5 + i] = m22;
            hm[4 * plane5 + i] = m12;
        }
        __syncthreads();
        for (int k = 0; k < 2; ++k) {
            if (!valid[k]) continue;
            const int ly = cy + 8 * k;
            double mu1 = 0, mu2 = 0, e11 = 0, e22 = 0, e12 = 0;
            for (int i = 0; i < g.wy; ++i) {
                const double w = wy.w[i];
                const int q = (ly + i) * kTx + cx;
                mu1 += w * hm[0 * plane5 + q];
                mu2 += w * hm[1 * plane5 + q];
                e11 += w * hm[2 * plane5 + q];
                e22 += w * hm[3 * plane5 + q];
                e12 += w * hm[4 * plane5 + q];
            }
            const double s11 = e11 - mu1 * mu1, s22 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
            const double A1 = 2.0 * mu1 * mu2 + a.c1, B1 = mu1 * mu1 + mu2 * mu2 + a.c1;
            const double A2 = 2.0 * s12 + a.c2, B2 = s11 + s22 + a.c2;
            if (kMode == 0) {
                acc[k] += (A1 / B1) * (A2 / B2);
            } else {
                const double gg = gq[k];
                const double L = A1 / B1, S = A2 / B2;
                const double d_s12 = gg * L * 2.0 / B2;
                const double d_sig = -gg * L * S / B2;            // d s11 == d s22
                const double dl_mu1 = gg * S * (2.0 * mu2 - L * 2.0 * mu1) / B1;
                const double dl_mu2 = gg * S * (2.0 * mu1 - L * 2.0 * mu2) / B1;
                const double dmu1 = dl_mu1 - 2.0 * mu1 * d_sig - mu2 * d_s12;
                const double dmu2 = dl_mu2 - 2.0 * mu2 * d_sig - mu1 * d_s12;
                const int oy = oy0 + ly, ox = ox0 + cx;
                const size_t q = ((size_t)img * g.c + c) * hvwv + (size_t)oy * g.wv + ox;
                const size_t stride = (size_t)g.b * g.c * hvwv;
                a.adj[q] = (float)dmu1;
                a.adj[stride + q] = (float)dmu2;
                a.adj[2 * stride + q] = (float)d_sig;
                a.adj[3 * stride + q] = (float)d_s12;
            }
        }
        __syncthreads();
    }
    if (kMode == 0) {
        double v = 0.0;
        for (int k = 0; k < 2; ++k) {
            if (!valid[k]) continue;
            const int oy = oy0 + cy + 8 * k, ox = ox0 + cx;
            const bool keep = !a.e || a.e[(size_t)img * hw + (size_t)(oy + g.r) * g.w + (ox + g.r)];
            if (keep) v += acc[k] / g.c;
        }
        const double s = block_sum<kThreads>(v, red);
        if (t == 0) a.part[((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void k_ssim_reduce(const double* __restrict__ spart, int ns, const double* __restrict__ epart,
                                                         int ne, double n_unmasked, double* __restrict__ stats, float* __restrict__ loss) {
    __shared__ double red[kThreads];
    const double s = slot_sum<kThreads>(spart, ns, 1, red);
    double n = n_unmasked, band = 0.0;
    if (epart) {
        n = slot_sum<kThreads>(epart, ne, 2, red);
        band = slot_sum<kThreads>(epart + 1, ne, 2, red);
    }
    if (threadIdx.x == 0) {
        stats[0] = n;
        loss[0] = (float)(1.0 - (s + band) / n);  // n == 0 (empty E): NaN, as the reference's mean of an empty selection
    }
}

// adjoint of the valid blur applied to the four adjoint maps, combined into dX, dY of one plane
constexpr int kAdjMaps = 4;
size_t ssim_adj_lds(const SsimGeom& g) {
    const size_t ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    return align256(kAdjMaps * ry * rx * sizeof(float)) + kAdjMaps * (size_t)kTy * rx * sizeof(double);
}

__global__ __launch_bounds__(kThreads) void k_ssim_adjoint(SsimGeom g, Win wy, Win wx, const float* __restrict__ x,
                                                          const float* __restrict__ y, const float* __restrict__ adj, float* __restrict__ dx,
                                                          float* __restrict__ dy) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int t = threadIdx.x;
    const int ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    float* sa = (float*)lds;
    double* vm = (double*)(lds + align256(kAdjMaps * (size_t)ry * rx * sizeof(float)));
    const int px0 = blockIdx.x * kTx, py0 = blockIdx.y * kTy;
    const int64_t plane = blockIdx.z;
    const size_t hvwv = (size_t)g.hv * g.wv, stride = (size_t)g.b * g.c * hvwv;
    // region row ly <-> valid row py0 - (wy - 1) + ly
    for (int i = t; i < ry * rx; i += kThreads) {
        const int ly = i / rx, lx = i % rx;
        const int qy = py0 - (g.wy - 1) + ly, qx = px0 - (g.wx - 1) + lx;
        const bool in = qy >= 0 && qy < g.hv && qx >= 0 && qx < g.wv;
        const size_t q = plane * hvwv + (size_t)(in ? qy : 0) * g.wv + (in ? qx : 0);
#pragma unroll
        for (int m = 0; m < kAdjMaps; ++m) sa[m * ry * rx + i] = in ? adj[m * stride + q] : 0.f;
    }
    __syncthreads();
    // vertical: vm[m][ly][lx] = sum_i wy[i] * a(py0 + ly - i)
    for (int i = t; i < kTy * rx; i += kThreads) {
        const int ly = i / rx, lx = i % rx;
        double s[kAdjMaps] = {0, 0, 0, 0};
        for (int k = 0; k < g.wy; ++k) {
            const double w = wy.w[k];
            const int row = ly + (g.wy - 1) - k;
#pragma unroll
            for (int m = 0; m < kAdjMaps; ++m) s[m] += w * sa[m * ry * rx + row * rx + lx];
        }
#pragma unroll
        for (int m = 0; m < kAdjMaps; ++m) vm[m * kTy * rx + i] = s[m];
    }
    __syncthreads();
    const size_t hw = (size_t)g.h * g.w;
    for (int i = t; i < kTy * kTx; i += kThreads) {
        const int ly = i / kTx, lx = i % kTx;
        const int py = py0 + ly, px = px0 + lx;
        if (py >= g.h || px >= g.w) continue;
        double s[kAdjMaps] = {0, 0, 0, 0};
        for (int k = 0; k < g.wx; ++k) {
            const double w = wx.w[k];
            const int col = lx + (g.wx - 1) - k;
#pragma unroll
            for (int m = 0; m < kAdjMaps; ++m) s[m] += w * vm[m * kTy * rx + ly * rx + col];
        }
        const size_t p = plane * hw + (size_t)py * g.w + px;
        const double vx = x[p], vy = y[p];
        dx[p] = (float)(s[0] + 2.0 * vx * s[2] + vy * s[3]);
        if (dy) dy[p] = (float)(s[1] + 2.0 * vy * s[2] + vx * s[3]);
    }
}

// gaussian_filter(): valid separable blur of one plane per blockIdx.z (the axes shorter than the window are passed through)
__global__ __launch_bounds__(kThreads) void k_blur_valid(SsimGeom g, Win wy, Win wx, const float* __restrict__ in, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int t = threadIdx.x;
    const int ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    float* s = (float*)lds;
    double* hm = (double*)(lds + align256((size_t)ry * rx * sizeof(float)));
    const int ox0 = blockIdx.x * kTx, oy0 = blockIdx.y * kTy;
    const int64_t plane = blockIdx.z;
    const float* src = in + plane * g.h * g.w;
    for (int i = t; i < ry * rx; i += kThreads) {
        const int ly = i / rx, lx = i % rx;
        const int gy = oy0 + ly, gx = ox0 + lx;
        s[i] = (gy < g.h && gx < g.w) ? src[(size_t)gy * g.w + gx] : 0.f;
    }
    __syncthreads();
    for (int i = t; i < ry * kTx; i += kThreads) {
        const int ly = i / kTx, lx = i % kTx;
        double v = 0.0;
        for (int j = 0; j < g.wx; ++j) v += (double)wx.w[j] * s[ly * rx + lx + j];
        hm[i] = v;
    }
    __syncthreads();
    for (int i = t; i < kTy * kTx; i += kThreads) {
        const int ly = i / kTx, lx = i % kTx;
        const int oy = oy0 + ly, ox = ox0 + lx;
        if (oy >= g.hv || ox >= g.wv) continue;
        double v = 0.0;
        for (int k = 0; k < g.wy; ++k) v += (double)wy.w[k] * hm[(ly + k) * kTx + lx];
        out[plane * g.hv * g.wv + (size_t)oy * g.wv + ox] = (float)v;
    }
}

int pyr_check(const float* x, const float* y, int64_t n, int32_t h, int32_t w) {
    if (!x || !y || n <= 0) return IRON_ERR_BAD_ARG;
    if (h < 16 || w < 16) return IRON_ERR_UNSUPPORTED;  // the fourth pooling would leave an empty level (torch raises there)
    if (n * (int64_t)h * w >= ((int64_t)1 << 31) || n > 65535) return IRON_ERR_UNSUPPORTED;
    return IRON_OK;
}

Taps49 load_taps(const float* taps) {
    Taps49 T;
    for (int i = 0; i < 49; ++i) T.f[i] = taps[i];
    return T;
}

}  // namespace

extern "C" size_t iron_pyramid_l2_workspace_bytes(int64_t n_planes, int32_t h, int32_t w) {
    if (n_planes <= 0 || h < 16 || w < 16) return 0;
    return pyr_layout(n_planes, h, w).bytes;
}

extern "C" int iron_pyramid_l2_forward(const float* x, const float* y, int64_t n_planes, int32_t h, int32_t w, const float* taps,
                                       float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = pyr_check(x, y, n_planes, h, w);
    if (rc != IRON_OK) return rc;
    if (!taps || !loss || !workspace) return IRON_ERR_BAD_ARG;
    const PyrLayout L = pyr_layout(n_planes, h, w);
    if (workspace_bytes < L.bytes) return IRON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const Taps49 T = load_taps(taps);
    PyrSums P{};
    for (int k = 0; k < 4; ++k) {
        const float* src = k == 0 ? nullptr : (const float*)(ws + L.d_off[k]);
        float* dst = (float*)(ws + L.d_off[k + 1]);
        double* part = (double*)(ws + L.part_off[k]);
        hipLaunchKernelGGL(k_pyr_down, dim3(L.nbx[k], L.nby[k], (unsigned)n_planes), dim3(16, 16), 0, st, src, x, y, L.h[k], L.w[k], dst,
                           L.h[k + 1], L.w[k + 1], T, part);
        P.part[k] = part;
        P.count[k] = L.nbx[k] * L.nby[k] * (int)n_planes;
    }
    for (int k = 0; k < kLevels; ++k) {
        const double s = (double)(1 << k);
        P.inv[k] = 1.0 / ((h / s) * (w / s));  // the reference's h / 2.0 ... divisors, not the floor-pooled sizes
    }
    hipLaunchKernelGGL(k_pyr_reduce, dim3(1), dim3(kThreads), 0, st, P, loss);
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_pyramid_l2_backward(const float* x, const float* y, int64_t n_planes, int32_t h, int32_t w, const float* taps,
                                        const float* d_loss, void* workspace, size_t workspace_bytes, float* dx, float* dy,
                                        void* stream) {
    int rc = pyr_check(x, y, n_planes, h, w);
    if (rc != IRON_OK) return rc;
    if (!taps || !d_loss || !workspace || !dx) return IRON_ERR_BAD_ARG;
    const PyrLayout L = pyr_layout(n_planes, h, w);
    if (workspace_bytes < L.bytes) return IRON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const Taps49 T = load_taps(taps);
    float coef[kLevels];
    for (int k = 0; k < kLevels; ++k) {
        const double s = (double)(1 << k);
        coef[k] = (float)(2.0 / ((h / s) * (w / s)));
    }
    for (int k = 3; k >= 0; --k) {
        const float* src = k == 0 ? nullptr : (const float*)(ws + L.d_off[k]);
        const float* gnext = k == 3 ? (const float*)(ws + L.d_off[4]) : (const float*)(ws + L.g_off[k + 1]);
        float* gk = k == 0 ? dx : (float*)(ws + L.g_off[k]);
        hipLaunchKernelGGL(k_pyr_up, dim3(L.nbx[k], L.nby[k], (unsigned)n_planes), dim3(16, 16), 0, st, src, x, y, L.h[k], L.w[k], gnext,
                           k == 3 ? 1 : 0, L.h[k + 1], L.w[k + 1], T, coef[k], coef[k + 1], d_loss, gk, k == 0 ? dy : nullptr);
    }
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_ssim_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t win_size, int32_t masked,
                                         size_t* state_bytes, size_t* scratch_bytes) {
    SsimGeom g;
    int rc = ssim_geom(b, c, h, w, win_size, masked, &g);
    if (rc != IRON_OK) return rc;
    if (state_bytes) *state_bytes = ssim_layout(g).bytes;
    if (scratch_bytes) *scratch_bytes = kAdjMaps * sizeof(float) * (size_t)b * c * g.hv * g.wv;
    return IRON_OK;
}

static int ssim_sizes_ok(const SsimGeom& g) {
    if ((int64_t)g.b * g.c * g.h * g.w >= ((int64_t)1 << 31) || g.b * (int64_t)g.c > 65535) return IRON_ERR_UNSUPPORTED;
    return IRON_OK;
}

extern "C" int iron_ssim_forward(const float* x, const float* y, int32_t b, int32_t c, int32_t h, int32_t w, const float* win,
                                 int32_t win_size, double c1, double c2, const void* mask, int32_t mask_kind, float* loss, void* state,
                                 size_t state_bytes, void* stream) {
    SsimGeom g;
    int rc = ssim_geom(b, c, h, w, win_size, mask != nullptr, &g);
    if (rc != IRON_OK) return rc;
    if ((rc = ssim_sizes_ok(g)) != IRON_OK) return rc;
    if (!x || !y || !win || !loss || !state) return IRON_ERR_BAD_ARG;
    if (mask && mask_kind != 1 && mask_kind != 2) return IRON_ERR_BAD_ARG;
    const SsimLayout L = ssim_layout(g);
    if (state_bytes < L.bytes) return IRON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)state;
    Win wy, wx;
    ssim_windows(win, win_size, g, &wy, &wx);
    SsimArgs a{};
    a.x = x;
    a.y = y;
    a.c1 = c1;
    a.c2 = c2;
    a.part = (double*)(ws + L.spart_off);
    if (mask) {
        a.e = (const uint8_t*)(ws + L.e_off);
        hipLaunchKernelGGL(k_erode, dim3(L.ebx, L.eby, b), dim3(kThreads), 0, st, mask, mask_kind, h, w, win_size, g.r, g.hv, g.wv,
                           (uint8_t*)(ws + L.e_off), (double*)(ws + L.epart_off));
    }
    hipLaunchKernelGGL(k_ssim_tile<0>, dim3(L.sbx, L.sby, b), dim3(kThreads), ssim_tile_lds(g), st, g, wy, wx, a);
    hipLaunchKernelGGL(k_ssim_reduce, dim3(1), dim3(kThreads), 0, st, (const double*)(ws + L.spart_off), L.sbx * L.sby * b,
                       mask ? (const double*)(ws + L.epart_off) : nullptr, L.ebx * L.eby * b, (double)b * g.hv * g.wv,
                       (double*)(ws + L.stats_off), loss);
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_ssim_backward(const float* x, const float* y, int32_t b, int32_t c, int32_t h, int32_t w, const float* win,
                                  int32_t win_size, double c1, double c2, int32_t masked, const float* d_loss, const void* state,
                                  size_t state_bytes, void* scratch, size_t scratch_bytes, float* dx, float* dy, void* stream) {
    SsimGeom g;
    int rc = ssim_geom(b, c, h, w, win_size, masked, &g);
    if (rc != IRON_OK) return rc;
    if ((rc = ssim_sizes_ok(g)) != IRON_OK) return rc;
    if (!x || !y || !win || !d_loss || !state || !scratch || !dx) return IRON_ERR_BAD_ARG;
    const SsimLayout L = ssim_layout(g);
    if (state_bytes < L.bytes || scratch_bytes < kAdjMaps * sizeof(float) * (size_t)b * c * g.hv * g.wv) return IRON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)state;
    Win wy, wx;
    ssim_windows(win, win_size, g, &wy, &wx);
    SsimArgs a{};
    a.x = x;
    a.y = y;
    a.c1 = c1;
    a.c2 = c2;
    a.e = masked ? (const uint8_t*)(ws + L.e_off) : nullptr;
    a.stats = (const double*)(ws + L.stats_off);
    a.d_loss = d_loss;
    a.adj = (float*)scratch;
    hipLaunchKernelGGL(k_ssim_tile<1>, dim3(L.sbx, L.sby, b), dim3(kThreads), ssim_tile_lds(g), st, g, wy, wx, a);
    hipLaunchKernelGGL(k_ssim_adjoint, dim3(cdiv64(w, kTx), cdiv64(h, kTy), b * c), dim3(kThreads), ssim_adj_lds(g), st, g, wy, wx, x, y,
                       (const float*)scratch, dx, dy);
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_gaussian_filter(const float* x, int64_t n_planes, int32_t h, int32_t w, const float* win, int32_t win_size,
                                    float* out, void* stream) {
    SsimGeom g;
    int rc = ssim_geom(1, 1, h, w, win_size, 0, &g);
    if (rc != IRON_OK) return rc;
    if (!x || !win || !out || n_planes <= 0) return IRON_ERR_BAD_ARG;
    if (n_planes > 65535 || n_planes * (int64_t)h * w >= ((int64_t)1 << 31)) return IRON_ERR_UNSUPPORTED;
    Win wy, wx;
    ssim_windows(win, win_size, g, &wy, &wx);
    const size_t ry = kTy + g.wy - 1, rx = kTx + g.wx - 1;
    const size_t lds = align256(ry * rx * sizeof(float)) + ry * kTx * sizeof(double);
    hipLaunchKernelGGL(k_blur_valid, dim3(cdiv64(g.wv, kTx), cdiv64(g.hv, kTy), (unsigned)n_planes), dim3(kThreads), lds, (hipStream_t)stream,
                       g, wy, wx, x, out);
    IRON_TRAIN_HIP(hipGetLastError());
    return IRON_OK;
}
