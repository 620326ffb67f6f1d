// Kernels on the h2 (split-fp16, LDS-ring) MLP core.
#include <stdlib.h>
#include <atomic>
#include "mlp_h2.h"
#include "h2_setup.h"

namespace iron {

#ifndef IRON_FAST_SOFTPLUS
#define IRON_FAST_SOFTPLUS 1
#endif
constexpr bool kFastActH = IRON_FAST_SOFTPLUS != 0;

#if IRON_H2_STAMP
__device__ unsigned long long g_h2_stamps[4 * kStampSteps * 8];
#endif

// x [n,3] -> out[n]: 4 waves x 32 points per pass
__global__ __launch_bounds__(256, 1) void k_sdf_values_h2(H2StreamDev s, H2Meta m, const float* __restrict__ x, int64_t n,
                                                         float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Ring ring;
    h2_setup(s, lds, ring);
    const int64_t n_groups = (n + 127) / 128;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t idx = g * 128 + wave * 32 + (lane & 31);
        const bool ok = idx < n;
        const int64_t src = ok ? idx : (n - 1);
        const float px = x[src * 3 + 0], py = x[src * 3 + 1], pz = x[src * 3 + 2];
        f32x16 hf[kHidTiles];
        sdf_hidden_stack_h2<kFastActH>(ring, lds, m.n_hidden_layers, m.skip_layer, m.scale, px, py, pz, lane, hf);
        const float v = (row_dot_lds(lds + kLdsRows, hf, lane >> 5) + m.b_last) / m.scale;
        if (ok && lane < 32) out[idx] = v;
    }
    ring.drain();
#if IRON_H2_STAMP
    if (blockIdx.x == 0) {
        const unsigned long long* st = reinterpret_cast<const unsigned long long*>(lds + kLdsStamp);
        for (int i = threadIdx.x; i < 4 * kStampSteps * 8; i += 256) g_h2_stamps[i] = st[i];
    }
#endif
}

// the sampler's screen (sdf_hidden_stack_h1: one product per MAC, fp16 operands) on the h1 stream (s = the network's h1_trace), NP x 32
// points per wave as the sampler runs it: tools/bench_screen.py times it against k_sdf_values_h2, tools/screen_margin.py / tests compare
// its values (NP = 1: the 32-sample form, for the bit-for-bit comparison of the two)
template <int NP>
__global__ __launch_bounds__(256, 1) void k_sdf_values_h1(H2StreamDev s, H2Meta m, const float* __restrict__ x, int64_t n,
                                                         float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Ring ring;
    h2_setup(s, lds, ring);
    constexpr int kPerWave = 32 * NP, kPerGroup = 4 * kPerWave;
    const int64_t n_groups = (n + kPerGroup - 1) / kPerGroup;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t idx = g * kPerGroup + wave * kPerWave + (lane & (kPerWave - 1));
        const bool ok = idx < n;
        const int64_t src = ok ? idx : (n - 1);
        const float px = x[src * 3 + 0], py = x[src * 3 + 1], pz = x[src * 3 + 2];
        const float v = sdf_screen_value<kFastActH, NP>(ring, lds, m.n_hidden_layers, m.skip_layer, m.scale, m.b_last, px, py, pz, lane);
        if (ok && lane < kPerWave) out[idx] = v;
    }
    ring.drain();
}

template <int NP>
static int launch_sdf_values_h1(const iron_net* net, const float* x, int64_t n, float* out, hipStream_t st) {
    static bool attr = false;
    if (!attr) {
        IRON_HIP_TRY(hipFuncSetAttribute((const void*)k_sdf_values_h1<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsH2Total));
        attr = true;
    }
    H2Meta m;
    m.n_hidden_layers = net->sdf.n_hidden_layers; m.skip_layer = net->sdf.skip_layer; m.scale = net->sdf.scale; m.b_last = net->sdf.b_last;
    const int64_t groups = (n + 128 * NP - 1) / (128 * NP);
    const int64_t cus = cu_budget();
    const unsigned grid = (unsigned)(groups < cus ? groups : cus);
    hipLaunchKernelGGL(k_sdf_values_h1<NP>, dim3(grid), dim3(256), kLdsH2Total, st, net->h1_trace, m, x, n, out);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

#if IRON_H2_STAMP
extern "C" int iron_debug_h2_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_h2_stamps), sizeof(unsigned long long) * 4 * kStampSteps * 8) == hipSuccess ? 0 : -1;
}
#endif

bool use_h2_core() {
    static int v = -1;
    if (v < 0) {
        // default: the split-fp16 "h2" core; IRON_MLP_CORE=f32 selects the exact-fp32 MFMA core (mlp_core.h)
        const char* e = getenv("IRON_MLP_CORE");
        v = (e && e[0] == 'f') ? 0 : 1;
    }
    return v == 1;
}

int launch_sdf_values_h2(const iron_net* net, const float* x, int64_t n, float* out, hipStream_t st) {
    static bool attr = false;
    if (!attr) {
        IRON_HIP_TRY(hipFuncSetAttribute((const void*)k_sdf_values_h2, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsH2Total + (IRON_H2_STAMP ? kLdsStampBytes : 0)));
        attr = true;
    }
    H2Meta m;
    m.n_hidden_layers = net->sdf.n_hidden_layers; m.skip_layer = net->sdf.skip_layer; m.scale = net->sdf.scale; m.b_last = net->sdf.b_last;
    const int64_t groups = (n + 127) / 128;
    const int64_t cus = cu_budget();
    const unsigned grid = (unsigned)(groups < cus ? groups : cus);
    hipLaunchKernelGGL(k_sdf_values_h2, dim3(grid), dim3(256), kLdsH2Total + (IRON_H2_STAMP ? kLdsStampBytes : 0), st, net->h2_trace, m, x, n, out);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

// iron_sampler_screen_debug(2, 1): iron_sdf_screen_forward runs the 32-sample form (tests compare the two bit for bit)
static std::atomic<int> g_screen_forward_tiles{0};
void set_screen_forward_tiles(int point_tiles) { g_screen_forward_tiles.store(point_tiles, std::memory_order_relaxed); }

}  // namespace iron

using namespace iron;

extern "C" int iron_sdf_screen_forward(const iron_net_t* net, const float* x, int64_t n, float* out, void* stream) {
    if (!net || net->desc.kind != IRON_NET_SDF || n < 0 || (n > 0 && (!x || !out))) return IRON_ERR_BAD_ARG;
    if (!h2_sdf_usable(net) || !net->h1_trace.base) return IRON_ERR_UNSUPPORTED;
    if (n == 0) return IRON_OK;
    if (g_screen_forward_tiles.load(std::memory_order_relaxed) == 1) return launch_sdf_values_h1<1>(net, x, n, out, (hipStream_t)stream);
    return launch_sdf_values_h1<kH1PointTiles>(net, x, n, out, (hipStream_t)stream);
}
