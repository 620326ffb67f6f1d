// The kernels and the host loop of pair_scan.h.  Kernel boundaries make every level visible to the next on all XCDs.
#include "pair_scan.h"

namespace iron {

__device__ __forceinline__ int64_t wave_incl_scan64(int64_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// exclusive scan of s[0..n) in place, kScanBlock entries per block; block totals -> up[blockIdx.x]
__global__ __launch_bounds__(kScanBlock) void k_pair_scan(Pair64* __restrict__ s, int64_t n, Pair64* __restrict__ up) {
    __shared__ int64_t wa[kScanBlock / 64], wb[kScanBlock / 64];
    const int64_t g = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const Pair64 x = g < n ? s[g] : Pair64{0, 0};
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ia = wave_incl_scan64(x.a), ib = wave_incl_scan64(x.b);
    if (lane == 63) { wa[w] = ia; wb[w] = ib; }
    __syncthreads();
    int64_t oa = 0, ob = 0, ta = 0, tb = 0;
    for (int i = 0; i < kScanBlock / 64; ++i) {
        if (i < w) { oa += wa[i]; ob += wb[i]; }
        ta += wa[i]; tb += wb[i];
    }
    if (g < n) s[g] = Pair64{oa + ia - x.a, ob + ib - x.b};
    if (threadIdx.x == 0) up[blockIdx.x] = Pair64{ta, tb};
}

__global__ void k_pair_add_down(Pair64* __restrict__ s, int64_t n, const Pair64* __restrict__ up) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) {
        const Pair64 o = up[g / kScanBlock];
        s[g].a += o.a;
        s[g].b += o.b;
    }
}

int pair_scan(const ScanLevels& S, void* ws, hipStream_t st) {
    for (int l = 0; l < S.levels; ++l)
        IRON_LAUNCH(k_pair_scan, (unsigned)S.level_len[l + 1], kScanBlock, st, S.level(ws, l), S.level_len[l], S.level(ws, l + 1));
    // level `levels - 1` is one block: already global; spread its offsets down
    for (int l = S.levels - 2; l >= 0; --l)
        IRON_LAUNCH(k_pair_add_down, blocks_for(S.level_len[l], 256), 256, st, S.level(ws, l), S.level_len[l],
                    (const Pair64*)S.level(ws, l + 1));
    return IRON_OK;
}

}  // namespace iron
