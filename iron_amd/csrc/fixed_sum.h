// Fixed-order fp64 sums: the one definition behind every "bitwise reproducible" reduction of both libraries.
// Device only; includes nothing but the HIP runtime.
//
// The order.  A thread adds its own items to an fp64 accumulator in the order it visits them.  The kBlock accumulators of a
// workgroup meet in LDS in a halving tree: for s = kBlock / 2, kBlock / 4, .., 1 thread t < s does red[t] += red[t + s]; red[0] is
// the workgroup's sum and goes to the workgroup's own slot of a workspace.  One workgroup then adds the slots: thread t takes
// slots t, t + kBlock, t + 2 kBlock, .. in that order, and the same tree follows.  No atomics anywhere.
//
// The rule that makes this reproducible: which items a thread visits, and which slot a workgroup writes, depend on the problem
// size alone -- never on the device, the occupancy or a tuning knob.  A kernel that cuts its work differently computes a
// different (equally valid) sum, and tests/test_gpu_fixed_sums.py will say so.
#pragma once
#include <hip/hip_runtime.h>

namespace fixed_sum {

// Sum of one double per thread of a kBlock-thread workgroup (1-D or 2-D); red: kBlock doubles of LDS.  The result is valid in
// thread 0.  The leading barrier is part of the contract: back-to-back calls on one `red` need no barrier from the caller.
template <int kBlock>
__device__ double block_sum(double v, double* red) {
    const int t = threadIdx.x + threadIdx.y * blockDim.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// Sum of part[0], part[stride], .., part[(n - 1) stride] by one workgroup: thread t adds i = t, t + kBlock, .. in that order.
template <int kBlock>
__device__ double slot_sum(const double* part, int64_t n, int64_t stride, double* red) {
    double v = 0.0;
    for (int64_t i = threadIdx.x + threadIdx.y * blockDim.x; i < n; i += kBlock) v += part[i * stride];
    return block_sum<kBlock>(v, red);
}

// Multi-value partials: a workgroup's kVals sums live side by side in its slot, part[blockIdx.x * kVals + j].  The pair is for
// one-dimensional workgroups and grids (thread 0 is threadIdx.x == 0 here).
template <int kBlock, int kVals>
__device__ void store_slot(const double (&acc)[kVals], double* part, double* red) {
    for (int j = 0; j < kVals; ++j) {
        const double s = block_sum<kBlock>(acc[j], red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * kVals + j] = s;
    }
}

// ... and the totals over nb such slots (valid in thread 0)
template <int kBlock, int kVals>
__device__ void load_slots(const double* part, int64_t nb, double (&tot)[kVals], double* red) {
    for (int j = 0; j < kVals; ++j) tot[j] = slot_sum<kBlock>(part + j, nb, kVals, red);
}

}  // namespace fixed_sum
