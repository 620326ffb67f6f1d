// Sphere tracer: RayTracer.forward = sphere_tracing + ray_sampler + rootfind
// (models/raytracer.py:45-220) as persistent kernels on one stream, no host sync: the four below, and on the h2 core the screened
// form of the sampler (k_sampler_screen + k_resolve_list / k_screen_resolve in two rounds + k_screen_fin_*, then k_sampler on the rays
// that overflowed).
//
//   k_sphere   one wave owns 32 ray slots.  Every pass evaluates the SDF MLP for all 32 slots, then
//              each slot steps or retires; retired slots are refilled from a global ray queue
//              (ballot -> rank among free slots -> one atomicAdd per wave), so MFMA tiles stay full
//              although rays finish after 1..17 evaluations.  Rays still unfinished after the
//              iteration cap are appended to the sampler list.
//   k_sampler  32 / kSamplerBlock ray slots per wave: a listed ray's dense samples are evaluated kSamplerBlock
//              at a time in march order, as work items of kSamplerSeg blocks, and the search stops at the
//              first block that holds a negative sample (the reference evaluates all n_steps and then
//              takes the first sign change: same result).
//   k_bisect_a 32 bracketed rays per wave, slots refilled like k_sphere's: each ray is bisected until ITS interval is
//              <= 2*threshold and then evaluates the mid-point it ends on -- its result if no ray of its chunk needs
//              more iterations, and the value the next iteration consumes if one does (made here too once the chunk's
//              table shows it is needed); the counts are atomicMax-ed into the ray's chunk, once per wave and chunk.
//   k_bisect_b the reference loops while ANY ray of the call is unfinished and updates ALL rays, so every ray runs the
//              chunk-wide maximum count: the rays whose own count is below it (k_bisect_list) finish the remaining
//              iterations on the value phase a kept; the last evaluation is the result.  No such ray: no weight ring.
//
// Tails (an experiment kept behind IRON_TRACE_SPLIT = 2..4, default 1 = off): a persistent kernel ends on its slowest rays'
// chains of dependent evaluations (up to 17 / 16 / 10 of ~90 us each) with part of the chip idle.  The split form cuts the
// rays into independent parts whose kernel chains run on separate streams (the caller's + library-owned low-priority side
// streams, forked and joined with events, so the call stays ordered on the caller's stream) so that one part's workgroups
// could take the CUs another part's draining kernel frees.  Rays are independent and the chunk-global bisection count is an
// atomicMax table shared by the parts, so the result does not depend on the split (tests/test_gpu_trace.py).  Measured on an
// 80 k-ray tile shard (tools/shard_step_time.py, round 3): the two parts' kernels share the CUs evenly instead of one
// filling in behind the other -- every kernel takes twice as long and the step 8.75 ms against 8.64 unsplit (unequal parts
// 65/35/80 %: 9.1-9.3) -- stream priorities do not order workgroup dispatch between two resident persistent grids.
#include <atomic>
#include <mutex>
#include <stddef.h>
#include <stdlib.h>
#include "mlp_h2.h"
#include "ggx_core.h"
#include "h2_setup.h"

namespace iron {

constexpr int kMaxTraceSplits = 4;

#ifndef IRON_FAST_SOFTPLUS
#define IRON_FAST_SOFTPLUS 1
#endif
constexpr bool kFastActT = IRON_FAST_SOFTPLUS != 0;

struct SamplerQ {       // one dense-sampler work queue
    int n_list;         // rays listed
    int head;           // tickets drawn
    int n_cont;         // continuation items published
    int n_done;         // listed rays whose sampling has ended
};

struct TraceCounters {  // zeroed at the start of every call
    int q_head;         // sphere-trace ray queue
    SamplerQ smp;       // the dense sampler's list: n_list = rays appended by k_sphere
    int n_root;         // rays with a sign-change bracket
    int root_head_a;
    int root_head_b;    // the queue of k_bisect_b's list; with n_root_b behind it, zeroed again at the start of phase b
    int n_root_b;       // rays whose chunk's count is above their own (k_bisect_list)
    long long n_evals;
    long long n_sphere_conv;
    long long n_evals_sphere;
    long long sampler_abort;   // k_sampler workgroups that left the queue protocol by the poll bound (0 unless the protocol is broken)
    // the screened sampler (k_sampler_screen; read through iron_trace_screen_counts, never through iron_trace_stats)
    SamplerQ ovf;       // rays whose uncertain samples did not fit the resolve list: marched again by the unscreened k_sampler
    int n_res;          // uncertain samples appended to the resolve list (may exceed its capacity: the excess rays overflowed)
    int res_head;       // k_screen_resolve's queue
    int n_pend;         // rays whose outcome waits for the resolve
    unsigned ratio_bits;   // largest |f_screen - f_h2| / delta over the resolved samples (f32 bits; non-negative floats order as uints)
    long long n_screen;    // screened evaluations, speculative ones included
    long long n_resolved;  // exact evaluations of listed samples
    long long n_ovf;       // rays that overflowed the resolve list
    // the screen's adaptive march (read through iron_trace_stride_counts)
    long long n_pass;      // slot-passes k_sampler_screen executed (one slot = 8 lanes of one ray)
    long long n_pass_strided;   // ... of them at a stride above 1
    unsigned slope_bits;   // the slope guard: the largest ratio any of its three sources below saw (f32 bits)
    int stride_mode;       // 1: the call marched with the slope bound, 0: stride 1 throughout
    // where the stride-1 passes go and what the slope guard sees (read through iron_trace_stride_detail)
    long long n_pass_behind;   // stride-1 passes of rays already pending whose samples were all certainly positive
    long long n_pass_fresh;    // stride-1 passes of rays not pending when the pass began
    long long n_restart;       // strided blocks discarded behind their last good sample
    long long n_obs_march;     // slope observations: adjacent screened samples of k_sampler_screen's stride-1 passes,
    long long n_obs_res;       // ... k_screen_resolve's exact value of a listed sample against its screened predecessor,
    long long n_obs_pair;      // ... k_screen_fin_entries' exact values of two adjacent listed samples
    unsigned slope_march_bits, slope_res_bits, slope_pair_bits;   // the largest ratio of each source (f32 bits)
    // the resolve's two rounds (read through iron_trace_resolve_counts)
    int n_res1, n_res2;    // entries on round 1's / round 2's index list (k_resolve_list)
    int res_head2;         // round 2's queue (round 1's: res_head)
    long long n_eval_r1, n_eval_r2;   // exact evaluations of listed samples made by each round (deferral off: all in n_eval_r1)
};

// The screened sampler's state (see k_sampler_screen)
struct ResolveEntry {   // one uncertain sample: written by k_sampler_screen, f_ex by k_screen_resolve
    int ray;
    int s;              // sample index
    float z;            // its depth
    float f1;           // screened value
    float f_prev1;      // screened value of sample s - 1 (the previous item's last sample for s % block == 0; 0 for s == 0)
    float f_ex;         // exact (h2) value
    float ld;           // the ray's ld (stride_ld; 0: the ray marched without the slope bound), for the resolve's slope guard
    int mark;           // kEntDeferred: listed behind a listed sample of its ray with f1 < 0 | kEntRound2: taken by round 2 after all
};
static_assert(sizeof(ResolveEntry) == 32, "resolve entry: two per 64-byte line");
struct PendRec {        // a ray whose outcome waits for the resolve, by ray id
    int first;          // first certainly-negative sample (n_steps: none); atomicMin-ed by the resolve with the negative listed samples
    float fhi, flo;     // bracket values at `first` (screened, or exact where the sample was listed)
    float flo_ex;       // exact value of sample first - 1 when it was listed
    int has_flo_ex;
    int first_lost;     // first listed sample whose exact value overflowed (0x7fffffff: none); atomicMin-ed by the resolve (lost_value)
    int pad[2];
};
struct ScreenWs {
    const unsigned* calib;   // per network, device (f32 bits): [0] max |f_screen - f_h2| over the calibration set, [kScreenCalibG] G = max |grad f|
    int* flag;               // per network, pinned host words, may be null: [0] the screen's guard flag, [1] the slope guard's
    float delta_override;    // test hook (> 0: this delta)
    int stride;              // kStrideOn: the adaptive march may run (switch on, guard not raised, n_steps <= kStrideMaxSteps,
                             // continuation items) | test hooks kStridePendingOff, kStrideMuteMarch, kStrideOneSided
    float l_override;        // test hook (> 0: this slope bound L)
    ResolveEntry* ent;       // [cap]
    int cap;
    PendRec* rec;            // [rays of the call] by ray id
    int* pend_list;          // [rays of the part]
    int* ovf_list;           // [rays of the part]
    uint8_t* ray_state;      // [rays of the call] by ray id (zeroed at the start of a call): kRayPending [| kRayNegListed] | kRayOverflowed
    int* res_idx;            // [cap] the resolve's index list of the round that runs (k_resolve_list)
    int defer;               // kDeferOn: samples behind a ray's first listed f1 < 0 wait for round 2 | kDeferAudit: round 2 takes them all
    int res_round;           // k_screen_resolve: 0 every listed sample in list order, 1 / 2 the round's index list
};

// margin of the screen: delta = max(K * max|f_screen - f_h2| on the calibration set, floor).  EMPIRICAL, not a certified bound:
// a worst-case elementwise bound grows by about || |W| ||_inf ~ 18 per 256-wide layer and is useless here.  The resolve kernel
// watches every sample it evaluates exactly; a ratio |f_screen - f_h2| / delta above kScreenGuard turns the screen off for the
// network for the calls that start after the one that raised it has completed.
constexpr float kScreenK = 12.0f;
constexpr float kScreenFloor = 1.0e-3f;
constexpr float kScreenGuard = 0.5f;
constexpr int kScreenCalibPoints = 8192;
constexpr int kScreenCalibF1 = 64;   // calibration buffer (32-bit words): [0] the max, [kScreenCalibF1 ..) the screen's values
constexpr size_t kScreenCalibBytes = (kScreenCalibF1 + kScreenCalibPoints) * 4;
// The adaptive march's slope bound: L = kStrideK * G, G = max |grad f| over the calibration set (central differences of the h2 value
// at kStrideCalibH, about one sample spacing), stored in calibration word kScreenCalibG.  EMPIRICAL like delta: the stride-1 passes
// watch the slope between adjacent samples and the resolve that of every listed sample (slope_guard_raise), and a ratio above
// kStrideGuard (relative to L) puts the network's later calls on stride 1.
constexpr float kStrideK = 2.0f;
constexpr float kStrideGuard = 0.75f;
constexpr float kStrideCalibH = 1.0f / 128.0f;
// A block's stride is doubled over its first gap when its predecessor's last two samples rise by at least this slope, relative to L
// (k_sampler_screen, *two-sided stride*): a flat tail is no evidence that the values behind it go on rising.
constexpr float kStrideRise = 1.0f / 12.0f;
constexpr int kScreenCalibG = 1;
#ifndef IRON_SAMPLER_STRIDE_MAX
#define IRON_SAMPLER_STRIDE_MAX 16   // 8: 0.2 ms more per C1 frame
#endif
constexpr int kStrideMax = IRON_SAMPLER_STRIDE_MAX;
constexpr int kStrideMaxSteps = 256;   // the continuation word carries a sample index in 8 bits
constexpr int kStrideOn = 1;           // ScreenWs::stride
constexpr int kStridePendingOff = 2;   // test hook: a pending ray keeps stride 1 (the march before pending rays strode; one-sided)
constexpr int kStrideMuteMarch = 4;    // test hook: k_sampler_screen's stride-1 passes do not feed the slope guard
constexpr int kStrideOneSided = 8;     // test hook: a block's stride is its first gap (the choice before the two-sided one)
static_assert(kStrideMax >= 1 && kStrideMax <= 16, "stride field of the slot's packed position");
constexpr int kResolvePerRay = 2;   // resolve list capacity: entries per ray of the call
constexpr uint8_t kRayPending = 2;     // ray_state: the ray has listed uncertain samples (carried across its continuation items)
constexpr uint8_t kRayOverflowed = 1;  // ray_state: the ray's samples did not fit the list; k_sampler marches it again
constexpr uint8_t kRayNegListed = 4;   // ray_state, with kRayPending: the ray has listed a sample with f1 < 0 (carried like kRayPending)
constexpr int kEntDeferred = 1, kEntRound2 = 2;   // ResolveEntry::mark
constexpr int kDeferOn = 1, kDeferAudit = 2;      // ScreenWs::defer
__device__ __forceinline__ float screen_delta(const ScreenWs& s) {
    return s.delta_override > 0.0f ? s.delta_override : fmaxf(kScreenK * __uint_as_float(*s.calib), kScreenFloor);
}

struct TraceWs {
    TraceCounters* cnt;
    int* sampler_list;  // [n] the rays k_sphere lists for the dense sampler (ovf_pass: the screen's overflow list)
    int* root_list;     // [n] rays with a bracket, appended by the sampler (k_sampler, k_sampler_screen, k_screen_fin_rays)
    float* root_lo;     // [n] by list position
    float* root_hi;
    float* root_flo;
    float* root_fhi;
    int* root_k;        // iterations done in phase A
    int* chunk_iters;   // [n_chunks]
    int* chunk_roots;   // [n_chunks] bisected rays per chunk (for the reference-equivalent eval count)
    int n_chunks;
    unsigned long long* cont;  // the sampler's continuation items (k_sampler's or k_sampler_screen's), [cont_cap] (zeroed at the start of a call)
    int cont_cap;       // 0: no items, a slot keeps its ray to the end
    int ovf_pass;       // k_sampler: 0 = the list k_sphere fills (cnt->smp), 1 = the screen's overflow list (cnt->ovf, sampler_list = it)
    ScreenWs scr;
};

struct TraceArgs {
    const float* ray_o;
    const float* ray_d;
    const float* near;
    const float* far;
    const uint8_t* work;
    const int64_t* ray_index;  // may be null
    const float* lin;
    uint8_t* conv;
    float* points;
    float* sdf;
    float* dist;
    int ray0;   // first ray of this part (rays [ray0, ray0 + n) are queued; ray ids stay global)
    int n;
    int n_steps;
    int iters;
    float thr;
    long long chunk;
};

__device__ __forceinline__ int lane_rank(unsigned mask, int j) { return __popc(mask & ((1u << j) - 1u)); }
__device__ __forceinline__ int lane_rank64(unsigned long long mask, int j) { return __popcll(mask & ((1ull << j) - 1ull)); }

// butterfly reductions over the lanes whose numbers differ in the bits HI .. LO: every such lane ends with the result
// (32, 1: the wave; 16, 1: each half of 32 lanes; 32, kSamplerBlock: the lanes with the same place in their slots)
template <int HI = 32, int LO = 1, class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int off = HI; off >= LO; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
template <int HI = 32, int LO = 1>
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int off = HI; off >= LO; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
    return x;
}

__device__ __forceinline__ void ray_origin_dir(const TraceArgs& a, int ray, float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
    ox = a.ray_o[3 * (size_t)ray]; oy = a.ray_o[3 * (size_t)ray + 1]; oz = a.ray_o[3 * (size_t)ray + 2];
    dx = a.ray_d[3 * (size_t)ray]; dy = a.ray_d[3 * (size_t)ray + 1]; dz = a.ray_d[3 * (size_t)ray + 2];
}

// ---- evaluation back ends ---------------------------------------------------------------------------------
// The tracer kernels are written once as per-wave state machines around three calls:
//   be.any(p)   workgroup-wide OR of a wave-uniform predicate (decides whether another evaluation pass runs)
//   be.eval()   SDF of the point on lane&31 -- collective over the workgroup
//   be.finish()
// BackendF32: one wave per workgroup, exact-fp32 MFMA core (mlp_core.h), weights streamed per wave from L2.
// BackendH2 : four waves per workgroup in lock step on the split-fp16 core (mlp_h2.h) sharing the LDS ring.
struct BackendF32 {
    static constexpr int kThreads = 64;
    static constexpr bool kSplit = false;   // a non-finite value of this core is the network's own, as the reference's would be
    SdfNetDev net;
    WStream ws;
    int lane;
    __device__ __forceinline__ void init(const SdfNetDev& n, const H2StreamDev&, const H2Meta&) {
        net = n;
        lane = threadIdx.x;
        ws.init(net.blob, net.blob_bytes, lane);
    }
    __device__ __forceinline__ bool any(bool p) { return p; }
    __device__ __forceinline__ float eval(float x, float y, float z) { return sdf_eval<kFastActT>(net, ws, x, y, z, lane); }
    __device__ __forceinline__ void finish() {}
    // per-lane state across an evaluation: this core leaves the registers for it
    __device__ __forceinline__ void park(int, float) {}
    __device__ __forceinline__ void park(int, int) {}
    __device__ __forceinline__ float unpark(int, float v) { return v; }
    __device__ __forceinline__ int unpark(int, int v) { return v; }
};

// The h2 evaluation wants all 512 registers of a lane, so whatever a tracer kernel keeps per ray across it (origin, direction, depths,
// counters: 15-17 values) was spilled to scratch by the compiler and re-read after every evaluation: 300+ MB of scratch writes per
// launch reached HBM (round 2's counters: 37x the kernel's algorithmic bytes).  The kernels now put that state into LDS themselves
// ([field][256 threads] behind the ring's map: conflict-free ds_write_b32 / ds_read_b32) and take it back after the evaluation.
constexpr int kParkFields = 17;
constexpr int kLdsPark = kLdsH2Total;
constexpr int kLdsTraceTotal = kLdsPark + kParkFields * 256 * 4;   // 162 048 B of the CU's 163 840
static_assert(kLdsTraceTotal <= 160 * 1024, "LDS of a tracer workgroup");

template <bool DEFER_TILES>
struct BackendH2T {
    static constexpr int kThreads = 256;
    static constexpr bool kSplit = true;    // a non-finite value of this core is an overflow of the fp16 split (envelope.hip): see lost_value
    Ring ring;
    char* lds;
    H2Meta m;
    int lane, wave, parity;
    __device__ __forceinline__ void init(const SdfNetDev&, const H2StreamDev& s, const H2Meta& meta) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        lds = smem;
        m = meta;
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        parity = 0;
        h2_setup(s, lds, ring);
    }
    __device__ __forceinline__ bool any(bool p) {
        volatile int* f = reinterpret_cast<volatile int*>(lds + kLdsMisc) + parity * 4;
        if (lane == 0) f[wave] = p ? 1 : 0;
        __syncthreads();
        const int r = f[0] | f[1] | f[2] | f[3];
        parity ^= 1;
        return r != 0;
    }
    __device__ __forceinline__ float eval(float x, float y, float z) {
        f32x16 hf[kHidTiles];
        sdf_hidden_stack_h2<kFastActT, DEFER_TILES>(ring, lds, m.n_hidden_layers, m.skip_layer, m.scale, x, y, z, lane, hf);
        return (row_dot_lds(lds + kLdsRows, hf, lane >> 5) + m.b_last) / m.scale;
    }
    // the screen: one product per MAC (sdf_hidden_stack_h1) on a ring started on the h1 stream, for sign decisions only.
    // NP x 32 points per wave: NP = 1, the point on lane & 31 (as eval); NP = 2, every lane's own point.
    template <int NP>
    __device__ __forceinline__ float eval_screen(float x, float y, float z) {
        return sdf_screen_value<kFastActT, NP>(ring, lds, m.n_hidden_layers, m.skip_layer, m.scale, m.b_last, x, y, z, lane);
    }
    __device__ __forceinline__ void finish() { ring.drain(); }
    __device__ __forceinline__ void park(int i, float v) { reinterpret_cast<float*>(lds + kLdsPark)[i * 256 + threadIdx.x] = v; }
    __device__ __forceinline__ void park(int i, int v) { reinterpret_cast<int*>(lds + kLdsPark)[i * 256 + threadIdx.x] = v; }
    __device__ __forceinline__ float unpark(int i, float) { return reinterpret_cast<const float*>(lds + kLdsPark)[i * 256 + threadIdx.x]; }
    __device__ __forceinline__ int unpark(int i, int) { return reinterpret_cast<const int*>(lds + kLdsPark)[i * 256 + threadIdx.x]; }
};

#ifndef IRON_TRACE_DEFER
#define IRON_TRACE_DEFER 1
#endif
typedef BackendH2T<IRON_TRACE_DEFER != 0> BackendH2;
#ifndef IRON_SAMPLER_DEFER
#define IRON_SAMPLER_DEFER 1  // see sdf_hidden_stack_h2 (0: the fallback if hipcc's vgpr-form pass crashes on k_sampler again)
#endif
typedef BackendH2T<IRON_SAMPLER_DEFER != 0> BackendH2Sampler;

// parked state that several kernels keep: a 64-bit counter in fields i, i + 1; two 3-vectors (a ray's origin or point, and its
// direction) in fields i .. i + 5
template <class BE>
__device__ __forceinline__ void park_i64(BE& be, int i, long long v) { be.park(i, (int)(unsigned)v); be.park(i + 1, (int)(v >> 32)); }
template <class BE>
__device__ __forceinline__ long long unpark_i64(BE& be, int i, long long v) {
    return (long long)(((unsigned long long)(unsigned)be.unpark(i + 1, (int)(v >> 32)) << 32) | (unsigned)be.unpark(i, (int)(unsigned)v));
}
template <class BE>
__device__ __forceinline__ void park_vec6(BE& be, int i, float ox, float oy, float oz, float dx, float dy, float dz) {
    be.park(i, ox); be.park(i + 1, oy); be.park(i + 2, oz); be.park(i + 3, dx); be.park(i + 4, dy); be.park(i + 5, dz);
}
template <class BE>
__device__ __forceinline__ void unpark_vec6(BE& be, int i, float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
    ox = be.unpark(i, ox); oy = be.unpark(i + 1, oy); oz = be.unpark(i + 2, oz);
    dx = be.unpark(i + 3, dx); dy = be.unpark(i + 4, dy); dz = be.unpark(i + 5, dz);
}

// The envelope guard of the tracer (envelope.hip).  On the h2 core a non-finite evaluation means that an activation left fp16's range
// where the reference's fp32 has an ordinary number, so nothing may be made of it: not "not negative" (the sampler would march on and
// return a later root, or zeros like any miss), not "f <= 0" (the bisection would take the upper half).  The ray that met it ends
// loud instead: NaN in sdf_out / dist / points, conv = 0 (the sampler) or the bracket's 1 (the bisection), and the scan of sdf_out
// behind the call raises the network's flag.  k_sphere needs nothing: a NaN step retires the ray with that NaN as its sdf.  No loop's
// exit depends on a finite value: the march counts samples, the bisection iterations (k < 64 / `remaining`).  On the exact core
// (kSplit false) a non-finite value is treated as the reference treats it.
template <class BE>
__device__ __forceinline__ bool lost_value(float f) { return BE::kSplit && !(fabsf(f) <= 3.0e38f); }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

#define IRON_TRACE_KERNEL_ARGS SdfNetDev net, H2StreamDev hs, H2Meta hm, TraceArgs a, TraceWs w

template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_sphere(IRON_TRACE_KERNEL_ARGS) {
    BE be;
    be.init(net, hs, hm);
    const int lane = be.lane;
    const int j = lane & 31;

    bool active = false, unf = false, work = false, exhausted = false;
    int ray = 0, steps = 0;
    float px = 0.f, py = 0.f, pz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, t = 0.f, far = 0.f;
    long long evals = 0, nconv = 0;

    for (;;) {
        // ---- refill free slots from the queue
        const unsigned act = (unsigned)__ballot(active);
        const int nfree = 32 - __popc(act);
        if (nfree > 0 && !exhausted) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&w.cnt->q_head, nfree);
            base = __shfl(base, 0, 64);
            int avail = a.n - base;
            avail = avail < 0 ? 0 : (avail > nfree ? nfree : avail);
            if (base + nfree >= a.n) exhausted = true;
            const int rank = lane_rank(~act, j);
            if (!active && rank < avail) {
                ray = a.ray0 + base + rank;
                const float ox = a.ray_o[3 * (size_t)ray], oy = a.ray_o[3 * (size_t)ray + 1], oz = a.ray_o[3 * (size_t)ray + 2];
                dx = a.ray_d[3 * (size_t)ray]; dy = a.ray_d[3 * (size_t)ray + 1]; dz = a.ray_d[3 * (size_t)ray + 2];
                t = a.near[ray];
                far = a.far[ray];
                work = a.work[ray] != 0;
                unf = work;
                px = ox + dx * t; py = oy + dy * t; pz = oz + dz * t;  // raytracer.py:110
                steps = 0;
                active = true;
            }
        }
        const unsigned act2 = (unsigned)__ballot(active);
        if (!be.any(act2 != 0u)) break;
        evals += __popc(act2);

        {   // the ray state waits in LDS while the evaluation has the registers (spelled out: with park_vec6 / park_i64 this kernel,
            // the frame's longest, comes out with another register assignment and 18 more spilled SGPRs)
            const int flags = (active ? 1 : 0) | (unf ? 2 : 0) | (work ? 4 : 0) | (exhausted ? 8 : 0);
            be.park(0, flags); be.park(1, ray); be.park(2, steps);
            be.park(3, px); be.park(4, py); be.park(5, pz); be.park(6, dx); be.park(7, dy); be.park(8, dz); be.park(9, t); be.park(10, far);
            be.park(11, (int)(unsigned)evals); be.park(12, (int)(evals >> 32)); be.park(13, (int)(unsigned)nconv); be.park(14, (int)(nconv >> 32));
        }
        const float s = be.eval(px, py, pz);
        {
            const int flags = be.unpark(0, (active ? 1 : 0) | (unf ? 2 : 0) | (work ? 4 : 0) | (exhausted ? 8 : 0));
            active = flags & 1; unf = flags & 2; work = flags & 4; exhausted = flags & 8;
            ray = be.unpark(1, ray); steps = be.unpark(2, steps);
            px = be.unpark(3, px); py = be.unpark(4, py); pz = be.unpark(5, pz); dx = be.unpark(6, dx); dy = be.unpark(7, dy); dz = be.unpark(8, dz);
            t = be.unpark(9, t); far = be.unpark(10, far);
            evals = (long long)(((unsigned long long)(unsigned)be.unpark(12, (int)(evals >> 32)) << 32) | (unsigned)be.unpark(11, (int)(unsigned)evals));
            nconv = (long long)(((unsigned long long)(unsigned)be.unpark(14, (int)(nconv >> 32)) << 32) | (unsigned)be.unpark(13, (int)(unsigned)nconv));
        }

        bool retire = false, to_sampler = false;
        if (active) {
            unf = unf && (fabsf(s) > a.thr) && (t < far);  // raytracer.py:114-116
            if (!unf || steps == a.iters) {
                retire = true;
                to_sampler = unf;
            } else {  // raytracer.py:123-125 (separate mul / add, p accumulates)
                t += s;
                px += dx * s; py += dy * s; pz += dz * s;
                ++steps;
            }
        }
        const unsigned samp = (unsigned)__ballot(to_sampler);
        int sbase = 0;
        if (samp) {
            if (lane == 0) sbase = atomicAdd(&w.cnt->smp.n_list, __popc(samp));
            sbase = __shfl(sbase, 0, 64);
        }
        if (retire) {
            if (lane < 32) {
                const bool conv = work && !unf && (fabsf(s) <= a.thr) && (t < far);  // raytracer.py:128-133
                a.conv[ray] = conv ? 1 : 0;
                a.points[3 * (size_t)ray] = px; a.points[3 * (size_t)ray + 1] = py; a.points[3 * (size_t)ray + 2] = pz;
                a.sdf[ray] = s;
                a.dist[ray] = t;
                if (to_sampler) w.sampler_list[sbase + lane_rank(samp, j)] = ray;
                if (conv) ++nconv;
            }
            active = false;
            px = py = pz = 0.f;
        }
    }
    be.finish();
    long long c = nconv;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) {
        atomicAdd((unsigned long long*)&w.cnt->n_evals, (unsigned long long)evals);
        atomicAdd((unsigned long long*)&w.cnt->n_evals_sphere, (unsigned long long)evals);
        atomicAdd((unsigned long long*)&w.cnt->n_sphere_conv, (unsigned long long)c);
    }
}

// Samples of one ray evaluated per pass.  A wave's 32 points per pass are 32 / kSamplerBlock rays ("slots"), each marching
// through its n_steps samples kSamplerBlock at a time and leaving at the first block that holds a negative sample; a finished
// slot is refilled at once.  The reference evaluates all n_steps samples of every listed ray
// (raytracer.py:153-166); the finer the block, the fewer evaluations behind the first sign change are executed (block 32:
// 77 of 128 on average at 800x800 S0; block 8: 65) -- the samples that ARE evaluated, and what is made of them, are the same.
//
// Work items and the drain (round 3).  A listed ray needs 1 .. n_steps / kSamplerBlock passes, which nobody knows in advance: when the
// list ran out, every workgroup sat on a few long rays (up to 16 passes of 84 us each at 4 slots per wave) while the rest of its
// lanes -- and, a little later, most of the chip -- had nothing to pull.  Now a ray is marched kSamplerSeg blocks at a time: a slot
// that reaches a segment's end without a negative sample PUBLISHES the rest of the ray as a new item (ray, next block, f of the last
// sample: one 64-bit word) behind the list and takes the next ticket like any free slot.  Items = the list's rays (tickets below
// n_list) followed by the continuations in publication order; a ticket beyond what has been published is held and polled once per
// pass.  The march order of a ray's samples, the samples evaluated and the outcome are those of the one-slot-per-ray form; only which
// slot of which workgroup evaluates a segment changes.  The kernel ends when every listed ray has ended (n_sampler_done == n_list);
// no workgroup waits on another's arrival -- every published item has exactly one ticket, held by a running wave or not yet drawn --
// so a grid that is not fully resident cannot deadlock.  Relaxed agent-scope atomics on the 64-bit word are all the ordering it needs
// (everything else an item refers to was written before the kernel started).
#ifndef IRON_SAMPLER_BLOCK
#define IRON_SAMPLER_BLOCK 8
#endif
#ifndef IRON_SAMPLER_SEG
#define IRON_SAMPLER_SEG 4   // blocks per work item; 0: a slot keeps its ray to the end (the round-2 form)
#endif
constexpr int kSamplerBlock = IRON_SAMPLER_BLOCK;
constexpr int kSamplerSlots = 32 / kSamplerBlock;
constexpr int kScreenSlots = 32 * kH1PointTiles / kSamplerBlock;   // k_sampler_screen: every lane a sample of its own (NP = 2: 8 slots)
static_assert(kScreenSlots <= 32, "screen slots: one bit each in a 32-bit slot mask");
constexpr int kSamplerSeg = IRON_SAMPLER_SEG;
static_assert(kSamplerBlock == 4 || kSamplerBlock == 8 || kSamplerBlock == 16 || kSamplerBlock == 32, "sampler block");
constexpr int kContRayBits = 24, kContBlkBits = 8;   // item word: [ray + 1 : 24][next block : 8][f of the previous sample : 32]

// continuation items a call of n rays can publish (0: the kernel keeps every ray in its slot)
static inline int64_t sampler_cont_cap(int64_t n, int n_steps) {
    if (kSamplerSeg <= 0) return 0;
    const int64_t blocks = (n_steps + kSamplerBlock - 1) / kSamplerBlock;
    if (n + 2 >= (1ll << kContRayBits) || blocks >= (1ll << kContBlkBits)) return 0;
    const int64_t segs = (blocks + kSamplerSeg - 1) / kSamplerSeg;
    if (n * (segs - 1) * 8 > (256ll << 20)) return 0;   // (unusual step counts on a large call: not worth more than 256 MiB of workspace)
    return n * (segs - 1);
}

__device__ __forceinline__ float sample_depth(float smin, float lin, float width) { return smin + lin * width; }   // raytracer.py:147-149

// ---- the queue protocol and the outcome writes, shared by k_sampler and k_sampler_screen (the outcomes by k_screen_fin_rays too) ------
// Per slot (uniform over its kSamplerBlock lanes): has_ray, or a ticket >= 0 for the next item, or retired (nothing more to draw);
// publish: the slot's last pass ended a work item whose ray goes back to the queue.

// the first-lane bits of a per-slot predicate's ballot, one bit per slot (Ballot: 32 bits where the slots are the lower wave half's)
template <int SLOTS, class Ballot>
__device__ __forceinline__ unsigned slot_heads(Ballot b) {
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) m |= (unsigned)((b >> (s * kSamplerBlock)) & (Ballot)1) << s;
    return m;
}

// Publishing the continuations of the last pass and drawing tickets for the free slots costs one atomicAdd each per wave: the
// bases of the wave's tickets and of its items, from the slot masks of the two ballots.  (The kernels keep the few lines that
// join these helpers: written as one function they compile to 20-30 more spilled VGPRs in both sampler kernels.)
struct QueueBases { int tbase, pbase; };
__device__ __forceinline__ QueueBases sampler_queue_bases(SamplerQ* q, int lane, unsigned need_slots, unsigned pub_slots) {
    int v = 0;
    if (lane == 0 && need_slots) v = atomicAdd(&q->head, __popc(need_slots));
    if (lane == 1 && pub_slots) v = atomicAdd(&q->n_cont, __popc(pub_slots));
    return QueueBases{__shfl(v, 0, 64), __shfl(v, 1, 64)};
}
// a publishing slot's item word [ray + 1][item_pos / item_unit][prev_f], stored by the slot's first lane with ORDER if it fits;
// state != 0: the ray's pending bits travel in ray_state, written before the item (so ORDER is release, and the taker acquires)
template <int ORDER>
__device__ __forceinline__ void sampler_publish_item(const TraceWs& w, int pbase, unsigned pub_slots, int slot, bool first_lane, int ray, int item_pos,
                                                     int item_unit, float prev_f, uint8_t state) {
    const int c = pbase + __popc(pub_slots & ((1u << slot) - 1u));
    if (first_lane && c < w.cont_cap) {
        if (state) w.scr.ray_state[ray] = state;
        const unsigned long long item = (unsigned long long)(unsigned)(ray + 1) | ((unsigned long long)(unsigned)(item_pos / item_unit) << kContRayBits) |
                                        ((unsigned long long)__float_as_uint(prev_f) << 32);
        __hip_atomic_store(&w.cont[c], item, ORDER, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// a free slot's ticket; -1: nothing beyond (every ray publishes at most segs - 1 items), the slot retires
__device__ __forceinline__ int sampler_draw(int tbase, unsigned need_slots, int slot, long long n_tickets) {
    const long long t = (long long)tbase + __popc(need_slots & ((1u << slot) - 1u));
    return (t >= n_tickets || tbase < 0) ? -1 : (int)t;
}

// A held ticket: the list's ray (item position 0), or the continuation item once it is there (false: not yet).  item_pos is the
// word's position field as published.  The word carries the value of the item's last sample and no slope: k_sampler_screen's taker
// cannot tell whether the values rose, and its first block keeps the one-sided stride (1 + reach, the first gap's size).
__device__ __forceinline__ bool sampler_take(const TraceWs& w, int n_list, int ticket, int& ray, int& item_pos, float& prev_f) {
    if (ticket < n_list) {
        ray = w.sampler_list[ticket];
        item_pos = 0;
        prev_f = 0.f;
        return true;
    }
    const unsigned long long item = __hip_atomic_load(&w.cont[ticket - n_list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (item == 0ull) return false;
    ray = (int)(item & ((1u << kContRayBits) - 1u)) - 1;
    item_pos = (int)((item >> kContRayBits) & ((1u << kContBlkBits) - 1u));
    prev_f = __uint_as_float((unsigned)(item >> 32));
    return true;
}

// raytracer.py:59-65: sample [t, far] if sdf > 0 else [near, t]
__device__ __forceinline__ void ray_interval(const TraceArgs& a, int ray, float& smin, float& width) {
    const float t = a.dist[ray], s0 = a.sdf[ray];
    const bool pos_side = s0 > 0.0f;
    smin = pos_side ? t : a.near[ray];
    const float smax = pos_side ? a.far[ray] : t;
    width = smax - smin;
}

// No ray in the workgroup: true when it is done -- no slot holds a ticket that can still be served (or a ray to publish), or every
// listed ray has ended.  Otherwise one poll of the queue; the bound is a few seconds and never reached unless the protocol is
// broken -- reported in the stats.
template <class BE>
__device__ __forceinline__ bool sampler_idle_done(BE& be, SamplerQ* q, int n_list, TraceCounters* cnt, bool holds, unsigned& idle_polls) {
    const bool all_ended = __hip_atomic_load(&q->n_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_list;
    const bool waiting = __ballot(holds) != 0ull && !all_ended;
    if (!be.any(waiting)) return true;
    if (++idle_polls > (1u << 22)) {
        if (threadIdx.x == 0) atomicAdd((unsigned long long*)&cnt->sampler_abort, 1ull);
        return true;
    }
    __builtin_amdgcn_s_sleep(16);
    return false;
}

// a ray's outcome: a bracket for the bisection ...
__device__ __forceinline__ void sampler_write_root(const TraceWs& w, int ray, float z_lo, float z_hi, float f_lo, float f_hi) {
    const int pos_l = atomicAdd(&w.cnt->n_root, 1);
    w.root_list[pos_l] = ray;
    w.root_lo[pos_l] = z_lo; w.root_hi[pos_l] = z_hi;
    w.root_flo[pos_l] = f_lo; w.root_fhi[pos_l] = f_hi;
}
// ... or none (raytracer.py:158-160, 75-78: sampled rays without a root get zeros).  `fill`: 0.f as the caller wants it held, or
// NaN for a ray that ended at an overflowed value (lost_value)
__device__ __forceinline__ void sampler_write_no_root(const TraceArgs& a, int ray, float fill) {
    a.conv[ray] = 0;
    a.points[3 * (size_t)ray] = fill; a.points[3 * (size_t)ray + 1] = fill; a.points[3 * (size_t)ray + 2] = fill;
    a.sdf[ray] = fill;
    a.dist[ray] = fill;
}

template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_sampler(IRON_TRACE_KERNEL_ARGS) {
    SamplerQ* const q = w.ovf_pass ? &w.cnt->ovf : &w.cnt->smp;
    const int n_list = q->n_list;
    if (n_list == 0) return;   // (uniform over the grid) an empty list, as the screen's overflow list usually is: no weight ring is started
    BE be;
    be.init(net, hs, hm);
    const int lane = be.lane;
    const int j = lane & 31;
    const int slot = j / kSamplerBlock, s_in = j % kSamplerBlock;   // this lane's ray slot and its sample within the slot's block
    const int slot_lane0 = slot * kSamplerBlock;
    const unsigned slot_bits = (kSamplerBlock == 32 ? 0xffffffffu : ((1u << kSamplerBlock) - 1u)) << slot_lane0;
    const bool dyn = w.cont_cap > 0;
    const long long n_tickets = (long long)n_list + (dyn ? (long long)w.cont_cap : 0ll);
    long long evals = 0;
    // per slot (uniform over its lanes): a ray, or a ticket for the next item, or nothing more to draw
    bool has_ray = false, retired = false, publish = false;
    int ticket = -1;
    int ray = 0, blk = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, smin = 0.f, width = 0.f, prev_z = 0.f, prev_f = 0.f;
    unsigned idle_polls = 0;
    for (;;) {
        const unsigned pub_slots = slot_heads<kSamplerSlots>((unsigned)__ballot(publish));
        const unsigned need_slots = slot_heads<kSamplerSlots>((unsigned)__ballot(!has_ray && ticket < 0 && !retired));
        if (pub_slots | need_slots) {
            const QueueBases qb = sampler_queue_bases(q, lane, need_slots, pub_slots);
            if (publish) {
                sampler_publish_item<__ATOMIC_RELAXED>(w, qb.pbase, pub_slots, slot, lane == slot_lane0, ray, blk, 1, prev_f, 0);
                publish = false;
            }
            if (!has_ray && ticket < 0 && !retired) {
                ticket = sampler_draw(qb.tbase, need_slots, slot, n_tickets);
                if (ticket < 0) retired = true;
            }
        }
        if (!has_ray && ticket >= 0 && sampler_take(w, n_list, ticket, ray, blk, prev_f)) {
            ray_origin_dir(a, ray, ox, oy, oz, dx, dy, dz);
            ray_interval(a, ray, smin, width);
            prev_z = blk > 0 ? sample_depth(smin, a.lin[blk * kSamplerBlock - 1], width) : 0.f;   // the sample before the item's first
            has_ray = true;
            ticket = -1;
        }
        if (!be.any(__ballot(has_ray) != 0ull)) {
            if (sampler_idle_done(be, q, n_list, w.cnt, ticket >= 0 || publish, idle_polls)) break;
            continue;
        }
        const int idx = blk * kSamplerBlock + s_in;
        const bool in_range = has_ray && idx < a.n_steps;
        const float z = sample_depth(smin, a.lin[in_range ? idx : a.n_steps - 1], width);
        const float qx = has_ray ? ox + dx * z : 0.f, qy = has_ray ? oy + dy * z : 0.f, qz = has_ray ? oz + dz * z : 0.f;  // :150
        {   // the slot's state waits in LDS while the evaluation has the registers
            const int flags = (has_ray ? 1 : 0) | (retired ? 2 : 0) | (publish ? 4 : 0) | (in_range ? 8 : 0);
            be.park(0, flags); be.park(1, ray); be.park(2, blk); be.park(3, ticket);
            park_vec6(be, 4, ox, oy, oz, dx, dy, dz);
            be.park(10, smin); be.park(11, width); be.park(12, prev_z); be.park(13, prev_f); be.park(14, z);
            park_i64(be, 15, evals);
        }
        const float f = be.eval(qx, qy, qz);
        const int flags_back = be.unpark(0, (has_ray ? 1 : 0) | (retired ? 2 : 0) | (publish ? 4 : 0) | (in_range ? 8 : 0));
        has_ray = flags_back & 1; retired = flags_back & 2; publish = flags_back & 4;
        const bool in_range_b = flags_back & 8;
        ray = be.unpark(1, ray); blk = be.unpark(2, blk); ticket = be.unpark(3, ticket);
        unpark_vec6(be, 4, ox, oy, oz, dx, dy, dz);
        smin = be.unpark(10, smin); width = be.unpark(11, width); prev_z = be.unpark(12, prev_z); prev_f = be.unpark(13, prev_f);
        const float zb = be.unpark(14, z);
        evals = unpark_i64(be, 15, evals);
        idle_polls = 0;
        evals += __popc((unsigned)__ballot(in_range_b));   // lanes 32..63 mirror 0..31: the low word counts every point once
        const unsigned neg_all = (unsigned)__ballot(in_range_b && f < 0.0f);  // sign(f) == -1 (raytracer.py:162-166)
        // the slot's neighbours' values, fetched by every lane (shuffles are wave-wide operations)
        const unsigned neg = neg_all & slot_bits;
        // envelope guard: an overflowed sample at or in front of the slot's first negative one (or without one) ends the ray, loud
        const unsigned bad = (unsigned)__ballot(in_range_b && lost_value<BE>(f)) & slot_bits;
        const bool lost = has_ray && bad != 0u && (neg == 0u || __ffs(bad) <= __ffs(neg));   // (<=: -inf is overflowed and negative)
        const int first = neg ? (__ffs(neg) - 1) : slot_lane0;          // wave lane of the slot's first negative sample
        const float z_first = __shfl(zb, first, 64), f_first = __shfl(f, first, 64);
        const float z_before = __shfl(zb, first > slot_lane0 ? first - 1 : slot_lane0, 64);
        const float f_before = __shfl(f, first > slot_lane0 ? first - 1 : slot_lane0, 64);
        const float z_last = __shfl(zb, slot_lane0 + kSamplerBlock - 1, 64), f_last = __shfl(f, slot_lane0 + kSamplerBlock - 1, 64);
        // outcome of this block for the slot (straight-line: every lane of the slot computes the same)
        const int gidx = blk * kSamplerBlock + (first - slot_lane0);          // index of the first negative sample, if any
        const bool found_neg = has_ray && neg != 0u && !lost;
        const bool root = found_neg && gidx >= 1;                              // raytracer.py:167
        const bool done = has_ray && (found_neg || lost || (blk + 1) * kSamplerBlock >= a.n_steps);
        const float z_lo = first > slot_lane0 ? z_before : prev_z, f_lo = first > slot_lane0 ? f_before : prev_f;
        if (done && lane == slot_lane0) {   // the slot's first lane (lower half of the wave) writes the outcome
            if (root) sampler_write_root(w, ray, z_lo, z_first, f_lo, f_first);
            else sampler_write_no_root(a, ray, lost ? quiet_nan() : 0.f);
            atomicAdd(&q->n_done, 1);
        }
        prev_z = z_last;
        prev_f = f_last;
        ++blk;
        // the end of a work item: the ray goes back to the queue (published at the top of the next pass), the slot draws the next ticket
        const bool hand_over = has_ray && !done && dyn && (blk % (kSamplerSeg > 0 ? kSamplerSeg : 1)) == 0;
        publish = hand_over;
        if (done || hand_over) has_ray = false;
    }
    be.finish();
    if (lane == 0) atomicAdd((unsigned long long*)&w.cnt->n_evals, (unsigned long long)evals);
}

// ---- the screened sampler -------------------------------------------------------------------------------------------------------
// The sampler consumes only signs: sign(f) < 0 for the first negative sample, f_low > 0 / f_high < 0 for the bracket (the bisection
// re-evaluates its points exactly).  k_sampler_screen marches the same blocks, work items and continuations as k_sampler, but on the
// screen (sdf_hidden_stack_h1: one product per MAC, ~0.62 of an h2 evaluation).  A sample is certainly positive if f1 > delta,
// certainly negative if f1 < -delta, uncertain otherwise (NaN and zeros included).  A ray whose samples before its first certainly-
// negative one are all certainly positive (or that ends with all of them certainly positive) is decided here, exactly as k_sampler
// decides it.  Otherwise its uncertain samples before that point go to the resolve list and the ray ends "pending" at its first
// certainly-negative sample (or its end); k_screen_resolve evaluates the listed samples on the h2 core, 32 per wave from any rays
// (those behind a ray's first listed f1 < 0 only where they can still matter: the rounds, see k_resolve_list),
// and k_screen_fin_* give each pending ray the bracket, root-list entry or zeros k_sampler would have written.  A ray whose samples
// do not fit the list is marched again from its start by k_sampler on a second list.  n_evals still counts what k_sampler evaluates.
// A wave screens 64 samples per pass, 8 ray slots of 8 (k_sampler: 32, 4 slots, lanes j and j + 32 on one point): the screen's
// weight fragments feed two point tiles each (mlp_h2.h), so that its slots, their LDS-DMA and barriers serve twice the samples.
//
// The adaptive march.  Most listed rays have no root: they graze the surface, and behind their closest approach the
// SDF climbs far above the sample spacing.  A slot therefore holds a start index `pos` and a stride `strd` (one parked int with the
// item's pass count and first segment) and a pass evaluates samples pos + strd * (0..7).  With ld = L * |width| * lin_step * |d| (L
// times the ray's sample spacing; a.lin is uniform), an evaluated sample e certifies the next stride_reach(f1(e)) samples behind and in
// front of it: f1(e) > delta + ld * m.  The block is walked in order: a gap between two evaluated samples is good when every skipped
// sample in it is certified from one side; a sample that is not certainly positive, or a gap that is not certified, in a block with
// strd > 1 discards the rest of the block and the slot resumes behind its last good sample at stride 1.  So a ray's first sample that
// is not certainly positive is always reached at stride 1, next to its evaluated predecessor, and everything that is made of it --
// brackets, resolve entries, PendRec, overflow -- is the stride-1 code.  After a good block the next one starts 1 + stride_reach(f1(e_7))
// (at most kStrideMax) behind e_7, and its own stride is that gap, or up to twice as wide where the values rise (*two-sided stride*,
// at the follow-up below; iron_sampler_screen_debug(6, 1): always that gap).
// A pending ray (one that has listed uncertain samples) strides by the same rules: most pending rays
// graze the surface, list a few samples at their closest approach and then climb far above delta + ld * m, and a strided block only
// ever accepts certainly positive samples, so every later uncertain or negative sample of the ray is still met at stride 1 and listed
// or bracketed by the stride-1 code (per C1 frame 288 k of the 551 k stride-1 passes were such rays' passes through certainly
// positive samples; 43 k are left).  A work item ends after kSamplerSeg passes once its position has entered a later segment
// (kSamplerSeg blocks of samples) than the one it started in: at stride 1 exactly the items of k_sampler, and never more than
// sampler_cont_cap() per ray.  The continuation word carries the next sample index where k_sampler's carries the block, and the
// taker recomputes the stride from the carried f (a pending ray's too: ray_state carries its pending bit): that needs the index in
// 8 bits, so a call with n_steps > kStrideMaxSteps (256) or without continuation items runs stride 1, as does a network whose G is zero or non-finite, a ray
// whose range is empty, reversed or non-finite, and everything after the slope guard was raised (IRON_SAMPLER_STRIDE=0 /
// iron_set_sampler_stride: off).
__device__ __forceinline__ int stride_reach(float f, float delta, float ld) {   // skipped samples next to a sample of value f that it certifies
    int c = 0;
#pragma unroll
    for (int m = 1; m < kStrideMax; ++m) c += (f > delta + ld * (float)m) ? 1 : 0;
    return c;
}
// L * the ray's sample spacing; 0: the ray runs stride 1
__device__ __forceinline__ float stride_ld(float Lg, float lin_step, float width, float dx, float dy, float dz) {
    const float ld = Lg * fabsf(width) * lin_step * sqrtf(dx * dx + dy * dy + dz * dz);
    return (width > 0.0f && ld > 0.0f && ld <= 3.0e38f) ? ld : 0.0f;
}
constexpr int kPosBits = 13, kStrdBits = 5, kPassBits = 3;   // the slot's parked int: [pos : 13][strd : 5][passes of the item : 3][first segment : 8]
constexpr int kSegSamples = (kSamplerSeg > 0 ? kSamplerSeg : 1) * kSamplerBlock;
static_assert(kSamplerSeg < (1 << kPassBits) && kStrideMax < (1 << kStrdBits), "fields of the slot's parked position");

// the per-lane counts of k_sampler_screen, by the lane's place in its slot (see there); ev_scr is the wave's
__device__ __forceinline__ void screen_flush_counts(TraceCounters* cnt, unsigned ev_ref, unsigned ev_scr, int me) {
    const unsigned long long r = wave_sum<32, kSamplerBlock>((unsigned long long)ev_ref);   // summed over the slots: lane k < kSamplerBlock ends with the total of place k
    static_assert(kSamplerBlock >= 7, "places of the per-lane counts");
    long long* const dst = me == 0 ? &cnt->n_evals : me == 1 ? &cnt->n_pass : me == 2 ? &cnt->n_pass_strided : me == 3 ? &cnt->n_pass_behind
                         : me == 4 ? &cnt->n_pass_fresh : me == 5 ? &cnt->n_restart : &cnt->n_obs_march;
    if (me < 7 && r) atomicAdd((unsigned long long*)dst, r);
    if (me == 0) atomicAdd((unsigned long long*)&cnt->n_screen, (unsigned long long)ev_scr);
}

// The slope guard (one lane per wave, r = the wave's largest ratio of a slope to L from one of the three sources): k_sampler_screen
// sees adjacent screened samples of its stride-1 passes (first blocks, restarts, the neighbourhoods of uncertain samples);
// k_screen_resolve sees the exact value of every listed sample against its screened predecessor, and k_screen_fin_entries the exact
// values of adjacent listed samples -- both where a ray is closest to the surface, and whatever the march strides over.
__device__ __forceinline__ void slope_guard_raise(const TraceWs& w, unsigned* source_bits, float r) {
    if (!(r > 0.0f)) return;
    // (a plain look first: the maxima only grow, and thousands of waves' atomics on one line would serialise)
    if (__float_as_uint(r) > *reinterpret_cast<volatile unsigned*>(source_bits)) atomicMax(source_bits, __float_as_uint(r));
    if (__float_as_uint(r) > *reinterpret_cast<volatile unsigned*>(&w.cnt->slope_bits)) atomicMax(&w.cnt->slope_bits, __float_as_uint(r));
    if (r > kStrideGuard && w.scr.flag) {   // the network's next call marches at stride 1
        *reinterpret_cast<volatile int*>(w.scr.flag + 1) = 1;
        __threadfence_system();
    }
}

template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_sampler_screen(IRON_TRACE_KERNEL_ARGS) {
    BE be;
    be.init(net, hs, hm);   // hs: the h1 stream
    const int lane = be.lane;   // every lane carries a sample of its own: 64 per wave, kScreenSlots ray slots
    const int slot = lane / kSamplerBlock, s_in = lane % kSamplerBlock;
    const int slot_lane0 = slot * kSamplerBlock;
    SamplerQ* const q = &w.cnt->smp;
    const int n_list = q->n_list;
    const bool dyn = w.cont_cap > 0;
    const long long n_tickets = (long long)n_list + (dyn ? (long long)w.cont_cap : 0ll);
    const float delta = screen_delta(w.scr);
    // the slope bound of the adaptive march (0: stride 1 throughout)
    float Lg = 0.0f;
    if (w.scr.stride & kStrideOn) {
        Lg =w.scr.l_override > 0.0f ? w.scr.l_override : kStrideK * __uint_as_float(w.scr.calib[kScreenCalibG]);
        if (!(Lg > 0.0f && Lg <= 3.0e38f)) Lg = 0.0f;
    }
    const bool stride_on = Lg > 0.0f;
    const float lin_step = a.lin[1] - a.lin[0];
    const int unit = stride_on ? 1 : kSamplerBlock;   // what the continuation word's position counts: samples | blocks
    if (stride_on && blockIdx.x == 0 && threadIdx.x == 0) w.cnt->stride_mode = 1;
    const bool pend_strides = !(w.scr.stride & kStridePendingOff), watch_march = !(w.scr.stride & kStrideMuteMarch);
    // (inf: no rise is enough.  kStridePendingOff is the march of a build that chose one-sided, and restores that too)
    const float rise_min = (w.scr.stride & (kStrideOneSided | kStridePendingOff)) ? __builtin_inff() : kStrideRise;
    // per lane: s_in 0: k_sampler's evaluations of the rays decided here, s_in 1: the slot's passes, s_in 2: those at a stride above 1,
    // s_in 3 / 4: the stride-1 passes of a ray already pending whose samples were all certainly positive / of a ray not yet pending,
    // s_in 5: discarded strided blocks, s_in 6: the slot's slope observations (screen_flush_counts)
    unsigned ev_ref = 0;
    unsigned ev_scr = 0;   // per wave: screened evaluations (parked by lane 0; the other lanes park their `slope` in that field)
    float slope = 0.0f;    // lanes with a predecessor in their block: the slope guard's ratio
    bool has_ray = false, retired = false, publish = false, pend = false;
    bool negl = false;     // the slot's ray has listed a sample with f1 < 0: what it lists from here on is deferred (k_resolve_list)
    int ticket = -1;
    int ray = 0, pos = 0, strd = 1, npass = 0, seg0 = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, smin = 0.f, width = 0.f, prev_z = 0.f, prev_f = 0.f;
    unsigned idle_polls = 0;
    for (;;) {
        const unsigned pub_slots = slot_heads<kScreenSlots>(__ballot(publish));
        const unsigned need_slots = slot_heads<kScreenSlots>(__ballot(!has_ray && ticket < 0 && !retired));
        if (pub_slots | need_slots) {
            const QueueBases qb = sampler_queue_bases(q, lane, need_slots, pub_slots);
            if (publish) {
                sampler_publish_item<__ATOMIC_RELEASE>(w, qb.pbase, pub_slots, slot, lane == slot_lane0, ray, pos, unit, prev_f,
                                                       (uint8_t)(pend ? (negl ? kRayPending | kRayNegListed : kRayPending) : 0));
                publish = false;
            }
            if (!has_ray && ticket < 0 && !retired) {
                ticket = sampler_draw(qb.tbase, need_slots, slot, n_tickets);
                if (ticket < 0) retired = true;
            }
        }
        if (!has_ray && ticket >= 0 && sampler_take(w, n_list, ticket, ray, pos, prev_f)) {
            pend = false;
            negl = false;
            if (ticket >= n_list) {
                // acquire only once the item is there (an acquiring poll invalidates the cache on every pass: +0.5 ms per frame)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                pos *= unit;
                const uint8_t st = w.scr.ray_state[ray];
                pend = (st & kRayPending) != 0;
                negl = (st & kRayNegListed) != 0;
            }
            ray_origin_dir(a, ray, ox, oy, oz, dx, dy, dz);
            ray_interval(a, ray, smin, width);
            // a continuation starts 1 + stride_reach(f of the item's last sample) behind that sample, as the publisher computed it;
            // the item carries no slope, so that first gap is the block's stride too and prev_z below is the sample strd in front of pos
            strd = 1;
            if (stride_on && pos > 0 && (pend_strides || !pend)) {
                const float ld = stride_ld(Lg, lin_step, width, dx, dy, dz);
                if (ld > 0.0f && prev_f > delta) strd = 1 + stride_reach(prev_f, delta, ld);
            }
            prev_z = pos > 0 ? sample_depth(smin, a.lin[pos > strd ? pos - strd : 0], width) : 0.f;   // the sample before the item's first
            npass = 0;
            seg0 = pos / kSegSamples;
            has_ray = true;
            ticket = -1;
        }
        if (!be.any(__ballot(has_ray) != 0ull)) {
            if (sampler_idle_done(be, q, n_list, w.cnt, ticket >= 0 || publish, idle_polls)) break;
            continue;
        }
        const int idx = pos + strd * s_in;
        const bool in_range = has_ray && idx < a.n_steps;
        const float z = sample_depth(smin, a.lin[in_range ? idx : a.n_steps - 1], width);
        const float qx = has_ray ? ox + dx * z : 0.f, qy = has_ray ? oy + dy * z : 0.f, qz = has_ray ? oz + dz * z : 0.f;
        {
            const int flags = (has_ray ? 1 : 0) | (retired ? 2 : 0) | (publish ? 4 : 0) | (in_range ? 8 : 0) | (pend ? 16 : 0) | (negl ? 32 : 0);
            const int ps = pos | (strd << kPosBits) | (npass << (kPosBits + kStrdBits)) | (seg0 << (kPosBits + kStrdBits + kPassBits));
            be.park(0, flags); be.park(1, ray); be.park(2, ps); be.park(3, ticket);
            park_vec6(be, 4, ox, oy, oz, dx, dy, dz);
            be.park(10, smin); be.park(11, width); be.park(12, prev_z); be.park(13, prev_f); be.park(14, z);
            be.park(15, (int)ev_ref); be.park(16, lane == 0 ? (int)ev_scr : __float_as_int(slope));
        }
        // envelope guard: an infinite screened value is no sign to rely on (+inf would pass as certainly positive and certify the
        // samples around it): as a NaN it is uncertain in every comparison below, is listed, and the resolve's exact value decides
        float f = be.template eval_screen<kH1PointTiles>(qx, qy, qz);
        if (!(fabsf(f) <= 3.0e38f)) f = quiet_nan();
        // the lane-derived masks after the evaluation come from an opaque copy of the lane: hoisted out of the loop, they are held
        // across the evaluation (in scratch, at 64 samples per wave)
        int me = lane;
        asm volatile("" : "+v"(me));
        const int sl0 = (me / kSamplerBlock) * kSamplerBlock, s_in_b = me % kSamplerBlock;
        const unsigned long long sbits = ((1ull << kSamplerBlock) - 1ull) << sl0;   // the slot's lanes
        const int flags_back = be.unpark(0, (has_ray ? 1 : 0) | (retired ? 2 : 0) | (publish ? 4 : 0) | (in_range ? 8 : 0) | (pend ? 16 : 0) | (negl ? 32 : 0));
        has_ray = flags_back & 1; retired = flags_back & 2; publish = flags_back & 4; pend = flags_back & 16; negl = flags_back & 32;
        const bool in_range_b = flags_back & 8;
        ray = be.unpark(1, ray); ticket = be.unpark(3, ticket);
        {
            const int ps = be.unpark(2, 0);
            pos = ps & ((1 << kPosBits) - 1); strd = (ps >> kPosBits) & ((1 << kStrdBits) - 1);
            npass = (ps >> (kPosBits + kStrdBits)) & ((1 << kPassBits) - 1); seg0 = (int)((unsigned)ps >> (kPosBits + kStrdBits + kPassBits));
        }
        unpark_vec6(be, 4, ox, oy, oz, dx, dy, dz);
        smin = be.unpark(10, smin); width = be.unpark(11, width); prev_z = be.unpark(12, prev_z); prev_f = be.unpark(13, prev_f);
        const float zb = be.unpark(14, z);
        ev_ref = (unsigned)be.unpark(15, (int)ev_ref);
        {
            const int v16 = be.unpark(16, 0);
            ev_scr = (unsigned)__shfl(v16, 0, 64);
            slope = me == 0 ? 0.0f : __int_as_float(v16);
        }
        idle_polls = 0;
        ev_scr += (unsigned)__popcll(__ballot(in_range_b));
        const int idx_b = pos + strd * s_in_b;
        const float ld = stride_on ? stride_ld(Lg, lin_step, width, dx, dy, dz) : 0.0f;
        const bool good = in_range_b && f > delta;                          // certainly positive
        const int reach = ld > 0.0f ? stride_reach(f, delta, ld) : 0;
        const int reach_next = __shfl(reach, me < 63 ? me + 1 : 63, 64);
        const float f_up = __shfl(f, me > 0 ? me - 1 : 0, 64);
        const unsigned long long rise = __ballot(f - f_up >= rise_min * (ld * (float)strd));   // (false with a NaN on either side)
        // a block at a stride above 1, walked in order: its first sample that is not certainly positive (the last good one is the
        // sample before it) or its first gap that is not certified from either end (the last good one is the sample in front of it)
        const bool strided = has_ray && strd > 1;
        const bool next_in = s_in_b < kSamplerBlock - 1 && idx_b + strd < a.n_steps;
        const int to_end = a.n_steps - 1 - idx_b;
        const int gap = s_in_b == kSamplerBlock - 1 ? 0 : (strd - 1 < to_end ? strd - 1 : to_end);   // skipped samples behind this one (the last lane's: the next block's start)
        const bool gap_ok = reach + (next_in ? reach_next : 0) >= gap;
        const unsigned long long bad_s = __ballot(strided && in_range_b && !good) & sbits;
        const unsigned long long bad_g = __ballot(strided && in_range_b && !gap_ok) & sbits;
        const bool restart = (bad_s | bad_g) != 0ull;
        const int k_s = bad_s ? (__ffsll((long long)bad_s) - 1 - sl0) : kSamplerBlock, k_g = bad_g ? (__ffsll((long long)bad_g) - 1 - sl0) : kSamplerBlock;
        const int last_good = k_s - 1 < k_g ? k_s - 1 : k_g;   // -1: the sample before the block
        const float z_good = __shfl(zb, sl0 + (last_good > 0 ? last_good : 0), 64), f_good = __shfl(f, sl0 + (last_good > 0 ? last_good : 0), 64);
        const bool counts = in_range_b && !restart;   // (nothing of a discarded block is used; a good strided block has only certainly positive samples)
        const bool is_neg = counts && f < -delta;                       // certainly negative
        const bool is_unc = counts && !(f > delta) && !(f < -delta);    // uncertain (NaN included)
        const unsigned long long neg = __ballot(is_neg) & sbits;
        const unsigned long long unc_all = __ballot(is_unc);
        const int first = neg ? (__ffsll((long long)neg) - 1) : sl0;
        const float z_first = __shfl(zb, first, 64), f_first = __shfl(f, first, 64);
        const float z_before = __shfl(zb, first > sl0 ? first - 1 : sl0, 64);
        const float f_before = __shfl(f, first > sl0 ? first - 1 : sl0, 64);
        const float z_last = __shfl(zb, sl0 + kSamplerBlock - 1, 64), f_last = __shfl(f, sl0 + kSamplerBlock - 1, 64);
        const int reach_last = __shfl(reach, sl0 + kSamplerBlock - 1, 64);
        const int gidx = pos + strd * (first - sl0);
        const bool found_neg = has_ray && neg != 0u;
        const float z_lo = first > sl0 ? z_before : prev_z, f_lo = first > sl0 ? f_before : prev_f;
        // the slope guard: adjacent samples of a stride-1 block, up to its first one that is not certainly positive
        const unsigned long long ngood = __ballot(in_range_b && !good) & sbits;
        {
            const int first_ng = ngood ? (__ffsll((long long)ngood) - 1) : 64;
            const bool obs = watch_march && has_ray && strd == 1 && ld > 0.0f && in_range_b && s_in_b > 0 && me <= first_ng;
            if (obs) slope = fmaxf(slope, fmaxf(fabsf(f - f_up) - 0.5f * delta, 0.0f) / ld);
            const unsigned long long obs_slot = __ballot(obs) & sbits;
            if (me == sl0 + 6) ev_ref += (unsigned)__popcll(obs_slot);
        }
        // uncertain samples in front of the slot's first certainly-negative one: to the resolve list, one atomicAdd per wave
        const unsigned long long before = neg ? (((1ull << first) - 1ull) & sbits) : sbits;
        const unsigned long long unc = has_ray ? (unc_all & before) : 0ull;
        const unsigned long long unc_wave = __ballot((unc >> me) & 1ull);   // (each lane sees its own slot's samples in unc)
        int rbase = 0;
        if (unc_wave) {
            if (me == 0) rbase = atomicAdd(&w.cnt->n_res, __popcll(unc_wave));
            rbase = __shfl(rbase, 0, 64);
        }
        // deferred: an earlier listed sample of the ray (of this pass or, negl, of an earlier one) has f1 < 0 -- strictly, as the
        // resolve's f < 0: NaN and zeros are not negative; the ray's first such sample itself is not deferred
        const unsigned long long unc_neg = __ballot(((unc >> me) & 1ull) && f < 0.0f) & sbits;
        const bool deferred = (w.scr.defer & kDeferOn) && (negl || (unc_neg & ((1ull << me) - 1ull)) != 0ull);
        negl = negl || unc_neg != 0ull;
        bool overflow = false;
        if (unc) {
            const int pos_last = rbase + lane_rank64(unc_wave, 63 - __clzll((long long)unc));
            overflow = pos_last >= w.scr.cap;
            const int pos_e = rbase + lane_rank64(unc_wave, me);
            if (((unc >> me) & 1ull) && pos_e < w.scr.cap) {   // written even for a ray that overflows: every slot below cap is valid
                ResolveEntry e;
                e.ray = ray; e.s = idx_b; e.z = zb; e.f1 = f; e.f_prev1 = s_in_b > 0 ? f_up : prev_f; e.f_ex = 0.f; e.ld = ld; e.mark = deferred ? kEntDeferred : 0;
                w.scr.ent[pos_e] = e;
            }
        }
        const bool pend_now = pend || unc != 0u;
        const bool to_ovf = has_ray && overflow;
        // where a good block is followed up: behind its last sample by what that sample certifies, for a pending ray too
        const bool last_in = pos + strd * (kSamplerBlock - 1) < a.n_steps;
        // The first gap has only e_7 to vouch for it: 1 + reach(e_7).  The gaps inside the next block have a sample at each end, and
        // where the values rise (behind a grazing ray's closest approach) each end certifies at least what e_7 did: the stride is
        // 1 + 2 * reach(e_7) when e_7 stands above e_6 by a slope of kStrideRise * L or more.  The choice is a guess about values not
        // yet seen; the walk above certifies every gap of the block from its evaluated ends, or discards it.
        const bool follow = ld > 0.0f && (pend_strides || !pend_now) && last_in && f_last > delta;
        const bool rising = (rise >> (sl0 + kSamplerBlock - 1)) & 1ull;
        const int next_gap = follow ? 1 + reach_last : 1;
        const int next_wide = 1 + 2 * reach_last < kStrideMax ? 1 + 2 * reach_last : kStrideMax;
        const int next_strd = (follow && rising) ? next_wide : next_gap;
        const int next_pos = pos + strd * (kSamplerBlock - 1) + next_gap;
        const bool done = has_ray && !restart && (found_neg || next_pos >= a.n_steps);
        if (has_ray && me == sl0 + 1) ++ev_ref;                 // the slot's passes
        if (strided && me == sl0 + 2) ++ev_ref;                 // ... at a stride above 1
        if (has_ray && strd == 1 && pend && ngood == 0ull && me == sl0 + 3) ++ev_ref;   // stride 1, already pending, all certainly positive
        if (has_ray && strd == 1 && !pend && me == sl0 + 4) ++ev_ref;                   // stride 1, not pending when the pass began
        if (restart && me == sl0 + 5) ++ev_ref;                 // discarded strided blocks
        if (to_ovf) {   // the ray goes to k_sampler's second list, marched from its start
            if (me == sl0) {
                w.scr.ray_state[ray] = kRayOverflowed;
                const int p = atomicAdd(&w.cnt->ovf.n_list, 1);
                w.scr.ovf_list[p] = ray;
                atomicAdd((unsigned long long*)&w.cnt->n_ovf, 1ull);
                atomicAdd(&q->n_done, 1);
            }
        } else if (done && me == sl0) {
            if (pend_now) {          // decided by k_screen_fin_* once the listed samples have their exact values
                PendRec r;
                r.first = found_neg ? gidx : a.n_steps;
                r.fhi = f_first; r.flo = f_lo; r.flo_ex = 0.f; r.has_flo_ex = 0; r.first_lost = 0x7fffffff; r.pad[0] = r.pad[1] = 0;
                w.scr.rec[ray] = r;
                const int p = atomicAdd(&w.cnt->n_pend, 1);
                w.scr.pend_list[p] = ray;
            } else {                 // exactly what k_sampler writes: every sample before gidx is positive, gidx is negative
                const int nb = found_neg ? (gidx / kSamplerBlock + 1) * kSamplerBlock : a.n_steps;   // k_sampler stops behind the block of gidx
                ev_ref += (unsigned)(nb < a.n_steps ? nb : a.n_steps);
                if (found_neg && gidx >= 1) {
                    sampler_write_root(w, ray, z_lo, z_first, f_lo, f_first);
                } else {
                    float zero = 0.f;
                    asm volatile("" : "+v"(zero));   // (else the zeros of these stores are held in registers across the loop)
                    sampler_write_no_root(a, ray, zero);
                }
            }
            atomicAdd(&q->n_done, 1);
        }
        pend = pend_now && !to_ovf;
        if (restart) {   // behind the last good sample, at stride 1
            // last_good < 0: the block's predecessor stays the previous sample.  It sits one first gap in front of pos, and the gap
            // was 1 + stride_reach of its value (the follow-up above or the taker; ld is the same product both times), whatever strd is.
            // Progress: the slot resumes one sample behind an evaluated, certainly positive sample -- of this block, or the previous
            // one -- at stride 1.  A stride-1 block never restarts (`strided` is false): it ends the ray or is followed up at least
            // one sample behind its last.  So pos exceeds the ray's last accepted sample after every pass, that sample moves forward
            // at least every second pass, and a ray ends after at most 2 * n_steps passes.
            if (last_good >= 0) {
                prev_z = z_good; prev_f = f_good;
                pos = pos + strd * last_good + 1;
            } else {
                pos = pos - stride_reach(prev_f, delta, ld);
            }
            strd = 1;
        } else {
            prev_z = z_last;
            prev_f = f_last;
            pos = next_pos;
            strd = next_strd;
        }
        if (npass < (1 << kPassBits) - 1) ++npass;
        // the end of a work item: after kSamplerSeg passes, in a later segment than the item's first (so a ray publishes at most one item per segment)
        const bool hand_over = has_ray && !to_ovf && !done && !restart && dyn && npass >= kSamplerSeg && pos / kSegSamples > seg0;
        publish = hand_over;
        if (done || hand_over || to_ovf) has_ray = false;
        if (ev_ref > (1u << 30) || ev_scr > (1u << 30)) {   // flush the 32-bit per-lane counts long before they can wrap
            screen_flush_counts(w.cnt, ev_ref, ev_scr, me);
            ev_ref = 0; ev_scr = 0;
        }
    }
    be.finish();
    screen_flush_counts(w.cnt, ev_ref, ev_scr, lane);
    const float r = wave_max(lane == 0 ? 0.0f : slope);
    if (lane == 0) slope_guard_raise(w, &w.cnt->slope_march_bits, r);
}

// The resolve's rounds.  A pending ray's outcome uses the exact value of its first listed sample that is negative
// (PendRec::first) and of the sample before it, nothing else; the screen's sign is right for all but a few samples, so the samples
// listed behind a ray's first one with f1 < 0 (kEntDeferred, marked by k_sampler_screen) almost never matter.  Round 1 evaluates the
// entries that are not deferred.  Round 2 takes a deferred entry only where it can still matter: e.s < first after round 1 (the
// screen called an earlier sample negative and its exact value is not); kDeferAudit: every deferred entry.  `first` only falls, and
// a deferred entry with e.s >= first after round 1 can neither lower it nor be the sample before it: the minimum over the rounds is
// the minimum over all listed samples.  Each round's entries are compacted into an index list so that its waves stay full.
// One atomicAdd per workgroup and batch of kListBatch entries per thread (per wave and 64 entries, the form of k_bisect_list, the
// 14 k atomics of a C1 frame's list on one counter took 0.16 ms, ten times the reading of the marks).
constexpr int kListBatch = 4;
__global__ __launch_bounds__(256) void k_resolve_list(TraceWs w, int round) {
    const int n_res = w.cnt->n_res;
    const int n_ent = n_res < w.scr.cap ? n_res : w.scr.cap;
    int* const count = round == 1 ? &w.cnt->n_res1 : &w.cnt->n_res2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_cnt[4];
    __shared__ int s_base;
    unsigned long long moot = 0;   // deferred entries round 2 leaves alone: settled without an evaluation
    for (long long i0 = (long long)blockIdx.x * (256 * kListBatch); i0 < n_ent; i0 += (long long)gridDim.x * (256 * kListBatch)) {
        bool take[kListBatch];
        int rank[kListBatch];
        int n_wave = 0;   // the wave's entries of this batch
#pragma unroll
        for (int k = 0; k < kListBatch; ++k) {
            const long long li = i0 + k * 256 + threadIdx.x;
            take[k] = false;
            if (li < n_ent) {
                ResolveEntry* const e = &w.scr.ent[li];
                const int mark = e->mark;
                if (round == 1) {
                    take[k] = mark == 0;
                } else if (mark == kEntDeferred) {
                    const int ray = e->ray;
                    take[k] = (w.scr.defer & kDeferAudit) || (w.scr.ray_state[ray] != kRayOverflowed && e->s < w.scr.rec[ray].first);
                    if (take[k]) e->mark = kEntDeferred | kEntRound2; else ++moot;
                }
            }
            const unsigned long long m = __ballot(take[k]);
            rank[k] = n_wave + lane_rank64(m, lane);
            n_wave += __popcll(m);
        }
        if (lane == 0) s_cnt[wave] = n_wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(count, total) : 0;
        }
        __syncthreads();
        int base = s_base;
        for (int v = 0; v < wave; ++v) base += s_cnt[v];
#pragma unroll
        for (int k = 0; k < kListBatch; ++k)
            if (take[k]) w.scr.res_idx[base + rank[k]] = (int)(i0 + k * 256 + threadIdx.x);
        __syncthreads();   // s_cnt and s_base are written again by the next batch
    }
    moot = wave_sum(moot);
    if (lane == 0 && moot) atomicAdd((unsigned long long*)&w.cnt->n_resolved, moot);
}

// exact (h2) values of listed samples, 32 per wave from any rays; the first negative one of each ray lowers its `first`
template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_screen_resolve(IRON_TRACE_KERNEL_ARGS) {
    const int round = w.scr.res_round;
    const int n_res = w.cnt->n_res;
    const int n_ent = round == 0 ? (n_res < w.scr.cap ? n_res : w.scr.cap) : round == 1 ? w.cnt->n_res1 : w.cnt->n_res2;
    if (n_ent == 0) return;   // (uniform over the grid) an empty round, as round 2 usually is: no weight ring is started
    int* const head = round == 2 ? &w.cnt->res_head2 : &w.cnt->res_head;
    BE be;
    be.init(net, hs, hm);
    const int lane = be.lane;
    const int j = lane & 31;
    const float delta = screen_delta(w.scr);
    long long resolved = 0;
    float ratio = 0.0f;
    float slope = 0.0f;   // the slope guard: |f_ex(s) - f1(s - 1)|, less delta / 2 for the screened side, relative to the ray's ld
    int n_obs = 0;
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(head, 32);
        base = __shfl(base, 0, 64);
        const bool valid = base + j < n_ent;
        const int li = !valid || round == 0 ? base + j : w.scr.res_idx[base + j];
        if (!be.any(base < n_ent)) break;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (valid) {
            const ResolveEntry& e = w.scr.ent[li];
            const int ray = e.ray;
            qx = a.ray_o[3 * (size_t)ray] + a.ray_d[3 * (size_t)ray] * e.z;
            qy = a.ray_o[3 * (size_t)ray + 1] + a.ray_d[3 * (size_t)ray + 1] * e.z;
            qz = a.ray_o[3 * (size_t)ray + 2] + a.ray_d[3 * (size_t)ray + 2] * e.z;
        }
        be.park(0, valid ? 1 : 0); be.park(1, li); be.park(2, ratio); park_i64(be, 3, resolved);
        be.park(5, slope); be.park(6, n_obs);
        const float f = be.eval(qx, qy, qz);
        const bool v = be.unpark(0, 0) != 0;
        const int lib = be.unpark(1, 0);
        ratio = be.unpark(2, 0.0f);
        resolved = unpark_i64(be, 3, resolved);
        slope = be.unpark(5, 0.0f); n_obs = be.unpark(6, 0);
        resolved += __popc((unsigned)__ballot(v));
        if (v && lane < 32) {
            ResolveEntry* e = &w.scr.ent[lib];
            e->f_ex = f;
            if (f < 0.0f) atomicMin(&w.scr.rec[e->ray].first, e->s);
            if (lost_value<BE>(f)) atomicMin(&w.scr.rec[e->ray].first_lost, e->s);   // (an overflowed ray's record is not read)
            const float f1 = e->f1;
            const float ld = e->ld;
            if (ld > 0.0f && e->s > 0) {   // sample s - 1 was screened at stride 1, next to s
                slope = fmaxf(slope, fmaxf(fabsf(f - e->f_prev1) - 0.5f * delta, 0.0f) / ld);
                ++n_obs;
            }
            float r = fabsf(f1 - f) / delta;
            if (!(r <= 3.0e38f)) r = ((fabsf(f1) <= 3.0e38f) != (fabsf(f) <= 3.0e38f)) ? 3.0e38f : 0.0f;   // one side non-finite: the screen failed
            ratio = fmaxf(ratio, r);
        }
    }
    be.finish();
    const float r = wave_max(ratio);
    const float sl = wave_max<16>(lane < 32 ? slope : 0.0f);   // (the lower half's lanes hold the samples)
    const int obs = wave_sum<16>(lane < 32 ? n_obs : 0);
    if (lane == 0) {
        if (obs) atomicAdd((unsigned long long*)&w.cnt->n_obs_res, (unsigned long long)obs);
        slope_guard_raise(w, &w.cnt->slope_res_bits, sl);
        atomicAdd((unsigned long long*)&w.cnt->n_resolved, (unsigned long long)resolved);
        atomicAdd((unsigned long long*)(round == 2 ? &w.cnt->n_eval_r2 : &w.cnt->n_eval_r1), (unsigned long long)resolved);
        atomicMax(&w.cnt->ratio_bits, __float_as_uint(r));
        if (r > kScreenGuard && w.scr.flag) {   // the guard: the network's next call runs the unscreened sampler
            *reinterpret_cast<volatile int*>(w.scr.flag) = 1;
            __threadfence_system();
        }
    }
}

// the exact values at each pending ray's bracket: its first negative sample and the one before it, where those were listed.
// A deferred entry no round evaluated (mark == kEntDeferred) has no f_ex, and is neither: it failed e.s < first after round 1, the
// final g is at or below that `first`, and e.s == g is impossible -- g is a sample some round found negative, or the march's
// certainly-negative one, which is not listed.  Sample g - 1, where listed, was evaluated: by round 1, or (deferred, g - 1 < g <= the
// `first` round 2 compared it with) by round 2.
__global__ void k_screen_fin_entries(TraceWs w) {
    const int n_res = w.cnt->n_res;
    const int n_ent = n_res < w.scr.cap ? n_res : w.scr.cap;
    float slope = 0.0f;   // the slope guard: exact values of adjacent listed samples (a pass lists its samples in order), relative to ld
    int n_obs = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_ent; i += gridDim.x * blockDim.x) {
        const ResolveEntry e = w.scr.ent[i];
        if (e.mark == kEntDeferred) continue;
        const float ld = e.ld;
        if (i > 0 && ld > 0.0f) {
            const ResolveEntry p = w.scr.ent[i - 1];
            if (p.ray == e.ray && p.s + 1 == e.s && p.mark != kEntDeferred) {
                slope = fmaxf(slope, fabsf(e.f_ex - p.f_ex) / ld);
                ++n_obs;
            }
        }
        if (w.scr.ray_state[e.ray] == kRayOverflowed) continue;
        PendRec* r = &w.scr.rec[e.ray];
        const int g = r->first;
        if (e.s == g) { r->fhi = e.f_ex; r->flo = e.f_prev1; }   // (overwritten below when sample g - 1 was listed too)
        if (e.s == g - 1) { r->flo_ex = e.f_ex; r->has_flo_ex = 1; }
    }
    slope = wave_max(slope);
    n_obs = wave_sum(n_obs);
    __shared__ float s_slope[16];   // one set of atomics per workgroup (blockDim.x <= 1024)
    __shared__ int s_obs[16];
    const int wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { s_slope[wave] = slope; s_obs[wave] = n_obs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < n_waves; ++k) { slope = fmaxf(slope, s_slope[k]); n_obs += s_obs[k]; }
        if (n_obs) atomicAdd((unsigned long long*)&w.cnt->n_obs_pair, (unsigned long long)n_obs);
        slope_guard_raise(w, &w.cnt->slope_pair_bits, slope);
    }
}

// each pending ray's outcome, as k_sampler writes it
__global__ void k_screen_fin_rays(TraceArgs a, TraceWs w) {
    const int n_pend = w.cnt->n_pend;
    unsigned long long ev = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pend; i += gridDim.x * blockDim.x) {
        const int ray = w.scr.pend_list[i];
        const PendRec r = w.scr.rec[ray];
        const int g = r.first;
        const int nb = (g / kSamplerBlock + 1) * kSamplerBlock;
        ev += (unsigned long long)(g < a.n_steps ? (nb < a.n_steps ? nb : a.n_steps) : a.n_steps);
        if (r.first_lost <= g) {   // envelope guard: an overflowed sample at or in front of the first negative one, as k_sampler ends such a ray
            sampler_write_no_root(a, ray, quiet_nan());
        } else if (g >= 1 && g < a.n_steps) {
            float smin, width;
            ray_interval(a, ray, smin, width);
            sampler_write_root(w, ray, sample_depth(smin, a.lin[g - 1], width), sample_depth(smin, a.lin[g], width),
                               r.has_flo_ex ? r.flo_ex : r.flo, r.fhi);
        } else {
            sampler_write_no_root(a, ray, 0.f);
        }
    }
    ev = wave_sum(ev);
    if ((threadIdx.x & 63) == 0 && ev) atomicAdd((unsigned long long*)&w.cnt->n_evals, ev);
}

// calibration of the margin: max |f_screen - f_h2| over a fixed set of points in the unit ball (a golden-angle spiral of
// directions, radii from the R2 sequence), once per network handle before its first screened trace.  Two ring passes over the
// block's points, one per stream: the screen on the h1 stream (hs1) leaves f1 in calib[kScreenCalibF1 + i] (every lane stores its own
// point's value and reads back only what it stored), then h2 (hs) compares.
__device__ __forceinline__ void screen_calib_point(int i, float& x, float& y, float& z) {
    const float u = (i + 0.5f) / kScreenCalibPoints;
    const float cz = 1.0f - 2.0f * u, sz = sqrtf(fmaxf(0.0f, 1.0f - cz * cz));
    const float phi = 2.39996323f * (float)i;
    float fr = 0.7548776662f * (float)i;
    fr -= floorf(fr);
    const float rad = cbrtf(0.5f / kScreenCalibPoints + fr * (1.0f - 1.0f / kScreenCalibPoints));
    x = rad * sz * cosf(phi); y = rad * sz * sinf(phi); z = rad * cz;
}

__global__ __launch_bounds__(256, 1) void k_screen_calib(SdfNetDev net, H2StreamDev hs, H2StreamDev hs1, H2Meta hm, unsigned* calib) {
    BackendH2 be;
    float* const f1s = reinterpret_cast<float*>(calib) + kScreenCalibF1;
    be.init(net, hs1, hm);
    for (int g = blockIdx.x; g < kScreenCalibPoints / 128; g += gridDim.x) {
        const int i = g * 128 + be.wave * 32 + (be.lane & 31);
        float x, y, z;
        screen_calib_point(i, x, y, z);
        const float f1 = be.eval_screen<1>(x, y, z);
        f1s[i] = f1;   // lanes j and j + 32: the same point, the same value
    }
    be.finish();
    be.init(net, hs, hm);
    const int lane = be.lane;
    float m = 0.0f;
    for (int g = blockIdx.x; g < kScreenCalibPoints / 128; g += gridDim.x) {
        const int i = g * 128 + be.wave * 32 + (lane & 31);
        float x, y, z;
        screen_calib_point(i, x, y, z);
        be.park(1, m);
        const float f2 = be.eval(x, y, z);
        const float d = fabsf(f1s[i] - f2);
        m = be.unpark(1, 0.0f);
        if (d <= 3.0e38f) m = fmaxf(m, d);
    }
    // G = max |grad f| over the same points for the adaptive march's slope bound: central differences of the h2 value at kStrideCalibH
    // (a non-finite one makes G infinite: the march stays at stride 1)
    float gm = 0.0f;
    for (int g = blockIdx.x; g < kScreenCalibPoints / 128; g += gridDim.x) {
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll 1
        for (int e = 0; e < 6; ++e) {
            const int i = g * 128 + be.wave * 32 + (lane & 31);
            float x, y, z;
            screen_calib_point(i, x, y, z);
            const float sg = (e & 1) ? -1.0f : 1.0f;
            const int ax = e >> 1;
            be.park(1, gm); be.park(2, gx); be.park(3, gy); be.park(4, gz); be.park(5, m);
            const float fv = be.eval(x + (ax == 0 ? sg * kStrideCalibH : 0.0f), y + (ax == 1 ? sg * kStrideCalibH : 0.0f),
                                     z + (ax == 2 ? sg * kStrideCalibH : 0.0f));
            gm = be.unpark(1, 0.0f); gx = be.unpark(2, 0.0f); gy = be.unpark(3, 0.0f); gz = be.unpark(4, 0.0f); m = be.unpark(5, 0.0f);
            const int axb = e >> 1;
            const float d = ((e & 1) ? -fv : fv) * (0.5f / kStrideCalibH);
            gx += axb == 0 ? d : 0.0f; gy += axb == 1 ? d : 0.0f; gz += axb == 2 ? d : 0.0f;
        }
        const float gn = sqrtf(gx * gx + gy * gy + gz * gz);
        gm = gn <= 3.0e38f ? fmaxf(gm, gn) : __uint_as_float(0x7f800000u);
    }
    be.finish();
    m = wave_max(m);
    gm = wave_max(gm);
    if (lane == 0) { atomicMax(calib, __float_as_uint(m)); atomicMax(calib + kScreenCalibG, __float_as_uint(gm)); }
}

__device__ __forceinline__ long long ray_chunk(const TraceArgs& a, int ray) {
    const long long gi = a.ray_index ? a.ray_index[ray] : (long long)ray;
    return a.chunk > 0 ? gi / a.chunk : 0;
}

// ---- rootfind (raytracer.py:199-220) ------------------------------------------------------------------------------------------------
// The reference evaluates T + 1 mid-points per bracketed ray, T = the largest own count among the rays of its chunk: mid_1 .. mid_T
// inside the loop (every ray is updated while ANY is unfinished) and mid_{T+1} after it.  "Iteration t" and "the final evaluation"
// compute the same thing, f(o + d * mid_t), so a ray that has done its own k iterations evaluates mid_{k+1} in the slot it already
// holds (k_bisect_a: k + 1 evaluations, or more where its chunk's count is already known to be higher) and leaves that value with
// lo, hi and k.  If T == k it is the ray's result; if T > k it is the f that iteration k + 1 consumes, and the ray needs exactly
// T - k more evaluations, the last of which is its result (k_bisect_b).
// Both kernels hold 32 rays per wave and refill a retired slot at once (ballot -> rank -> one atomicAdd per wave, as k_sphere).
// A ray's evaluations, their order and what is made of them are the reference's; only where they run changes.

// the chunk counters after a pass, by one leader lane per distinct chunk among the wave's rays: chunk_roots += the rays loaded for
// this pass, chunk_iters = max(.., bound), a lane's bound being a count its chunk is now known to reach (0: none).  A plain look
// first: the table only grows and every wave posts the same few counts, so nearly all of the atomicMax-es are never issued.
// Returns the largest bound among the wave's rays of the lane's chunk.  (ballots are read by their low word: lanes 32..63 mirror 0..31)
__device__ __forceinline__ int bisect_count_chunks(const TraceWs& w, int lane, bool active, bool fresh, int ch, int bound) {
    unsigned left = (unsigned)__ballot(active);
    int wave_bound = 0;
    while (left) {
        const int lead = __ffs(left) - 1;
        const int ch0 = __shfl(ch, lead, 64);
        const bool mine = active && ch == ch0;
        const unsigned came = (unsigned)__ballot(mine && fresh);
        int b = mine ? bound : 0;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) b = max(b, __shfl_xor(b, off, 64));
        if (lane == lead) {
            if (came) atomicAdd(&w.chunk_roots[ch0], __popc(came));
            if (b > __hip_atomic_load(&w.chunk_iters[ch0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&w.chunk_iters[ch0], b);
        }
        if (mine) wave_bound = b;
        left &= ~(unsigned)__ballot(mine);
    }
    return wave_bound;
}

// the free slots' places in a list of n entries behind *head: the wave's base, and how many of its nfree requests are served
struct SlotDraw { int base, avail; };
__device__ __forceinline__ SlotDraw bisect_draw(int* head, int lane, int nfree, int n) {
    int base = 0;
    if (lane == 0) base = atomicAdd(head, nfree);
    base = __shfl(base, 0, 64);
    const int left = n - base;
    return SlotDraw{base, left < 0 ? 0 : (left > nfree ? nfree : left)};
}

// a retired ray's result (raytracer.py:75-78: the sampler's mask overwrites convergent)
__device__ __forceinline__ void bisect_write(const TraceArgs& a, int ray, float qx, float qy, float qz, float f, float mid) {
    if (!(mid == mid)) f = mid;   // a NaN interval (lost_value, or the caller's): sdf, the output the envelope scan reads, says so itself
    a.conv[ray] = 1;
    a.points[3 * (size_t)ray] = qx; a.points[3 * (size_t)ray + 1] = qy; a.points[3 * (size_t)ray + 2] = qz;
    a.sdf[ray] = f;
    a.dist[ray] = mid;
}

// per-ray part (raytracer.py:199-217): the ray's own iterations until ITS interval is <= 2 * threshold (none for a bracket without
// a sign change), then the evaluation of the mid-point it ends on.  Leaves lo, hi, the iterations done k and that value (in root_flo,
// dead once the ray is loaded), writes the ray's outputs as if it were final, and counts the ray into its chunk.
// The chunk table is kept as a running lower bound of the chunk's count T: a ray posts k + 1 while it still has an iteration of its own
// to make, so the table ends as the largest own count, as the reference's loop counts it.  A ray whose own iterations are done looks
// at it, and at what its own wave's rays of the same chunk post in this pass: a bound above its k proves that iteration k + 1 is
// needed, and the ray makes it here, in its slot, on the value it has just evaluated ("follows") instead of waiting for phase b.
// That matters because a ray far below its chunk's count (a bracket without a sign change in a chunk that runs 7) is a chain of
// T + 1 dependent evaluations: left to phase b, the chain is that kernel's whole duration with the chip idle around it (measured:
// phase b took the same 0.63 ms with two thirds of its evaluations removed); here it runs under the other rays' work.  How many of a
// ray's T + 1 evaluations run in which phase depends on timing; which points are evaluated, and every result, do not.
template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_bisect_a(IRON_TRACE_KERNEL_ARGS) {
    const int n_root = w.cnt->n_root;
    if (n_root == 0) return;   // (uniform over the grid) nothing to bisect: no weight ring is started
    BE be;
    be.init(net, hs, hm);
    const int lane = be.lane;
    const int j = lane & 31;
    const float thr2 = 2.0f * a.thr;
    long long evals = 0;
    bool active = false, exhausted = false, work = false, fresh = false;
    int li = 0, ray = 0, k = 0, ch = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, lo = 0.f, hi = 0.f, mid = 0.f;
    for (;;) {
        // ---- refill free slots from the root list
        const unsigned act = (unsigned)__ballot(active);
        const int nfree = 32 - __popc(act);
        if (nfree > 0 && !exhausted) {
            const SlotDraw dr = bisect_draw(&w.cnt->root_head_a, lane, nfree, n_root);
            if (dr.base + nfree >= n_root) exhausted = true;
            if (!active && lane_rank(~act, j) < dr.avail) {
                li = dr.base + lane_rank(~act, j);
                ray = w.root_list[li];
                ch = (int)ray_chunk(a, ray);
                ray_origin_dir(a, ray, ox, oy, oz, dx, dy, dz);
                lo = w.root_lo[li]; hi = w.root_hi[li];
                work = (w.root_flo[li] > 0.0f) && (w.root_fhi[li] < 0.0f);
                mid = (lo + hi) / 2.0f;
                k = 0;
                active = true;
                fresh = true;
            }
        }
        const unsigned act2 = (unsigned)__ballot(active);
        if (!be.any(act2 != 0u)) break;
        evals += __popc(act2);
        {   // the rays' state waits in LDS while the evaluation has the registers
            const int flags = (active ? 1 : 0) | (exhausted ? 2 : 0) | (work ? 4 : 0) | (fresh ? 8 : 0);
            be.park(0, flags); be.park(1, li); be.park(2, ray); be.park(3, k);
            park_vec6(be, 4, ox, oy, oz, dx, dy, dz);
            be.park(10, lo); be.park(11, hi); be.park(12, mid); park_i64(be, 13, evals);
            be.park(15, ch);
        }
        const float f = be.eval(ox + dx * mid, oy + dy * mid, oz + dz * mid);
        {
            const int flags = be.unpark(0, (active ? 1 : 0) | (exhausted ? 2 : 0) | (work ? 4 : 0) | (fresh ? 8 : 0));
            active = flags & 1; exhausted = flags & 2; work = flags & 4; fresh = flags & 8;
            li = be.unpark(1, li); ray = be.unpark(2, ray); k = be.unpark(3, k);
            unpark_vec6(be, 4, ox, oy, oz, dx, dy, dz);
            lo = be.unpark(10, lo); hi = be.unpark(11, hi); mid = be.unpark(12, mid);
            evals = unpark_i64(be, 13, evals);
            ch = be.unpark(15, ch);
        }
        if (lost_value<BE>(f)) mid = quiet_nan();   // envelope guard: the interval, every later mid-point and the ray's outputs are NaN from here
        // outcome of the pass for the slot (straight-line): an iteration of the ray's own, one its chunk is known to need, or the
        // ray's last evaluation here
        const bool own = active && work;
        const float qx = ox + dx * mid, qy = oy + dy * mid, qz = oz + dz * mid;   // (the same expressions: the evaluated point)
        const float f_lo = (f > 0.0f) ? mid : lo, f_hi = (f > 0.0f) ? hi : mid;    // the interval after an iteration on f
        int bound = 0;
        if (own) {
            work = ((f_hi - f_lo) > thr2) && (k + 1 < 64);  // k < 64: exit bound for non-finite intervals
            bound = k + 1 + (work ? 1 : 0);
        }
        const int wave_bound = bisect_count_chunks(w, lane, active, fresh, ch, bound);
        fresh = false;
        const int table = (active && !own) ? __hip_atomic_load(&w.chunk_iters[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const bool follow = active && !own && max(table, wave_bound) > k;
        const bool retire = active && !own && !follow;
        if (retire && lane < 32) {
            w.root_lo[li] = lo; w.root_hi[li] = hi;
            w.root_k[li] = k;
            w.root_flo[li] = f;
            bisect_write(a, ray, qx, qy, qz, f, mid);
        }
        if (own || follow) {
            lo = f_lo; hi = f_hi;
            mid = (lo + hi) / 2.0f;
            ++k;
        }
        if (retire) {
            active = false;
            ox = oy = oz = dx = dy = dz = mid = 0.f;
        }
    }
    be.finish();
    if (lane == 0) atomicAdd((unsigned long long*)&w.cnt->n_evals, (unsigned long long)evals);
}

// the rays phase b has to touch: those whose chunk's count (MAX-reduced over the ranks by then, in the multi-rank form) is above
// their own.  Their list positions are compacted into root_fhi's storage (dead like root_flo); cnt->n_root_b counts them.
__global__ void k_bisect_list(TraceArgs a, TraceWs w) {
    const int n_root = w.cnt->n_root;
    int* const list = reinterpret_cast<int*>(w.root_fhi);
    const int lane = threadIdx.x & 63;
    for (int i0 = blockIdx.x * blockDim.x; i0 < n_root; i0 += gridDim.x * blockDim.x) {
        const int li = i0 + threadIdx.x;
        const bool more = li < n_root && w.chunk_iters[ray_chunk(a, w.root_list[li])] - w.root_k[li] > 0;
        const unsigned long long m = __ballot(more);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(&w.cnt->n_root_b, __popcll(m));
        base = __shfl(base, 0, 64);
        if (more) list[base + lane_rank64(m, lane)] = li;
    }
}

// chunk-global remainder (raytracer.py:204-219): a listed ray applies the update its stored value decides and evaluates
// `remaining` more mid-points; the last one is its result.
template <class BE>
__global__ __launch_bounds__(BE::kThreads, 1) void k_bisect_b(IRON_TRACE_KERNEL_ARGS) {
    const int n_list = w.cnt->n_root_b;
    if (n_list == 0) return;   // (uniform over the grid) every ray ran to its chunk's count in phase a: no weight ring is started
    BE be;
    be.init(net, hs, hm);
    const int lane = be.lane;
    const int j = lane & 31;
    const int* const list = reinterpret_cast<const int*>(w.root_fhi);
    long long evals = 0;
    bool active = false, exhausted = false;
    int ray = 0, remaining = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, lo = 0.f, hi = 0.f, mid = 0.f;
    for (;;) {
        const unsigned act = (unsigned)__ballot(active);
        const int nfree = 32 - __popc(act);
        if (nfree > 0 && !exhausted) {
            const SlotDraw dr = bisect_draw(&w.cnt->root_head_b, lane, nfree, n_list);
            if (dr.base + nfree >= n_list) exhausted = true;
            if (!active && lane_rank(~act, j) < dr.avail) {
                const int li = list[dr.base + lane_rank(~act, j)];
                ray = w.root_list[li];
                ray_origin_dir(a, ray, ox, oy, oz, dx, dy, dz);
                lo = w.root_lo[li]; hi = w.root_hi[li];
                mid = (lo + hi) / 2.0f;
                if (w.root_flo[li] > 0.0f) lo = mid; else hi = mid;   // iteration k + 1 on the value phase a left
                mid = (lo + hi) / 2.0f;
                remaining = w.chunk_iters[ray_chunk(a, ray)] - w.root_k[li];
                active = true;
            }
        }
        const unsigned act2 = (unsigned)__ballot(active);
        if (!be.any(act2 != 0u)) break;
        evals += __popc(act2);
        {   // the rays' state waits in LDS while the evaluation has the registers
            const int flags = (active ? 1 : 0) | (exhausted ? 2 : 0);
            be.park(0, flags); be.park(1, ray); be.park(2, remaining);
            park_vec6(be, 3, ox, oy, oz, dx, dy, dz);
            be.park(9, lo); be.park(10, hi); be.park(11, mid); park_i64(be, 12, evals);
        }
        const float f = be.eval(ox + dx * mid, oy + dy * mid, oz + dz * mid);
        {
            const int flags = be.unpark(0, (active ? 1 : 0) | (exhausted ? 2 : 0));
            active = flags & 1; exhausted = flags & 2;
            ray = be.unpark(1, ray); remaining = be.unpark(2, remaining);
            unpark_vec6(be, 3, ox, oy, oz, dx, dy, dz);
            lo = be.unpark(9, lo); hi = be.unpark(10, hi); mid = be.unpark(11, mid);
            evals = unpark_i64(be, 12, evals);
        }
        if (lost_value<BE>(f)) mid = quiet_nan();   // envelope guard, as in k_bisect_a
        // outcome of the pass for the slot (straight-line): the ray's last evaluation, or one more iteration
        const bool retire = active && remaining <= 1;
        const float qx = ox + dx * mid, qy = oy + dy * mid, qz = oz + dz * mid;   // (the same expressions: the evaluated point)
        if (retire && lane < 32) bisect_write(a, ray, qx, qy, qz, f, mid);
        if (active && !retire) {
            if (f > 0.0f) lo = mid; else hi = mid;
            mid = (lo + hi) / 2.0f;
            --remaining;
        }
        if (retire) {
            active = false;
            ox = oy = oz = dx = dy = dz = mid = 0.f;
        }
    }
    be.finish();
    if (lane == 0) atomicAdd((unsigned long long*)&w.cnt->n_evals, (unsigned long long)evals);
}

// `w.cnt` = the first part's counters; the parts' counter blocks are kCntStride bytes apart
constexpr size_t kCntStride = 256;
__global__ void k_trace_stats(TraceWs w, int n_parts, int n_steps, iron_trace_stats* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        long long n_evals = 0, n_sphere_conv = 0, n_sampler = 0, n_root = 0, n_evals_sphere = 0, n_abort = 0;
        for (int p = 0; p < n_parts; ++p) {
            const TraceCounters* c = (const TraceCounters*)((const char*)w.cnt + (size_t)p * kCntStride);
            n_evals += c->n_evals; n_sphere_conv += c->n_sphere_conv; n_sampler += c->smp.n_list; n_root += c->n_root;
            n_evals_sphere += c->n_evals_sphere;
            n_abort += c->sampler_abort;
        }
        out->n_evals = n_evals;
        out->n_sphere_conv = n_sphere_conv;
        out->n_sampler = n_sampler;
        out->n_bisect = n_root;
        out->n_conv = n_sphere_conv + n_root;
        long long e = n_evals_sphere + n_sampler * n_steps;
        for (int c = 0; c < w.n_chunks; ++c) e += (long long)w.chunk_roots[c] * (w.chunk_iters[c] + 1);
        out->n_evals_ref = e;
        out->n_evals_sphere = n_evals_sphere;
        out->reserved = n_abort;   // k_sampler workgroups that gave up polling (iron_hip.h)
    }
}

// ---- single stages (iron_trace_stage: RayTracer.sphere_tracing / ray_sampler / rootfind as callable methods) ---------------------
__global__ void k_stage_mark_list(const int* __restrict__ list, const int* __restrict__ count, uint8_t* __restrict__ mask) {
    const int n = *count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mask[list[i]] = 1;
}

// ray_sampler (raytracer.py:142-197) takes every ray of the call with its own interval [min_dis, max_dis]: the list is the
// identity and the per-ray state the dense sampler reads is set so that it samples exactly that interval (sdf > 0: [dist, far])
__global__ void k_stage_sampler_init(TraceArgs a, TraceWs w, const float* __restrict__ min_dis) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
        w.sampler_list[i] = i;
        a.dist[i] = min_dis[i];
        a.sdf[i] = 1.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) w.cnt->smp.n_list = a.n;
}

// rootfind (raytracer.py:199-220) on caller-given brackets
__global__ void k_stage_root_init(TraceWs w, int n, const float* __restrict__ f_low, const float* __restrict__ f_high,
                                  const float* __restrict__ d_low, const float* __restrict__ d_high) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        w.root_list[i] = i;
        w.root_lo[i] = d_low[i]; w.root_hi[i] = d_high[i];
        w.root_flo[i] = f_low[i]; w.root_fhi[i] = f_high[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) w.cnt->n_root = n;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct WsLayout {
    size_t cnt, sampler_list, root_list, lo, hi, flo, fhi, k, chunk_iters, chunk_roots, cont, total;
    size_t s_rec, s_pend, s_ovf, s_flag, s_ent, s_idx;   // the screened sampler's arrays
    int64_t n_chunks, cont_cap;
};

static WsLayout ws_layout(int64_t n, const iron_trace_params* p) {
    WsLayout L;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    L.n_chunks = (p && p->chunk > 0) ? (n + p->chunk - 1) / p->chunk : 1;
    if (L.n_chunks < 1) L.n_chunks = 1;
    size_t o = 0;
    static_assert(sizeof(TraceCounters) <= kCntStride, "counter block");
    L.cnt = o; o += kCntStride * kMaxTraceSplits;
    L.chunk_iters = o; o += align256(sizeof(int) * (size_t)L.n_chunks);
    L.chunk_roots = o; o += align256(sizeof(int) * (size_t)L.n_chunks);
    L.sampler_list = o; o += align256(sizeof(int) * nn);
    L.root_list = o; o += align256(sizeof(int) * nn);
    L.lo = o; o += align256(sizeof(float) * nn);
    L.hi = o; o += align256(sizeof(float) * nn);
    L.flo = o; o += align256(sizeof(float) * nn);
    L.fhi = o; o += align256(sizeof(float) * nn);
    L.k = o; o += align256(sizeof(int) * nn);
    L.cont_cap = sampler_cont_cap(n, p ? p->n_steps : 128);   // k_sampler's continuation items
    L.cont = o; o += align256(sizeof(unsigned long long) * (size_t)(L.cont_cap > 0 ? L.cont_cap : 1));
    L.s_rec = o; o += align256(sizeof(PendRec) * nn);
    L.s_pend = o; o += align256(sizeof(int) * nn);
    L.s_ovf = o; o += align256(sizeof(int) * nn);
    L.s_flag = o; o += align256(nn);
    L.s_ent = o; o += align256(sizeof(ResolveEntry) * nn * kResolvePerRay);
    L.s_idx = o; o += align256(sizeof(int) * nn * kResolvePerRay);   // the resolve's index list (whatever the deferral's switch says)
    L.total = o;
    return L;
}

static int resident_waves() {
    // single-wave workgroups, one wave per SIMD (the kernels need > 256 registers per lane); iron_set_cu_limit narrows it
    return cu_budget() * 4;
}

// the last three on the h2 core only; `units` = wave-sized work items available
enum TraceKernel { kSphere = 0, kSampler = 1, kBisectA = 2, kBisectB = 3, kSamplerScreen = 4, kScreenResolve = 5, kScreenCalib = 6 };

static void launch_trace_kernel(TraceKernel which, bool h2, const iron_net* sdf, const TraceArgs& a, const TraceWs& w, int64_t units,
                                hipStream_t st) {
    H2Meta m;
    m.n_hidden_layers = sdf->sdf.n_hidden_layers; m.skip_layer = sdf->sdf.skip_layer; m.scale = sdf->sdf.scale; m.b_last = sdf->sdf.b_last;
    if (units < 1) units = 1;
    if (h2) {
        static bool attr = false;
        if (!attr) {
            const void* const kernels[] = {(const void*)k_sphere<BackendH2>, (const void*)k_sampler<BackendH2Sampler>, (const void*)k_bisect_a<BackendH2>,
                                           (const void*)k_bisect_b<BackendH2>, (const void*)k_sampler_screen<BackendH2Sampler>,
                                           (const void*)k_screen_resolve<BackendH2>, (const void*)k_screen_calib};
            for (const void* k : kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTraceTotal);
            attr = true;
        }
        const int64_t wgs = (units + 3) / 4;
        const int cus = resident_waves() / 4;
        const dim3 grid((unsigned)(wgs < cus ? wgs : cus)), block(256);
        switch (which) {
            case kSphere: hipLaunchKernelGGL(k_sphere<BackendH2>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kSampler: hipLaunchKernelGGL(k_sampler<BackendH2Sampler>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kBisectA: hipLaunchKernelGGL(k_bisect_a<BackendH2>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kSamplerScreen: hipLaunchKernelGGL(k_sampler_screen<BackendH2Sampler>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h1_trace, m, a, w); break;
            case kScreenResolve: hipLaunchKernelGGL(k_screen_resolve<BackendH2>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kScreenCalib: hipLaunchKernelGGL(k_screen_calib, dim3(cus < kScreenCalibPoints / 128 ? cus : kScreenCalibPoints / 128), block,
                                                  kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, sdf->h1_trace, m, sdf->screen_calib); break;
            default: hipLaunchKernelGGL(k_bisect_b<BackendH2>, grid, block, kLdsTraceTotal, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
        }
    } else {
        const int waves = resident_waves();
        const dim3 grid((unsigned)(units < waves ? units : waves)), block(64);
        switch (which) {
            case kSphere: hipLaunchKernelGGL(k_sphere<BackendF32>, grid, block, 0, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kSampler: hipLaunchKernelGGL(k_sampler<BackendF32>, grid, block, 0, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            case kBisectA: hipLaunchKernelGGL(k_bisect_a<BackendF32>, grid, block, 0, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
            default: hipLaunchKernelGGL(k_bisect_b<BackendF32>, grid, block, 0, st, sdf->sdf, sdf->h2_trace, m, a, w); break;
        }
    }
}

// ---- the screened sampler's host side ----------------------------------------------------------------------------------------
std::atomic<int> g_screen_switch{-1};           // iron_set_sampler_screen; -1 = the environment's (IRON_SAMPLER_SCREEN=0: off) / default on
std::atomic<float> g_screen_delta_override{0.0f};   // test hooks (iron_sampler_screen_debug)
std::atomic<int> g_screen_cap_override{0};
std::atomic<int> g_stride_switch{-1};           // iron_set_sampler_stride; -1 = the environment's (IRON_SAMPLER_STRIDE=0: off) / default on
std::atomic<float> g_stride_l_override{0.0f};   // test hook (iron_sampler_screen_debug 3)
std::atomic<int> g_stride_hooks{0};             // test hooks (iron_sampler_screen_debug 4, 5, 6): kStridePendingOff | kStrideMuteMarch | kStrideOneSided
std::atomic<int> g_defer_switch{-1};            // iron_set_resolve_defer; -1 = the environment's (IRON_RESOLVE_DEFER=0: off) / default on
void set_screen_forward_tiles(int point_tiles);   // h2_kernels.hip

// a switch set by its setter (>= 0), else by the environment (NAME=0: off, read once), else on
static bool env_switch(const char* name, const std::atomic<int>& set, int* from_env) {
    if (*from_env < 0) {
        const char* e = getenv(name);
        *from_env = (e && e[0] == '0') ? 0 : 1;
    }
    const int v = set.load(std::memory_order_relaxed);
    return v < 0 ? *from_env != 0 : v != 0;
}
static bool screen_switch() { static int from_env = -1; return env_switch("IRON_SAMPLER_SCREEN", g_screen_switch, &from_env); }
static bool stride_switch() { static int from_env = -1; return env_switch("IRON_SAMPLER_STRIDE", g_stride_switch, &from_env); }
static bool defer_switch() { static int from_env = -1; return env_switch("IRON_RESOLVE_DEFER", g_defer_switch, &from_env); }

// at the start of a call: act on a guard flag an earlier call raised, then decide whether this call screens (h2 core only)
static int screen_begin(const iron_net* cnet, bool h2, hipStream_t st, bool* use) {
    iron_net* net = const_cast<iron_net*>(cnet);
    *use = false;
    if (net->flag_host && *(volatile int*)(net->flag_host + 1)) net->screen_off = 1;
    if (net->flag_host && *(volatile int*)(net->flag_host + 2)) net->stride_off = 1;   // the slope guard: stride 1 from now on
    if (!h2 || !screen_switch() || net->screen_off || !net->h1_trace.base) return IRON_OK;
    if (!net->screen_calib) IRON_HIP_TRY(hipMalloc((void**)&net->screen_calib, kScreenCalibBytes));
    if (!net->screen_calibrated) {   // once per handle (a re-pack is a new handle): stream-ordered, no synchronisation
        IRON_HIP_TRY(hipMemsetAsync(net->screen_calib, 0, 256, st));
        TraceArgs a{};
        TraceWs w{};
        launch_trace_kernel(kScreenCalib, true, net, a, w, kScreenCalibPoints / 32, st);
        net->screen_calibrated = 1;
    }
    *use = true;
    return IRON_OK;
}

// `audit`: the call collects statistics -- its resolve evaluates every listed sample, so that the counts and the guards' maxima it
// reports are those of the whole list (the deferral then only orders the work: round 2 takes every deferred entry)
static void screen_ws(TraceWs& w, const iron_net* net, char* base, const WsLayout& L, int64_t b0, int64_t nk, int n_steps, bool audit) {
    w.scr.calib = net->screen_calib;
    w.scr.stride = (stride_switch() && !net->stride_off && n_steps <= kStrideMaxSteps && w.cont_cap > 0)
                       ? (kStrideOn | g_stride_hooks.load(std::memory_order_relaxed)) : 0;
    w.scr.l_override = g_stride_l_override.load(std::memory_order_relaxed);
    w.scr.flag = net->flag_dev ? net->flag_dev + 1 : nullptr;
    w.scr.delta_override = g_screen_delta_override.load(std::memory_order_relaxed);
    w.scr.rec = (PendRec*)(base + L.s_rec);
    w.scr.ray_state = (uint8_t*)(base + L.s_flag);
    w.scr.pend_list = (int*)(base + L.s_pend) + b0;
    w.scr.ovf_list = (int*)(base + L.s_ovf) + b0;
    w.scr.ent = (ResolveEntry*)(base + L.s_ent) + b0 * kResolvePerRay;
    w.scr.res_idx = (int*)(base + L.s_idx) + b0 * kResolvePerRay;
    w.scr.defer = defer_switch() ? (kDeferOn | (audit ? kDeferAudit : 0)) : 0;
    w.scr.res_round = 0;
    int64_t cap = nk * kResolvePerRay;
    const int ov = g_screen_cap_override.load(std::memory_order_relaxed);
    if (ov > 0 && ov < cap) cap = ov;
    w.scr.cap = (int)cap;
}

// the dense sampler of one part: k_sampler, or (screen) k_sampler_screen + resolve + finalize + k_sampler on the overflow list
static void run_sampler(bool h2, bool screen, const iron_net* sdf, const TraceArgs& a, const TraceWs& w, int64_t nk, hipStream_t st) {
    const int64_t units = (nk + kSamplerSlots - 1) / kSamplerSlots;
    if (!screen) { launch_trace_kernel(kSampler, h2, sdf, a, w, units, st); return; }
    launch_trace_kernel(kSamplerScreen, true, sdf, a, w, (nk + kScreenSlots - 1) / kScreenSlots, st);
    const int64_t ge = ((int64_t)w.scr.cap + 255) / 256, gr = (nk + 255) / 256;
    if (w.scr.defer & kDeferOn) {   // the resolve in two rounds, each on its compacted index list; round 2's is almost always empty
        TraceWs wr = w;
        const int64_t gl = ((int64_t)w.scr.cap + 256 * kListBatch - 1) / (256 * kListBatch);
        for (int round = 1; round <= 2; ++round) {
            wr.scr.res_round = round;
            hipLaunchKernelGGL(k_resolve_list, dim3((unsigned)(gl < 1024 ? (gl > 0 ? gl : 1) : 1024)), dim3(256), 0, st, wr, round);
            launch_trace_kernel(kScreenResolve, true, sdf, a, wr, ((int64_t)w.scr.cap + 31) / 32, st);
        }
    } else {
        launch_trace_kernel(kScreenResolve, true, sdf, a, w, ((int64_t)w.scr.cap + 31) / 32, st);
    }
    hipLaunchKernelGGL(k_screen_fin_entries, dim3((unsigned)(ge < 1024 ? (ge > 0 ? ge : 1) : 1024)), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_screen_fin_rays, dim3((unsigned)(gr < 1024 ? (gr > 0 ? gr : 1) : 1024)), dim3(256), 0, st, a, w);
    TraceWs w2 = w;   // rays that overflowed the resolve list: k_sampler from their first sample (one slot per ray to the end)
    w2.ovf_pass = 1;
    w2.sampler_list = w.scr.ovf_list;
    w2.cont_cap = 0;
    launch_trace_kernel(kSampler, true, sdf, a, w2, units, st);
}

// phase b of the bisection: the list of the rays that have iterations left, then the kernel that runs them.  `again`: the
// counters are not fresh from the call's memset (iron_trace_phase 1: the chunk table may have changed since phase 0, and a
// repeated phase 1 starts over from what phase a left)
static int run_bisect_b(bool h2, const iron_net* sdf, const TraceArgs& a, const TraceWs& w, int64_t nk, bool again, hipStream_t st) {
    static_assert(offsetof(TraceCounters, n_root_b) == offsetof(TraceCounters, root_head_b) + sizeof(int), "zeroed together");
    if (again) IRON_HIP_TRY(hipMemsetAsync(&w.cnt->root_head_b, 0, 2 * sizeof(int), st));
    const int64_t gb = (nk + 255) / 256;
    hipLaunchKernelGGL(k_bisect_list, dim3((unsigned)(gb < 1024 ? (gb > 0 ? gb : 1) : 1024)), dim3(256), 0, st, a, w);
    launch_trace_kernel(kBisectB, h2, sdf, a, w, (nk + 31) / 32, st);
    return IRON_OK;
}

// what iron_trace_phase and iron_trace_stage check alike; `args_ok`: the entry's own pointers, which count only for a call
// that has rays.  IRON_OK with n == 0: nothing to do (L is not set).
static int check_trace_call(const iron_net_t* sdf, const iron_trace_params* p, int64_t n, bool args_ok, int64_t chunk, const void* workspace,
                            size_t workspace_bytes, WsLayout* L) {
    if (!sdf || sdf->desc.kind != IRON_NET_SDF || !p || n < 0) return IRON_ERR_BAD_ARG;
    if (n > 0x7fffffffLL - 64) return IRON_ERR_BAD_ARG;
    if (p->n_steps < 2 || p->n_steps > 4096 || p->sphere_tracing_iters < 0 || !(p->sdf_threshold > 0.0f)) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!args_ok || !workspace) return IRON_ERR_BAD_ARG;
    iron_trace_params q = *p;
    q.chunk = chunk;
    *L = ws_layout(n, &q);
    if (workspace_bytes < L->total) return IRON_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return IRON_ERR_BAD_ARG;
    return IRON_OK;
}

// the workspace's arrays as one part that holds all rays sees them (chunk table: the workspace's own)
static TraceWs bind_workspace(char* base, const WsLayout& L) {
    TraceWs w{};
    w.cnt = (TraceCounters*)(base + L.cnt);
    w.sampler_list = (int*)(base + L.sampler_list);
    w.root_list = (int*)(base + L.root_list);
    w.root_lo = (float*)(base + L.lo); w.root_hi = (float*)(base + L.hi);
    w.root_flo = (float*)(base + L.flo); w.root_fhi = (float*)(base + L.fhi);
    w.root_k = (int*)(base + L.k);
    w.chunk_iters = (int*)(base + L.chunk_iters);
    w.chunk_roots = (int*)(base + L.chunk_roots);
    w.n_chunks = (int)L.n_chunks;
    w.cont = (unsigned long long*)(base + L.cont);
    w.cont_cap = (int)L.cont_cap;
    return w;
}

}  // namespace iron

using namespace iron;

static int32_t set_switch(std::atomic<int>& set, bool prev, int32_t on) {
    set.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed);
    return prev ? 1 : 0;
}
extern "C" int32_t iron_set_sampler_screen(int32_t on) { return set_switch(g_screen_switch, screen_switch(), on); }
extern "C" int32_t iron_set_sampler_stride(int32_t on) { return set_switch(g_stride_switch, stride_switch(), on); }
extern "C" int32_t iron_set_resolve_defer(int32_t on) { return set_switch(g_defer_switch, defer_switch(), on); }

extern "C" int iron_sampler_screen_debug(int32_t what, double value) {
    if (what == 0) { g_screen_delta_override.store(value > 0.0 ? (float)value : 0.0f, std::memory_order_relaxed); return IRON_OK; }
    if (what == 1) { g_screen_cap_override.store(value >= 1.0 ? (int)value : 0, std::memory_order_relaxed); return IRON_OK; }
    if (what == 2) { set_screen_forward_tiles(value == 1.0 ? 1 : 0); return IRON_OK; }
    if (what == 3) { g_stride_l_override.store(value > 0.0 ? (float)value : 0.0f, std::memory_order_relaxed); return IRON_OK; }
    if (what == 4 || what == 5 || what == 6) {
        const int bit = what == 4 ? kStridePendingOff : what == 5 ? kStrideMuteMarch : kStrideOneSided;
        if (value != 0.0) g_stride_hooks.fetch_or(bit, std::memory_order_relaxed);
        else g_stride_hooks.fetch_and(~bit, std::memory_order_relaxed);
        return IRON_OK;
    }
    return IRON_ERR_BAD_ARG;
}

// the parts' counter blocks of a finished call, for the three entries below (synchronises the stream)
static int read_counters(const void* workspace, hipStream_t stream, TraceCounters out[kMaxTraceSplits]) {
    for (int k = 0; k < kMaxTraceSplits; ++k)
        IRON_HIP_TRY(hipMemcpyAsync(&out[k], (const char*)workspace + (size_t)k * kCntStride, sizeof(TraceCounters), hipMemcpyDeviceToHost, stream));
    IRON_HIP_TRY(hipStreamSynchronize(stream));
    return IRON_OK;
}
static void max_f32_bits(double* m, unsigned bits) {
    const float r = __builtin_bit_cast(float, bits);
    if (r > *m) *m = r;
}

extern "C" int iron_trace_screen_counts(const void* workspace, double* out, void* stream) {
    if (!workspace || !out) return IRON_ERR_BAD_ARG;
    TraceCounters c[kMaxTraceSplits];
    const int rc = read_counters(workspace, (hipStream_t)stream, c);
    if (rc != IRON_OK) return rc;
    double scr = 0, res = 0, ovf = 0, ratio = 0, pend = 0;
    for (int k = 0; k < kMaxTraceSplits; ++k) {
        scr += (double)c[k].n_screen; res += (double)c[k].n_resolved; ovf += (double)c[k].n_ovf; pend += (double)c[k].n_pend;
        max_f32_bits(&ratio, c[k].ratio_bits);
    }
    out[0] = scr; out[1] = res; out[2] = ovf; out[3] = ratio; out[4] = pend;
    return IRON_OK;
}

extern "C" int iron_trace_stride_counts(const void* workspace, double* out, void* stream) {
    if (!workspace || !out) return IRON_ERR_BAD_ARG;
    TraceCounters c[kMaxTraceSplits];
    const int rc = read_counters(workspace, (hipStream_t)stream, c);
    if (rc != IRON_OK) return rc;
    double passes = 0, strided = 0, ratio = 0, mode = 0;
    for (int k = 0; k < kMaxTraceSplits; ++k) {
        passes += (double)c[k].n_pass; strided += (double)c[k].n_pass_strided;
        max_f32_bits(&ratio, c[k].slope_bits);
        if (c[k].stride_mode) mode = 1;
    }
    out[0] = passes; out[1] = strided; out[2] = ratio; out[3] = mode;
    return IRON_OK;
}

extern "C" int iron_trace_stride_detail(const void* workspace, double* out, void* stream) {
    if (!workspace || !out) return IRON_ERR_BAD_ARG;
    TraceCounters c[kMaxTraceSplits];
    const int rc = read_counters(workspace, (hipStream_t)stream, c);
    if (rc != IRON_OK) return rc;
    for (int i = 0; i < 9; ++i) out[i] = 0.0;
    for (int k = 0; k < kMaxTraceSplits; ++k) {
        out[0] += (double)c[k].n_pass_behind; out[1] += (double)c[k].n_pass_fresh; out[2] += (double)c[k].n_restart;
        out[3] += (double)c[k].n_obs_march; out[4] += (double)c[k].n_obs_res; out[5] += (double)c[k].n_obs_pair;
        max_f32_bits(&out[6], c[k].slope_march_bits); max_f32_bits(&out[7], c[k].slope_res_bits); max_f32_bits(&out[8], c[k].slope_pair_bits);
    }
    return IRON_OK;
}

extern "C" int iron_trace_resolve_counts(const void* workspace, double* out, void* stream) {
    if (!workspace || !out) return IRON_ERR_BAD_ARG;
    TraceCounters c[kMaxTraceSplits];
    const int rc = read_counters(workspace, (hipStream_t)stream, c);
    if (rc != IRON_OK) return rc;
    for (int i = 0; i < 4; ++i) out[i] = 0.0;
    for (int k = 0; k < kMaxTraceSplits; ++k) {
        out[0] += (double)c[k].n_eval_r1; out[1] += (double)c[k].n_eval_r2; out[2] += (double)c[k].n_res1; out[3] += (double)c[k].n_res2;
    }
    return IRON_OK;
}

extern "C" size_t iron_trace_workspace_bytes(int64_t n, const iron_trace_params* p) {
    if (n < 0) return 0;
    // + room for a whole-image chunk table (multi-rank form): 64 Ki chunks
    return ws_layout(n, p).total + align256(sizeof(int) * 65536);
}

// ---- side streams of the split form -------------------------------------------------------------------------------------
namespace iron {
namespace {
struct SideStreams {
    bool ready = false;
    hipStream_t s[kMaxTraceSplits - 1];
    hipEvent_t fork, join[kMaxTraceSplits - 1];
};
std::mutex g_side_mu;           // serialises the enqueue of split calls (streams and events are shared per device)
SideStreams g_side[64];

// IRON_TRACE_SPLIT = k (2..4) runs a call as k parts; unset / 0 / 1 = one part (the measured optimum, see the head of this file)
std::atomic<int> g_trace_split{0};   // iron_set_trace_split; 0 = the environment's / default
int trace_splits(int64_t n) {
    static int from_env = -1;
    if (from_env < 0) {
        const char* e = getenv("IRON_TRACE_SPLIT");
        from_env = e ? atoi(e) : 0;
        if (from_env < 0) from_env = 0;
    }
    int k = g_trace_split.load(std::memory_order_relaxed);
    if (k <= 0) k = from_env;
    if (k < 1) k = 1;
    if (k > kMaxTraceSplits) k = kMaxTraceSplits;
    while (k > 1 && n < (int64_t)k * 256) --k;   // a part is at least two workgroup-passes of rays
    return k;
}

int side_streams(SideStreams** out) {
    int dev = 0;
    IRON_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return IRON_ERR_UNSUPPORTED;
    SideStreams& S = g_side[dev];
    if (!S.ready) {
        int least = 0, greatest = 0;
        IRON_HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        // lowest priority: a side part's workgroups take the CUs the caller-stream part leaves idle, not the other way round
        for (int i = 0; i < kMaxTraceSplits - 1; ++i) {
            IRON_HIP_TRY(hipStreamCreateWithPriority(&S.s[i], hipStreamNonBlocking, least));
            IRON_HIP_TRY(hipEventCreateWithFlags(&S.join[i], hipEventDisableTiming));
        }
        IRON_HIP_TRY(hipEventCreateWithFlags(&S.fork, hipEventDisableTiming));
        S.ready = true;
    }
    *out = &S;
    return IRON_OK;
}
}  // namespace
}  // namespace iron

extern "C" int32_t iron_set_trace_split(int32_t parts) {
    return g_trace_split.exchange(parts > 0 ? (parts > kMaxTraceSplits ? kMaxTraceSplits : parts) : 0, std::memory_order_relaxed);
}

// `mask_only` (iron_trace_occluded): phase 0 without the bisection; every bracketed ray is marked convergent instead
static int trace_phase(int32_t phase, const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps,
                       const float* ray_o, const float* ray_d, const float* near, const float* far,
                       const uint8_t* work, const int64_t* ray_index, int64_t n, int32_t* chunk_iters,
                       int64_t n_chunks, uint8_t* conv, float* points, float* sdf_out, float* dist,
                       iron_trace_stats* stats, void* workspace, size_t workspace_bytes, void* stream, bool mask_only) {
    if (phase != 0 && phase != 1) return IRON_ERR_BAD_ARG;
    const bool args_ok = lin_steps && ray_o && ray_d && near && far && work && conv && points && sdf_out && dist;
    WsLayout L;
    const int rcc = check_trace_call(sdf, p, n, args_ok, p ? p->chunk : 0, workspace, workspace_bytes, &L);
    if (rcc != IRON_OK || n == 0) return rcc;
    if (chunk_iters && (n_chunks < 1 || n_chunks > 65536)) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)workspace;
    TraceWs w0 = bind_workspace(base, L);
    if (chunk_iters) { w0.chunk_iters = chunk_iters; w0.n_chunks = (int)n_chunks; }
    if (chunk_iters && n_chunks > L.n_chunks) {
        // multi-rank: the chunk table covers the whole image, not just this rank's rays
        if (workspace_bytes < L.total + align256(sizeof(int) * (size_t)n_chunks)) return IRON_ERR_WORKSPACE;
        w0.chunk_roots = (int*)(base + L.total);
    }
    TraceArgs a0;
    a0.ray_o = ray_o; a0.ray_d = ray_d; a0.near = near; a0.far = far; a0.work = work; a0.ray_index = ray_index;
    a0.lin = lin_steps; a0.conv = conv; a0.points = points; a0.sdf = sdf_out; a0.dist = dist;
    a0.ray0 = 0; a0.n = (int)n; a0.n_steps = p->n_steps; a0.iters = p->sphere_tracing_iters; a0.thr = p->sdf_threshold;
    a0.chunk = p->chunk > 0 ? p->chunk : 0;
    if (phase == 0) { const int rce = envelope_begin(sdf); if (rce != IRON_OK) return rce; }
    const bool h2 = h2_sdf_usable(sdf);
    bool screen = false;
    if (phase == 0) { const int rcs = screen_begin(sdf, h2, st, &screen); if (rcs != IRON_OK) return rcs; }

    // the parts: rays [b_k, b_{k+1}), own counters, own stretch [b_k, ..) of every list (a part lists at most its own rays);
    // both phases of a call see the same n, hence the same split
    const int parts = trace_splits(n);
    int64_t bnd[kMaxTraceSplits + 1];
    for (int k = 0; k <= parts; ++k) bnd[k] = k == parts ? n : ((n * k / parts) + 31) / 32 * 32;
    if (parts == 2) {   // experiment: IRON_TRACE_SPLIT_FRAC = percent of the rays in the caller-stream part
        static int frac = -1;
        if (frac < 0) { const char* e = getenv("IRON_TRACE_SPLIT_FRAC"); frac = e ? atoi(e) : 50; if (frac < 5 || frac > 95) frac = 50; }
        bnd[1] = ((n * frac / 100) + 31) / 32 * 32;
    }
    SideStreams* S = nullptr;
    std::unique_lock<std::mutex> lock(g_side_mu, std::defer_lock);
    if (parts > 1) {
        lock.lock();
        const int rc = side_streams(&S);
        if (rc != IRON_OK) return rc;
    }
    if (phase == 0) {
        IRON_HIP_TRY(hipMemsetAsync(base + L.cnt, 0, kCntStride * kMaxTraceSplits, st));
        if (chunk_iters) IRON_HIP_TRY(hipMemsetAsync(chunk_iters, 0, sizeof(int) * (size_t)n_chunks, st));
        else IRON_HIP_TRY(hipMemsetAsync(base + L.chunk_iters, 0, align256(sizeof(int) * (size_t)L.n_chunks), st));
        IRON_HIP_TRY(hipMemsetAsync(w0.chunk_roots, 0, sizeof(int) * (size_t)w0.n_chunks, st));
        if (L.cont_cap > 0) IRON_HIP_TRY(hipMemsetAsync(base + L.cont, 0, sizeof(unsigned long long) * (size_t)L.cont_cap, st));
        if (screen) IRON_HIP_TRY(hipMemsetAsync(base + L.s_flag, 0, (size_t)n, st));
    }
    if (parts > 1) IRON_HIP_TRY(hipEventRecord(S->fork, st));
    // side parts first: their launches are queued before the caller-stream part occupies the chip
    for (int k = parts - 1; k >= 0; --k) {
        hipStream_t sk = k == 0 ? st : S->s[k - 1];
        if (k > 0) IRON_HIP_TRY(hipStreamWaitEvent(sk, S->fork, 0));
        TraceWs w = w0;
        TraceArgs a = a0;
        const int64_t b0 = bnd[k], nk = bnd[k + 1] - bnd[k];
        if (nk <= 0) continue;
        w.cnt = (TraceCounters*)(base + L.cnt + (size_t)k * kCntStride);
        w.sampler_list += b0; w.root_list += b0; w.root_lo += b0; w.root_hi += b0; w.root_flo += b0; w.root_fhi += b0; w.root_k += b0;
        a.ray0 = (int)b0; a.n = (int)nk;
        if (L.cont_cap > 0) { const int64_t per_ray = L.cont_cap / n; w.cont += b0 * per_ray; w.cont_cap = (int)(nk * per_ray); }
        if (screen) screen_ws(w, sdf, base, L, b0, nk, p->n_steps, stats != nullptr);
        const int64_t tiles = (nk + 31) / 32;
        if (phase == 0) {
            {
                ProfScope ps(IRON_PROF_SPHERE, sk);
                launch_trace_kernel(kSphere, h2, sdf, a, w, tiles, sk);
            }
            {
                ProfScope ps(IRON_PROF_SAMPLER, sk);
                run_sampler(h2, screen, sdf, a, w, nk, sk);
            }
            if (mask_only) {
                const unsigned gb = (unsigned)((nk + 255) / 256 < 1024 ? (nk + 255) / 256 : 1024);
                hipLaunchKernelGGL(k_stage_mark_list, dim3(gb), dim3(256), 0, sk, w.root_list, &w.cnt->n_root, a.conv);
            } else {
                ProfScope ps(IRON_PROF_BISECT_A, sk);
                launch_trace_kernel(kBisectA, h2, sdf, a, w, tiles, sk);
            }
        } else {
            ProfScope ps(IRON_PROF_BISECT_B, sk);
            const int rcb = run_bisect_b(h2, sdf, a, w, nk, true, sk);
            if (rcb != IRON_OK) return rcb;
        }
        if (k > 0) IRON_HIP_TRY(hipEventRecord(S->join[k - 1], sk));
    }
    for (int k = 1; k < parts; ++k)   // join: everything behind this call on the caller's stream sees all parts finished
        if (bnd[k + 1] > bnd[k]) IRON_HIP_TRY(hipStreamWaitEvent(st, S->join[k - 1], 0));
    const bool last = phase == 1 || mask_only;
    if (last && h2) envelope_scan(sdf, sdf_out, n, nullptr, 1, st);   // envelope guard (envelope.hip): every ray's last sdf value
    if (last && stats) hipLaunchKernelGGL(k_trace_stats, dim3(1), dim3(64), 0, st, w0, parts, p->n_steps, stats);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_trace_phase(int32_t phase, const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps,
                                const float* ray_o, const float* ray_d, const float* near, const float* far,
                                const uint8_t* work, const int64_t* ray_index, int64_t n, int32_t* chunk_iters,
                                int64_t n_chunks, uint8_t* conv, float* points, float* sdf_out, float* dist,
                                iron_trace_stats* stats, void* workspace, size_t workspace_bytes, void* stream) {
    return trace_phase(phase, sdf, p, lin_steps, ray_o, ray_d, near, far, work, ray_index, n, chunk_iters, n_chunks, conv, points, sdf_out,
                       dist, stats, workspace, workspace_bytes, stream, false);
}

// the per-ray scratch behind the tracer's own workspace: the points, sdf and distance the sphere and sampler kernels keep per ray
static size_t occluded_scratch(int64_t n) { return align256(sizeof(float) * 3 * (size_t)n) + 2 * align256(sizeof(float) * (size_t)n); }

extern "C" size_t iron_trace_occluded_workspace_bytes(int64_t n, const iron_trace_params* p) {
    if (n <= 0) return 0;
    return align256(iron_trace_workspace_bytes(n, p)) + occluded_scratch(n);
}

extern "C" int iron_trace_occluded(const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps, const float* ray_o,
                                   const float* ray_d, const float* near, const float* far, const uint8_t* work, int64_t n,
                                   uint8_t* occluded, iron_trace_stats* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || !p) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!workspace) return IRON_ERR_BAD_ARG;
    const size_t head = align256(iron_trace_workspace_bytes(n, p));
    if (workspace_bytes < head + occluded_scratch(n)) return IRON_ERR_WORKSPACE;
    char* s = (char*)workspace + head;
    float* points = (float*)s;
    float* sdf_out = (float*)(s + align256(sizeof(float) * 3 * (size_t)n));
    float* dist = (float*)((char*)sdf_out + align256(sizeof(float) * (size_t)n));
    return trace_phase(0, sdf, p, lin_steps, ray_o, ray_d, near, far, work, nullptr, n, nullptr, 0, occluded, points, sdf_out, dist, stats,
                       workspace, head, stream, true);
}

extern "C" int iron_trace_stage(int32_t stage, const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps,
                                const float* ray_o, const float* ray_d, const float* in0, const float* in1, const float* in2,
                                const float* in3, const uint8_t* work, int64_t n, uint8_t* mask_out, uint8_t* unfinished_out,
                                float* points, float* sdf_out, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    if (stage < 0 || stage > 2) return IRON_ERR_BAD_ARG;
    const bool args_ok = lin_steps && ray_o && ray_d && in0 && in1 && mask_out && points && sdf_out && dist &&
                         !(stage == 0 && (!work || !unfinished_out)) && !(stage == 2 && (!in2 || !in3));
    WsLayout L;
    const int rcc = check_trace_call(sdf, p, n, args_ok, 0, workspace, workspace_bytes, &L);   // chunk 0: one reference call = one chunk
    if (rcc != IRON_OK || n == 0) return rcc;
    { const int rce = envelope_begin(sdf); if (rce != IRON_OK) return rce; }
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)workspace;
    TraceWs w = bind_workspace(base, L);
    TraceArgs a;
    a.ray_o = ray_o; a.ray_d = ray_d; a.work = work; a.ray_index = nullptr; a.lin = lin_steps;
    a.conv = mask_out; a.points = points; a.sdf = sdf_out; a.dist = dist;
    a.ray0 = 0; a.n = (int)n; a.n_steps = p->n_steps; a.iters = p->sphere_tracing_iters; a.thr = p->sdf_threshold; a.chunk = 0;
    a.near = in0; a.far = in1;
    const bool h2 = h2_sdf_usable(sdf);
    bool screen = false;
    if (stage == 1) {
        const int rcs = screen_begin(sdf, h2, st, &screen);
        if (rcs != IRON_OK) return rcs;
        if (screen) { IRON_HIP_TRY(hipMemsetAsync(base + L.s_flag, 0, (size_t)n, st)); screen_ws(w, sdf, base, L, 0, n, p->n_steps, false); }
    }
    IRON_HIP_TRY(hipMemsetAsync(base + L.cnt, 0, kCntStride * kMaxTraceSplits, st));
    IRON_HIP_TRY(hipMemsetAsync(base + L.chunk_iters, 0, align256(sizeof(int)), st));
    IRON_HIP_TRY(hipMemsetAsync(base + L.chunk_roots, 0, align256(sizeof(int)), st));
    if (L.cont_cap > 0) IRON_HIP_TRY(hipMemsetAsync(base + L.cont, 0, sizeof(unsigned long long) * (size_t)L.cont_cap, st));
    const int64_t tiles = (n + 31) / 32;
    const unsigned gb = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    if (stage == 0) {            // sphere_tracing (raytracer.py:105-140): in0 = min_dis, in1 = max_dis
        IRON_HIP_TRY(hipMemsetAsync(unfinished_out, 0, (size_t)n, st));
        launch_trace_kernel(kSphere, h2, sdf, a, w, tiles, st);
        hipLaunchKernelGGL(k_stage_mark_list, dim3(gb), dim3(256), 0, st, w.sampler_list, &w.cnt->smp.n_list, unfinished_out);
    } else if (stage == 1) {     // ray_sampler (:142-197): in0 = min_dis, in1 = max_dis, every ray sampled on its own interval
        hipLaunchKernelGGL(k_stage_sampler_init, dim3(gb), dim3(256), 0, st, a, w, in0);
        run_sampler(h2, screen, sdf, a, w, n, st);
        launch_trace_kernel(kBisectA, h2, sdf, a, w, tiles, st);
        { const int rcb = run_bisect_b(h2, sdf, a, w, n, false, st); if (rcb != IRON_OK) return rcb; }
    } else {                     // rootfind (:199-220): in0 = f_low, in1 = f_high, in2 = d_low, in3 = d_high
        hipLaunchKernelGGL(k_stage_root_init, dim3(gb), dim3(256), 0, st, w, (int)n, in0, in1, in2, in3);
        launch_trace_kernel(kBisectA, h2, sdf, a, w, tiles, st);
        { const int rcb = run_bisect_b(h2, sdf, a, w, n, false, st); if (rcb != IRON_OK) return rcb; }
    }
    if (h2) envelope_scan(sdf, sdf_out, n, nullptr, 1, st);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

extern "C" int iron_trace(const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps, const float* ray_o,
                          const float* ray_d, const float* near, const float* far, const uint8_t* work, int64_t n,
                          uint8_t* conv, float* points, float* sdf_out, float* dist, iron_trace_stats* stats,
                          void* workspace, size_t workspace_bytes, void* stream) {
    int rc = iron_trace_phase(0, sdf, p, lin_steps, ray_o, ray_d, near, far, work, nullptr, n, nullptr, 0, conv, points,
                              sdf_out, dist, stats, workspace, workspace_bytes, stream);
    if (rc != IRON_OK) return rc;
    return iron_trace_phase(1, sdf, p, lin_steps, ray_o, ray_d, near, far, work, nullptr, n, nullptr, 0, conv, points,
                            sdf_out, dist, stats, workspace, workspace_bytes, stream);
}
