// Device-resident sphere tracer of the hash-grid SDF field (include/iron_hip.h, iron_hashgrid_trace_* block):
// RayTracer.forward (models/raytracer.py:45-220) with the field evaluated INSIDE the tracing kernels, a fixed launch sequence with
// every count left on the device.  No entry copies to the host or waits for the stream.  Per ray the arithmetic is that of the
// callable tracer (trace_any.hip) on TCNNSDF.as_callable: the formulas of trace_ray.h around field_value (hashgrid_field_common.h),
// which is k_hg_field's value path; rows of that evaluation are independent, so the grouping of points into waves changes no bit.
//
//   k_hgt_sphere     one wave64 per workgroup owns 64 rays: evaluate -> flag -> step, until a ballot shows no unfinished ray or
//                    iters + 1 evaluations were made.  Writes p, s, t, conv, the unfinished flag.
//   pair_scan + k_hgt_list       the unfinished rays, ascending, the count in a workspace word.
//   k_hgt_sampler    grid bounded by the machine, grid-stride over the list (its length read from the device word): a wave takes a
//                    ray's n_steps samples in passes of 64, the first negative index from a ballot, the last value of a pass
//                    carried so that a bracket may straddle two passes; passes behind the first negative sample are not made.
//   pair_scan + k_hgt_brackets   the rooted rays, ascending.
//   k_hgt_bisect_a   one lane per bracket: its own iterations (at most 256), the count posted by atomicMax into the chunk table.
//   k_hgt_bisect_b   every bracket goes on from its own count to its chunk's T, then the final mid point is evaluated and the
//                    ray's slot written.  A bracket's evaluations are mid_1 .. mid_{T+1} in that order whichever kernel makes them.
//
// A lane without a live point evaluates the map's image of the origin and its value is dropped; the encoding clamps and wraps
// every index, so no evaluation reads outside the table.  Integer atomics only (counts, a max); no float atomics, no scratch lists.
#include "hashgrid_field_common.h"
#include "pair_scan.h"
#include "trace_ray.h"

#include <limits.h>

namespace iron {
namespace {

constexpr int kBlk = 256;
constexpr int kBisectCap = 256;   // fp32 brackets halve to nothing long before; a NaN inside an open bracket would never end
enum { ST_ISSUED = 0, ST_LIVE = 1, ST_SAMPLER = 2, ST_BISECT = 3, ST_ITERS = 4, ST_INCOMPLETE = 5 };
enum { W_UNFINISHED = 0, W_BRACKETS = 1 };

struct RayArgs {
    const float *o, *d;
    int64_t n;
};

struct HgtLayout {
    size_t unf, list, sdf, dist, lo, hi, u_dlo, u_dhi, u_flo, u_fhi, b_ray, b_dlo, b_dhi, b_flo, b_fhi, b_mid, b_own, iters, words, scan;
    int64_t n_chunks;
    size_t total;
};

HgtLayout hgt_layout(int64_t n, int64_t chunk) {
    const size_t c1 = (size_t)(n > 0 ? n : 1);
    Carver c;
    HgtLayout L{};
    L.unf = c.take(c1);
    size_t* w32[] = {&L.list, &L.sdf, &L.dist, &L.lo, &L.hi, &L.u_dlo, &L.u_dhi, &L.u_flo, &L.u_fhi, &L.b_ray, &L.b_dlo, &L.b_dhi, &L.b_flo, &L.b_fhi,
                     &L.b_mid, &L.b_own};
    for (size_t* f : w32) *f = c.take(4 * c1);
    L.n_chunks = chunk > 0 ? (int64_t)((c1 + (size_t)chunk - 1) / (size_t)chunk) : 1;
    L.iters = c.take(4 * (size_t)L.n_chunks);
    L.words = c.take(2 * sizeof(int64_t));
    L.scan = c.off;
    scan_levels((int64_t)c1, c);
    L.total = c.off;
    return L;
}

struct Ws {
    HgtLayout L;
    void* base;
    ScanLevels S;
    uint8_t* unf() const { return ws_ptr<uint8_t>(base, L.unf); }
    int32_t* i32(size_t off) const { return ws_ptr<int32_t>(base, off); }
    float* f(size_t off) const { return ws_ptr<float>(base, off); }
    int64_t* words() const { return ws_ptr<int64_t>(base, L.words); }
    Pair64* flags() const { return S.level(base, 0); }
};

Ws open_ws(int64_t n, int64_t chunk, void* workspace) {
    Ws w;
    w.L = hgt_layout(n, chunk);
    w.base = workspace;
    Carver c;
    c.off = w.L.scan;
    w.S = scan_levels(n > 0 ? n : 1, c);
    return w;
}

struct Brackets {
    int32_t* ray;
    float *dlo, *dhi, *flo, *fhi, *mid;
    int32_t* own;
};
Brackets brackets_of(const Ws& w) {
    return Brackets{w.i32(w.L.b_ray), w.f(w.L.b_dlo), w.f(w.L.b_dhi), w.f(w.L.b_flo), w.f(w.L.b_fhi), w.f(w.L.b_mid), w.i32(w.L.b_own)};
}

__device__ __forceinline__ void stat_add(int64_t* stats, int word, int64_t v) {
    if (stats && v) atomicAdd((unsigned long long*)(stats + word), (unsigned long long)v);
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}

// the field at the 64 points of the wave, each lane its own; `live` lanes count as evaluations that belonged to a ray.  The barrier
// behind the value keeps the next evaluation's encode from overwriting rows the last layer is still reading.
template <int ACT, int NT>
__device__ __forceinline__ float eval_at(const FieldBinding& F, float* lds, const float* p, bool live, int lane, int64_t& issued, int64_t& lived) {
    float xs[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xs[c] = fmaf(p[c], F.map.a[c], F.map.b[c]);
    const float v = field_value<ACT, NT>(F.L, F.pl, lds, xs, F.table, F.packed, lane);
    __syncthreads();
    issued += 64;
    lived += __popcll(__ballot(live));
    return v;
}

// ---- sphere tracing (raytracer.py:105-137) ----
struct SphereArgs {
    const float *near, *far;
    const uint8_t* work;
    float thr;
    int iters;
    uint8_t* conv;
    float *points, *sdf, *dist;   // points may be null (occlusion query)
    uint8_t *unf, *unf_out;       // unf_out may be null
    Pair64* flags;
    int64_t* stats;
};

template <int ACT, int NT>
__global__ __launch_bounds__(64) void k_hgt_sphere(FieldBinding F, RayArgs R, SphereArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool have = i < R.n;
    float t = 0.0f, s = 0.0f, fr = 0.0f, p[3] = {0.0f, 0.0f, 0.0f}, dd[3] = {0.0f, 0.0f, 0.0f};
    bool work = false;
    if (have) {
        t = A.near[i];
        fr = A.far[i];
        work = A.work[i] != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) dd[c] = R.d[i * 3 + c];
        ray::ray_point(R.o, R.d, i, t, p);
    }
    bool u = work, need = have;   // the first evaluation is made on every ray, the later ones on the unfinished
    int64_t issued = 0, lived = 0;
    for (int e = 0; e <= A.iters; ++e) {
        const float v = eval_at<ACT, NT>(F, lds, p, need, lane, issued, lived);
        if (need) {
            s = v;
            u = ray::still_unfinished(u, s, A.thr, t, fr);
        }
        need = u;
        if (__ballot(u) == 0) break;
        if (u && e < A.iters) {
            t = t + s;
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = ray::advance(p[c], dd[c], s);
        }
    }
    if (have) {
        if (A.points) {
#pragma unroll
            for (int c = 0; c < 3; ++c) A.points[i * 3 + c] = p[c];
        }
        A.sdf[i] = s;
        A.dist[i] = t;
        A.conv[i] = ray::sphere_converged(work, u, s, A.thr, t, fr) ? 1 : 0;
        A.unf[i] = u ? 1 : 0;
        if (A.unf_out) A.unf_out[i] = u ? 1 : 0;
        A.flags[i] = Pair64{u ? 1 : 0, 0};
    }
    if (lane == 0) {
        stat_add(A.stats, ST_ISSUED, issued);
        stat_add(A.stats, ST_LIVE, lived);
    }
}

// the flagged entries, ascending; the total in words[word] and added to a stats word
__global__ __launch_bounds__(kBlk) void k_hgt_list(const uint8_t* __restrict__ unf, const Pair64* __restrict__ prefix, int64_t n,
                                                   int32_t* __restrict__ list, int64_t* __restrict__ words, int64_t* __restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const bool u = unf[i] != 0;
    const int64_t pos = prefix[i].a;
    if (u) list[pos] = (int32_t)i;
    if (i == n - 1) {
        words[W_UNFINISHED] = pos + (u ? 1 : 0);
        stat_add(stats, ST_SAMPLER, pos + (u ? 1 : 0));
    }
}

// ray_sampler called on its own: every ray, on the interval given
__global__ __launch_bounds__(kBlk) void k_hgt_all(int64_t n, int32_t* __restrict__ list, int64_t* __restrict__ words, int64_t* __restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    list[i] = (int32_t)i;
    if (i == n - 1) {
        words[W_UNFINISHED] = n;
        stat_add(stats, ST_SAMPLER, n);
    }
}

// ---- the dense sampler (raytracer.py:56-63, 142-197) ----
struct SamplerArgs {
    const int32_t* list;
    const int64_t* words;
    const float *near, *far, *sdf_in, *dist_in;   // the interval from the sphere tracer's state ...
    const float *lo, *hi;                         // ... or given per ray (both non-null)
    const float* lin;
    int n_steps;
    float *u_dlo, *u_dhi, *u_flo, *u_fhi;
    Pair64* flags;
    uint8_t* conv;
    float *points, *sdf, *dist;   // null for the occlusion query: the mask alone
    int64_t* stats;
};

template <int ACT, int NT>
__global__ __launch_bounds__(64) void k_hgt_sampler(FieldBinding F, RayArgs R, SamplerArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t m = A.words[W_UNFINISHED];
    if ((int64_t)blockIdx.x >= m) return;   // nothing of the field or LDS is touched
    int64_t issued = 0, lived = 0;
    for (int64_t k = blockIdx.x; k < m; k += gridDim.x) {
        const int64_t i = A.list[k];
        float lo, hi;
        if (A.lo) {
            lo = A.lo[i];
            hi = A.hi[i];
        } else {
            ray::sampler_interval(A.sdf_in[i], A.dist_in[i], A.near[i], A.far[i], &lo, &hi);
        }
        int first = -1;
        float flo = 0.0f, fhi = 0.0f, carry = 0.0f;
        for (int j0 = 0; j0 < A.n_steps; j0 += 64) {
            const int j = j0 + lane;
            const bool live = j < A.n_steps;
            float p[3] = {0.0f, 0.0f, 0.0f};
            if (live) ray::ray_point(R.o, R.d, i, ray::sample_z(lo, hi, A.lin[j]), p);
            const float v = eval_at<ACT, NT>(F, lds, p, live, lane, issued, lived);
            const unsigned long long neg = __ballot(live && v < 0.0f);   // a NaN or zero sample is neither sign
            const int q = neg ? __ffsll(neg) - 1 : 0;
            const float at = __shfl(v, q, 64), before = __shfl(v, q > 0 ? q - 1 : 0, 64), last = __shfl(v, 63, 64);
            if (neg) {
                first = j0 + q;
                fhi = at;
                flo = q > 0 ? before : carry;
                break;
            }
            carry = last;
        }
        if (lane == 0) {
            const bool root = first >= 1;
            A.flags[k] = Pair64{root ? 1 : 0, 0};
            if (root) {
                A.u_dlo[k] = ray::sample_z(lo, hi, A.lin[first - 1]);
                A.u_dhi[k] = ray::sample_z(lo, hi, A.lin[first]);
                A.u_flo[k] = flo;
                A.u_fhi[k] = fhi;
            }
            if (!A.points) {
                A.conv[i] = root ? 1 : 0;   // final here: every bracketed ray ends convergent (raytracer.py:192-197)
            } else if (!root) {
                A.conv[i] = 0;
                A.points[i * 3 + 0] = 0.0f; A.points[i * 3 + 1] = 0.0f; A.points[i * 3 + 2] = 0.0f;
                A.sdf[i] = 0.0f;
                A.dist[i] = 0.0f;
            }
        }
    }
    if (lane == 0) {
        stat_add(A.stats, ST_ISSUED, issued);
        stat_add(A.stats, ST_LIVE, lived);
    }
}

// the rooted entries of the list become the bracket slots, ascending
__global__ __launch_bounds__(kBlk) void k_hgt_brackets(const int32_t* __restrict__ list, int64_t* __restrict__ words, const Pair64* __restrict__ prefix,
                                                       const Pair64* __restrict__ total, int64_t n, const float* __restrict__ u_dlo,
                                                       const float* __restrict__ u_dhi, const float* __restrict__ u_flo,
                                                       const float* __restrict__ u_fhi, Brackets B, int64_t* __restrict__ stats) {
    const int64_t k = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    const int64_t m = words[W_UNFINISHED];
    if (k == 0) {
        words[W_BRACKETS] = total->a;
        stat_add(stats, ST_BISECT, total->a);
    }
    if (k >= m || k >= n) return;
    const int64_t b = prefix[k].a;
    const bool root = (k + 1 < n ? prefix[k + 1].a : total->a) > b;
    if (!root) return;
    B.ray[b] = list[k];
    B.dlo[b] = u_dlo[k]; B.dhi[b] = u_dhi[k]; B.flo[b] = u_flo[k]; B.fhi[b] = u_fhi[k];
}

// rootfind called on its own: bracket b is ray b, as given
__global__ __launch_bounds__(kBlk) void k_hgt_brackets_given(const float* __restrict__ f_low, const float* __restrict__ f_high,
                                                             const float* __restrict__ d_low, const float* __restrict__ d_high, int64_t n, Brackets B,
                                                             int64_t* __restrict__ words, int64_t* __restrict__ stats) {
    const int64_t b = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (b >= n) return;
    B.ray[b] = (int32_t)b;
    B.dlo[b] = d_low[b]; B.dhi[b] = d_high[b]; B.flo[b] = f_low[b]; B.fhi[b] = f_high[b];
    if (b == n - 1) {
        words[W_BRACKETS] = n;
        stat_add(stats, ST_BISECT, n);
    }
}

// ---- bisection (raytracer.py:199-220) ----
struct BisectArgs {
    const int64_t* words;
    Brackets B;
    int32_t* chunk_iters;
    int64_t chunk;     // rays per chunk; <= 0: one chunk
    float two_thr;
    uint8_t* conv;     // may be null (rootfind on its own)
    float *points, *sdf, *dist;
    int64_t* stats;
};

__device__ __forceinline__ int64_t chunk_of(int64_t ray, int64_t chunk) { return chunk > 0 ? ray / chunk : 0; }

// a bracket's own iterations: while it is open and wider than 2 thr
template <int ACT, int NT>
__global__ __launch_bounds__(64) void k_hgt_bisect_a(FieldBinding F, RayArgs R, BisectArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t nb = A.words[W_BRACKETS];
    const int64_t b = (int64_t)blockIdx.x * 64 + lane;
    if ((int64_t)blockIdx.x * 64 >= nb) return;
    const bool have = b < nb;
    int64_t i = 0;
    float dlo = 0.0f, dhi = 0.0f, flo = 0.0f, fhi = 0.0f;
    if (have) {
        i = A.B.ray[b];
        dlo = A.B.dlo[b]; dhi = A.B.dhi[b]; flo = A.B.flo[b]; fhi = A.B.fhi[b];
    }
    bool w = have && ray::bracket_open(flo, fhi);
    float mid = ray::bracket_mid(dlo, dhi);
    int own = 0;
    int64_t issued = 0, lived = 0;
    for (int it = 0; it < kBisectCap && __ballot(w) != 0; ++it) {
        float p[3] = {0.0f, 0.0f, 0.0f};
        if (w) ray::ray_point(R.o, R.d, i, mid, p);
        const float fm = eval_at<ACT, NT>(F, lds, p, w, lane, issued, lived);
        if (w) {
            ray::bracket_update(fm, mid, &dlo, &dhi, &flo, &fhi);
            mid = ray::bracket_mid(dlo, dhi);
            w = ray::bracket_wide(dlo, dhi, A.two_thr);
            ++own;
        }
    }
    if (w && A.stats) A.stats[ST_INCOMPLETE] = 1;   // still open after kBisectCap iterations
    if (have) {
        A.B.dlo[b] = dlo; A.B.dhi[b] = dhi; A.B.mid[b] = mid; A.B.own[b] = own;
    }
    // the chunk's count: one atomic per wave where the wave lies inside one chunk, else one per bracket
    const int64_t ch = chunk_of(i, A.chunk);
    const int64_t ch0 = __shfl((int)ch, 0, 64);   // chunk ids fit an int: n < 2^31
    const bool same = __ballot(have && ch != ch0) == 0;
    if (same) {
        const int top = wave_max(have ? own : 0);
        if (lane == 0 && top > 0) atomicMax(A.chunk_iters + ch0, top);
    } else if (have && own > 0) {
        atomicMax(A.chunk_iters + ch, own);
    }
    if (lane == 0) {
        stat_add(A.stats, ST_ISSUED, issued);
        stat_add(A.stats, ST_LIVE, lived);
    }
}

// from a bracket's own count to its chunk's: every slot moves, open or not (raytracer.py:205-217); then the final mid point
template <int ACT, int NT>
__global__ __launch_bounds__(64) void k_hgt_bisect_b(FieldBinding F, RayArgs R, BisectArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t nb = A.words[W_BRACKETS];
    const int64_t b = (int64_t)blockIdx.x * 64 + lane;
    if ((int64_t)blockIdx.x * 64 >= nb) return;
    const bool have = b < nb;
    int64_t i = 0;
    float dlo = 0.0f, dhi = 0.0f, flo = 0.0f, fhi = 0.0f, mid = 0.0f;
    int rem = 0;
    if (have) {
        i = A.B.ray[b];
        dlo = A.B.dlo[b]; dhi = A.B.dhi[b]; mid = A.B.mid[b];
        const int64_t ch = chunk_of(i, A.chunk);
        const int T = A.chunk_iters[ch];
        rem = T - A.B.own[b];
        if (b == 0 || chunk_of(A.B.ray[b - 1], A.chunk) != ch) stat_add(A.stats, ST_ITERS, T);   // once per chunk: the slots ascend
    }
    const int steps = wave_max(rem);
    int64_t issued = 0, lived = 0;
    float fm = 0.0f;
    for (int it = 0; it <= steps; ++it) {
        const bool last = it == steps;
        const bool act = have && (last || it < rem);
        float p[3] = {0.0f, 0.0f, 0.0f};
        if (act) ray::ray_point(R.o, R.d, i, mid, p);
        fm = eval_at<ACT, NT>(F, lds, p, act, lane, issued, lived);
        if (act && !last) {
            ray::bracket_update(fm, mid, &dlo, &dhi, &flo, &fhi);
            mid = ray::bracket_mid(dlo, dhi);
        }
    }
    if (have) {
        ray::ray_point(R.o, R.d, i, mid, A.points + i * 3);
        A.sdf[i] = fm;
        A.dist[i] = mid;
        if (A.conv) A.conv[i] = 1;
    }
    if (lane == 0) {
        stat_add(A.stats, ST_ISSUED, issued);
        stat_add(A.stats, ST_LIVE, lived);
    }
}

// one call's validated arguments
struct Call {
    FieldBinding F;
    size_t lds_bytes;
    iron_trace_params prm;
    int64_t n;
    Ws ws;
    hipStream_t st;
};

#define HGT_TRY(expr)                  \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != IRON_OK) return _rc; \
    } while (0)

// The house order of the checks: null descriptor / parameters -> BAD_ARG, a refused shape or n_steps -> RANGE, n -> BAD_ARG.
// *go is set when there is work to enqueue (n > 0); the pointer checks of the entry follow.
int open_call(Call& c, const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3, const float* map_b3, const float* table,
              const void* packed, int64_t n, void* workspace, size_t workspace_bytes, void* stream, bool* go) {
    *go = false;
    if (!desc || !p) return IRON_ERR_BAD_ARG;
    HGT_TRY(field_open(desc, &c.F));
    if (p->n_steps < 2 || p->n_steps > 4096) return IRON_ERR_RANGE;
    if (p->sphere_tracing_iters < 0 || !(p->sdf_threshold >= 0.0f)) return IRON_ERR_BAD_ARG;
    if (n < 0 || n > (int64_t)INT_MAX - 1) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    HGT_TRY(field_bind(&c.F, map_a3, map_b3, table, packed));
    if (!workspace) return IRON_ERR_BAD_ARG;
    c.prm = *p;
    c.n = n;
    c.ws = open_ws(n, p->chunk, workspace);
    if (workspace_bytes < c.ws.L.total) return IRON_ERR_BAD_ARG;
    c.lds_bytes = lds_layout(c.F.pl, false, 64, nullptr);
    c.st = (hipStream_t)stream;
    *go = true;
    return IRON_OK;
}

// K<ACT, NT>, one wave64 per workgroup, `grid` of them on the call's stream with the LDS of the value path
template <class A>
int launch_wave(void (*k)(FieldBinding, RayArgs, A), unsigned grid, const Call& c, const RayArgs& R, const A& a) {
    hipLaunchKernelGGL(k, dim3(grid), dim3(64), c.lds_bytes, c.st, c.F, R, a);
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

int begin(const Call& c) {
    IRON_HIP_TRY(hipMemsetAsync(c.ws.words(), 0, 2 * sizeof(int64_t), c.st));
    IRON_HIP_TRY(hipMemsetAsync(c.ws.i32(c.ws.L.iters), 0, 4 * (size_t)c.ws.L.n_chunks, c.st));
    return IRON_OK;
}

int run_sphere(const Call& c, const RayArgs& R, const float* near, const float* far, const uint8_t* work, uint8_t* conv, float* points, float* sdf,
               float* dist, uint8_t* unf_out, int64_t* stats) {
    const Ws& w = c.ws;
    SphereArgs A{near, far, work, c.prm.sdf_threshold, c.prm.sphere_tracing_iters, conv, points, sdf, dist, w.unf(), unf_out, w.flags(), stats};
    {
        ProfScope ps(IRON_PROF_SPHERE, c.st);
        HGT_TRY(with_value_path(c.F.pl, [&](auto act, auto nt) { return launch_wave(k_hgt_sphere<act(), nt()>, blocks_for(c.n, 64), c, R, A); }));
    }
    const int rc = pair_scan(w.S, w.base, c.st);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_hgt_list, blocks_for(c.n, kBlk), kBlk, c.st, (const uint8_t*)w.unf(), (const Pair64*)w.flags(), c.n, w.i32(w.L.list), w.words(), stats);
    return IRON_OK;
}

// the sampler on the listed rays and the compaction of its brackets; with points == nullptr the mask alone (no bracket is listed)
int run_sampler(const Call& c, const RayArgs& R, const float* near, const float* far, const float* sdf_in, const float* dist_in, const float* lo,
                const float* hi, const float* lin, uint8_t* conv, float* points, float* sdf, float* dist, int64_t* stats) {
    const Ws& w = c.ws;
    IRON_HIP_TRY(hipMemsetAsync(w.flags(), 0, sizeof(Pair64) * (size_t)c.n, c.st));   // entries past the list's end count as rootless
    SamplerArgs A{w.i32(w.L.list), w.words(), near, far, sdf_in, dist_in, lo, hi, lin, c.prm.n_steps, w.f(w.L.u_dlo), w.f(w.L.u_dhi), w.f(w.L.u_flo),
                  w.f(w.L.u_fhi), w.flags(), conv, points, sdf, dist, stats};
    const int64_t cap = (int64_t)cu_total() * 8;
    {
        ProfScope ps(IRON_PROF_SAMPLER, c.st);
        HGT_TRY(with_value_path(c.F.pl, [&](auto act, auto nt) { return launch_wave(k_hgt_sampler<act(), nt()>, (unsigned)(c.n < cap ? c.n : cap), c, R, A); }));
    }
    const int rc = pair_scan(w.S, w.base, c.st);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_hgt_brackets, blocks_for(c.n, kBlk), kBlk, c.st, (const int32_t*)w.i32(w.L.list), w.words(), (const Pair64*)w.flags(),
                (const Pair64*)w.S.level(w.base, w.S.levels), c.n, (const float*)w.f(w.L.u_dlo), (const float*)w.f(w.L.u_dhi),
                (const float*)w.f(w.L.u_flo), (const float*)w.f(w.L.u_fhi), brackets_of(w), stats);
    return IRON_OK;
}

int run_bisect(const Call& c, const RayArgs& R, int64_t chunk, uint8_t* conv, float* points, float* sdf, float* dist, int64_t* stats) {
    const Ws& w = c.ws;
    BisectArgs A{w.words(), brackets_of(w), w.i32(w.L.iters), chunk, 2.0f * c.prm.sdf_threshold, conv, points, sdf, dist, stats};
    {
        ProfScope ps(IRON_PROF_BISECT_A, c.st);
        HGT_TRY(with_value_path(c.F.pl, [&](auto act, auto nt) { return launch_wave(k_hgt_bisect_a<act(), nt()>, blocks_for(c.n, 64), c, R, A); }));
    }
    ProfScope ps(IRON_PROF_BISECT_B, c.st);
    HGT_TRY(with_value_path(c.F.pl, [&](auto act, auto nt) { return launch_wave(k_hgt_bisect_b<act(), nt()>, blocks_for(c.n, 64), c, R, A); }));
    return IRON_OK;
}

}  // namespace
}  // namespace iron

using namespace iron;

extern "C" {

size_t iron_hashgrid_trace_workspace_bytes(int64_t n, const iron_trace_params* p) {
    if (n < 0 || n > (int64_t)INT_MAX - 1) return 0;
    return hgt_layout(n, p ? p->chunk : 0).total;   // no parameters: one chunk
}

int iron_hashgrid_trace(const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3, const float* map_b3, const float* table,
                        const void* packed, const float* lin_steps, const float* ray_o, const float* ray_d, const float* near, const float* far,
                        const uint8_t* work, int64_t n, uint8_t* conv, float* points, float* sdf_out, float* dist, int64_t* stats, void* workspace,
                        size_t workspace_bytes, void* stream) {
    Call c;
    bool go;
    HGT_TRY(open_call(c, desc, p, map_a3, map_b3, table, packed, n, workspace, workspace_bytes, stream, &go));
    if (!go) return IRON_OK;
    if (!lin_steps || !ray_o || !ray_d || !near || !far || !work || !conv || !points || !sdf_out || !dist) return IRON_ERR_BAD_ARG;
    const RayArgs R{ray_o, ray_d, n};
    HGT_TRY(begin(c));
    HGT_TRY(run_sphere(c, R, near, far, work, conv, points, sdf_out, dist, nullptr, stats));
    HGT_TRY(run_sampler(c, R, near, far, sdf_out, dist, nullptr, nullptr, lin_steps, conv, points, sdf_out, dist, stats));
    return run_bisect(c, R, p->chunk, conv, points, sdf_out, dist, stats);
}

int iron_hashgrid_trace_occluded(const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3, const float* map_b3,
                                 const float* table, const void* packed, const float* lin_steps, const float* ray_o, const float* ray_d,
                                 const float* near, const float* far, const uint8_t* work, int64_t n, uint8_t* occluded, int64_t* stats,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    Call c;
    bool go;
    HGT_TRY(open_call(c, desc, p, map_a3, map_b3, table, packed, n, workspace, workspace_bytes, stream, &go));
    if (!go) return IRON_OK;
    if (!lin_steps || !ray_o || !ray_d || !near || !far || !work || !occluded) return IRON_ERR_BAD_ARG;
    const RayArgs R{ray_o, ray_d, n};
    float *s = c.ws.f(c.ws.L.sdf), *t = c.ws.f(c.ws.L.dist);
    HGT_TRY(begin(c));
    HGT_TRY(run_sphere(c, R, near, far, work, occluded, nullptr, s, t, nullptr, stats));
    return run_sampler(c, R, near, far, s, t, nullptr, nullptr, lin_steps, occluded, nullptr, nullptr, nullptr, stats);
}

int iron_hashgrid_trace_stage(int32_t stage, const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3,
                              const float* map_b3, const float* table, const void* packed, const float* lin_steps, const float* ray_o,
                              const float* ray_d, const float* in0, const float* in1, const float* in2, const float* in3, const uint8_t* work,
                              int64_t n, uint8_t* mask_out, uint8_t* unfinished_out, float* points, float* sdf_out, float* dist, int64_t* stats,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (stage < 0 || stage > 2) return IRON_ERR_BAD_ARG;
    Call c;
    bool go;
    HGT_TRY(open_call(c, desc, p, map_a3, map_b3, table, packed, n, workspace, workspace_bytes, stream, &go));
    if (!go) return IRON_OK;
    if (!ray_o || !ray_d || !in0 || !in1 || !mask_out || !points || !sdf_out || !dist) return IRON_ERR_BAD_ARG;
    if ((stage == 0 && !work) || (stage == 1 && !lin_steps) || (stage == 2 && (!in2 || !in3))) return IRON_ERR_BAD_ARG;
    const RayArgs R{ray_o, ray_d, n};
    const Ws& w = c.ws;
    HGT_TRY(begin(c));
    if (stage == 0) return run_sphere(c, R, in0, in1, work, mask_out, points, sdf_out, dist, unfinished_out, stats);
    if (stage == 1) {
        IRON_LAUNCH(k_hgt_all, blocks_for(n, kBlk), kBlk, c.st, n, w.i32(w.L.list), w.words(), stats);
        HGT_TRY(run_sampler(c, R, nullptr, nullptr, nullptr, nullptr, in0, in1, lin_steps, mask_out, points, sdf_out, dist, stats));
        return run_bisect(c, R, 0, mask_out, points, sdf_out, dist, stats);
    }
    IRON_LAUNCH(k_hgt_brackets_given, blocks_for(n, kBlk), kBlk, c.st, in0, in1, in2, in3, n, brackets_of(w), w.words(), stats);
    return run_bisect(c, R, 0, nullptr, points, sdf_out, dist, stats);
}

}  // extern "C"
