// The callable tracer's bookkeeping (include/iron_hip.h: iron_trace_any_*).  RayTracer.forward on an opaque SDF callable
// (models/raytracer.py:45-220): the caller's function supplies the values, batch by batch, from the host; everything between two
// evaluations -- the termination tests, the ray advance, the stable compaction of the unfinished rays, the sampler's points, the
// row reduction to a bracket, the bisection update -- is one or two small launches here.  Every kernel is one thread per list entry
// (one wave per ray row in the reduction) and bounded by the count it was launched with; the formulas are the reference's, one
// rounding per product and sum (-ffp-contract=off), and the comparisons are the reference's own so that NaN and zero fall where
// torch puts them.  Compaction is pair_scan over 0/1 flags: ascending ray index, bitwise deterministic.
#include "pair_scan.h"
#include "trace_ray.h"

#include <limits.h>

namespace iron {
namespace {

constexpr int kBlk = 256;

struct AnyLayout {
    size_t unf, rootf, list[2], smin, smax, u_dlo, u_dhi, u_flo, u_fhi, b_ray, b_dlo, b_dhi, b_flo, b_fhi, b_dmid, b_work, words, scan;
    size_t total;
};

AnyLayout any_layout(int64_t n) {
    const size_t c1 = (size_t)(n > 0 ? n : 1);
    Carver c;
    AnyLayout L{};
    L.unf = c.take(c1);
    L.rootf = c.take(c1);
    L.list[0] = c.take(4 * c1);
    L.list[1] = c.take(4 * c1);
    size_t* f32[] = {&L.smin, &L.smax, &L.u_dlo, &L.u_dhi, &L.u_flo, &L.u_fhi, &L.b_dlo, &L.b_dhi, &L.b_flo, &L.b_fhi, &L.b_dmid};
    for (size_t* f : f32) *f = c.take(4 * c1);
    L.b_ray = c.take(4 * c1);
    L.b_work = c.take(c1);
    L.words = c.take(2 * sizeof(int64_t));
    L.scan = c.off;
    scan_levels((int64_t)c1, c);
    L.total = c.off;
    return L;
}

// the scan over the first m entries, carved where the layout keeps the scan of n (m <= n: never larger)
ScanLevels scan_at(const AnyLayout& L, int64_t m) {
    Carver c;
    c.off = L.scan;
    return scan_levels(m, c);
}

struct Ws {
    AnyLayout L;
    void* base;
    uint8_t* unf() const { return ws_ptr<uint8_t>(base, L.unf); }
    uint8_t* rootf() const { return ws_ptr<uint8_t>(base, L.rootf); }
    int32_t* list(int i) const { return ws_ptr<int32_t>(base, L.list[i]); }
    float* f(size_t off) const { return ws_ptr<float>(base, off); }
    int32_t* b_ray() const { return ws_ptr<int32_t>(base, L.b_ray); }
    uint8_t* b_work() const { return ws_ptr<uint8_t>(base, L.b_work); }
    int64_t* words() const { return ws_ptr<int64_t>(base, L.words); }
};

// capacity n of the call (its rays), the workspace it was sized for
bool open_ws(Ws& w, int64_t n, void* workspace, size_t workspace_bytes) {
    if (n < 0 || n > (int64_t)INT_MAX - 1 || !workspace) return false;
    w.L = any_layout(n);
    w.base = workspace;
    return workspace_bytes >= w.L.total;
}

__device__ __forceinline__ int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the per-ray formulas (trace_ray.h), shared with the hash-grid field's device tracer
using ray::ray_point;
using ray::sample_z;

__global__ __launch_bounds__(kBlk) void k_any_start(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ near,
                                                    int64_t n, float* __restrict__ points, float* __restrict__ dist) {
    const int64_t i = gid();
    if (i >= n) return;
    const float t = near[i];
    dist[i] = t;
    ray_point(o, d, i, t, points + i * 3);
}

// raytracer.py:113-117: the values of the current list land in sdf; unfinished &= |s| > thr & t < max_dis.  list_in == nullptr: the
// first evaluation, on all rays (unfinished starts as work_mask).
__global__ __launch_bounds__(kBlk) void k_any_sphere_flag(const float* __restrict__ values, const int32_t* __restrict__ list_in, int64_t m, float thr,
                                                          const float* __restrict__ far, const uint8_t* __restrict__ work, float* __restrict__ sdf,
                                                          const float* __restrict__ dist, uint8_t* __restrict__ unf, Pair64* __restrict__ flags) {
    const int64_t k = gid();
    if (k >= m) return;
    const int64_t ray = list_in ? list_in[k] : k;
    const float s = values[k];
    sdf[ray] = s;
    const bool before = list_in ? unf[ray] != 0 : work[ray] != 0;
    const bool u = ray::still_unfinished(before, s, thr, dist[ray], far[ray]);
    unf[ray] = u ? 1 : 0;
    flags[k] = Pair64{u ? 1 : 0, 0};
}

// raytracer.py:123-130: the unfinished rays, listed in ascending order, step by their value; their new points are the next batch
__global__ __launch_bounds__(kBlk) void k_any_sphere_emit(const int32_t* __restrict__ list_in, int64_t m, int advance, const float* __restrict__ d,
                                                          float* __restrict__ points, const float* __restrict__ sdf, float* __restrict__ dist,
                                                          const uint8_t* __restrict__ unf, const Pair64* __restrict__ prefix,
                                                          int32_t* __restrict__ list_out, float* __restrict__ pts_out, int64_t* __restrict__ words) {
    const int64_t k = gid();
    if (k >= m) return;
    const int64_t ray = list_in ? list_in[k] : k;
    const bool u = unf[ray] != 0;
    const int64_t pos = prefix[k].a;
    if (u) {
        list_out[pos] = (int32_t)ray;
        if (advance) {
            const float s = sdf[ray];
            dist[ray] = dist[ray] + s;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p = ray::advance(points[ray * 3 + c], d[ray * 3 + c], s);
                points[ray * 3 + c] = p;
                pts_out[pos * 3 + c] = p;
            }
        }
    }
    if (k == m - 1) words[0] = pos + (u ? 1 : 0);
}

// raytracer.py:132-137
__global__ __launch_bounds__(kBlk) void k_any_sphere_finish(const uint8_t* __restrict__ work, const float* __restrict__ far, float thr, int64_t n,
                                                            const float* __restrict__ sdf, const float* __restrict__ dist,
                                                            const uint8_t* __restrict__ unf, uint8_t* __restrict__ conv, uint8_t* __restrict__ unf_out) {
    const int64_t i = gid();
    if (i >= n) return;
    const bool u = unf[i] != 0;
    conv[i] = ray::sphere_converged(work[i] != 0, u, sdf[i], thr, dist[i], far[i]) ? 1 : 0;
    if (unf_out) unf_out[i] = u ? 1 : 0;
}

// raytracer.py:56-63: sample behind the last sphere-tracing point when it is outside the surface, in front of it otherwise
__global__ __launch_bounds__(kBlk) void k_any_interval(const int32_t* __restrict__ list, int64_t m, const float* __restrict__ near,
                                                       const float* __restrict__ far, const float* __restrict__ sdf, const float* __restrict__ dist,
                                                       float* __restrict__ smin, float* __restrict__ smax) {
    const int64_t k = gid();
    if (k >= m) return;
    const int64_t ray = list[k];
    ray::sampler_interval(sdf[ray], dist[ray], near[ray], far[ray], smin + k, smax + k);
}

// raytracer.py:144-150 for the rays [k0, k0 + nk) of the list: point q of the batch is sample q % n_steps of ray k0 + q / n_steps
__global__ __launch_bounds__(kBlk) void k_any_sampler_points(const int32_t* __restrict__ list, int64_t k0, int64_t nk, int n_steps,
                                                             const float* __restrict__ lin, const float* __restrict__ o, const float* __restrict__ d,
                                                             const float* __restrict__ smin, const float* __restrict__ smax, float* __restrict__ pts_out) {
    const int64_t q = gid();
    if (q >= nk * n_steps) return;
    const int64_t k = k0 + q / n_steps;
    const int j = (int)(q % n_steps);
    const int64_t ray = list ? list[k] : k;
    ray_point(o, d, ray, sample_z(smin[k], smax[k], lin[j]), pts_out + q * 3);
}

// raytracer.py:162-177, one wave per row: torch.min over sign(val) * (n_steps - j) picks the smallest j with val < 0 (the weights
// fall with j); a root needs that j >= 1.  torch.sign is (0 < x) - (x < 0): a NaN sample counts like a zero one, neither sign, and
// that is what `x < 0` says of it too.  The bracket (z, f) pairs are those of samples j - 1 and j (f_low may then be 0 or NaN:
// such a bracket opens no loop of its own, raytracer.py:203).
__global__ __launch_bounds__(kBlk) void k_any_sampler_reduce(int64_t k0, int64_t nk, int n_steps, const float* __restrict__ lin,
                                                             const float* __restrict__ values, const float* __restrict__ smin,
                                                             const float* __restrict__ smax, uint8_t* __restrict__ rootf, float* __restrict__ u_dlo,
                                                             float* __restrict__ u_dhi, float* __restrict__ u_flo, float* __restrict__ u_fhi) {
    const int64_t row = gid() >> 6;   // uniform over the wave
    if (row >= nk) return;
    const int lane = threadIdx.x & 63;
    const float* v = values + row * n_steps;
    int first = INT_MAX;
    for (int j = lane; j < n_steps; j += 64)
        if (v[j] < 0.0f && j < first) first = j;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) first = min(first, __shfl_xor(first, s, 64));
    if (lane != 0) return;
    const int64_t k = k0 + row;
    const bool root = first != INT_MAX && first >= 1;
    rootf[k] = root ? 1 : 0;
    if (root) {
        const float lo = smin[k], hi = smax[k];
        u_dlo[k] = sample_z(lo, hi, lin[first - 1]);
        u_dhi[k] = sample_z(lo, hi, lin[first]);
        u_flo[k] = v[first - 1];
        u_fhi[k] = v[first];
    }
}

__global__ __launch_bounds__(kBlk) void k_any_root_flags(const uint8_t* __restrict__ rootf, int64_t m, Pair64* __restrict__ flags) {
    const int64_t k = gid();
    if (k < m) flags[k] = Pair64{rootf[k], 0};
}

struct Bisect {
    int32_t* ray;
    float *dlo, *dhi, *flo, *fhi, *dmid;
    uint8_t* work;
};

// raytracer.py:200-203 for slot b, and the mid point as the next batch's entry b
__device__ __forceinline__ void bisect_open(const Bisect& B, int64_t b, int64_t ray, float dlo, float dhi, float flo, float fhi,
                                            const float* __restrict__ o, const float* __restrict__ d, float* __restrict__ pts_out,
                                            int64_t* __restrict__ words) {
    const bool w = ray::bracket_open(flo, fhi);
    const float mid = ray::bracket_mid(dlo, dhi);
    B.ray[b] = (int32_t)ray;
    B.dlo[b] = dlo; B.dhi[b] = dhi; B.flo[b] = flo; B.fhi[b] = fhi; B.dmid[b] = mid;
    B.work[b] = w ? 1 : 0;
    ray_point(o, d, ray, mid, pts_out + b * 3);
    if (w) words[1] = 1;
}

// raytracer.py:158-160, 178-197: rootless rays of the sampler hold zeros; the others are listed, in order, for the bisection
__global__ __launch_bounds__(kBlk) void k_any_sampler_gather(const int32_t* __restrict__ list, int64_t m, const uint8_t* __restrict__ rootf,
                                                             const Pair64* __restrict__ prefix, const float* __restrict__ u_dlo,
                                                             const float* __restrict__ u_dhi, const float* __restrict__ u_flo,
                                                             const float* __restrict__ u_fhi, const float* __restrict__ o, const float* __restrict__ d,
                                                             uint8_t* __restrict__ conv, float* __restrict__ points, float* __restrict__ sdf,
                                                             float* __restrict__ dist, Bisect B, float* __restrict__ pts_out, int64_t* __restrict__ words) {
    const int64_t k = gid();
    if (k >= m) return;
    const int64_t ray = list ? list[k] : k;
    const bool root = rootf[k] != 0;
    const int64_t b = prefix[k].a;
    if (root) {
        bisect_open(B, b, ray, u_dlo[k], u_dhi[k], u_flo[k], u_fhi[k], o, d, pts_out, words);
    } else {
        conv[ray] = 0;
        points[ray * 3 + 0] = 0.0f; points[ray * 3 + 1] = 0.0f; points[ray * 3 + 2] = 0.0f;
        sdf[ray] = 0.0f;
        dist[ray] = 0.0f;
    }
    if (k == m - 1) words[0] = b + (root ? 1 : 0);
}

__global__ __launch_bounds__(kBlk) void k_any_bisect_load(const float* __restrict__ f_low, const float* __restrict__ f_high, const float* __restrict__ d_low,
                                                          const float* __restrict__ d_high, int64_t n, const float* __restrict__ o,
                                                          const float* __restrict__ d, Bisect B, float* __restrict__ pts_out, int64_t* __restrict__ words) {
    const int64_t b = gid();
    if (b < n) bisect_open(B, b, b, d_low[b], d_high[b], f_low[b], f_high[b], o, d, pts_out, words);
}

// raytracer.py:205-217: every slot moves, bracket or not; `work` only decides whether the call goes on
__global__ __launch_bounds__(kBlk) void k_any_bisect_step(const float* __restrict__ values, int64_t nb, float two_thr, const float* __restrict__ o,
                                                          const float* __restrict__ d, Bisect B, float* __restrict__ pts_out, int64_t* __restrict__ words) {
    const int64_t b = gid();
    if (b >= nb) return;
    const float fm = values[b];
    const float mid0 = B.dmid[b];
    float dlo = B.dlo[b], dhi = B.dhi[b], flo = B.flo[b], fhi = B.fhi[b];
    ray::bracket_update(fm, mid0, &dlo, &dhi, &flo, &fhi);
    B.dlo[b] = dlo; B.dhi[b] = dhi; B.flo[b] = flo; B.fhi[b] = fhi;
    const float mid = ray::bracket_mid(dlo, dhi);
    B.dmid[b] = mid;
    const bool w = B.work[b] != 0 && ray::bracket_wide(dlo, dhi, two_thr);
    B.work[b] = w ? 1 : 0;
    ray_point(o, d, B.ray[b], mid, pts_out + b * 3);
    if (w) words[1] = 1;
}

// raytracer.py:218-220 and 192-197 / 66-79: the final mid point, its value and distance go to the ray's own slot
__global__ __launch_bounds__(kBlk) void k_any_finish(const float* __restrict__ values, int64_t nb, const float* __restrict__ o, const float* __restrict__ d,
                                                     Bisect B, uint8_t* __restrict__ conv, float* __restrict__ points, float* __restrict__ sdf,
                                                     float* __restrict__ dist) {
    const int64_t b = gid();
    if (b >= nb) return;
    const int64_t ray = B.ray[b];
    const float mid = B.dmid[b];
    ray_point(o, d, ray, mid, points + ray * 3);
    sdf[ray] = values[b];
    dist[ray] = mid;
    if (conv) conv[ray] = 1;
}

Bisect bisect_of(const Ws& w) {
    return Bisect{w.b_ray(), w.f(w.L.b_dlo), w.f(w.L.b_dhi), w.f(w.L.b_flo), w.f(w.L.b_fhi), w.f(w.L.b_dmid), w.b_work()};
}

}  // namespace
}  // namespace iron

using namespace iron;

extern "C" {

size_t iron_trace_any_workspace_bytes(int64_t n) {
    if (n < 0 || n > (int64_t)INT_MAX - 1) return 0;
    return any_layout(n).total;
}

int iron_trace_any_start(const float* ray_o, const float* ray_d, const float* near, int64_t n, float* points, float* dist, void* stream) {
    if (n < 0 || (n > 0 && (!ray_o || !ray_d || !near || !points || !dist))) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    IRON_LAUNCH(k_any_start, blocks_for(n, kBlk), kBlk, (hipStream_t)stream, ray_o, ray_d, near, n, points, dist);
    return IRON_OK;
}

int iron_trace_any_sphere_step(const float* values, int64_t m, int32_t list_in, int32_t advance, float sdf_threshold, const float* ray_d,
                               const float* far, const uint8_t* work, int64_t n, float* points, float* sdf, float* dist, float* pts_out,
                               int64_t pts_capacity, void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || m <= 0 || m > n || list_in < -1 || list_in > 1) return IRON_ERR_BAD_ARG;
    if (list_in < 0 && m != n) return IRON_ERR_BAD_ARG;
    if (!values || !ray_d || !far || !work || !points || !sdf || !dist || !pts_out || pts_capacity < m) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int32_t* in = list_in < 0 ? nullptr : w.list(list_in);
    int32_t* out = w.list(list_in < 0 ? 0 : 1 - list_in);
    const ScanLevels S = scan_at(w.L, m);
    IRON_LAUNCH(k_any_sphere_flag, blocks_for(m, kBlk), kBlk, st, values, in, m, sdf_threshold, far, work, sdf, (const float*)dist, w.unf(),
                S.level(w.base, 0));
    const int rc = pair_scan(S, w.base, st);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_any_sphere_emit, blocks_for(m, kBlk), kBlk, st, in, m, (int)(advance != 0), ray_d, points, (const float*)sdf, dist,
                (const uint8_t*)w.unf(), (const Pair64*)S.level(w.base, 0), out, pts_out, w.words());
    return IRON_OK;
}

int iron_trace_any_read(const void* workspace, size_t workspace_bytes, int64_t n, int64_t* out2, void* stream) {
    Ws w;
    if (!open_ws(w, n, (void*)workspace, workspace_bytes) || !out2) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    IRON_HIP_TRY(hipMemcpyAsync(out2, w.words(), 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    return IRON_OK;
}

int iron_trace_any_sphere_finish(const uint8_t* work, const float* far, float sdf_threshold, int64_t n, const float* sdf, const float* dist,
                                 uint8_t* conv, uint8_t* unfinished_out, void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || n <= 0 || !work || !far || !sdf || !dist || !conv) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_any_sphere_finish, blocks_for(n, kBlk), kBlk, (hipStream_t)stream, work, far, sdf_threshold, n, sdf, dist,
                (const uint8_t*)w.unf(), conv, unfinished_out);
    return IRON_OK;
}

int iron_trace_any_sampler_interval(int32_t list_sel, int64_t m, const float* a, const float* b, const float* sdf, const float* dist, int64_t n,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || m <= 0 || m > n || list_sel < -1 || list_sel > 1 || !a || !b) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (list_sel < 0) {
        IRON_HIP_TRY(hipMemcpyAsync(w.f(w.L.smin), a, 4 * (size_t)m, hipMemcpyDeviceToDevice, st));
        IRON_HIP_TRY(hipMemcpyAsync(w.f(w.L.smax), b, 4 * (size_t)m, hipMemcpyDeviceToDevice, st));
        return IRON_OK;
    }
    if (!sdf || !dist) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_any_interval, blocks_for(m, kBlk), kBlk, st, (const int32_t*)w.list(list_sel), m, a, b, sdf, dist, w.f(w.L.smin), w.f(w.L.smax));
    return IRON_OK;
}

int iron_trace_any_sampler_points(int32_t list_sel, int64_t m, int64_t k0, int64_t nk, int32_t n_steps, const float* lin_steps,
                                  const float* ray_o, const float* ray_d, int64_t n, float* pts_out, int64_t pts_capacity, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || m <= 0 || m > n || list_sel < -1 || list_sel > 1) return IRON_ERR_BAD_ARG;
    if (k0 < 0 || nk <= 0 || k0 + nk > m || n_steps < 2 || n_steps > 4096 || !lin_steps || !ray_o || !ray_d || !pts_out) return IRON_ERR_BAD_ARG;
    if (pts_capacity < nk * n_steps) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_any_sampler_points, blocks_for(nk * n_steps, kBlk), kBlk, (hipStream_t)stream,
                list_sel < 0 ? (const int32_t*)nullptr : (const int32_t*)w.list(list_sel), k0, nk, (int)n_steps, lin_steps, ray_o, ray_d,
                (const float*)w.f(w.L.smin), (const float*)w.f(w.L.smax), pts_out);
    return IRON_OK;
}

int iron_trace_any_sampler_reduce(int64_t m, int64_t k0, int64_t nk, int32_t n_steps, const float* lin_steps, const float* values, int64_t n,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || m <= 0 || m > n || k0 < 0 || nk <= 0 || k0 + nk > m) return IRON_ERR_BAD_ARG;
    if (n_steps < 2 || n_steps > 4096 || !lin_steps || !values) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_any_sampler_reduce, blocks_for(nk * 64, kBlk), kBlk, (hipStream_t)stream, k0, nk, (int)n_steps, lin_steps, values,
                (const float*)w.f(w.L.smin), (const float*)w.f(w.L.smax), w.rootf(), w.f(w.L.u_dlo), w.f(w.L.u_dhi), w.f(w.L.u_flo),
                w.f(w.L.u_fhi));
    return IRON_OK;
}

int iron_trace_any_sampler_gather(int32_t list_sel, int64_t m, const float* ray_o, const float* ray_d, int64_t n, uint8_t* conv, float* points,
                                  float* sdf, float* dist, float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || m <= 0 || m > n || list_sel < -1 || list_sel > 1) return IRON_ERR_BAD_ARG;
    if (!ray_o || !ray_d || !conv || !points || !sdf || !dist || !pts_out || pts_capacity < m) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const ScanLevels S = scan_at(w.L, m);
    IRON_HIP_TRY(hipMemsetAsync(w.words(), 0, 2 * sizeof(int64_t), st));
    IRON_LAUNCH(k_any_root_flags, blocks_for(m, kBlk), kBlk, st, (const uint8_t*)w.rootf(), m, S.level(w.base, 0));
    const int rc = pair_scan(S, w.base, st);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_any_sampler_gather, blocks_for(m, kBlk), kBlk, st, list_sel < 0 ? (const int32_t*)nullptr : (const int32_t*)w.list(list_sel), m,
                (const uint8_t*)w.rootf(), (const Pair64*)S.level(w.base, 0), (const float*)w.f(w.L.u_dlo), (const float*)w.f(w.L.u_dhi),
                (const float*)w.f(w.L.u_flo), (const float*)w.f(w.L.u_fhi), ray_o, ray_d, conv, points, sdf, dist, bisect_of(w), pts_out,
                w.words());
    return IRON_OK;
}

int iron_trace_any_bisect_load(const float* f_low, const float* f_high, const float* d_low, const float* d_high, const float* ray_o,
                               const float* ray_d, int64_t n, float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes,
                               void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || n <= 0 || !f_low || !f_high || !d_low || !d_high || !ray_o || !ray_d || !pts_out ||
        pts_capacity < n)
        return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    IRON_HIP_TRY(hipMemsetAsync(w.words(), 0, 2 * sizeof(int64_t), st));
    IRON_LAUNCH(k_any_bisect_load, blocks_for(n, kBlk), kBlk, st, f_low, f_high, d_low, d_high, n, ray_o, ray_d, bisect_of(w), pts_out, w.words());
    return IRON_OK;
}

int iron_trace_any_bisect_step(const float* values, int64_t nb, float sdf_threshold, const float* ray_o, const float* ray_d, int64_t n,
                               float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || nb <= 0 || nb > n || !values || !ray_o || !ray_d || !pts_out || pts_capacity < nb)
        return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    IRON_HIP_TRY(hipMemsetAsync(w.words() + 1, 0, sizeof(int64_t), st));
    IRON_LAUNCH(k_any_bisect_step, blocks_for(nb, kBlk), kBlk, st, values, nb, 2.0f * sdf_threshold, ray_o, ray_d, bisect_of(w), pts_out, w.words());
    return IRON_OK;
}

int iron_trace_any_finish(const float* values, int64_t nb, const float* ray_o, const float* ray_d, int64_t n, uint8_t* conv, float* points,
                          float* sdf, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    Ws w;
    if (!open_ws(w, n, workspace, workspace_bytes) || nb <= 0 || nb > n || !values || !ray_o || !ray_d || !points || !sdf || !dist)
        return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_any_finish, blocks_for(nb, kBlk), kBlk, (hipStream_t)stream, values, nb, ray_o, ray_d, bisect_of(w), conv, points, sdf, dist);
    return IRON_OK;
}

}  // extern "C"
