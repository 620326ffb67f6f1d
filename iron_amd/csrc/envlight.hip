// Environment-map relighting of an exported asset: an occlusion query over the linear BVH, a lat-long
// environment map with its sampling distribution, a direct-illumination integrator that combines environment samples and BRDF
// samples with the multi-sample balance heuristic, and a path integrator for the interreflections.  Conventions: include/iron_hip.h,
// iron_mesh_occluded block.
//
// Occlusion (bvh_any_hit): the walk of k_raycast (meshrender.hip) with the primitive tests of ray_core.h, a fixed far end t_max in
// place of the shrinking best t, and an exit at the first accepted face.  A face is accepted under exactly k_raycast's condition
// (ray_tri and t <= t_max), and the walk visits a superset of the boxes k_raycast visits; a ray for which k_raycast finds nothing
// walks exactly the same boxes here.  Hence occluded == (raycast.face_idx >= 0), bitwise.
//
// Environment map: lat-long [He, We, 3], Mitsuba 0.6's convention: a local direction d has u = atan2(d.x, -d.z) / 2 pi wrapped to
// [0, 1), v = acos(d.y) / pi, texel (floor(v He), floor(u We)) clamped; world = to_world local.  Radiance is constant per texel.
// The distribution is over texels, weight = luminance sin(pi (row + 1/2) / He), as fp64 row CDFs and a marginal CDF (block scans in
// a fixed order: reproducible); a direction is uniform in (u, v) inside its texel, so its solid-angle density is
// P(texel) We He / (2 pi^2 sin theta).
//
// Integrators: the estimator (vertex, sample draws, terms, pixel reduction) is written once, in the section of that name; a pixel's
// sums depend on nothing but its own samples.  k_shade_env runs the direct estimator on the mesh.  Random numbers: env_rand, a pure
// function of (seed, pixel index, sample, dimension).
//
// Interreflections (k_shade_env_indirect): the light that reaches a primary hit after at least one more surface, by
// paths of a fixed largest length; the bounce rays walk bvh_closest_hit of ray_walk.h (k_raycast's walk), the shadow rays
// bvh_any_hit, both on the one LDS stack in turn.  The direct term stays k_shade_env's.  The k_nenv_* and k_npath_* kernels run the
// same two estimators on the neural scene.
#include "asset_common.h"
#include "ggx_core.h"
#include "pair_scan.h"
#include "ray_walk.h"

namespace iron {

// ---- occlusion ----
__device__ __forceinline__ bool tri_blocks(const float4* __restrict__ tris, int32_t k, const RayPre& r, float t_min, float t_max,
                                           int32_t skip) {
    TriHit x;
    return ray_tri(tris, k, r, t_min, x) && x.t <= t_max && x.face != skip;
}

// is any face other than `skip` met with t in (t_min, t_max]?  `stack`: the per-lane LDS stack of k_raycast
__device__ __forceinline__ bool bvh_any_hit(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf, const RayPre& r,
                                            float t_min, float t_max, int32_t skip, int32_t (*stack)[kBvQueryBlock], int lane) {
    if (nf == 1) return tri_blocks(tris, 0, r, t_min, t_max, skip);
    int32_t node = 0, sp = 0;
    for (;;) {
        const float4* nd = nodes + 4 * (int64_t)node;
        const float4 l0 = nd[0], h0 = nd[1], l1 = nd[2], h1 = nd[3];
        const int32_t c0 = __float_as_int(l0.w), c1 = __float_as_int(h0.w);
        float n0, n1;
        const bool v0 = ray_box(r, l0, h0, t_min, t_max, n0);
        if (c0 < 0 && v0 && tri_blocks(tris, ~c0, r, t_min, t_max, skip)) return true;
        const bool v1 = ray_box(r, l1, h1, t_min, t_max, n1);
        if (c1 < 0 && v1 && tri_blocks(tris, ~c1, r, t_min, t_max, skip)) return true;
        const bool g0 = c0 >= 0 && v0, g1 = c1 >= 0 && v1;
        if (g0 && g1) {
            const bool first1 = n1 < n0;
            if (sp < kBvStack) stack[sp++][lane] = first1 ? c0 : c1;  // never full (kBvStack)
            node = first1 ? c1 : c0;
        } else if (g0) {
            node = c0;
        } else if (g1) {
            node = c1;
        } else {
            if (sp == 0) return false;
            node = stack[--sp][lane];
        }
    }
}

__global__ __launch_bounds__(kBvQueryBlock) void k_occluded(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf,
                                                             const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t n,
                                                             float t_min, float t_max, const int32_t* __restrict__ skip_face,
                                                             uint8_t* __restrict__ occluded) {
    __shared__ int32_t stack[kBvStack][kBvQueryBlock];
    const int lane = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * kBvQueryBlock + lane;
    if (q >= n) return;
    const float3 o = ld3(ray_o, q), d = ld3(ray_d, q);
    bool hit = false;
    if (ray_valid(o, d) && t_min <= t_max) {  // NaN bounds fail
        RayPre r;
        ray_setup(o, d, r);
        hit = bvh_any_hit(nodes, tris, nf, r, t_min, t_max, skip_face ? skip_face[q] : -1, stack, lane);
    }
    occluded[q] = hit ? 1 : 0;
}

// the diagonal of the root box (the box of every referenced vertex)
__device__ __forceinline__ float bvh_diagonal(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf) {
    float4 a, b, c, d;
    if (nf == 1) {
        a = tris[0]; b = tris[1]; c = d = tris[2];
    } else {
        a = nodes[0]; b = nodes[1]; c = nodes[2]; d = nodes[3];
    }
    const float lx = fminf(fminf(a.x, b.x), fminf(c.x, d.x)), ly = fminf(fminf(a.y, b.y), fminf(c.y, d.y)),
                lz = fminf(fminf(a.z, b.z), fminf(c.z, d.z));
    const float hx = fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x)), hy = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y)),
                hz = fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z));
    const float ex = hx - lx, ey = hy - ly, ez = hz - lz;
    return sqrtf((ex * ex + ey * ey) + ez * ez);
}

// ---- environment map ----
constexpr double kPiD = 3.141592653589793;
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kTwoPiSq = 19.7392088021787172376f;  // 2 pi^2
constexpr int kEnvBlock = 256;

struct EnvLayout {
    size_t total_off, mcdf_off, rowsum_off, rowcdf_off, ptex_off, bytes;
};

inline EnvLayout env_layout(int64_t He, int64_t We) {
    EnvLayout L{};
    Carver c;
    L.total_off = c.take(8);
    L.mcdf_off = c.take(8 * (size_t)(He + 1));
    L.rowsum_off = c.take(8 * (size_t)He);
    L.rowcdf_off = c.take(8 * (size_t)(He * (We + 1)));
    L.ptex_off = c.take(4 * (size_t)(He * We));
    L.bytes = c.off;
    return L;
}

struct EnvDev {
    const float* image;    // [He, We, 3]
    const double* total;   // the sum of the weights
    const double* mcdf;    // [He + 1] marginal CDF over rows, 0 .. 1
    const double* rowcdf;  // [He, We + 1] CDF of every row, 0 .. 1 (zeros for a row without weight)
    const float* ptex;     // [He, We] P(texel)
    int32_t He, We;
    float R[9];            // world = R local
};

__device__ __forceinline__ double env_weight(const float* __restrict__ img, int64_t r, int64_t c, int64_t He, int64_t We) {
    const float* p = img + 3 * (r * We + c);
    const double lum = (0.2126 * (double)p[0] + 0.7152 * (double)p[1]) + 0.0722 * (double)p[2];
    return lum * sin(kPiD * ((double)r + 0.5) / (double)He);
}

// inclusive scan of n values w(k) by one block, in a fixed order: out[k + 1] = w(0) + .. + w(k), out[0] = 0; returns (to every
// thread) the last entry.  Thread t owns a contiguous segment; the segment sums are scanned in LDS.
template <class W>
__device__ __forceinline__ double block_cdf(int64_t n, W w, double* __restrict__ out, double* sh) {
    const int t = threadIdx.x;
    const int64_t seg = (n + kEnvBlock - 1) / kEnvBlock, k0 = min((int64_t)t * seg, n), k1 = min(k0 + seg, n);
    double s = 0.0;
    for (int64_t k = k0; k < k1; ++k) s += w(k);
    sh[t] = s;
    __syncthreads();
    for (int h = 1; h < kEnvBlock; h <<= 1) {
        const double add = t >= h ? sh[t - h] : 0.0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    double run = t > 0 ? sh[t - 1] : 0.0;
    __syncthreads();
    if (t == 0) out[0] = 0.0;
    for (int64_t k = k0; k < k1; ++k) {
        run += w(k);
        out[k + 1] = run;
    }
    if (k1 == n && k0 < n) sh[kEnvBlock] = run;  // the owner of the last entry
    __syncthreads();
    return sh[kEnvBlock];
}

__global__ __launch_bounds__(kEnvBlock) void k_env_rows(const float* __restrict__ img, int He, int We, double* __restrict__ rowcdf,
                                                         double* __restrict__ rowsum) {
    __shared__ double sh[kEnvBlock + 1];
    const int64_t r = blockIdx.x;
    const double last = block_cdf(We, [&](int64_t c) { return env_weight(img, r, c, He, We); }, rowcdf + r * (We + 1), sh);
    if (threadIdx.x == 0) rowsum[r] = last;
}

__global__ __launch_bounds__(kEnvBlock) void k_env_marginal(const double* __restrict__ rowsum, int He, double* __restrict__ mcdf,
                                                             double* __restrict__ total) {
    __shared__ double sh[kEnvBlock + 1];
    const double tot = block_cdf(He, [&](int64_t r) { return rowsum[r]; }, mcdf, sh);
    if (threadIdx.x == 0) *total = tot;
    __syncthreads();
    for (int k = threadIdx.x; k <= He; k += kEnvBlock) mcdf[k] = tot > 0.0 ? (k == He ? 1.0 : mcdf[k] / tot) : 0.0;
}

__global__ void k_env_normalise(const float* __restrict__ img, int He, int We, const double* __restrict__ rowsum,
                                const double* __restrict__ total, double* __restrict__ rowcdf, float* __restrict__ ptex) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)He * (We + 1)) return;
    const int64_t r = i / (We + 1), c = i % (We + 1);
    const double rs = rowsum[r], tot = *total;
    rowcdf[i] = rs > 0.0 ? (c == We ? 1.0 : rowcdf[i] / rs) : 0.0;
    if (c < We) ptex[r * We + c] = tot > 0.0 ? (float)(env_weight(img, r, c, He, We) / tot) : 0.0f;
}

__device__ __forceinline__ float3 mat_mul(const float R[9], float3 d) {
    return make_float3((R[0] * d.x + R[1] * d.y) + R[2] * d.z, (R[3] * d.x + R[4] * d.y) + R[5] * d.z, (R[6] * d.x + R[7] * d.y) + R[8] * d.z);
}
__device__ __forceinline__ float3 mat_tmul(const float R[9], float3 d) {
    return make_float3((R[0] * d.x + R[3] * d.y) + R[6] * d.z, (R[1] * d.x + R[4] * d.y) + R[7] * d.z, (R[2] * d.x + R[5] * d.y) + R[8] * d.z);
}

// the texel a world direction looks up, and sin theta of its local direction; false for a zero or non-finite direction
__device__ __forceinline__ bool env_texel(const EnvDev& E, float3 world, int& r, int& c, float& sin_theta) {
    const float3 d = mat_tmul(E.R, world);
    const float len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    r = c = 0; sin_theta = 0.0f;
    if (!(len > 0.0f) || !(len < kInfF)) return false;
    float u = atan2f(d.x, -d.z) / kTwoPi;
    if (u < 0.0f) u += 1.0f;
    const float v = acosf(fminf(fmaxf(d.y / len, -1.0f), 1.0f)) / kPi;
    r = min(max((int)floorf(v * (float)E.He), 0), E.He - 1);
    c = min(max((int)floorf(u * (float)E.We), 0), E.We - 1);
    sin_theta = sqrtf(d.x * d.x + d.z * d.z) / len;
    return true;
}

__device__ __forceinline__ float env_density(const EnvDev& E, int r, int c, float sin_theta) {
    const float p = E.ptex[(int64_t)r * E.We + c];
    return p > 0.0f ? p * ((float)E.We * (float)E.He) / (kTwoPiSq * sin_theta) : 0.0f;
}

// radiance and solid-angle density of the map at a world direction
__device__ __forceinline__ float env_eval(const EnvDev& E, float3 world, float L[3]) {
    int r, c;
    float st;
    L[0] = L[1] = L[2] = 0.0f;
    if (!env_texel(E, world, r, c, st)) return 0.0f;
    const float* p = E.image + 3 * ((int64_t)r * E.We + c);
    L[0] = p[0]; L[1] = p[1]; L[2] = p[2];
    return env_density(E, r, c, st);
}

// the number of entries of cdf[1 .. n] that are <= u: the interval [cdf[k], cdf[k + 1]) that holds u, never an empty one
__device__ __forceinline__ int cdf_find(const double* __restrict__ cdf, int n, double u) {
    int lo = 0, hi = n;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid + 1] <= u) lo = mid + 1; else hi = mid;
    }
    return min(lo, n - 1);
}

__device__ __forceinline__ float cdf_remap(const double* __restrict__ cdf, int k, double u) {
    const double w = cdf[k + 1] - cdf[k];
    const float f = w > 0.0 ? (float)((u - cdf[k]) / w) : 0.5f;
    return fminf(fmaxf(f, 0.0f), 0.99999994f);
}

// u0 picks the column, u1 the row; the direction is uniform in (u, v) inside the texel.  An all-black map: texel (0, 0), pdf 0.
__device__ __forceinline__ float env_sample(const EnvDev& E, float u0, float u1, int& r, int& c, float3& world) {
    const bool black = !(*E.total > 0.0);
    r = black ? 0 : cdf_find(E.mcdf, E.He, (double)u1);
    const double* row = E.rowcdf + (int64_t)r * (E.We + 1);
    c = black ? 0 : cdf_find(row, E.We, (double)u0);
    const float dv = black ? 0.5f : cdf_remap(E.mcdf, r, (double)u1), du = black ? 0.5f : cdf_remap(row, c, (double)u0);
    const float phi = kTwoPi * (((float)c + du) / (float)E.We), theta = kPi * (((float)r + dv) / (float)E.He);
    // sin(theta) through the nearer pole: pi v loses (1 - v)'s leading digits as v -> 1, (He - 1 - r) + (1 - dv) does not
    const float to_south = kPi * (((float)(E.He - 1 - r) + (1.0f - dv)) / (float)E.He);
    const float st = sinf(fminf(theta, to_south));
    world = mat_mul(E.R, make_float3(st * sinf(phi), cosf(theta), -(st * cosf(phi))));
    return black ? 0.0f : env_density(E, r, c, st);
}

__global__ void k_env_sample(EnvDev E, const float* __restrict__ u, int64_t n, int32_t* __restrict__ texel, float* __restrict__ dir,
                             float* __restrict__ pdf) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r, c;
    float3 w;
    const float p = env_sample(E, u[2 * i], u[2 * i + 1], r, c, w);
    texel[2 * i] = r; texel[2 * i + 1] = c;
    dir[3 * i] = w.x; dir[3 * i + 1] = w.y; dir[3 * i + 2] = w.z;
    pdf[i] = p;
}

__global__ void k_env_eval(EnvDev E, const float* __restrict__ dir, int64_t n, float* __restrict__ pdf, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float L[3];
    const float p = env_eval(E, ld3(dir, i), L);
    if (pdf) pdf[i] = p;
    if (rgb) { rgb[3 * i] = L[0]; rgb[3 * i + 1] = L[1]; rgb[3 * i + 2] = L[2]; }
}

// ---- BRDF sampling ----
// 23 random bits k -> (2 k + 1) 2^-24: the odd points of the 24-bit grid, exact in fp32, never 0 or 1
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float env_rand(uint32_t seed, uint32_t pixel, uint32_t sample, uint32_t dim) {
    uint32_t h = lowbias32(seed);
    h = lowbias32(h ^ pixel);
    h = lowbias32(h + sample);
    h = lowbias32(h + 0x9e3779b9u * (dim + 1u));
    return (float)(((h >> 9) << 1) | 1u) * 5.9604644775390625e-08f;
}

// orthonormal tangent frame of a unit normal (Duff et al., "Building an Orthonormal Basis, Revisited", JCGT 2017)
__device__ __forceinline__ void tangent_frame(float3 n, float3& t, float3& b) {
    const float sg = copysignf(1.0f, n.z), a = -1.0f / (sg + n.z), q = n.x * n.y * a;
    t = make_float3(1.0f + sg * n.x * n.x * a, sg * q, -sg * n.x);
    b = make_float3(q, sg + n.y * n.y * a, -n.y);
}

// density of the BRDF technique at w: half cosine-weighted (n.w / pi), half GGX half-vector sampling (D(h) n.h / (4 v.h), D the
// exact GGX density alpha^2 / (pi (alpha^2 cos^2 + sin^2)^2) with sin^2 = |n x h|^2, h = normalize(v + w))
__device__ __forceinline__ float brdf_pdf(float3 n, float3 v, float3 w, float alpha) {
    const float nw = dot3(n, w);
    const float pc = nw > 0.0f ? nw / kPi : 0.0f;
    float pg = 0.0f;
    float3 h = make_float3(v.x + w.x, v.y + w.y, v.z + w.z);
    const float hl = sqrtf(dot3(h, h));
    if (hl > 0.0f) {
        h = make_float3(h.x / hl, h.y / hl, h.z / hl);
        const float c = dot3(n, h), vh = dot3(v, h);
        if (c > 0.0f && vh > 0.0f) {
            const float3 x = cross3(n, h);
            const float a2 = alpha * alpha, den = a2 * c * c + dot3(x, x);
            pg = (a2 / (kPi * den * den)) * c / (4.0f * vh);
        }
    }
    return 0.5f * (pc + pg);
}

// u2 < 1/2: cosine-weighted about n; else a GGX half vector h (tan^2 = alpha^2 u0 / (1 - u0)) and w = 2 (v.h) h - v, which is
// no sample (false) when v.h <= 0
__device__ __forceinline__ bool brdf_sample(float3 n, float3 v, float alpha, float u0, float u1, float u2, float3& w) {
    float3 t, b;
    tangent_frame(n, t, b);
    const float phi = kTwoPi * u1, cp = cosf(phi), sp = sinf(phi);
    float x, y, z;
    const bool cosine = u2 < 0.5f;
    if (cosine) {
        const float rr = sqrtf(u0);
        x = rr * cp; y = rr * sp; z = sqrtf(1.0f - u0);
    } else {
        const float tan2 = alpha * alpha * u0 / (1.0f - u0);
        z = 1.0f / sqrtf(1.0f + tan2);
        const float s = sqrtf(tan2) * z;
        x = s * cp; y = s * sp;
    }
    const float3 d = make_float3((x * t.x + y * b.x) + z * n.x, (x * t.y + y * b.y) + z * n.y, (x * t.z + y * b.z) + z * n.z);
    if (cosine) { w = d; return true; }
    const float vh = dot3(v, d);
    w = make_float3(2.0f * vh * d.x - v.x, 2.0f * vh * d.y - v.y, 2.0f * vh * d.z - v.z);
    return vh > 0.0f;
}

__global__ void k_roughplastic(const float* __restrict__ n, const float* __restrict__ v, const float* __restrict__ l,
                               const float* __restrict__ kd, const float* __restrict__ ks, const float* __restrict__ rough,
                               const float* __restrict__ tab_trans, const float* __restrict__ tab_diff, int64_t cnt,
                               float* __restrict__ diffuse, float* __restrict__ specular) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    PlasticOut o;
    roughplastic_point(n + 3 * i, v + 3 * i, l + 3 * i, kd + 3 * i, ks + 3 * i, rough[i], tab_trans, tab_diff, o);
    st3(diffuse, i, o.diffuse[0], o.diffuse[1], o.diffuse[2]);
    st3(specular, i, o.specular[0], o.specular[1], o.specular[2]);
}

// ---- the integrator ----
constexpr int kEnvGroup = 16;  // lanes per pixel
constexpr int kEnvPixels = kBvQueryBlock / kEnvGroup;

struct EnvShadeArgs {
    iron_asset_mesh m;
    iron_asset_out o;
    iron_env_dump dump;
    EnvDev env;
    const float4 *nodes, *tris;
    const float *tab_trans, *tab_diff, *ray_o, *ray_d, *t, *bary;
    const int32_t *face_idx, *pixel_idx;
    int64_t n;
    int32_t n_light, n_brdf;
    uint32_t seed;
    float shadow_eps;
};

// the origin of a ray that leaves x along w: x moved by `off` along n_g to w's side
__device__ __forceinline__ float3 leave_origin(float3 x, float3 ng, float ngw, float off) {
    const float sg = ngw > 0.0f ? off : -off;
    return make_float3(x.x + sg * ng.x, x.y + sg * ng.y, x.z + sg * ng.z);
}

// may a sample direction w count at a vertex (shading normal n, geometric normal n_g, n_g.v)?  Above the shading horizon, on the
// viewer's side of the face, finite
__device__ __forceinline__ bool dir_counts(float3 n, float3 ng, float ngv, float3 w) {
    return dot3(n, w) > 0.0f && dot3(ng, w) * ngv > 0.0f && finite3(w);
}

// ---- the estimator ----
// What the four integrators below share, written once: the shading vertex, the two sample draws, the terms, the pixel reduction.
// A scene supplies two things.  The origin of a ray that leaves a vertex: leave_origin along n_g on the mesh, offset_origin on the
// neural scene, whose vertices carry the shading normal in the geometric normal's place.  And the answer to visibility and closest
// hit: the mesh walks its BVH in place, the neural scene reads the sphere tracer's listed answer.  With -ffp-contract=off one
// expression gives one result, so the scenes agree bit for bit where their inputs do.
struct EnvVertex {
    float3 pt, n, ng, v;  // point, shading normal, geometric normal, direction back to the viewer or along the path
    float mat[7];         // diffuse albedo, specular albedo, roughness
};

__device__ __forceinline__ void vertex_clear(EnvVertex& x) {
    x.pt = x.n = x.ng = x.v = make_float3(0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 7; ++c) x.mat[c] = 0.0f;
}

__device__ __forceinline__ float vertex_alpha(const EnvVertex& x) { return fmaxf(x.mat[6], 0.0001f); }

// BRDF . cos of the vertex for the light direction w
__device__ __forceinline__ void vertex_brdf(const EnvVertex& x, float3 w, const float* __restrict__ tab_trans,
                                            const float* __restrict__ tab_diff, PlasticOut& f) {
    const float nn[3] = {x.n.x, x.n.y, x.n.z}, vv[3] = {x.v.x, x.v.y, x.v.z}, ww[3] = {w.x, w.y, w.z};
    roughplastic_point(nn, vv, ww, x.mat, x.mat + 3, x.mat[6], tab_trans, tab_diff, f);
}

// the neural scene's ray origin: x + eps n, each product and sum rounded on its own
__device__ __forceinline__ float3 offset_origin(float3 x, float3 n, float eps) {
    const float ex = eps * n.x, ey = eps * n.y, ez = eps * n.z;
    return make_float3(x.x + ex, x.y + ey, x.z + ez);
}

// Sample k of a vertex's direct light: an environment sample for k < n_light, else a BRDF sample; random dimensions 0, 1, 2 of
// (seed, pixel, k).  As declared: no sample.
struct DirectDraw {
    float3 w = make_float3(0.f, 0.f, 0.f);  // the direction (zero: no sample)
    float denom = 0.0f;                     // the balance heuristic's n_light p_light + n_brdf p_brdf
    float L[3] = {0.f, 0.f, 0.f};           // the map's radiance along w
    bool counts = false;                    // w is a sample, and one that dir_counts lets through
};

__device__ __forceinline__ void draw_direct(const EnvDev& env, uint32_t seed, uint32_t pixel, int32_t k, int32_t n_light, int32_t n_brdf,
                                            const EnvVertex& x, DirectDraw& s) {
    const float alpha = vertex_alpha(x);
    float pl;
    bool ok;
    if (k < n_light) {
        int r, c;
        pl = env_sample(env, env_rand(seed, pixel, k, 0), env_rand(seed, pixel, k, 1), r, c, s.w);
        const float* p = env.image + 3 * ((int64_t)r * env.We + c);
        s.L[0] = p[0]; s.L[1] = p[1]; s.L[2] = p[2];
        ok = true;
    } else {
        ok = brdf_sample(x.n, x.v, alpha, env_rand(seed, pixel, k, 0), env_rand(seed, pixel, k, 1), env_rand(seed, pixel, k, 2), s.w);
        if (!ok) s.w = make_float3(0.f, 0.f, 0.f);
        pl = env_eval(env, s.w, s.L);
    }
    const float pb = ok ? brdf_pdf(x.n, x.v, s.w, alpha) : 0.0f;
    s.denom = (n_light > 0 ? (float)n_light * pl : 0.0f) + (n_brdf > 0 ? (float)n_brdf * pb : 0.0f);
    s.counts = dir_counts(x.n, x.ng, dot3(x.ng, x.v), s.w);  // no sample: w is zero, which never counts
}

// The two samples of vertex j of path p (vertex 0 is the primary hit), random dimensions 8 (j + 1) + c of (seed, pixel, p):
// c = 0, 1, 2 the BRDF sample that continues the path, c = 3, 4 the environment sample (vertices j >= 1: the primary's direct light
// is the direct estimator's).  As declared: no sample.
struct VertexDraw {
    float3 wl = make_float3(0.f, 0.f, 0.f), wb = wl;         // light direction, bounce direction (zero: no sample)
    float dl = 0.0f, db = 0.0f, pb = 0.0f;                   // the two denominators p_light + p_brdf, and p_brdf(w_b)
    float Ll[3] = {0.f, 0.f, 0.f}, Lb[3] = {0.f, 0.f, 0.f};  // the map's radiance along the two
    bool lcounts = false, bcounts = false;                   // the light / the bounce direction is a sample that dir_counts lets through
};

__device__ __forceinline__ void draw_vertex(const EnvDev& env, uint32_t seed, uint32_t pixel, int32_t p, int32_t j, const EnvVertex& x,
                                            VertexDraw& s) {
    const uint32_t dim = 8u * (uint32_t)(j + 1);
    const float alpha = vertex_alpha(x), ngv = dot3(x.ng, x.v);
    if (j >= 1) {
        int r, c;
        const float pl = env_sample(env, env_rand(seed, pixel, p, dim + 3u), env_rand(seed, pixel, p, dim + 4u), r, c, s.wl);
        const float* L = env.image + 3 * ((int64_t)r * env.We + c);
        s.Ll[0] = L[0]; s.Ll[1] = L[1]; s.Ll[2] = L[2];
        s.dl = pl + brdf_pdf(x.n, x.v, s.wl, alpha);
        s.lcounts = dir_counts(x.n, x.ng, ngv, s.wl);
    }
    const bool ok = brdf_sample(x.n, x.v, alpha, env_rand(seed, pixel, p, dim), env_rand(seed, pixel, p, dim + 1u),
                                env_rand(seed, pixel, p, dim + 2u), s.wb);
    if (!ok) s.wb = make_float3(0.f, 0.f, 0.f);
    s.bcounts = ok && dir_counts(x.n, x.ng, ngv, s.wb);
    if (s.bcounts) {
        const float pl = env_eval(env, s.wb, s.Lb);
        s.pb = brdf_pdf(x.n, x.v, s.wb, alpha);
        s.db = pl + s.pb;
    }
}

// the two lobes of a direct sample
__device__ __forceinline__ void direct_terms(const float L[3], const PlasticOut& f, float denom, float cd[3], float cs[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cd[c] = L[c] * f.diffuse[c] / denom;  // an infinite density (the map's poles) gives 0
        cs[c] = L[c] * f.specular[c] / denom;
    }
}

// what a path of throughput T gathers at a vertex from its environment sample ...
__device__ __forceinline__ void light_term(const float T[3], const float L[3], const PlasticOut& f, float dl, float lt[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lt[c] = (T[c] * L[c]) * (f.diffuse[c] + f.specular[c]) / dl;  // an infinite density gives 0
}

// ... and through its BRDF sample when that escapes: the same estimator over the other denominator
__device__ __forceinline__ void escape_term(const float T[3], const float L[3], const PlasticOut& f, float db, float et[3]) {
    light_term(T, L, f, db, et);
}

// is y, met along w_b, the path's next vertex?  A surface met from behind is black, like a back-facing primary hit
__device__ __forceinline__ bool path_goes_on(const EnvVertex& y, float3 wb, float pb) { return -dot3(y.ng, wb) > 0.0f && pb > 0.0f; }

// the step to the next vertex: the primary's two lobe weights f_d / p_brdf and f_s / p_brdf stay apart (they multiply what the path
// gathered when it ends); after it T, the throughput past the primary, takes (f_d + f_s) / p_brdf
__device__ __forceinline__ void advance(int32_t j, const PlasticOut& f, float pb, float T[3], float bd[3], float bs[3]) {
    if (j == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bd[c] = f.diffuse[c] / pb;
            bs[c] = f.specular[c] / pb;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[c] = T[c] * (f.diffuse[c] + f.specular[c]) / pb;
    }
}

__device__ __forceinline__ void add3(float acc[3], const float t[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += t[c];
}

// The pixel reduction: kEnvGroup lanes work one pixel, item k (a sample, a path) on lane k % kEnvGroup in round k / kEnvGroup;
// every lane adds its rounds in order and a fixed butterfly adds the lanes.  The order is part of the contract.
template <class Body>
__device__ __forceinline__ void for_each_of_pixel(int32_t n, int sl, Body body) {
    for (int32_t base = 0; base < n; base += kEnvGroup) {
        const int32_t k = base + sl;
        if (k >= n) break;  // the ragged tail of the last round
        body(k);
    }
}

__device__ __forceinline__ void group_sum16(float accd[3], float accs[3]) {
#pragma unroll
    for (int m = kEnvGroup / 2; m > 0; m >>= 1)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            accd[c] += __shfl_xor(accd[c], m, kEnvGroup);
            accs[c] += __shfl_xor(accs[c], m, kEnvGroup);
        }
}

__device__ __forceinline__ void store_direct_dump(const iron_env_dump& dump, int64_t at, const DirectDraw& q, bool vis, const float cd[3],
                                                  const float cs[3]) {
    st3(dump.dir, at, q.w.x, q.w.y, q.w.z);
    if (dump.denom) dump.denom[at] = q.denom;
    if (dump.vis) dump.vis[at] = vis ? 1 : 0;
    st3(dump.contrib, at, cd[0] + cs[0], cd[1] + cs[1], cd[2] + cs[2]);
}

// what both scenes' path dumps record of vertex j (iron_env_path_dump, iron_neural_path_dump: the fields of the same name)
template <class Dump>
__device__ __forceinline__ void store_vertex_dump(const Dump& dump, int64_t at, const VertexDraw& q, float3 org, bool lvis, const float lt[3],
                                                  const float et[3], const float tp[3]) {
    st3(dump.bounce_dir, at, q.wb.x, q.wb.y, q.wb.z);
    st3(dump.bounce_org, at, org.x, org.y, org.z);
    st3(dump.light_dir, at, q.wl.x, q.wl.y, q.wl.z);
    if (dump.light_vis) dump.light_vis[at] = lvis ? 1 : 0;
    if (dump.denom_light) dump.denom_light[at] = q.dl;
    if (dump.denom_brdf) dump.denom_brdf[at] = q.db;
    st3(dump.light_term, at, lt[0], lt[1], lt[2]);
    st3(dump.escape_term, at, et[0], et[1], et[2]);
    st3(dump.throughput, at, tp[0], tp[1], tp[2]);
}

// ---- the mesh ----
__device__ __forceinline__ void mesh_vertex(const iron_asset_mesh& m, const SurfHit& s, EnvVertex& x) {
    x.pt = s.pt; x.n = s.nrm;
    x.ng = asset_face_normal(m, s);
    x.v = make_float3(-s.d.x, -s.d.y, -s.d.z);
#pragma unroll
    for (int c = 0; c < 7; ++c) x.mat[c] = s.mat[c];
}

// V(w) for a direction that counts at x: the shadow ray from x meets no face other than x's own
__device__ __forceinline__ bool mesh_unoccluded(const float4* __restrict__ nodes, const float4* __restrict__ tris, int64_t nf,
                                                const EnvVertex& x, int32_t face, float3 w, float off, int32_t (*stack)[kBvQueryBlock],
                                                int lane) {
    const float3 org = leave_origin(x.pt, x.ng, dot3(x.ng, w), off);
    if (!ray_valid(org, w)) return false;
    RayPre r;
    ray_setup(org, w, r);
    return !bvh_any_hit(nodes, tris, nf, r, 0.0f, kInfF, face, stack, lane);
}

__global__ __launch_bounds__(kBvQueryBlock) void k_shade_env(EnvShadeArgs a) {
    __shared__ int32_t stack[kBvStack][kBvQueryBlock];
    const int lane = threadIdx.x, sl = lane % kEnvGroup;
    const int64_t i = (int64_t)blockIdx.x * kEnvPixels + lane / kEnvGroup;
    if (i >= a.n) return;  // a whole group leaves together
    SurfHit s;
    asset_surface(a.m, a.face_idx, a.t, a.ray_o, a.ray_d, a.bary, i, s);
    EnvVertex x;
    mesh_vertex(a.m, s, x);
    const int32_t N = a.n_light + a.n_brdf;
    const uint32_t pixel = a.pixel_idx ? (uint32_t)a.pixel_idx[i] : (uint32_t)i;
    const float off = a.shadow_eps * bvh_diagonal(a.nodes, a.tris, a.m.n_faces);
    float accd[3] = {0.f, 0.f, 0.f}, accs[3] = {0.f, 0.f, 0.f};
    for_each_of_pixel(N, sl, [&](int32_t k) {
        DirectDraw q;
        float cd[3] = {0.f, 0.f, 0.f}, cs[3] = {0.f, 0.f, 0.f};
        bool vis = false;
        if (s.hit) {
            draw_direct(a.env, a.seed, pixel, k, a.n_light, a.n_brdf, x, q);
            // the shadow ray is cast, and its answer dumped, whatever the denominator
            vis = q.counts && mesh_unoccluded(a.nodes, a.tris, a.m.n_faces, x, (int32_t)s.face, q.w, off, stack, lane);
            if (vis && q.denom > 0.0f) {
                PlasticOut f;
                vertex_brdf(x, q.w, a.tab_trans, a.tab_diff, f);
                direct_terms(q.L, f, q.denom, cd, cs);
                add3(accd, cd);
                add3(accs, cs);
            }
        }
        store_direct_dump(a.dump, i * N + k, q, vis, cd, cs);
    });
    group_sum16(accd, accs);
    if (sl != 0) return;
    st3(a.o.color, i, accd[0] + accs[0], accd[1] + accs[1], accd[2] + accs[2]);
    st3(a.o.diffuse_color, i, accd[0], accd[1], accd[2]);
    st3(a.o.specular_color, i, accs[0], accs[1], accs[2]);
    asset_store_maps(a.o, i, s);
}

// ---- the path integrator ----
struct EnvPathArgs {
    iron_asset_mesh m;
    iron_env_path_dump dump;
    EnvDev env;
    const float4 *nodes, *tris;
    const float *tab_trans, *tab_diff, *ray_o, *ray_d, *t, *bary;
    const int32_t *face_idx, *pixel_idx;
    float *indirect_diffuse, *indirect_specular;
    int64_t n;
    int32_t n_paths, max_depth;
    uint32_t seed;
    float shadow_eps;
};

// A path in a sample's place in the pixel reduction; C is what the path gathered.  Every vertex runs the same code, the last one
// included (its closest hit decides between the escape term and nothing), so the first D' vertices of a path do not depend on
// max_depth.
__global__ __launch_bounds__(kBvQueryBlock) void k_shade_env_indirect(EnvPathArgs a) {
    __shared__ int32_t stack[kBvStack][kBvQueryBlock];
    const int lane = threadIdx.x, sl = lane % kEnvGroup;
    const int64_t i = (int64_t)blockIdx.x * kEnvPixels + lane / kEnvGroup;
    if (i >= a.n) return;  // a whole group leaves together
    const uint32_t pixel = a.pixel_idx ? (uint32_t)a.pixel_idx[i] : (uint32_t)i;
    const float off = a.shadow_eps * bvh_diagonal(a.nodes, a.tris, a.m.n_faces);
    const int32_t D = a.max_depth;
    SurfHit s0;
    asset_surface(a.m, a.face_idx, a.t, a.ray_o, a.ray_d, a.bary, i, s0);
    EnvVertex x0;
    mesh_vertex(a.m, s0, x0);
    float accd[3] = {0.f, 0.f, 0.f}, accs[3] = {0.f, 0.f, 0.f};
    for_each_of_pixel(a.n_paths, sl, [&](int32_t p) {
        EnvVertex x = x0;
        int32_t face = (int32_t)s0.face;
        float T[3] = {1.f, 1.f, 1.f}, C[3] = {0.f, 0.f, 0.f}, bd[3] = {0.f, 0.f, 0.f}, bs[3] = {0.f, 0.f, 0.f};
        bool alive = s0.hit;
        for (int32_t j = 0; j < D; ++j) {
            VertexDraw q;
            float3 org = make_float3(0.f, 0.f, 0.f);
            float th = 0.0f, lt[3] = {0.f, 0.f, 0.f}, et[3] = {0.f, 0.f, 0.f}, tp[3] = {0.f, 0.f, 0.f};
            bool lvis = false;
            int32_t reached = -2;
            if (alive) {
                alive = false;  // until the vertex hands the path on
                draw_vertex(a.env, a.seed, pixel, p, j, x, q);
                lvis = q.lcounts && mesh_unoccluded(a.nodes, a.tris, a.m.n_faces, x, face, q.wl, off, stack, lane);
                if (lvis && q.dl > 0.0f) {
                    PlasticOut f;
                    vertex_brdf(x, q.wl, a.tab_trans, a.tab_diff, f);
                    light_term(T, q.Ll, f, q.dl, lt);
                    add3(C, lt);
                }
                if (q.bcounts) {
                    org = leave_origin(x.pt, x.ng, dot3(x.ng, q.wb), off);
                    if (ray_valid(org, q.wb)) {
                        RayPre r;
                        ray_setup(org, q.wb, r);
                        RayHit h = ray_hit_none(kInfF);
                        bvh_closest_hit(a.nodes, a.tris, a.m.n_faces, r, 0.0f, face, stack, lane, h);
                        const bool hit = h.face != kNoFace;
                        if (hit) refine_bary(a.tris, org, q.wb, h);
                        reached = hit ? h.face : -1;
                        th = hit ? h.t : kInfF;
                        PlasticOut f;
                        vertex_brdf(x, q.wb, a.tab_trans, a.tab_diff, f);
                        if (!hit) {
                            if (j >= 1 && q.db > 0.0f) {  // the environment through the BRDF sample; the primary's is direct light
                                escape_term(T, q.Lb, f, q.db, et);
                                add3(C, et);
                            }
                        } else {
                            SurfHit s;
                            asset_surface_at(a.m, h.face, h.t, org, q.wb, h.b1, h.b2, s);
                            EnvVertex y;
                            mesh_vertex(a.m, s, y);
                            if (s.hit && path_goes_on(y, q.wb, q.pb)) {
                                advance(j, f, q.pb, T, bd, bs);
#pragma unroll
                                for (int c = 0; c < 3; ++c) tp[c] = T[c];
                                x = y;
                                face = (int32_t)s.face;
                                alive = true;
                            }
                        }
                    }
                }
            }
            const int64_t at = ((int64_t)i * a.n_paths + p) * D + j;
            store_vertex_dump(a.dump, at, q, org, lvis, lt, et, tp);
            if (a.dump.face) a.dump.face[at] = reached;
            if (a.dump.t) a.dump.t[at] = th;
        }
        st3(a.dump.lobe_diffuse, (int64_t)i * a.n_paths + p, bd[0], bd[1], bd[2]);
        st3(a.dump.lobe_specular, (int64_t)i * a.n_paths + p, bs[0], bs[1], bs[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            accd[c] += bd[c] * C[c];
            accs[c] += bs[c] * C[c];
        }
    });
    group_sum16(accd, accs);
    if (sl != 0) return;
    const float np = (float)a.n_paths;
    st3(a.indirect_diffuse, i, accd[0] / np, accd[1] / np, accd[2] / np);
    st3(a.indirect_specular, i, accs[0] / np, accs[1] / np, accs[2] / np);
}

// ---- the neural scene ----
// The direct estimator on a G-buffer of the neural scene (iron_amd/neural_relight.py), its shadow rays answered by the sphere
// tracer (iron_trace_occluded) instead of a BVH walk, in three steps on one stream:
//   k_nenv_emit     draws every sample of the pixel reduction; its direction goes to a dense [pixels, N, 3] array and a 0/1 flag
//                   -- the sample counts and its denominator is > 0 -- to level 0 of a pair_scan; k_nenv_compact then lists the
//                   flagged samples' rays in ascending (pixel, sample) order;
//   (the caller)    intersect_sphere and iron_trace_occluded on the list;
//   k_nenv_scatter  the answers back to a [pixels, N] byte array of visibilities, and k_nenv_resolve draws every sample again
//                   from the hash and adds the visible ones' terms.
// There is no geometric normal: a vertex carries the shading normal in its place, so a sample counts when n.w > 0, n.v > 0 and w is
// finite.  A block of pixels [p0, p0 + nb) is worked per call; nothing a pixel gets depends on the block it is in.
struct NeuralEnvArgs {
    iron_neural_gbuffer g;
    iron_env_dump dump;
    EnvDev env;
    const float *tab_trans, *tab_diff;
    int64_t p0, nb;          // the block of pixels
    int32_t n_light, n_brdf;
    uint32_t seed;
    float shadow_eps;
    Pair64* flags;           // [nb N] (emit)
    float* dir;              // [nb N, 3] (emit)
    const uint8_t* vis;      // [nb N] (resolve)
    float *color, *diffuse_color, *specular_color;
};

struct NeuralEnvLayout {
    ScanLevels scan;
    size_t dir_off, vis_off, bytes;
};

inline NeuralEnvLayout nenv_layout(int64_t n_samples) {
    NeuralEnvLayout L{};
    Carver c;
    L.scan = scan_levels(n_samples, c);
    L.dir_off = c.take(sizeof(float) * 3 * (size_t)n_samples);
    L.vis_off = c.take((size_t)n_samples);
    L.bytes = c.off;
    return L;
}

// pixel i of the G-buffer as a vertex (zeros on a miss); true on a hit
__device__ __forceinline__ bool gbuffer_vertex(const iron_neural_gbuffer& g, int64_t i, EnvVertex& x) {
    vertex_clear(x);
    if (g.hit[i] == 0) return false;
    x.pt = ld3(g.points, i);
    x.n = x.ng = ld3(g.normal, i);
    const float3 d = ld3(g.ray_d, i);
    x.v = make_float3(-d.x, -d.y, -d.z);
#pragma unroll
    for (int c = 0; c < 3; ++c) { x.mat[c] = g.diffuse_albedo[3 * i + c]; x.mat[3 + c] = g.specular_albedo[3 * i + c]; }
    x.mat[6] = g.specular_roughness[i];
    return true;
}

__device__ __forceinline__ uint32_t gbuffer_pixel(const iron_neural_gbuffer& g, int64_t i) {
    return g.pixel_idx ? (uint32_t)g.pixel_idx[i] : (uint32_t)i;
}

__global__ __launch_bounds__(kBvQueryBlock) void k_nenv_emit(NeuralEnvArgs a) {
    const int lane = threadIdx.x, sl = lane % kEnvGroup;
    const int64_t j = (int64_t)blockIdx.x * kEnvPixels + lane / kEnvGroup;   // the pixel's place in the block
    if (j >= a.nb) return;
    EnvVertex x;
    const bool hit = gbuffer_vertex(a.g, a.p0 + j, x);
    const uint32_t pixel = gbuffer_pixel(a.g, a.p0 + j);
    const int32_t N = a.n_light + a.n_brdf;
    for_each_of_pixel(N, sl, [&](int32_t k) {
        DirectDraw q;
        if (hit) draw_direct(a.env, a.seed, pixel, k, a.n_light, a.n_brdf, x, q);
        const int64_t at = j * N + k;
        st3(a.dir, at, q.w.x, q.w.y, q.w.z);
        a.flags[at] = Pair64{q.counts && q.denom > 0.0f ? 1 : 0, 0};
    });
}

// the flagged samples' shadow rays, in the order of their flags: origin offset_origin, direction w.  count[0] = their number.
__global__ __launch_bounds__(256) void k_nenv_compact(NeuralEnvArgs a, const Pair64* __restrict__ prefix, const Pair64* __restrict__ total,
                                                      int64_t capacity, float* __restrict__ ray_o, float* __restrict__ ray_d,
                                                      int32_t* __restrict__ sample_idx, int64_t* __restrict__ count) {
    const int32_t N = a.n_light + a.n_brdf;
    const int64_t M = a.nb * N, at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at == 0) count[0] = total[0].a;
    if (at >= M) return;
    const int64_t pos = prefix[at].a, next = at + 1 < M ? prefix[at + 1].a : total[0].a;
    if (next == pos || pos >= capacity) return;   // not flagged (the capacity holds every sample: the second test never fires)
    const int64_t i = a.p0 + at / N;
    const float3 org = offset_origin(ld3(a.g.points, i), ld3(a.g.normal, i), a.shadow_eps), w = ld3(a.dir, at);
    st3(ray_o, pos, org.x, org.y, org.z);
    st3(ray_d, pos, w.x, w.y, w.z);
    sample_idx[pos] = (int32_t)at;
}

__global__ __launch_bounds__(256) void k_nenv_scatter(const uint8_t* __restrict__ occluded, const int32_t* __restrict__ sample_idx,
                                                      int64_t n_rays, int64_t M, uint8_t* __restrict__ vis) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rays) return;
    const int64_t at = sample_idx[q];
    if (at >= 0 && at < M) vis[at] = occluded[q] ? 0 : 1;
}

__global__ __launch_bounds__(kBvQueryBlock) void k_nenv_resolve(NeuralEnvArgs a) {
    const int lane = threadIdx.x, sl = lane % kEnvGroup;
    const int64_t j = (int64_t)blockIdx.x * kEnvPixels + lane / kEnvGroup;
    if (j >= a.nb) return;  // a whole group leaves together
    const int64_t i = a.p0 + j;
    EnvVertex x;
    const bool hit = gbuffer_vertex(a.g, i, x);
    const uint32_t pixel = gbuffer_pixel(a.g, i);
    const int32_t N = a.n_light + a.n_brdf;
    float accd[3] = {0.f, 0.f, 0.f}, accs[3] = {0.f, 0.f, 0.f};
    for_each_of_pixel(N, sl, [&](int32_t k) {
        DirectDraw q;
        float cd[3] = {0.f, 0.f, 0.f}, cs[3] = {0.f, 0.f, 0.f};
        bool vis = false;
        if (hit) {
            draw_direct(a.env, a.seed, pixel, k, a.n_light, a.n_brdf, x, q);
            vis = q.counts && q.denom > 0.0f && a.vis[j * N + k] != 0;  // a listed sample that the tracer found unoccluded
            if (vis) {
                PlasticOut f;
                vertex_brdf(x, q.w, a.tab_trans, a.tab_diff, f);
                direct_terms(q.L, f, q.denom, cd, cs);
                add3(accd, cd);
                add3(accs, cs);
            }
        }
        store_direct_dump(a.dump, i * N + k, q, vis, cd, cs);
    });
    group_sum16(accd, accs);
    if (sl != 0) return;
    st3(a.color, i, accd[0] + accs[0], accd[1] + accs[1], accd[2] + accs[2]);
    st3(a.diffuse_color, i, accd[0], accd[1], accd[2]);
    st3(a.specular_color, i, accs[0], accs[1], accs[2]);
}

// ---- interreflections on the neural scene ----
// The path estimator on the neural scene, as a wavefront over depth: a path's closest hit is the sphere tracer's, which is a call
// of its own, so a path's state lives in a workspace between two tracer calls.  Per block of pixels [p0, p0 + nb), slot
// s = (pixel - p0) n_paths + path, on one stream:
//   k_npath_begin    the state of every slot from the G-buffer: alive, the vertex (x, n, v, the seven material channels), T = 1,
//                    C = b_d = b_s = 0;
//   k_npath_emit     depth j: per alive slot the two samples of draw_vertex; their directions to the workspace, the two flags --
//                    the light sample counts with dl > 0; the BRDF sample counts and its ray is valid -- to level 0 of one
//                    pair_scan (Pair64 carries both); k_npath_compact then lists the shadow rays and the bounce rays (origin
//                    offset_origin for both, direction, slot) in ascending slot order;
//   (the caller)     intersect_sphere with occluded on the shadow list, with forward(chunk = 1) and the surface record on the
//                    bounce list;
//   k_npath_resolve  depth j: draws both samples again, adds the visible light term and the escape term to C, forms the next vertex
//                    and T (b_d, b_s at j = 0) or ends the path, writes the dumps.  A slot finds its rays' answers through the
//                    scan's prefixes, which stay in the workspace;
//   k_npath_finish   the pixel's sums of b_d C and b_s C by the pixel reduction, one division by n_paths.
constexpr int kPathState = 28;  // floats per slot: x 0-2, n 3-5, v 6-8, material 9-15, T 16-18, C 19-21, b_d 22-24, b_s 25-27
constexpr int kPathBlock = 256;

struct NeuralPathLayout {
    ScanLevels scan;
    size_t state_off, dir_off, alive_off, cast_off, bytes;
};

inline NeuralPathLayout npath_layout(int64_t capacity) {
    NeuralPathLayout L{};
    Carver c;
    L.scan = scan_levels(capacity, c);
    L.state_off = c.take(sizeof(float) * kPathState * (size_t)capacity);
    L.dir_off = c.take(sizeof(float) * 6 * (size_t)capacity);
    L.alive_off = c.take((size_t)capacity);
    L.cast_off = c.take((size_t)capacity);
    L.bytes = c.off;
    return L;
}

struct NeuralPathArgs {
    iron_neural_gbuffer g;
    iron_neural_path_dump dump;
    EnvDev env;
    const float *tab_trans, *tab_diff;
    int64_t p0, nb, capacity;
    int32_t n_paths, max_depth, depth;
    uint32_t seed;
    float shadow_eps;
    float* state;    // [kPathState][capacity]
    float* dir;      // [capacity, 6]: w_l, w_b of the depth under way
    uint8_t* alive;  // [capacity]
    uint8_t* cast;   // [capacity]: bit 0 a shadow ray is listed, bit 1 a bounce ray
    Pair64* flags;   // level 0 of the scan: the flags (emit), then their exclusive prefixes
    // the caller's answers (resolve)
    const uint8_t *occluded, *bounce_hit;
    const float *bounce_dist, *bounce_points, *bounce_normal, *bounce_kd, *bounce_ks, *bounce_rough;
    int64_t n_shadow, n_bounce;
    float *indirect_diffuse, *indirect_specular;  // finish
};

__device__ __forceinline__ float3 npath_ld3(const float* __restrict__ state, int64_t cap, int f, int64_t s) {
    return make_float3(state[(int64_t)f * cap + s], state[(int64_t)(f + 1) * cap + s], state[(int64_t)(f + 2) * cap + s]);
}
__device__ __forceinline__ void npath_st3(float* __restrict__ state, int64_t cap, int f, int64_t s, float a, float b, float c) {
    state[(int64_t)f * cap + s] = a; state[(int64_t)(f + 1) * cap + s] = b; state[(int64_t)(f + 2) * cap + s] = c;
}
__device__ __forceinline__ void npath_load_vertex(const float* __restrict__ state, int64_t cap, int64_t s, EnvVertex& x) {
    x.pt = npath_ld3(state, cap, 0, s); x.n = x.ng = npath_ld3(state, cap, 3, s); x.v = npath_ld3(state, cap, 6, s);
#pragma unroll
    for (int c = 0; c < 7; ++c) x.mat[c] = state[(int64_t)(9 + c) * cap + s];
}
__device__ __forceinline__ void npath_store_vertex(float* __restrict__ state, int64_t cap, int64_t s, const EnvVertex& x) {
    npath_st3(state, cap, 0, s, x.pt.x, x.pt.y, x.pt.z);
    npath_st3(state, cap, 3, s, x.n.x, x.n.y, x.n.z);
    npath_st3(state, cap, 6, s, x.v.x, x.v.y, x.v.z);
#pragma unroll
    for (int c = 0; c < 7; ++c) state[(int64_t)(9 + c) * cap + s] = x.mat[c];
}

__global__ __launch_bounds__(kPathBlock) void k_npath_begin(NeuralPathArgs a) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.nb * a.n_paths) return;
    EnvVertex x;
    const bool hit = gbuffer_vertex(a.g, a.p0 + s / a.n_paths, x);
    npath_store_vertex(a.state, a.capacity, s, x);
    npath_st3(a.state, a.capacity, 16, s, 1.f, 1.f, 1.f);
    npath_st3(a.state, a.capacity, 19, s, 0.f, 0.f, 0.f);
    npath_st3(a.state, a.capacity, 22, s, 0.f, 0.f, 0.f);
    npath_st3(a.state, a.capacity, 25, s, 0.f, 0.f, 0.f);
    a.alive[s] = hit ? 1 : 0;
}

// counts[2] += the alive slots (one atomic per wave: integer, so the order does not matter)
__global__ __launch_bounds__(kPathBlock) void k_npath_emit(NeuralPathArgs a, unsigned long long* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = s < a.nb * a.n_paths;
    const bool alive = in && a.alive[s] != 0;
    VertexDraw q;
    bool lcast = false, bcast = false;  // a shadow ray / a bounce ray is cast
    if (alive) {
        EnvVertex x;
        npath_load_vertex(a.state, a.capacity, s, x);
        draw_vertex(a.env, a.seed, gbuffer_pixel(a.g, a.p0 + s / a.n_paths), (int32_t)(s % a.n_paths), a.depth, x, q);
        lcast = q.lcounts && q.dl > 0.0f;
        bcast = q.bcounts && ray_valid(offset_origin(x.pt, x.n, a.shadow_eps), q.wb);
    }
    if (in) {
        float* d = a.dir + 6 * s;
        d[0] = q.wl.x; d[1] = q.wl.y; d[2] = q.wl.z; d[3] = q.wb.x; d[4] = q.wb.y; d[5] = q.wb.z;
        a.flags[s] = Pair64{lcast ? 1 : 0, bcast ? 1 : 0};
        a.cast[s] = (uint8_t)((lcast ? 1 : 0) | (bcast ? 2 : 0));
    }
    const unsigned long long wave = __ballot(alive);
    if ((threadIdx.x & (warpSize - 1)) == 0 && wave != 0) atomicAdd(counts + 2, (unsigned long long)__popcll(wave));
}

__global__ __launch_bounds__(kPathBlock) void k_npath_compact(NeuralPathArgs a, const Pair64* __restrict__ prefix, const Pair64* __restrict__ total,
                                                              float* __restrict__ shadow_o, float* __restrict__ shadow_d,
                                                              int32_t* __restrict__ shadow_idx, float* __restrict__ bounce_o,
                                                              float* __restrict__ bounce_d, int32_t* __restrict__ bounce_idx,
                                                              unsigned long long* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) { counts[0] = (unsigned long long)total[0].a; counts[1] = (unsigned long long)total[0].b; }
    if (s >= a.nb * a.n_paths) return;
    const uint8_t cast = a.cast[s];
    if (cast == 0) return;
    const float3 org = offset_origin(npath_ld3(a.state, a.capacity, 0, s), npath_ld3(a.state, a.capacity, 3, s), a.shadow_eps);
    const float* d = a.dir + 6 * s;
    const Pair64 at = prefix[s];
    if ((cast & 1) && at.a < a.capacity) {
        st3(shadow_o, at.a, org.x, org.y, org.z);
        st3(shadow_d, at.a, d[0], d[1], d[2]);
        shadow_idx[at.a] = (int32_t)s;
    }
    if ((cast & 2) && at.b < a.capacity) {
        st3(bounce_o, at.b, org.x, org.y, org.z);
        st3(bounce_d, at.b, d[3], d[4], d[5]);
        bounce_idx[at.b] = (int32_t)s;
    }
}

__global__ __launch_bounds__(kPathBlock) void k_npath_resolve(NeuralPathArgs a) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.nb * a.n_paths) return;
    const int64_t i = a.p0 + s / a.n_paths;
    const int32_t p = (int32_t)(s % a.n_paths), j = a.depth;
    const int64_t cap = a.capacity;
    VertexDraw q;
    EnvVertex y;  // the surface the bounce ray met
    vertex_clear(y);
    float3 org = make_float3(0.f, 0.f, 0.f);
    float th = 0.0f, lt[3] = {0.f, 0.f, 0.f}, et[3] = {0.f, 0.f, 0.f}, tp[3] = {0.f, 0.f, 0.f};
    bool lvis = false;
    int32_t reached = -2;
    if (a.alive[s] != 0) {
        bool alive = false;  // until the vertex hands the path on
        EnvVertex x;
        npath_load_vertex(a.state, cap, s, x);
        const float3 Ts = npath_ld3(a.state, cap, 16, s), Cs = npath_ld3(a.state, cap, 19, s);
        float T[3] = {Ts.x, Ts.y, Ts.z}, C[3] = {Cs.x, Cs.y, Cs.z};
        draw_vertex(a.env, a.seed, gbuffer_pixel(a.g, i), p, j, x, q);
        const uint8_t cast = a.cast[s];
        const Pair64 at = a.flags[s];
        if ((cast & 1) && at.a < a.n_shadow) {  // the environment sample: listed means it counts and dl > 0
            lvis = a.occluded[at.a] == 0;
            if (lvis) {
                PlasticOut f;
                vertex_brdf(x, q.wl, a.tab_trans, a.tab_diff, f);
                light_term(T, q.Ll, f, q.dl, lt);
                add3(C, lt);
            }
        }
        if ((cast & 2) && at.b < a.n_bounce) {  // the BRDF sample and its ray
            org = offset_origin(x.pt, x.n, a.shadow_eps);
            const bool hit = a.bounce_hit[at.b] != 0;
            reached = hit ? 1 : -1;
            th = hit ? a.bounce_dist[at.b] : kInfF;
            PlasticOut f;
            vertex_brdf(x, q.wb, a.tab_trans, a.tab_diff, f);
            if (!hit) {
                if (j >= 1 && q.db > 0.0f) {  // the environment through the BRDF sample; the primary's is direct light
                    escape_term(T, q.Lb, f, q.db, et);
                    add3(C, et);
                }
            } else {
                y.pt = ld3(a.bounce_points, at.b);
                y.n = y.ng = ld3(a.bounce_normal, at.b);
                y.v = make_float3(-q.wb.x, -q.wb.y, -q.wb.z);
#pragma unroll
                for (int c = 0; c < 3; ++c) { y.mat[c] = a.bounce_kd[3 * at.b + c]; y.mat[3 + c] = a.bounce_ks[3 * at.b + c]; }
                y.mat[6] = a.bounce_rough[at.b];
                if (path_goes_on(y, q.wb, q.pb)) {
                    float bd[3] = {0.f, 0.f, 0.f}, bs[3] = {0.f, 0.f, 0.f};
                    advance(j, f, q.pb, T, bd, bs);
                    if (j == 0) {
                        npath_st3(a.state, cap, 22, s, bd[0], bd[1], bd[2]);
                        npath_st3(a.state, cap, 25, s, bs[0], bs[1], bs[2]);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) tp[c] = T[c];
                    npath_store_vertex(a.state, cap, s, y);
                    npath_st3(a.state, cap, 16, s, T[0], T[1], T[2]);
                    alive = true;
                }
            }
        }
        npath_st3(a.state, cap, 19, s, C[0], C[1], C[2]);
        a.alive[s] = alive ? 1 : 0;
    }
    const int64_t at = ((int64_t)i * a.n_paths + p) * a.max_depth + j;
    store_vertex_dump(a.dump, at, q, org, lvis, lt, et, tp);
    if (a.dump.reached) a.dump.reached[at] = reached;
    if (a.dump.distance) a.dump.distance[at] = th;
    st3(a.dump.vertex_points, at, y.pt.x, y.pt.y, y.pt.z);
    st3(a.dump.vertex_normal, at, y.n.x, y.n.y, y.n.z);
    st3(a.dump.vertex_diffuse_albedo, at, y.mat[0], y.mat[1], y.mat[2]);
    st3(a.dump.vertex_specular_albedo, at, y.mat[3], y.mat[4], y.mat[5]);
    if (a.dump.vertex_roughness) a.dump.vertex_roughness[at] = y.mat[6];
}

__global__ __launch_bounds__(kBvQueryBlock) void k_npath_finish(NeuralPathArgs a) {
    const int lane = threadIdx.x, sl = lane % kEnvGroup;
    const int64_t k = (int64_t)blockIdx.x * kEnvPixels + lane / kEnvGroup;  // the pixel's place in the block
    if (k >= a.nb) return;  // a whole group leaves together
    const int64_t i = a.p0 + k, cap = a.capacity;
    float accd[3] = {0.f, 0.f, 0.f}, accs[3] = {0.f, 0.f, 0.f};
    for_each_of_pixel(a.n_paths, sl, [&](int32_t p) {
        const int64_t s = k * a.n_paths + p;
        const float3 C = npath_ld3(a.state, cap, 19, s), bd = npath_ld3(a.state, cap, 22, s), bs = npath_ld3(a.state, cap, 25, s);
        const float Cv[3] = {C.x, C.y, C.z}, bdv[3] = {bd.x, bd.y, bd.z}, bsv[3] = {bs.x, bs.y, bs.z};
        st3(a.dump.lobe_diffuse, i * a.n_paths + p, bdv[0], bdv[1], bdv[2]);
        st3(a.dump.lobe_specular, i * a.n_paths + p, bsv[0], bsv[1], bsv[2]);
        st3(a.dump.path_value, i * a.n_paths + p, (bdv[0] + bsv[0]) * Cv[0], (bdv[1] + bsv[1]) * Cv[1], (bdv[2] + bsv[2]) * Cv[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            accd[c] += bdv[c] * Cv[c];
            accs[c] += bsv[c] * Cv[c];
        }
    });
    group_sum16(accd, accs);
    if (sl != 0) return;
    const float np = (float)a.n_paths;
    st3(a.indirect_diffuse, i, accd[0] / np, accd[1] / np, accd[2] / np);
    st3(a.indirect_specular, i, accs[0] / np, accs[1] / np, accs[2] / np);
}

static bool env_dev(const iron_envmap* env, EnvDev& E) {
    if (!env || !env->image || !env->dist || env->h <= 0 || env->w <= 0 || (int64_t)env->h * env->w > (1 << 24)) return false;
    const EnvLayout L = env_layout(env->h, env->w);
    E.image = env->image;
    E.total = ws_ptr<double>(env->dist, L.total_off);
    E.mcdf = ws_ptr<double>(env->dist, L.mcdf_off);
    E.rowcdf = ws_ptr<double>(env->dist, L.rowcdf_off);
    E.ptex = ws_ptr<float>(env->dist, L.ptex_off);
    E.He = env->h; E.We = env->w;
    for (int k = 0; k < 9; ++k) E.R[k] = env->to_world[k];
    return true;
}

static bool asset_mesh_ok(const iron_asset_mesh* mesh) {
    if (!mesh) return false;
    if (mesh->n_faces <= 0 || mesh->n_faces >= 0x7fffffffLL || mesh->n_verts <= 0 || mesh->n_uvs <= 0 || mesh->tex_h <= 0 || mesh->tex_w <= 0 ||
        (int64_t)mesh->tex_h * mesh->tex_w > (1 << 24))
        return false;
    return mesh->verts && mesh->faces && mesh->uvs && mesh->face_uvs && mesh->material;
}

static bool shadow_eps_ok(float e) { return e >= 0.0f && e < kInfF; }  // NaN fails

}  // namespace iron

using namespace iron;

extern "C" int iron_mesh_occluded(const void* workspace, int64_t n_faces, const float* ray_o, const float* ray_d, int64_t n_rays, float t_min,
                                  float t_max, const int32_t* skip_face, uint8_t* occluded, void* stream) {
    if (n_faces <= 0 || n_faces >= 0x7fffffffLL || n_rays < 0 || !workspace) return IRON_ERR_BAD_ARG;
    if (n_rays == 0) return IRON_OK;
    if (!ray_o || !ray_d || !occluded) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(n_faces);
    IRON_LAUNCH(k_occluded, blocks_for(n_rays, kBvQueryBlock), kBvQueryBlock, (hipStream_t)stream, ws_ptr<float4>(workspace, L.nodes_off),
                ws_ptr<float4>(workspace, L.tris_off), n_faces, ray_o, ray_d, n_rays, t_min, t_max, skip_face, occluded);
    return IRON_OK;
}

extern "C" int iron_envmap_workspace_bytes(int32_t h, int32_t w, size_t* bytes) {
    if (!bytes || h <= 0 || w <= 0 || (int64_t)h * w > (1 << 24)) return IRON_ERR_BAD_ARG;
    *bytes = env_layout(h, w).bytes;
    return IRON_OK;
}

extern "C" int iron_envmap_build(const float* image, int32_t h, int32_t w, void* workspace, void* stream) {
    if (!image || !workspace || h <= 0 || w <= 0 || (int64_t)h * w > (1 << 24)) return IRON_ERR_BAD_ARG;
    const EnvLayout L = env_layout(h, w);
    hipStream_t st = (hipStream_t)stream;
    double* rowcdf = ws_ptr<double>(workspace, L.rowcdf_off);
    double* rowsum = ws_ptr<double>(workspace, L.rowsum_off);
    double* total = ws_ptr<double>(workspace, L.total_off);
    IRON_LAUNCH(k_env_rows, h, kEnvBlock, st, image, h, w, rowcdf, rowsum);
    IRON_LAUNCH(k_env_marginal, 1, kEnvBlock, st, (const double*)rowsum, h, ws_ptr<double>(workspace, L.mcdf_off), total);
    IRON_LAUNCH(k_env_normalise, blocks_for((int64_t)h * (w + 1), 256), 256, st, image, h, w, (const double*)rowsum, (const double*)total, rowcdf,
                ws_ptr<float>(workspace, L.ptex_off));
    return IRON_OK;
}

extern "C" int iron_envmap_sample(const iron_envmap* env, const float* u, int64_t n, int32_t* texel, float* dir, float* pdf, void* stream) {
    EnvDev E;
    if (!env_dev(env, E) || n < 0) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!u || !texel || !dir || !pdf) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_env_sample, blocks_for(n, 256), 256, (hipStream_t)stream, E, u, n, texel, dir, pdf);
    return IRON_OK;
}

static int env_eval_entry(const iron_envmap* env, const float* dir, int64_t n, float* pdf, float* rgb, void* stream) {
    EnvDev E;
    if (!env_dev(env, E) || n < 0) return IRON_ERR_BAD_ARG;
    if (n == 0) return IRON_OK;
    if (!dir || (!pdf && !rgb)) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_env_eval, blocks_for(n, 256), 256, (hipStream_t)stream, E, dir, n, pdf, rgb);
    return IRON_OK;
}

extern "C" int iron_envmap_pdf(const iron_envmap* env, const float* dir, int64_t n, float* pdf, void* stream) {
    return env_eval_entry(env, dir, n, pdf, nullptr, stream);
}

extern "C" int iron_envmap_lookup(const iron_envmap* env, const float* dir, int64_t n, float* rgb, void* stream) {
    return env_eval_entry(env, dir, n, nullptr, rgb, stream);
}

extern "C" int iron_roughplastic(const float* n, const float* v, const float* l, const float* kd, const float* ks, const float* rough,
                                 const float* tab_trans, const float* tab_diff_trans, int64_t count, float* diffuse, float* specular,
                                 void* stream) {
    if (count < 0) return IRON_ERR_BAD_ARG;
    if (count == 0) return IRON_OK;
    if (!n || !v || !l || !kd || !ks || !rough || !tab_trans || !tab_diff_trans || !diffuse || !specular) return IRON_ERR_BAD_ARG;
    IRON_LAUNCH(k_roughplastic, blocks_for(count, 256), 256, (hipStream_t)stream, n, v, l, kd, ks, rough, tab_trans, tab_diff_trans, count, diffuse,
                specular);
    return IRON_OK;
}

extern "C" int iron_asset_shade_env(const iron_asset_mesh* mesh, const void* bvh_workspace, const iron_envmap* env, const float* tab_trans,
                                    const float* tab_diff_trans, const float* ray_o, const float* ray_d, const float* t,
                                    const int32_t* face_idx, const float* bary, const int32_t* pixel_idx, int64_t n_rays, int32_t n_light,
                                    int32_t n_brdf, uint32_t seed, float shadow_eps, const iron_asset_out* out, const iron_env_dump* dump,
                                    void* stream) {
    if (!out || !bvh_workspace || n_rays < 0 || n_light < 0 || n_brdf < 0 || (int64_t)n_light + n_brdf > (1 << 20)) return IRON_ERR_BAD_ARG;
    if (!asset_mesh_ok(mesh) || !tab_trans || !tab_diff_trans || !shadow_eps_ok(shadow_eps)) return IRON_ERR_BAD_ARG;
    EnvShadeArgs a;
    if (!env_dev(env, a.env)) return IRON_ERR_BAD_ARG;
    if (n_rays == 0) return IRON_OK;
    if (!ray_o || !ray_d || !t || !face_idx || !bary) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(mesh->n_faces);
    a.m = *mesh; a.o = *out;
    a.dump = dump ? *dump : iron_env_dump{nullptr, nullptr, nullptr, nullptr};
    a.nodes = ws_ptr<float4>(bvh_workspace, L.nodes_off); a.tris = ws_ptr<float4>(bvh_workspace, L.tris_off);
    a.tab_trans = tab_trans; a.tab_diff = tab_diff_trans; a.ray_o = ray_o; a.ray_d = ray_d; a.t = t; a.bary = bary; a.face_idx = face_idx;
    a.pixel_idx = pixel_idx; a.n = n_rays; a.n_light = n_light; a.n_brdf = n_brdf; a.seed = seed; a.shadow_eps = shadow_eps;
    IRON_LAUNCH(k_shade_env, blocks_for(n_rays, kEnvPixels), kBvQueryBlock, (hipStream_t)stream, a);
    return IRON_OK;
}

extern "C" int iron_asset_shade_env_indirect(const iron_asset_mesh* mesh, const void* bvh_workspace, const iron_envmap* env, const float* tab_trans,
                                             const float* tab_diff_trans, const float* ray_o, const float* ray_d, const float* t,
                                             const int32_t* face_idx, const float* bary, const int32_t* pixel_idx, int64_t n_rays,
                                             int32_t n_paths, int32_t max_depth, uint32_t seed, float shadow_eps, float* indirect_diffuse,
                                             float* indirect_specular, const iron_env_path_dump* dump, void* stream) {
    if (!bvh_workspace || n_rays < 0 || n_paths < 1 || n_paths > (1 << 16) || max_depth < 2 || max_depth > 8) return IRON_ERR_BAD_ARG;
    if (!asset_mesh_ok(mesh) || !tab_trans || !tab_diff_trans || !shadow_eps_ok(shadow_eps)) return IRON_ERR_BAD_ARG;
    EnvPathArgs a;
    if (!env_dev(env, a.env)) return IRON_ERR_BAD_ARG;
    if (n_rays == 0) return IRON_OK;
    if (!ray_o || !ray_d || !t || !face_idx || !bary) return IRON_ERR_BAD_ARG;
    const BvLayout L = bv_layout(mesh->n_faces);
    a.m = *mesh;
    a.dump = dump ? *dump : iron_env_path_dump{};
    a.nodes = ws_ptr<float4>(bvh_workspace, L.nodes_off); a.tris = ws_ptr<float4>(bvh_workspace, L.tris_off);
    a.tab_trans = tab_trans; a.tab_diff = tab_diff_trans; a.ray_o = ray_o; a.ray_d = ray_d; a.t = t; a.bary = bary; a.face_idx = face_idx;
    a.pixel_idx = pixel_idx; a.indirect_diffuse = indirect_diffuse; a.indirect_specular = indirect_specular; a.n = n_rays;
    a.n_paths = n_paths; a.max_depth = max_depth; a.seed = seed; a.shadow_eps = shadow_eps;
    IRON_LAUNCH(k_shade_env_indirect, blocks_for(n_rays, kEnvPixels), kBvQueryBlock, (hipStream_t)stream, a);
    return IRON_OK;
}

// ---- the neural scene ----
// what the three entries check alike, and the argument block of a pixel block
static int nenv_args(const iron_neural_gbuffer* g, const iron_envmap* env, int64_t p0, int64_t nb, int32_t n_light, int32_t n_brdf,
                     int64_t capacity, const void* workspace, size_t workspace_bytes, NeuralEnvArgs& a, NeuralEnvLayout& L) {
    if (!g || g->n < 0 || n_light < 0 || n_brdf < 0 || (int64_t)n_light + n_brdf < 1 || (int64_t)n_light + n_brdf > (1 << 20)) return IRON_ERR_BAD_ARG;
    if (p0 < 0 || nb < 1 || p0 + nb > g->n || capacity < 1) return IRON_ERR_BAD_ARG;
    const int64_t N = (int64_t)n_light + n_brdf;
    if (nb * N > capacity || capacity > 0x7fffffffLL - 64) return IRON_ERR_BAD_ARG;   // the samples of a block: int32 list entries
    if (!g->hit || !g->points || !g->normal || !g->ray_d || !g->diffuse_albedo || !g->specular_albedo || !g->specular_roughness)
        return IRON_ERR_BAD_ARG;
    if (!env_dev(env, a.env)) return IRON_ERR_BAD_ARG;
    L = nenv_layout(capacity);
    if (!workspace || ((uintptr_t)workspace & 15) != 0) return IRON_ERR_BAD_ARG;
    if (workspace_bytes < L.bytes) return IRON_ERR_WORKSPACE;
    a.g = *g;
    a.dump = iron_env_dump{nullptr, nullptr, nullptr, nullptr};
    a.tab_trans = a.tab_diff = nullptr;
    a.p0 = p0; a.nb = nb; a.n_light = n_light; a.n_brdf = n_brdf; a.seed = 0; a.shadow_eps = 0.0f;
    a.flags = nullptr; a.dir = nullptr; a.vis = nullptr;
    a.color = a.diffuse_color = a.specular_color = nullptr;
    return IRON_OK;
}

extern "C" int iron_neural_env_workspace_bytes(int64_t capacity, size_t* bytes) {
    if (!bytes || capacity < 1 || capacity > 0x7fffffffLL - 64) return IRON_ERR_BAD_ARG;
    *bytes = nenv_layout(capacity).bytes;
    return IRON_OK;
}

extern "C" int iron_neural_env_emit(const iron_neural_gbuffer* g, const iron_envmap* env, int64_t p0, int64_t nb, int32_t n_light,
                                    int32_t n_brdf, uint32_t seed, float shadow_eps, int64_t capacity, void* workspace, size_t workspace_bytes,
                                    float* ray_o, float* ray_d, int32_t* sample_idx, int64_t* count, void* stream) {
    NeuralEnvArgs a;
    NeuralEnvLayout L;
    const int rc = nenv_args(g, env, p0, nb, n_light, n_brdf, capacity, workspace, workspace_bytes, a, L);
    if (rc != IRON_OK) return rc;
    if (!ray_o || !ray_d || !sample_idx || !count || !shadow_eps_ok(shadow_eps)) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = nb * ((int64_t)n_light + n_brdf);
    a.seed = seed; a.shadow_eps = shadow_eps;
    a.flags = L.scan.level(workspace, 0);
    a.dir = ws_ptr<float>(workspace, L.dir_off);
    // the scan runs over the whole capacity: the entries behind this block's samples are zero
    if (capacity > M) IRON_HIP_TRY(hipMemsetAsync(a.flags + M, 0, sizeof(Pair64) * (size_t)(capacity - M), st));
    IRON_LAUNCH(k_nenv_emit, blocks_for(nb, kEnvPixels), kBvQueryBlock, st, a);
    const int rs = pair_scan(L.scan, workspace, st);
    if (rs != IRON_OK) return rs;
    IRON_LAUNCH(k_nenv_compact, blocks_for(M, 256), 256, st, a, (const Pair64*)L.scan.level(workspace, 0),
                (const Pair64*)L.scan.level(workspace, L.scan.levels), capacity, ray_o, ray_d, sample_idx, count);
    return IRON_OK;
}

extern "C" int iron_neural_env_resolve(const iron_neural_gbuffer* g, const iron_envmap* env, const float* tab_trans, const float* tab_diff_trans,
                                       int64_t p0, int64_t nb, int32_t n_light, int32_t n_brdf, uint32_t seed, int64_t capacity,
                                       void* workspace, size_t workspace_bytes, const uint8_t* occluded, const int32_t* sample_idx,
                                       int64_t n_rays, float* color, float* diffuse_color, float* specular_color, const iron_env_dump* dump,
                                       void* stream) {
    NeuralEnvArgs a;
    NeuralEnvLayout L;
    const int rc = nenv_args(g, env, p0, nb, n_light, n_brdf, capacity, workspace, workspace_bytes, a, L);
    if (rc != IRON_OK) return rc;
    const int64_t M = nb * ((int64_t)n_light + n_brdf);
    if (!tab_trans || !tab_diff_trans || n_rays < 0 || n_rays > M || (n_rays > 0 && (!occluded || !sample_idx))) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* vis = ws_ptr<uint8_t>(workspace, L.vis_off);
    IRON_HIP_TRY(hipMemsetAsync(vis, 0, (size_t)M, st));
    if (n_rays > 0) IRON_LAUNCH(k_nenv_scatter, blocks_for(n_rays, 256), 256, st, occluded, sample_idx, n_rays, M, vis);
    a.seed = seed; a.tab_trans = tab_trans; a.tab_diff = tab_diff_trans; a.vis = vis;
    a.dump = dump ? *dump : iron_env_dump{nullptr, nullptr, nullptr, nullptr};
    a.color = color; a.diffuse_color = diffuse_color; a.specular_color = specular_color;
    IRON_LAUNCH(k_nenv_resolve, blocks_for(nb, kEnvPixels), kBvQueryBlock, st, a);
    return IRON_OK;
}

// ---- interreflections on the neural scene ----
// what the entries of a block check alike, and the argument block
static int npath_args(const iron_neural_gbuffer* g, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int64_t capacity,
                      void* workspace, size_t workspace_bytes, NeuralPathArgs& a) {
    if (!g || g->n < 0 || n_paths < 1 || n_paths > (1 << 16) || max_depth < 2 || max_depth > 8) return IRON_ERR_BAD_ARG;
    if (p0 < 0 || nb < 1 || p0 + nb > g->n || capacity < 1 || capacity > 0x7fffffffLL - 64) return IRON_ERR_BAD_ARG;
    if (nb > capacity / n_paths) return IRON_ERR_BAD_ARG;   // the slots of a block: int32 list entries
    if (!g->hit || !g->points || !g->normal || !g->ray_d || !g->diffuse_albedo || !g->specular_albedo || !g->specular_roughness)
        return IRON_ERR_BAD_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) != 0) return IRON_ERR_BAD_ARG;
    const NeuralPathLayout L = npath_layout(capacity);
    if (workspace_bytes < L.bytes) return IRON_ERR_WORKSPACE;
    a = NeuralPathArgs{};
    a.g = *g;
    a.p0 = p0; a.nb = nb; a.capacity = capacity; a.n_paths = n_paths; a.max_depth = max_depth;
    a.state = ws_ptr<float>(workspace, L.state_off);
    a.dir = ws_ptr<float>(workspace, L.dir_off);
    a.alive = ws_ptr<uint8_t>(workspace, L.alive_off);
    a.cast = ws_ptr<uint8_t>(workspace, L.cast_off);
    a.flags = L.scan.level(workspace, 0);
    return IRON_OK;
}

extern "C" int iron_neural_path_workspace_bytes(int64_t capacity, size_t* bytes) {
    if (!bytes || capacity < 1 || capacity > 0x7fffffffLL - 64) return IRON_ERR_BAD_ARG;
    *bytes = npath_layout(capacity).bytes;
    return IRON_OK;
}

extern "C" int iron_neural_path_begin(const iron_neural_gbuffer* g, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int64_t capacity,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    NeuralPathArgs a;
    const int rc = npath_args(g, p0, nb, n_paths, max_depth, capacity, workspace, workspace_bytes, a);
    if (rc != IRON_OK) return rc;
    IRON_LAUNCH(k_npath_begin, blocks_for(nb * n_paths, kPathBlock), kPathBlock, (hipStream_t)stream, a);
    return IRON_OK;
}

extern "C" int iron_neural_path_emit(const iron_neural_gbuffer* g, const iron_envmap* env, int64_t p0, int64_t nb, int32_t n_paths,
                                     int32_t max_depth, int32_t depth, uint32_t seed, float shadow_eps, int64_t capacity, void* workspace,
                                     size_t workspace_bytes, float* shadow_o, float* shadow_d, int32_t* shadow_idx, float* bounce_o,
                                     float* bounce_d, int32_t* bounce_idx, int64_t* counts, void* stream) {
    NeuralPathArgs a;
    const int rc = npath_args(g, p0, nb, n_paths, max_depth, capacity, workspace, workspace_bytes, a);
    if (rc != IRON_OK) return rc;
    if (depth < 0 || depth >= max_depth || !shadow_eps_ok(shadow_eps)) return IRON_ERR_BAD_ARG;
    if (!shadow_o || !shadow_d || !shadow_idx || !bounce_o || !bounce_d || !bounce_idx || !counts) return IRON_ERR_BAD_ARG;
    if (!env_dev(env, a.env)) return IRON_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const NeuralPathLayout L = npath_layout(capacity);
    const int64_t M = nb * n_paths;
    a.depth = depth; a.seed = seed; a.shadow_eps = shadow_eps;
    // the scan runs over the whole capacity: the entries behind this block's slots are zero
    if (capacity > M) IRON_HIP_TRY(hipMemsetAsync(a.flags + M, 0, sizeof(Pair64) * (size_t)(capacity - M), st));
    IRON_HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
    IRON_LAUNCH(k_npath_emit, blocks_for(M, kPathBlock), kPathBlock, st, a, (unsigned long long*)counts);
    const int rs = pair_scan(L.scan, workspace, st);
    if (rs != IRON_OK) return rs;
    IRON_LAUNCH(k_npath_compact, blocks_for(M, kPathBlock), kPathBlock, st, a, (const Pair64*)L.scan.level(workspace, 0),
                (const Pair64*)L.scan.level(workspace, L.scan.levels), shadow_o, shadow_d, shadow_idx, bounce_o, bounce_d, bounce_idx,
                (unsigned long long*)counts);
    return IRON_OK;
}

extern "C" int iron_neural_path_resolve(const iron_neural_gbuffer* g, const iron_envmap* env, const float* tab_trans, const float* tab_diff_trans,
                                        int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int32_t depth, uint32_t seed,
                                        float shadow_eps, int64_t capacity, void* workspace, size_t workspace_bytes, const uint8_t* occluded,
                                        int64_t n_shadow, const iron_neural_bounce* bounce, int64_t n_bounce,
                                        const iron_neural_path_dump* dump, void* stream) {
    NeuralPathArgs a;
    const int rc = npath_args(g, p0, nb, n_paths, max_depth, capacity, workspace, workspace_bytes, a);
    if (rc != IRON_OK) return rc;
    const int64_t M = nb * n_paths;
    if (depth < 0 || depth >= max_depth || !shadow_eps_ok(shadow_eps) || !tab_trans || !tab_diff_trans) return IRON_ERR_BAD_ARG;
    if (n_shadow < 0 || n_shadow > M || n_bounce < 0 || n_bounce > M || (n_shadow > 0 && !occluded)) return IRON_ERR_BAD_ARG;
    if (n_bounce > 0 && (!bounce || !bounce->hit || !bounce->distance || !bounce->points || !bounce->normal || !bounce->diffuse_albedo ||
                         !bounce->specular_albedo || !bounce->specular_roughness))
        return IRON_ERR_BAD_ARG;
    if (!env_dev(env, a.env)) return IRON_ERR_BAD_ARG;
    a.depth = depth; a.seed = seed; a.shadow_eps = shadow_eps; a.tab_trans = tab_trans; a.tab_diff = tab_diff_trans;
    a.occluded = occluded; a.n_shadow = n_shadow; a.n_bounce = n_bounce;
    if (n_bounce > 0) {
        a.bounce_hit = bounce->hit; a.bounce_dist = bounce->distance; a.bounce_points = bounce->points; a.bounce_normal = bounce->normal;
        a.bounce_kd = bounce->diffuse_albedo; a.bounce_ks = bounce->specular_albedo; a.bounce_rough = bounce->specular_roughness;
    }
    if (dump) a.dump = *dump;
    IRON_LAUNCH(k_npath_resolve, blocks_for(M, kPathBlock), kPathBlock, (hipStream_t)stream, a);
    return IRON_OK;
}

extern "C" int iron_neural_path_finish(const iron_neural_gbuffer* g, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int64_t capacity,
                                       void* workspace, size_t workspace_bytes, float* indirect_diffuse, float* indirect_specular,
                                       const iron_neural_path_dump* dump, void* stream) {
    NeuralPathArgs a;
    const int rc = npath_args(g, p0, nb, n_paths, max_depth, capacity, workspace, workspace_bytes, a);
    if (rc != IRON_OK) return rc;
    a.indirect_diffuse = indirect_diffuse; a.indirect_specular = indirect_specular;
    if (dump) a.dump = *dump;
    IRON_LAUNCH(k_npath_finish, blocks_for(nb, kEnvPixels), kBvQueryBlock, (hipStream_t)stream, a);
    return IRON_OK;
}
