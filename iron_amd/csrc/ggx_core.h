// Pointwise geometry + co-located GGX BRDF device functions (fp32, one rounding per reference op;
// the translation unit is compiled with -ffp-contract=off so a*b+c stays two roundings like the
// reference's separate torch kernels).
#pragma once
#include <hip/hip_runtime.h>

namespace iron {

// ---- number types: float, or first-order dual numbers for the backward passes (train.hip) -----------------------------------
// Dual<N>: a value and its derivatives in N variables.  A float converts to a constant, so one templated formula below serves
// both; the operators are hidden friends so that conversion applies to `1.0f - c2` and the like.
template <int N>
struct Dual {
    float v, d[N];
    Dual() = default;
    __device__ __forceinline__ Dual(float c) : v(c) {
        for (int i = 0; i < N; ++i) d[i] = 0.f;
    }
    __device__ __forceinline__ static Dual var(float x, int k) {
        Dual r(x);
        r.d[k] = 1.f;
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(Dual a, Dual b) {
        Dual r; r.v = a.v + b.v;
        for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(Dual a, Dual b) {
        Dual r; r.v = a.v - b.v;
        for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(Dual a, Dual b) {
        Dual r; r.v = a.v * b.v;
        for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
        return r;
    }
    friend __device__ __forceinline__ Dual operator/(Dual a, Dual b) {
        Dual r; r.v = a.v / b.v;
        const float ib = 1.0f / b.v;
        for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
        return r;
    }
    friend __device__ __forceinline__ Dual sqrt_t(Dual a) {
        Dual r; r.v = sqrtf(a.v);
        const float k = 0.5f / r.v;
        for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * k;
        return r;
    }
    // hypot(x, 1): the value is hypotf as in the forward, the derivative x / h
    friend __device__ __forceinline__ Dual hypot1(Dual a) {
        Dual r; r.v = hypotf(a.v, 1.0f);
        const float k = a.v / r.v;
        for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * k;
        return r;
    }
};
__device__ __forceinline__ float sqrt_t(float x) { return sqrtf(x); }
__device__ __forceinline__ float hypot1(float x) { return hypotf(x, 1.0f); }

// ---- the reference's constants -------------------------------------------------------------------------------------------------
constexpr double kEta = 1.48958738;                             // the rough-plastic interior IOR the reference hard-codes
constexpr float kPi = 3.14159274101257324219f;                  // float32(np.pi)
constexpr float kInvEta2 = (float)(1.0 / (kEta * kEta));
constexpr float kEta2 = (float)(kEta * kEta + 1e-10);          // alpha^2 + 1e-10 of the composite NDF (alpha := eta)
constexpr float kPiEta2 = (float)(3.141592653589793 * kEta * kEta);
constexpr float kFr = 0.03867f;                                 // GGXColocatedRenderer's specular Fresnel
constexpr float kThinSpec = (float)(0.04 + 0.96 * 0.96 * 0.04 / (1.0 - 0.04 * 0.04));  // ThinDielectric's specular scale

// ---- BRDF building blocks, T = float or Dual<N> -------------------------------------------------------------------------------
// intensity of a point light at distance d
template <class T>
__device__ __forceinline__ T intensity_at(float light, T d) { return light / (d * d + 1e-10f); }

// GGX NDF at cos theta = c (models/renderer_ggx.py:106-108)
template <class T>
__device__ __forceinline__ T ggx_ndf(T c, T alpha) {
    const T c2 = c * c;
    const T root = c2 + (1.0f - c2) / (alpha * alpha + 1e-10f);
    return 1.0f / (kPi * alpha * alpha * root * root + 1e-10f);
}

// CompositeRenderer's NDF: alpha := eta (renderer_ggx.py:806), pi * alpha^2 folded into one constant
template <class T>
__device__ __forceinline__ T composite_ndf(T c) {
    const T c2 = c * c;
    const T root = c2 + (1.0f - c2) / kEta2;
    return 1.0f / (kPiEta2 * root * root + 1e-10f);
}

// smithG1 (models/renderer_ggx.py:12-16)
template <class T>
__device__ __forceinline__ T smith_g1(T cos_theta, T alpha) {
    const T sin_theta = sqrt_t(1.0f - cos_theta * cos_theta);
    const T tan_theta = sin_theta / (cos_theta + 1e-10f);
    const T root = alpha * tan_theta;
    return 2.0f / (1.0f + hypot1(root));
}

// fresnel_conductor_exact (renderer_ggx.py:419-432 = CompositeRenderer.fresnel_conductor_exact :592-605)
template <class T>
__device__ __forceinline__ T fresnel_conductor_exact(T cos_i, T eta, T k) {
    const T c2 = cos_i * cos_i;
    const T s2 = 1.0f - c2;
    const T s4 = s2 * s2;
    const T temp1 = eta * eta - k * k - s2;
    const T a2pb2 = sqrt_t(temp1 * temp1 + 4.0f * k * k * eta * eta);
    const T a = sqrt_t(0.5f * (a2pb2 + temp1));
    const T term1 = a2pb2 + c2;
    const T term2 = 2.0f * a * cos_i;
    const T rs2 = (term1 - term2) / (term1 + term2);
    const T term3 = a2pb2 * c2 + s4;
    const T term4 = term2 * s2;
    const T rp2 = rs2 * (term3 - term4) / (term3 + term4);
    return 0.5f * (rp2 + rs2);
}

// fresnel_dielectric (renderer_ggx.py:398-416) for cos_i > 0 (the callers clamp it to [1e-5, 0.99999])
template <class T>
__device__ __forceinline__ T fresnel_dielectric_pos(T cos_i, T eta) {
    const T scale = 1.0f / eta;
    const T cos_t_sqr = 1.0f - (1.0f - cos_i * cos_i) * (scale * scale);
    const T cos_t = sqrt_t(cos_t_sqr);
    const T rs = (cos_i - eta * cos_t) / (cos_i + eta * cos_t);
    const T rp = (eta * cos_i - cos_t) / (eta * cos_i + cos_t);
    return 0.5f * (rs * rs + rp * rp);
}

// the Mitsuba rough-plastic diffuse term through the two tables (CompositeRenderer.diffuse_reflection_ggx :654-681);
// returns the factor that multiplies intensity * kd: 1 / (1 - Fdr + 1e-10) / pi * cos * T12^2 / eta^2 is applied by the caller.
// Piecewise constant: the backward passes take it as a constant.
// tab_trans: 5000 floats (100 theta x 50 alpha), tab_diff: 50 floats.
__device__ __forceinline__ void rtrans_lookup(float cos_theta, float alpha, const float* tab_trans, const float* tab_diff,
                                              float& T12, float& fd) {
    const float warped_cos = powf(cos_theta, 0.25f);
    const float warped_alpha = powf(alpha / 4.0f, 0.25f);
    const long long tx = (long long)floorf(warped_cos * 100.0f);
    const long long ty = (long long)floorf(warped_alpha * 50.0f);
    long long ti = ty * 100 + tx;
    ti = ti < 0 ? 0 : (ti > 4999 ? 4999 : ti);
    T12 = fminf(fmaxf(tab_trans[ti], 0.0f), 1.0f);
    const long long ai = ty < 0 ? 0 : (ty > 49 ? 49 : ty);
    const float Fdr = fminf(fmaxf(1.0f - tab_diff[ai], 0.0f), 1.0f);
    fd = 1.0f - Fdr + 1e-10f;
}

// ---- the forward heads, one point each ---------------------------------------------------------------------------------------
struct GgxOut {
    float diffuse[3];
    float specular[3];
    float rgb[3];
};

// torch.clamp keeps a NaN; fminf / fmaxf return the OTHER operand, so a clamped NaN input (a normal or a material value the h2 core
// lost to an overflow, csrc/envelope.hip, or a NaN of the network's own) would come out as a finite, plausible colour.  The heads
// below add nan_of() of every input they clamp to what depends on it: 0 for any number, the NaN itself otherwise.
__device__ __forceinline__ float nan_of(float x) { return x != x ? x : 0.0f; }

// GGXColocatedRenderer.forward (models/renderer_ggx.py:82-146) for one point.
__device__ __forceinline__ void ggx_colocated_point(float light, float distance, const float n[3], const float v[3],
                                                    const float kd[3], const float ks[3], float rough,
                                                    const float* __restrict__ tab_trans,
                                                    const float* __restrict__ tab_diff, GgxOut& o) {
    const float intensity = intensity_at(light, distance);
    float dot = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    const float lost = nan_of(dot) + nan_of(rough);
    dot = fminf(fmaxf(dot, 0.00001f), 0.99999f);
    const float alpha = fmaxf(rough, 0.0001f);
    const float D = ggx_ndf(dot, alpha);
    const float g1 = smith_g1(dot, alpha);
    const float G = g1 * g1;
    const float denom = 4.0f * dot + 1e-10f;
    float T12, fd;
    rtrans_lookup(dot, alpha, tab_trans, tab_diff, T12, fd);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.specular[c] = intensity * ks[c] * kFr * D * G / denom + lost;
        o.diffuse[c] = intensity * (kd[c] / fd / kPi) * dot * T12 * T12 * kInvEta2 + lost;
        o.rgb[c] = o.diffuse[c] + o.specular[c];
    }
}

// The same rough plastic for a light direction l other than the view direction v (the environment render, envlight.hip): the
// BRDF times cos_i, split like GgxOut, from the blocks above only.  h = normalize(v + l); cos_o = n.v, cos_i = n.l, cos_h = n.h
// and cos_d = v.h are clamped to [1e-5, 0.99999] as in every co-located head; n.l <= 0 (or v + l = 0) gives zero.
//   specular cos_i = ks F(cos_d) D(cos_h) G1(cos_i) G1(cos_o) / (4 cos_o + 1e-10)
//   diffuse cos_i  = (kd / fd / pi) cos_i T12(cos_i) T12(cos_o) / eta^2
// At l = v this is ggx_colocated_point with intensity 1, except that the Fresnel term is computed (0.0386729 at normal incidence)
// where that head takes its 4-digit rounding kFr.
struct PlasticOut {
    float diffuse[3];
    float specular[3];
};

__device__ __forceinline__ float clamp_cos(float c) { return fminf(fmaxf(c, 0.00001f), 0.99999f); }

__device__ __forceinline__ void roughplastic_point(const float n[3], const float v[3], const float l[3], const float kd[3],
                                                   const float ks[3], float rough, const float* __restrict__ tab_trans,
                                                   const float* __restrict__ tab_diff, PlasticOut& o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o.diffuse[c] = o.specular[c] = 0.0f;
    const float nl = (l[0] * n[0] + l[1] * n[1]) + l[2] * n[2];
    const float hx = v[0] + l[0], hy = v[1] + l[1], hz = v[2] + l[2];
    const float hl = sqrtf((hx * hx + hy * hy) + hz * hz);
    if (!(nl > 0.0f) || !(hl > 0.0f)) return;
    const float h[3] = {hx / hl, hy / hl, hz / hl};
    const float cos_o = clamp_cos((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]);
    const float cos_i = clamp_cos(nl);
    const float cos_h = clamp_cos((h[0] * n[0] + h[1] * n[1]) + h[2] * n[2]);
    const float cos_d = clamp_cos((h[0] * v[0] + h[1] * v[1]) + h[2] * v[2]);
    const float alpha = fmaxf(rough, 0.0001f);
    const float F = fresnel_dielectric_pos(cos_d, (float)kEta);
    const float D = ggx_ndf(cos_h, alpha);
    const float G = smith_g1(cos_i, alpha) * smith_g1(cos_o, alpha);
    const float denom = 4.0f * cos_o + 1e-10f;
    float Ti, To, fd, fd_o;
    rtrans_lookup(cos_i, alpha, tab_trans, tab_diff, Ti, fd);
    rtrans_lookup(cos_o, alpha, tab_trans, tab_diff, To, fd_o);  // fd depends on alpha alone
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.specular[c] = ks[c] * F * D * G / denom;
        o.diffuse[c] = (kd[c] / fd / kPi) * cos_i * Ti * To * kInvEta2;
    }
}

// ---- the fork's other co-located heads (models/renderer_ggx.py:149-517, 520-858) -----------------

struct CompositeOut {
    float specular[3], metallic[3], dielectric[3], rgb[3];
};

// CompositeRenderer.forward (renderer_ggx.py:781-858) for one point, quirks included: the NDF takes alpha := 1.48958738
// (:806), the metallic / dielectric weights are unused (:829-831), diffuse_rgb is rgb (in-place alias :847-853).
// `intensity` = light / (d^2 + 1e-10) or the clamped env light.
__device__ __forceinline__ void composite_point(float intensity, const float n[3], const float v[3], const float kd_in[3],
                                                const float ks_in[3], float rough_in, float m_eta_in, float m_k_in,
                                                float d_eta_in, const float* __restrict__ tab_trans,
                                                const float* __restrict__ tab_diff, CompositeOut& o) {
    const float rough = fmaxf(rough_in, 0.00001f);
    const float d_eta = fminf(fmaxf(d_eta_in, 1.000001f), 1.999999f);
    const float m_eta = fminf(fmaxf(m_eta_in, 0.099999f), 4.999999f);
    const float m_k = fminf(fmaxf(m_k_in, 0.099999f), 9.999999f);
    float cos_i = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    const float lost_m = (nan_of(cos_i) + nan_of(m_eta_in)) + nan_of(m_k_in);        // what the metallic term clamps
    const float lost_d = (nan_of(cos_i) + nan_of(d_eta_in)) + nan_of(rough_in);      // ... the dielectric term, and the diffuse one
    cos_i = fminf(fmaxf(cos_i, 0.00001f), 0.99999f);
    const float D = composite_ndf(cos_i);
    const float g1 = smith_g1(cos_i, rough);
    const float G = g1 * g1;
    const float Fm = fresnel_conductor_exact(cos_i, m_eta, m_k);
    const float Fd = fresnel_dielectric_pos(cos_i, d_eta);
    const float denom = 4.0f * fabsf(cos_i);
    float T12, fd;
    rtrans_lookup(cos_i, fmaxf(rough, 0.0001f), tab_trans, tab_diff, T12, fd);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ks = fmaxf(ks_in[c], 0.00001f);
        const float kd = fmaxf(kd_in[c], 0.00001f);
        o.metallic[c] = (ks * Fm) * intensity + (lost_m + nan_of(ks_in[c]));
        o.dielectric[c] = (ks * Fd * D * G / denom) * intensity + (lost_d + nan_of(ks_in[c]));
        o.specular[c] = o.dielectric[c] + o.metallic[c];
        const float diffuse = intensity * (kd / fd / kPi) * cos_i * T12 * T12 * kInvEta2 + (lost_d + nan_of(kd_in[c]));
        o.rgb[c] = diffuse + o.specular[c];
    }
}

// SmoothDielectric (:171-204), ThinDielectric (:229-267), SmoothConductorCoLoc (:299-319), RoughConductorCoLoc (:351-395)
enum { kHeadSmoothDielectric = 0, kHeadThinDielectric = 1, kHeadSmoothConductor = 2, kHeadRoughConductor = 3 };

__device__ __forceinline__ void coloc_head_point(int kind, float light, float distance, const float n[3], const float v[3],
                                                 const float kd[3], const float ks[3], float rough, float eta, float k,
                                                 GgxOut& o) {
    const float intensity = intensity_at(light, distance);
    float dot = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    dot = fminf(fmaxf(dot, 0.00001f), 0.99999f);
    float spec_scale;  // specular_rgb = intensity * ks * spec_scale  (left-to-right products below keep the reference order)
    float denom = 1.0f, G = 1.0f, D = 1.0f;
    if (kind == kHeadSmoothDielectric) {
        spec_scale = 0.04f;
    } else if (kind == kHeadThinDielectric) {
        spec_scale = kThinSpec;
    } else {
        spec_scale = fresnel_conductor_exact(dot, eta, k);
        if (kind == kHeadRoughConductor) {
            const float alpha = fmaxf(rough, 0.0001f);
            D = ggx_ndf(dot, alpha);
            const float g1 = smith_g1(dot, alpha);
            G = g1 * g1;
            denom = 4.0f * dot + 1e-10f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.specular[c] = kind == kHeadRoughConductor ? intensity * ks[c] * spec_scale * D * G / denom : intensity * ks[c] * spec_scale;
        o.diffuse[c] = intensity * kd[c] * 0.0001f;
        o.rgb[c] = o.diffuse[c] + o.specular[c];
    }
}

// intersect_sphere (models/raytracer.py:223-237) for one ray
__device__ __forceinline__ void intersect_sphere_ray(const float o[3], const float d[3], float r, bool& hit,
                                                     float& near, float& far) {
    const float dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float d1 = -((d[0] * o[0] + d[1] * o[1]) + d[2] * o[2]) / dd;
    const float px = o[0] + d1 * d[0], py = o[1] + d1 * d[1], pz = o[2] + d1 * d[2];
    const float tmp = r * r - ((px * px + py * py) + pz * pz);
    hit = tmp > 0.0f;
    const float d2 = sqrtf(fmaxf(tmp, 0.0f)) / sqrtf(dd);
    near = fmaxf(d1 - d2, 0.0f);
    far = d1 + d2;
}

}  // namespace iron
