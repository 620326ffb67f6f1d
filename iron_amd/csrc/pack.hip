// Network handles: weight-norm folding + repacking of reference state_dict tensors into the MFMA
// fragment layout (iron_common.h).  Replaces the parameter side of models/fields.py:9-98,141-201.
#include <math.h>
#include <string.h>
#include <new>
#include "iron_common.h"
#include "pack_common.h"

namespace iron {

thread_local int g_last_hip_error = 0;

// scale[o] = g[o] / ||v[o,:]||_2   (old-style weight_norm, dim=0; fields.py:75-76), 1 if g == NULL
__global__ void k_row_scale(const float* __restrict__ v, const float* __restrict__ g, int out_dim, int in_dim,
                            float* __restrict__ scale) {
    const int o = blockIdx.x;
    if (o >= out_dim) return;
    if (g == nullptr) {
        if (threadIdx.x == 0) scale[o] = 1.0f;
        return;
    }
    float s = 0.0f;
    for (int k = threadIdx.x; k < in_dim; k += 64) {
        const float a = v[(size_t)o * in_dim + k];
        s = fmaf(a, a, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (threadIdx.x == 0) scale[o] = g[o] / sqrtf(s);
}

// dst [pairs][8][4][2][64] float4 : lane (i,h) of (pair p, which w, in-tile ti, quad q) holds
//   W[32*(2p+w) + i][col_off + 32*ti + 8*q + 4*h + 0..3]
__global__ void k_pack_hidden(float4* __restrict__ dst, PackSrc s, int col_off, int cols_valid) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kPairs * kHidTiles * 4 * 2 * 64) return;
    const int lane = e & 63;
    const int w = (e >> 6) & 1;
    const int q = (e >> 7) & 3;
    const int ti = (e >> 9) & 7;
    const int p = e >> 12;
    const int i = lane & 31, h = lane >> 5;
    const int row = 32 * (2 * p + w) + i;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = 32 * ti + 8 * q + 4 * h + c;
        float x = 0.0f;
        if (row < s.rows_valid && col < cols_valid)
            x = s.w[(size_t)(s.row_off + row) * s.ld + col_off + col] * s.scale[s.row_off + row] * s.mul;
        v[c] = x;
    }
    dst[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// dst [pairs][NQ][2][64] float4 : lane (i,h) of (pair, quad q, which w) holds the weights of head
// slots 4q..4q+3 (their lane-half-h columns) for output row 32*(2p+w)+i
__global__ void k_pack_head(float4* __restrict__ dst, PackSrc s, HeadSrcs hs, int nq) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kPairs * nq * 2 * 64) return;
    const int lane = e & 63;
    const int w = (e >> 6) & 1;
    const int q = (e >> 7) % nq;
    const int p = (e >> 7) / nq;
    const int i = lane & 31, h = lane >> 5;
    const int row = 32 * (2 * p + w) + i;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int slot = 4 * q + c;
        float x = 0.0f;
        for (int k = 0; k < hs.n; ++k) {
            const int local = slot - hs.slot_base[k];
            if (local >= 0 && local < head_slots(hs.levels[k])) {
                const int col = head_slot_column(local, h, hs.levels[k]);
                if (col >= 0 && row < s.rows_valid)
                    x = s.w[(size_t)(s.row_off + row) * s.ld + hs.col_off[k] + col] * s.scale[s.row_off + row] * s.mul;
            }
        }
        v[c] = x;
    }
    dst[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// The same for ONE 4-component source with `levels` PE levels (NeRF background points; slot layout of head_fill4):
// reference column order (models/embedder.py:27-36) [v(4), sin(2^0 v)(4), cos(2^0 v)(4), ...]
__global__ void k_pack_head4(float4* __restrict__ dst, PackSrc s, int levels, int col_off, int nq) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kPairs * nq * 2 * 64) return;
    const int lane = e & 63;
    const int w = (e >> 6) & 1;
    const int q = (e >> 7) % nq;
    const int p = (e >> 7) / nq;
    const int i = lane & 31, h = lane >> 5;
    const int row = 32 * (2 * p + w) + i;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int slot = 4 * q + c;
        int col = -1;
        if (slot == 0) col = h;
        else if (slot == 1) col = 2 + h;
        else if (slot < 2 + 4 * levels) col = 4 + 8 * ((slot - 2) / 4) + 4 * h + ((slot - 2) % 4);
        float x = 0.0f;
        if (col >= 0 && row < s.rows_valid)
            x = s.w[(size_t)(s.row_off + row) * s.ld + col_off + col] * s.scale[s.row_off + row] * s.mul;
        v[c] = x;
    }
    dst[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// dst [8][2][16] floats: element (tile, h, r) = bias[row_off + 32*tile + (r&3) + 8*(r>>2) + 4*h]
__global__ void k_pack_bias(float* __restrict__ dst, const float* __restrict__ bias, int row_off, int rows_valid) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kHidTiles * 2 * 16) return;
    const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
    const int row = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
    dst[e] = row < rows_valid ? bias[row_off + row] : 0.0f;
}

// dst [8][2][16] floats: element (tile, h, r) = W[row][col_off + 32*tile + (r&3) + 8*(r>>2) + 4*h] * scale[row]
__global__ void k_pack_row(float* __restrict__ dst, PackSrc s, int row, int col_off, int cols_valid) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kHidTiles * 2 * 16) return;
    const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
    const int col = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
    dst[e] = col < cols_valid ? s.w[(size_t)row * s.ld + col_off + col] * s.scale[row] * s.mul : 0.0f;
}

static inline size_t align_f4(size_t n_f4) { return (n_f4 + 15) & ~(size_t)15; }

}  // namespace iron

using namespace iron;

extern "C" int iron_version(void) { return IRON_ABI_VERSION; }

extern "C" int iron_last_hip_error(void) { return g_last_hip_error; }

extern "C" const char* iron_strerror(int status) {
    switch (status) {
        case IRON_OK: return "ok";
        case IRON_ERR_BAD_ARG: return "bad argument (null pointer, negative size or misaligned buffer; for a mesh: a face index out of "
                                     "range or a non-finite vertex)";
        case IRON_ERR_UNSUPPORTED: return "unsupported network shape or mode for the gfx950 kernels";
        case IRON_ERR_HIP: return "HIP runtime error (see iron_last_hip_error)";
        case IRON_ERR_NO_DEVICE: return "no gfx950 device visible";
        case IRON_ERR_WORKSPACE: return "workspace too small";
        case IRON_ERR_RANGE: return "an activation or feature left the fp16 range of the h2 core (|x| >= 65504 or non-finite): results of the "
                                    "previous call on this network were non-finite; iron_net_force_exact(net, 1) puts the handle back to work on the exact core (or start with "
                                    "IRON_MLP_CORE=f32)";
        default: return "unknown iron status";
    }
}

static int check_device(int* dev_out) {
    int dev = 0;
    IRON_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    IRON_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return IRON_ERR_NO_DEVICE;
    *dev_out = dev;
    return IRON_OK;
}


namespace {

struct Blob {
    size_t n_f4 = 0;
    size_t take(size_t f4) { size_t o = n_f4; n_f4 += align_f4(f4); return o; }
};

// per-layer fold factors live in the blob too (kept: cheap, and lets create stay allocation-light)
int fold_scales(const iron_linear* L, int nl, float* scale_base, size_t* scale_off, hipStream_t st) {
    size_t off = 0;
    for (int l = 0; l < nl; ++l) {
        scale_off[l] = off;
        hipLaunchKernelGGL(k_row_scale, dim3(L[l].out_dim), dim3(64), 0, st, L[l].weight_v, L[l].weight_g,
                           L[l].out_dim, L[l].in_dim, scale_base + off);
        off += (size_t)L[l].out_dim;
    }
    IRON_HIP_TRY(hipGetLastError());
    return IRON_OK;
}

inline void launch_pack_hidden(float4* dst, const PackSrc& s, int col_off, int cols_valid, hipStream_t st) {
    hipLaunchKernelGGL(k_pack_hidden, dim3(kF4PerHidLayer / 256), dim3(256), 0, st, dst, s, col_off, cols_valid);
}
inline void launch_pack_head(float4* dst, const PackSrc& s, const HeadSrcs& hs, int nq, hipStream_t st) {
    const int n = kPairs * nq * 2 * 64;
    hipLaunchKernelGGL(k_pack_head, dim3((n + 255) / 256), dim3(256), 0, st, dst, s, hs, nq);
}
inline void launch_pack_bias(float4* dst, const float* bias, int row_off, int rows_valid, hipStream_t st) {
    hipLaunchKernelGGL(k_pack_bias, dim3(1), dim3(256), 0, st, (float*)dst, bias, row_off, rows_valid);
}
inline void launch_pack_row(float4* dst, const PackSrc& s, int row, int col_off, int cols_valid, hipStream_t st) {
    hipLaunchKernelGGL(k_pack_row, dim3(1), dim3(256), 0, st, (float*)dst, s, row, col_off, cols_valid);
}


int create_sdf(iron_net* net, const iron_linear* L, hipStream_t st) {
    const iron_net_desc& d = net->desc;
    const int nl = d.n_linear;
    const int pe = pe_width(d.multires);
    const int skip = d.skip_layer;
    if (d.d_hidden != kHidden || d.multires != 6 || nl < 3 || nl > 17) return IRON_ERR_UNSUPPORTED;
    if (!(skip == -1 || (skip >= 2 && skip <= nl - 2))) return IRON_ERR_UNSUPPORTED;
    if (!(d.d_out == 1 || d.d_out == kHidden + 1)) return IRON_ERR_UNSUPPORTED;
    if (!(d.scale > 0.0f)) return IRON_ERR_BAD_ARG;
    for (int l = 0; l < nl; ++l) {
        if (!L[l].weight_v || !L[l].bias) return IRON_ERR_BAD_ARG;
        const int want_in = (l == 0) ? pe : kHidden;
        int want_out = (l == nl - 1) ? d.d_out : kHidden;
        if (l + 1 == skip) want_out = kHidden - pe;
        if (L[l].in_dim != want_in || L[l].out_dim != want_out) return IRON_ERR_UNSUPPORTED;
    }
    const int nq = head_slots(d.multires) / 4;  // 5
    Blob b;
    b.take(16);  // offset 0 is reserved as "absent"
    const size_t o_pe0 = b.take((size_t)kPairs * nq * 2 * 64);
    const int n_hid_blocks = (nl - 2) + (skip != -1 ? 1 : 0);
    const size_t o_head_skip = skip != -1 ? b.take((size_t)kPairs * nq * 2 * 64) : 0;
    const size_t o_hid = b.take((size_t)n_hid_blocks * kF4PerHidLayer);
    const size_t o_pes = b.take((size_t)kPairs * nq * 2 * 64);
    const size_t o_bias = b.take((size_t)(nl - 1) * kF4PerBiasLayer);
    const size_t o_last = b.take(kF4PerBiasLayer);
    const size_t o_feat = b.take(kF4PerHidLayer);
    const size_t o_bfeat = b.take(kF4PerBiasLayer);
    size_t n_scale = 0;
    for (int l = 0; l < nl; ++l) n_scale += (size_t)L[l].out_dim;
    const size_t o_scale = b.take((n_scale + 3) / 4);

    net->blob_bytes = b.n_f4 * sizeof(float4);
    IRON_HIP_TRY(hipMalloc(&net->blob, net->blob_bytes));
    IRON_HIP_TRY(hipMemsetAsync(net->blob, 0, net->blob_bytes, st));
    float4* base = (float4*)net->blob;
    float* scale_base = (float*)(base + o_scale);
    size_t soff[32];
    int rc = fold_scales(L, nl, scale_base, soff, st);
    if (rc != IRON_OK) return rc;

    HeadSrcs hs;
    memset(&hs, 0, sizeof(hs));
    hs.n = 1; hs.slot_base[0] = 0; hs.levels[0] = d.multires; hs.col_off[0] = 0;
    // layer 0
    launch_pack_head(base + o_pe0, make_pack_src(L[0], scale_base + soff[0], kHidden, 0, 1.0f), hs, nq, st);
    launch_pack_bias(base + o_bias, L[0].bias, 0, L[0].out_dim, st);
    // hidden layers 1..nl-2
    for (int l = 1; l <= nl - 2; ++l) {
        const bool is_skip = (l == skip);
        const float mul = is_skip ? kInvSqrt2 : 1.0f;
        const int cols_valid = is_skip ? kHidden - pe : kHidden;
        launch_pack_hidden(base + o_hid + (size_t)(l - 1) * kF4PerHidLayer,
                           make_pack_src(L[l], scale_base + soff[l], L[l].out_dim, 0, mul), 0, cols_valid, st);
        launch_pack_bias(base + o_bias + (size_t)l * kF4PerBiasLayer, L[l].bias, 0, L[l].out_dim, st);
        if (is_skip) {
            HeadSrcs h2 = hs;
            h2.col_off[0] = kHidden - pe;
            launch_pack_head(base + o_pes, make_pack_src(L[l], scale_base + soff[l], L[l].out_dim, 0, mul), h2, nq, st);
        }
    }
    // last layer: row 0 = sdf, rows 1.. = feature
    const iron_linear& last = L[nl - 1];
    launch_pack_row(base + o_last, make_pack_src(last, scale_base + soff[nl - 1], 1, 0, 1.0f), 0, 0, kHidden, st);
    if (d.d_out == kHidden + 1) {
        launch_pack_hidden(base + o_feat, make_pack_src(last, scale_base + soff[nl - 1], kHidden, 1, 1.0f), 0, kHidden, st);
        launch_pack_bias(base + o_bfeat, last.bias, 1, kHidden, st);
    }
    IRON_HIP_TRY(hipGetLastError());
    float b_last = 0.0f;
    IRON_HIP_TRY(hipMemcpyAsync(&b_last, last.bias, sizeof(float), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));

    SdfNetDev& s = net->sdf;
    s.blob = net->blob;
    s.blob_bytes = (uint32_t)net->blob_bytes;
    s.w_pe0 = (uint32_t)(o_pe0 * 16);
    s.w_hid = (uint32_t)(o_hid * 16);
    s.w_pe_skip = (uint32_t)(o_pes * 16);
    s.bias = (uint32_t)(o_bias * 16);
    s.w_last = (uint32_t)(o_last * 16);
    s.w_feat = (d.d_out == kHidden + 1) ? (uint32_t)(o_feat * 16) : 0u;
    s.b_feat = (uint32_t)(o_bfeat * 16);
    s.b_last = b_last;
    s.scale = d.scale;
    s.n_hidden_layers = nl - 1;
    s.skip_layer = skip;
    { const int rc_h2 = build_h2_sdf(net, L, scale_base, soff, st); if (rc_h2 != IRON_OK) return rc_h2; }
    return build_w16_sdf(net, L, scale_base, soff, st);
}

int create_render(iron_net* net, const iron_linear* L, hipStream_t st) {
    const iron_net_desc& d = net->desc;
    const int nl = d.n_linear;
    if (d.d_hidden != kHidden || d.d_feature != kHidden || nl < 2 || nl > 17) return IRON_ERR_UNSUPPORTED;
    // a skip connection is supported at a hidden layer (the stage-1 colour net: 8 layers, skip_in = [4]); the reference
    // also builds 4-layer nets with skip_in = (4,), i.e. at the OUTPUT layer: not built
    const int skip = d.skip_layer;
    if (!(skip == -1 || (skip >= 1 && skip <= nl - 2))) return IRON_ERR_UNSUPPORTED;
    if (d.d_out < 1 || d.d_out > 3) return IRON_ERR_UNSUPPORTED;

    RenderNetDev& r = net->rnd;
    memset(&r, 0, sizeof(r));
    HeadSrcs hs;
    memset(&hs, 0, sizeof(hs));
    const int lv_p = d.multires > 0 ? d.multires : 0;
    const int lv_v = d.multires_view > 0 ? d.multires_view : 0;
    auto add_src = [&](int kind, int levels, int& slot, int& col) {
        const int k = hs.n++;
        hs.slot_base[k] = slot; hs.levels[k] = levels; hs.col_off[k] = col;
        r.src_kind[k] = kind; r.src_levels[k] = levels;
        slot += head_slots(levels);
        col += pe_width(levels);
    };
    int slot = 0, col = 0;
    switch (d.mode) {  // input order: models/fields.py:213-220
        case IRON_MODE_IDR: add_src(0, lv_p, slot, col); add_src(1, lv_v, slot, col); add_src(2, 0, slot, col); break;
        case IRON_MODE_NO_VIEW_DIR: add_src(0, lv_p, slot, col); add_src(2, 0, slot, col); break;
        case IRON_MODE_NO_NORMAL: add_src(0, lv_p, slot, col); add_src(1, lv_v, slot, col); break;
        case IRON_MODE_POINTS_ONLY: add_src(0, lv_p, slot, col); break;
        default: return IRON_ERR_UNSUPPORTED;
    }
    r.n_src = hs.n;
    const int head_w = col;
    int nq;
    if (slot <= 20) nq = 5; else if (slot <= 24) nq = 6; else if (slot <= 48) nq = (slot + 3) / 4; else return IRON_ERR_UNSUPPORTED;
    for (int l = 0; l < nl; ++l) {
        if (!L[l].weight_v || !L[l].bias) return IRON_ERR_BAD_ARG;
        const int want_in = (l == 0) ? head_w + d.d_feature : (l == skip ? kHidden + head_w + d.d_feature : kHidden);
        const int want_out = (l == nl - 1) ? d.d_out : kHidden;
        if (L[l].in_dim != want_in || L[l].out_dim != want_out) return IRON_ERR_UNSUPPORTED;
    }
    Blob b;
    b.take(16);
    const size_t o_head = b.take((size_t)kPairs * nq * 2 * 64);
    const size_t o_head_skip = skip != -1 ? b.take((size_t)kPairs * nq * 2 * 64) : 0;
    // the feature block of layer 0 and the hidden blocks form ONE contiguous stream (the kernel's weight FIFO runs through)
    const size_t o_feat0 = b.take(kF4PerHidLayer);
    const int n_hid_blocks = (nl - 2) + (skip != -1 ? 1 : 0);
    const size_t o_hid = b.take((size_t)n_hid_blocks * kF4PerHidLayer);
    const size_t o_bias = b.take((size_t)(nl - 1) * kF4PerBiasLayer);
    const size_t o_last = b.take(3 * kF4PerBiasLayer);
    size_t n_scale = 0;
    for (int l = 0; l < nl; ++l) n_scale += (size_t)L[l].out_dim;
    const size_t o_scale = b.take((n_scale + 3) / 4);
    net->blob_bytes = b.n_f4 * sizeof(float4);
    IRON_HIP_TRY(hipMalloc(&net->blob, net->blob_bytes));
    IRON_HIP_TRY(hipMemsetAsync(net->blob, 0, net->blob_bytes, st));
    float4* base = (float4*)net->blob;
    float* scale_base = (float*)(base + o_scale);
    size_t soff[32];
    int rc = fold_scales(L, nl, scale_base, soff, st);
    if (rc != IRON_OK) return rc;

    launch_pack_head(base + o_head, make_pack_src(L[0], scale_base + soff[0], kHidden, 0, 1.0f), hs, nq, st);
    launch_pack_hidden(base + o_feat0, make_pack_src(L[0], scale_base + soff[0], kHidden, 0, 1.0f), head_w, kHidden, st);
    launch_pack_bias(base + o_bias, L[0].bias, 0, kHidden, st);
    for (int l = 1, blk = 0; l <= nl - 2; ++l) {
        if (l == skip) {  // [x | head inputs | features] / sqrt(2): x block, head block, feature block
            const PackSrc ps = make_pack_src(L[l], scale_base + soff[l], kHidden, 0, kInvSqrt2);
            launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer, ps, 0, kHidden, st);
            HeadSrcs hs2 = hs;
            for (int k = 0; k < hs2.n; ++k) hs2.col_off[k] += kHidden;
            launch_pack_head(base + o_head_skip, ps, hs2, nq, st);
            launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer, ps, kHidden + head_w, kHidden, st);
        } else {
            launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer,
                               make_pack_src(L[l], scale_base + soff[l], kHidden, 0, 1.0f), 0, kHidden, st);
        }
        launch_pack_bias(base + o_bias + (size_t)l * kF4PerBiasLayer, L[l].bias, 0, kHidden, st);
    }
    const iron_linear& last = L[nl - 1];
    for (int o = 0; o < d.d_out; ++o)
        launch_pack_row(base + o_last + (size_t)o * kF4PerBiasLayer, make_pack_src(last, scale_base + soff[nl - 1], d.d_out, 0, 1.0f),
                        o, 0, kHidden, st);
    IRON_HIP_TRY(hipGetLastError());
    float bl[3] = {0, 0, 0};
    IRON_HIP_TRY(hipMemcpyAsync(bl, last.bias, sizeof(float) * d.d_out, hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));

    r.blob = net->blob;
    r.blob_bytes = (uint32_t)net->blob_bytes;
    r.w_head0 = (uint32_t)(o_head * 16);
    r.w_feat0 = (uint32_t)(o_feat0 * 16);
    r.w_hid = (uint32_t)(o_hid * 16);
    r.bias = (uint32_t)(o_bias * 16);
    r.w_last = (uint32_t)(o_last * 16);
    for (int o = 0; o < 3; ++o) r.b_last[o] = bl[o];
    r.d_out = d.d_out;
    r.n_hidden_layers = nl - 1;
    r.head_quads = nq;
    r.skip_layer = skip;
    r.w_head_skip = (uint32_t)(o_head_skip * 16);
    r.squeeze_out = d.squeeze_out;
    r.squeeze_out_scale = d.squeeze_out_scale;
    r.output_bias = d.output_bias;
    r.output_scale = d.output_scale;
    return build_h2_render(net, L, scale_base, soff, hs, head_w, st);
}

// NeRF background field (models/fields.py:243-297).  layers: pts_linears[0..D-1], alpha_linear, feature_linear,
// views_linears[0], rgb_linear.
int create_nerf(iron_net* net, const iron_linear* L, hipStream_t st) {
    const iron_net_desc& d = net->desc;
    const int D = d.n_linear - 4;
    const int lp = d.multires > 0 ? d.multires : 0, lv = d.multires_view > 0 ? d.multires_view : 0;
    const int skip = d.skip_layer;  // h = cat([x, h]) after layer `skip`
    if (d.d_hidden != kHidden || D < 2 || D > 14 || lp < 1 || lp > 10) return IRON_ERR_UNSUPPORTED;
    if (!(skip == -1 || (skip >= 0 && skip <= D - 2))) return IRON_ERR_UNSUPPORTED;
    const int in_p = 4 + 8 * lp, in_v = pe_width(lv);
    const int nq4 = (2 + 4 * lp + 3) / 4, nqv = (head_slots(lv) + 3) / 4;
    if (nq4 > 12 || nqv > 12) return IRON_ERR_UNSUPPORTED;
    for (int l = 0; l < d.n_linear; ++l) {
        if (!L[l].weight_v || !L[l].bias) return IRON_ERR_BAD_ARG;
        int want_in = kHidden, want_out = kHidden;
        if (l == 0) want_in = in_p;
        else if (l < D && l == skip + 1 && skip != -1) want_in = kHidden + in_p;
        if (l == D) want_out = 1;                                   // alpha_linear
        if (l == D + 2) { want_in = in_v + kHidden; want_out = kHidden / 2; }  // views_linears[0]
        if (l == D + 3) { want_in = kHidden / 2; want_out = 3; }    // rgb_linear
        if (L[l].in_dim != want_in || L[l].out_dim != want_out) return IRON_ERR_UNSUPPORTED;
    }
    NerfNetDev& r = net->nerf;
    memset(&r, 0, sizeof(r));
    Blob b;
    b.take(16);
    const size_t o_head0 = b.take((size_t)kPairs * nq4 * 2 * 64);
    const size_t o_head_skip = b.take((size_t)kPairs * nq4 * 2 * 64);
    const size_t o_head_view = b.take((size_t)kPairs * nqv * 2 * 64);
    const int n_blocks = (D - 1) + 2;  // hidden layers 1..D-1, feature layer, view layer
    const size_t o_hid = b.take((size_t)n_blocks * kF4PerHidLayer + kF4PerHidLayer / 8);  // + slack for the FIFO's look-ahead
    const size_t o_bias = b.take((size_t)(D + 2) * kF4PerBiasLayer);
    const size_t o_alpha = b.take(kF4PerBiasLayer);
    const size_t o_rgb = b.take(3 * kF4PerBiasLayer);
    size_t n_scale = 0;
    for (int l = 0; l < d.n_linear; ++l) n_scale += (size_t)L[l].out_dim;
    const size_t o_scale = b.take((n_scale + 3) / 4);
    net->blob_bytes = b.n_f4 * sizeof(float4);
    IRON_HIP_TRY(hipMalloc(&net->blob, net->blob_bytes));
    IRON_HIP_TRY(hipMemsetAsync(net->blob, 0, net->blob_bytes, st));
    float4* base = (float4*)net->blob;
    float* scale_base = (float*)(base + o_scale);
    size_t soff[32];
    int rc = fold_scales(L, d.n_linear, scale_base, soff, st);  // plain nn.Linear: weight_g == NULL -> scale 1
    if (rc != IRON_OK) return rc;
    auto head4 = [&](size_t dst, const iron_linear& lin, const float* sc, int col_off) {
        const int n = kPairs * nq4 * 2 * 64;
        hipLaunchKernelGGL(k_pack_head4, dim3((n + 255) / 256), dim3(256), 0, st, base + dst, make_pack_src(lin, sc, kHidden, 0, 1.0f), lp,
                           col_off, nq4);
    };
    head4(o_head0, L[0], scale_base + soff[0], 0);
    launch_pack_bias(base + o_bias, L[0].bias, 0, kHidden, st);
    int blk = 0;
    for (int l = 1; l < D; ++l) {
        const bool skip_in = (skip != -1 && l == skip + 1);  // input = [x (in_p) | h (256)]
        if (skip_in) head4(o_head_skip, L[l], scale_base + soff[l], 0);
        launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer, make_pack_src(L[l], scale_base + soff[l], kHidden, 0, 1.0f),
                           skip_in ? in_p : 0, kHidden, st);
        launch_pack_bias(base + o_bias + (size_t)l * kF4PerBiasLayer, L[l].bias, 0, kHidden, st);
    }
    // feature_linear (no activation)
    launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer, make_pack_src(L[D + 1], scale_base + soff[D + 1], kHidden, 0, 1.0f), 0,
                       kHidden, st);
    launch_pack_bias(base + o_bias + (size_t)D * kF4PerBiasLayer, L[D + 1].bias, 0, kHidden, st);
    // views_linears[0]: input = [feature (256) | PE(view)], 128 outputs (rows 128..255 of the block stay zero)
    launch_pack_hidden(base + o_hid + (size_t)(blk++) * kF4PerHidLayer, make_pack_src(L[D + 2], scale_base + soff[D + 2], kHidden / 2, 0, 1.0f),
                       0, kHidden, st);
    {
        HeadSrcs hv;
        memset(&hv, 0, sizeof(hv));
        hv.n = 1; hv.slot_base[0] = 0; hv.levels[0] = lv; hv.col_off[0] = kHidden;
        launch_pack_head(base + o_head_view, make_pack_src(L[D + 2], scale_base + soff[D + 2], kHidden / 2, 0, 1.0f), hv, nqv, st);
    }
    launch_pack_bias(base + o_bias + (size_t)(D + 1) * kF4PerBiasLayer, L[D + 2].bias, 0, kHidden / 2, st);
    launch_pack_row(base + o_alpha, make_pack_src(L[D], scale_base + soff[D], 1, 0, 1.0f), 0, 0, kHidden, st);
    for (int o = 0; o < 3; ++o)
        launch_pack_row(base + o_rgb + (size_t)o * kF4PerBiasLayer, make_pack_src(L[D + 3], scale_base + soff[D + 3], 3, 0, 1.0f), o, 0,
                        kHidden / 2, st);
    IRON_HIP_TRY(hipGetLastError());
    float ba = 0.f, brgb[3] = {0, 0, 0};
    IRON_HIP_TRY(hipMemcpyAsync(&ba, L[D].bias, sizeof(float), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipMemcpyAsync(brgb, L[D + 3].bias, 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    IRON_HIP_TRY(hipStreamSynchronize(st));
    r.blob = net->blob;
    r.blob_bytes = (uint32_t)net->blob_bytes;
    r.w_head0 = (uint32_t)(o_head0 * 16);
    r.w_head_skip = (uint32_t)(o_head_skip * 16);
    r.w_hid = (uint32_t)(o_hid * 16);
    r.w_head_view = (uint32_t)(o_head_view * 16);
    r.bias = (uint32_t)(o_bias * 16);
    r.w_alpha = (uint32_t)(o_alpha * 16);
    r.w_rgb = (uint32_t)(o_rgb * 16);
    r.b_alpha = ba;
    for (int o = 0; o < 3; ++o) r.b_rgb[o] = brgb[o];
    r.n_layers = D;
    r.skip_after = skip;
    r.levels = lp;
    r.levels_view = lv;
    return build_h2_nerf(net, L, scale_base, soff, st);
}

}  // namespace

extern "C" int iron_net_create(iron_net_t** out, const iron_net_desc* desc, const iron_linear* layers, void* stream) {
    if (!out || !desc || !layers) return IRON_ERR_BAD_ARG;
    *out = nullptr;
    int dev = 0;
    int rc = check_device(&dev);
    if (rc != IRON_OK) return rc;
    iron_net* net = new (std::nothrow) iron_net();
    if (!net) return IRON_ERR_BAD_ARG;
    memset(net, 0, sizeof(*net));
    net->desc = *desc;
    net->device = dev;
    hipStream_t st = (hipStream_t)stream;
    if (desc->kind == IRON_NET_SDF) rc = create_sdf(net, layers, st);
    else if (desc->kind == IRON_NET_RENDER) rc = create_render(net, layers, st);
    else if (desc->kind == IRON_NET_NERF) rc = create_nerf(net, layers, st);
    else rc = IRON_ERR_UNSUPPORTED;
    if (rc == IRON_OK && net->h2_blob) rc = envelope_create(net);
    if (rc != IRON_OK) {
        if (net->blob) (void)hipFree(net->blob);
        if (net->h2_blob) (void)hipFree(net->h2_blob);
        if (net->h2_rev_blob) (void)hipFree(net->h2_rev_blob);
        envelope_destroy(net);
        if (net->h2_scratch) (void)hipFree(net->h2_scratch);
        if (net->w16_blob) (void)hipFree(net->w16_blob);
        delete net;
        return rc;
    }
    *out = net;
    return IRON_OK;
}

extern "C" int iron_net_destroy(iron_net_t* net) {
    if (!net) return IRON_OK;
    if (net->blob) IRON_HIP_TRY(hipFree(net->blob));
    if (net->h2_blob) IRON_HIP_TRY(hipFree(net->h2_blob));
    if (net->h2_rev_blob) IRON_HIP_TRY(hipFree(net->h2_rev_blob));
    envelope_destroy(net);
    if (net->h2_scratch) IRON_HIP_TRY(hipFree(net->h2_scratch));
    if (net->w16_blob) IRON_HIP_TRY(hipFree(net->w16_blob));
    if (net->screen_calib) IRON_HIP_TRY(hipFree(net->screen_calib));
    delete net;
    return IRON_OK;
}
