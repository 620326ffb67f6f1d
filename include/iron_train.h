/* iron_train.h -- C ABI of iron_amd/csrc/libiron_train.so: the BACKWARD passes of the stage-2 render operators
 * (BASELINE config C3).  gfx950 only.
 *
 * The reference trains through torch.autograd: `SDFNetwork.get_all(is_training=True)` builds a second-order graph
 * (models/fields.py:120-137), `RenderingNetwork.forward` and `GGXColocatedRenderer.forward` are ordinary differentiable
 * torch code (models/fields.py:203-239, models/renderer_ggx.py:82-146), and `loss.backward()` in render_surface.py:533-653
 * walks that graph.  Each entry below is the backward of ONE of those operators, evaluated in closed form on the GPU; the
 * Python side (iron_amd/autograd.py) wraps forward (libiron_hip.so) + backward (this library) as torch.autograd.Function
 * so the reference's own render_fn / reparam_points / loss code runs unchanged on top.
 *
 * Method: the hit points of one call are processed as a batch, layer by layer, in fp32.  The forward activations are
 * recomputed from the inputs and kept in the caller's workspace (HBM is 288 GB: 37 KB per point for the SDF net), the
 * per-layer products (Z = X W^T, dX = dZ W, dW = dZ^T X with K = number of points) are this library's own split-fp16 MFMA GEMMs
 * (csrc/gemm_h2.h, exported as iron_train_gemm; no BLAS library is linked),
 * everything between them (positional encoding and its derivative, softplus-100 first and second derivative, the
 * forward-mode tangent rows that carry d(normal)/d(theta), weight-norm fold and its backward, column sums, the GGX
 * derivative) is hand-written HIP.
 *
 * Conventions as iron_hip.h: device pointers, fp32 row-major contiguous, caller-owned buffers and workspace, work enqueued
 * on `stream`, IRON_OK or a negative iron_status.  Parameter gradients are WRITTEN (not accumulated) to the d_* pointers
 * of each layer.  Threading: the two GEMM-based entries (iron_sdf_backward, iron_render_backward) serialise their host-side
 * enqueue per process; the work itself runs asynchronously on the caller's stream.
 * Operand range: every GEMM operand is split into two fp16 pieces; gradient operands are rescaled by a power of two from their
 * absolute maximum, all other operands (weights, recomputed activations, tangent rows) must stay below 65 504 in magnitude.
 */
#ifndef IRON_TRAIN_H
#define IRON_TRAIN_H

#include "iron_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One linear layer as the reference stores it (nn.utils.weight_norm: W = weight_g * weight_v / ||weight_v||_row). */
typedef struct iron_train_layer {
    const float* weight_v; /* [out,in]                                        */
    const float* weight_g; /* [out] or NULL (plain nn.Linear: W = weight_v)   */
    const float* bias;     /* [out]                                           */
    float* d_weight_v;     /* [out,in] out                                    */
    float* d_weight_g;     /* [out] out (ignored when weight_g is NULL)       */
    float* d_bias;         /* [out] out                                       */
    int32_t out_dim, in_dim;
} iron_train_layer;

/* SDFNetwork (models/fields.py:9-98): PE(multires) -> n_linear layers, softplus(beta=100) between them, one skip layer
 * whose input is cat[x, PE]/sqrt(2); scale must be 1. */
typedef struct iron_sdf_train_desc {
    int32_t n_linear;   /* 9 for the 8x256 network */
    int32_t multires;   /* 6 */
    int32_t skip_layer; /* 4, or -1 */
    const iron_train_layer* layers;
} iron_sdf_train_desc;

/* Backward of get_all (fields.py:120-137): given dL/d sdf [n], dL/d feature [n, d_out-1], dL/d gradient [n,3] (each may
 * be NULL = zero) at the points x [n,3], writes dL/d(weight_v, weight_g, bias) of every layer.  The second-order part
 * (dL/d gradient) is the reverse pass over a forward-mode tangent along v = dL/d gradient: <v, grad_x sdf> is the
 * directional derivative of the network along v, so its parameter gradient is one more (value, tangent) reverse sweep. */
size_t iron_sdf_backward_workspace_bytes(const iron_sdf_train_desc* desc, int64_t n);
int iron_sdf_backward(const iron_sdf_train_desc* desc, const float* x, int64_t n, const float* d_sdf, const float* d_feature,
                      const float* d_gradient, void* workspace, size_t workspace_bytes, void* stream);

/* RenderingNetwork (models/fields.py:141-239): input cat per `mode` (IRON_MODE_*), ReLU MLP with an optional skip layer,
 * y = output_scale * (z + output_bias), optional squeeze_out_scale * sigmoid(y). */
typedef struct iron_render_train_desc {
    int32_t n_linear;
    int32_t mode;
    int32_t multires, multires_view;
    int32_t d_feature, d_out;
    int32_t skip_layer; /* -1: none */
    int32_t squeeze_out;
    float output_bias, output_scale, squeeze_out_scale;
    const iron_train_layer* layers;
} iron_render_train_desc;

/* Backward of RenderingNetwork.forward: d_out [n,d_out] -> parameter gradients and (each nullable) d_points [n,3],
 * d_normals [n,3], d_view_dirs [n,3], d_features [n,d_feature].  normals / view_dirs may be NULL where the mode ignores
 * them. */
size_t iron_render_backward_workspace_bytes(const iron_render_train_desc* desc, int64_t n);
int iron_render_backward(const iron_render_train_desc* desc, const float* points, const float* normals, const float* view_dirs,
                         const float* features, int64_t n, const float* d_out, float* d_points, float* d_normals, float* d_view_dirs,
                         float* d_features, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of GGXColocatedRenderer.forward (models/renderer_ggx.py:82-146).  Upstream d_diffuse_rgb / d_specular_rgb /
 * d_rgb [n,3] (each nullable); outputs (each nullable): d_light [1] (device, written), d_distance [n], d_normal [n,3],
 * d_viewdir [n,3], d_diffuse_albedo [n,3], d_specular_albedo [n,3], d_roughness [n].  The two Mitsuba tables are
 * piecewise constant in (cos, alpha), so they carry no gradient (torch gives none either: integer indexing). */
int iron_ggx_colocated_backward(float light, const float* distance, const float* normal, const float* viewdir,
                                const float* diffuse_albedo, const float* specular_albedo, const float* roughness,
                                const float* tab_trans, const float* tab_diff, int64_t n, const float* d_diffuse_rgb,
                                const float* d_specular_rgb, const float* d_rgb, float* d_light, float* d_distance, float* d_normal,
                                float* d_viewdir, float* d_diffuse_albedo, float* d_specular_albedo, float* d_roughness, void* stream);

/* Backward of CompositeRenderer.forward (models/renderer_ggx.py:781-858), both branches (p->env_light != NULL: use_env_light,
 * intensity = clamp(env_light, 1e-6, 20); d_light / d_distance are then zero and d_env_light receives the gradient, including
 * that of the returned "env_light" key, d_env_light_out).  Upstream: d_rgb (the reference returns the SAME tensor as "rgb" and "diffuse_rgb"; pass
 * the sum of both keys' gradients), d_specular_rgb, d_metallic_rgb, d_dielectric_rgb, each [n,3] or NULL.  Outputs, each
 * nullable: d_light [1]; d_distance, the four scalar maps [n]; d_normal, d_viewdir, the two albedos [n,3].  Clamped inputs
 * carry gradient on the closed clamp interval, the diffuse tables none. */
typedef struct iron_composite_grads_in {
    const float* d_rgb;
    const float* d_specular_rgb;
    const float* d_metallic_rgb;
    const float* d_dielectric_rgb;
    const float* d_env_light_out; /* [n] or NULL (env-light branch: upstream of the returned clamped env light) */
} iron_composite_grads_in;
typedef struct iron_composite_grads_out {
    float* d_light;
    float* d_distance;
    float* d_normal;
    float* d_viewdir;
    float* d_diffuse_albedo;
    float* d_specular_albedo;
    float* d_specular_roughness;
    float* d_metallic_eta;
    float* d_metallic_k;
    float* d_dielectric_eta;
    float* d_env_light; /* [n] or NULL */
} iron_composite_grads_out;
int iron_composite_colocated_backward(float light, const float* distance, const float* normal, const float* viewdir,
                                      const iron_composite_params* p, const float* tab_trans, const float* tab_diff, int64_t n,
                                      const iron_composite_grads_in* upstream, const iron_composite_grads_out* out, void* stream);

/* Backward of iron_coloc_head (SmoothDielectric / ThinDielectric / SmoothConductorCoLoc / RoughConductorCoLoc renderers,
 * models/renderer_ggx.py:149-395; same `kind`, eta, k).  Upstream d_diffuse_rgb / d_specular_rgb / d_rgb [n,3], each nullable;
 * outputs as iron_ggx_colocated_backward (d_roughness is non-zero for kind 3 only). */
int iron_coloc_head_backward(int32_t kind, float light, float eta, float k, const float* distance, const float* normal,
                             const float* viewdir, const float* diffuse_albedo, const float* specular_albedo, const float* roughness,
                             int64_t n, const float* d_diffuse_rgb, const float* d_specular_rgb, const float* d_rgb, float* d_light,
                             float* d_distance, float* d_normal, float* d_viewdir, float* d_diffuse_albedo, float* d_specular_albedo,
                             float* d_roughness, void* stream);

/* NeRF (models/fields.py:243-327, use_viewdirs=True): D ReLU layers of width W on PE(input_pts), `skip` = the layer after
 * whose activation the encoded input is concatenated IN FRONT (fields.py:309-310; -1: none), then alpha (1), feature (W), one
 * view layer on cat[feature, PE(views)] and rgb (3).  layers = the D point layers followed by alpha, feature, view, rgb; plain
 * nn.Linear (weight_g NULL).  Backward: d_alpha [n,1] / d_rgb [n,3] (each nullable) -> parameter gradients; the inputs get
 * none (the reference feeds sample positions computed without grad, renderer.py:163-172). */
typedef struct iron_nerf_train_desc {
    int32_t D, W;
    int32_t d_in, d_in_view;
    int32_t multires, multires_view;
    int32_t skip;
    const iron_train_layer* layers;
} iron_nerf_train_desc;
size_t iron_nerf_backward_workspace_bytes(const iron_nerf_train_desc* desc, int64_t n);
int iron_nerf_backward(const iron_nerf_train_desc* desc, const float* pts, const float* views, int64_t n, const float* d_alpha,
                       const float* d_rgb, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of iron_neus_composite (the compositing of NeuSRenderer.render_core, models/renderer.py:279-344, with the
 * background blend of :174-178).  `fwd` = the forward call's argument block (its output pointers are ignored).  Upstream,
 * each nullable: d_color [n,3], d_weight_sum [n], d_weights [n, mo or m], d_gradient_error [1] (device; needs relax_count =
 * the forward's gradient_error_acc + 1, i.e. the sum of the relax mask).  Outputs, each nullable: d_sdf [n*m], d_grad
 * [n*m,3] (through the annealed cosine and the eikonal statistic), d_sample_color [n*m,3], d_inv_s [1], d_bg_density
 * [n*mo], d_bg_color [n*mo,3]. */
typedef struct iron_neus_composite_grads {
    const float* d_color;
    const float* d_weight_sum;
    const float* d_weights;
    const float* d_gradient_error;
    const float* relax_count;
    float* d_sdf;
    float* d_grad;
    float* d_sample_color;
    float* d_inv_s;
    float* d_bg_density;
    float* d_bg_color;
} iron_neus_composite_grads;
int iron_neus_composite_backward(const iron_neus_composite_args* fwd, const iron_neus_composite_grads* grads, void* stream);

/* The layer product every backward pass above is built from, on its own (tests / micro-benchmarks): row-major
 * C[m,n] = op(A) op(B) + beta C in fp32, computed by the library's hand-written split-fp16 MFMA GEMMs (csrc/gemm_h2.h; no BLAS
 * library).  op = 0: operand as stored ([m,k] / [k,n]); 1: transposed ([k,m] / [n,k]).  (0,1) = Z = X W^T, (0,0) = dX = dZ W,
 * (1,0) = dW = dZ^T X (there lda = m, ldb = n, ldc = n are implied: tightly packed, as inside the library); (1,1) is refused.
 * In (0,0) and (1,0) A is treated as a gradient: scaled by a power of two from its absolute maximum before the fp16 split. */
size_t iron_train_gemm_workspace_bytes(int32_t op_a, int32_t m, int32_t n);
int iron_train_gemm(int32_t op_a, int32_t op_b, int32_t m, int32_t n, int32_t k, const float* A, int32_t lda, const float* B, int32_t ldb,
                    float beta, float* C, int32_t ldc, void* workspace, size_t workspace_bytes, void* stream);

/* Operand range of the backward passes.  Their layer products split every fp32 operand into two fp16 pieces (csrc/gemm_h2.h); a
 * gradient operand is scaled by a power of two from its absolute maximum first, the other operands (activations, tangent rows,
 * weights) are split as they are, so an element beyond fp16's largest number (|x| > 65 504) or a non-finite one yields inf / NaN
 * gradients where the reference's fp32 autograd (render_surface.py:533-653) has ordinary numbers.  Every splitting kernel raises
 * a sticky device flag when it meets such an element; this call synchronises `stream` and returns IRON_ERR_RANGE if the flag is
 * up (and lowers it when `reset` is non-zero), IRON_OK otherwise.  The networks of the reference's scenes stay far inside the
 * range (weight_g up to 137, pre-activations about 10). */
int iron_train_numeric_status(int32_t reset, void* stream);

/* Stage-2 image losses (models/image_losses.py, used by render_surface.py:597-598), csrc/losses.hip.  Images are [B, C, H, W]
 * fp32 contiguous.  The loss is written to a DEVICE scalar `loss` [1]; the backward reads the upstream gradient from the DEVICE
 * scalar `d_loss` [1] and WRITES dx (and dy = d loss / d Y when non-NULL).  Every reduction is a fixed-order sum of per-workgroup
 * partials (no atomics): loss and gradients are bitwise reproducible.
 *
 * Pyramid L2 (PyramidL2Loss): n_planes = B*C planes of h x w, h and w >= 16 (IRON_ERR_UNSUPPORTED below).  `taps` (HOST [49])
 * is the 7x7 filter, row-major; it must be point symmetric (taps[48 - i] == taps[i]), which the backward relies on.  The
 * workspace holds the levels d_1..d_4 between the forward and the backward (pass the same one to both) and the backward's
 * scratch; it is under 2/3 of one input's size. */
size_t iron_pyramid_l2_workspace_bytes(int64_t n_planes, int32_t h, int32_t w);
int iron_pyramid_l2_forward(const float* x, const float* y, int64_t n_planes, int32_t h, int32_t w, const float* taps, float* loss,
                            void* workspace, size_t workspace_bytes, void* stream);
int iron_pyramid_l2_backward(const float* x, const float* y, int64_t n_planes, int32_t h, int32_t w, const float* taps,
                             const float* d_loss, void* workspace, size_t workspace_bytes, float* dx, float* dy, void* stream);

/* SSIM loss (ssim_loss_fn): `win` (HOST [win_size], odd, <= 21, else IRON_ERR_UNSUPPORTED) is the 1-D Gaussian applied along every
 * axis not shorter than win_size (a shorter axis is not smoothed); c1, c2 as the reference's (K1 data_range)^2, (K2 data_range)^2.
 * mask: NULL, or [B, 1, H, W] with mask_kind 1 (uint8 / bool: kept where non-zero) or 2 (fp32: kept where > 0.5); it is eroded by
 * a win x win window over the in-image pixels, and a masked call needs both axes >= win_size (IRON_ERR_UNSUPPORTED otherwise).
 * `state` (state_bytes from iron_ssim_workspace_bytes) carries the eroded mask and |E| from the forward to the backward;
 * `scratch` (scratch_bytes) is the backward's own. */
int iron_ssim_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t win_size, int32_t masked, size_t* state_bytes,
                              size_t* scratch_bytes);
int iron_ssim_forward(const float* x, const float* y, int32_t b, int32_t c, int32_t h, int32_t w, const float* win, int32_t win_size,
                      double c1, double c2, const void* mask, int32_t mask_kind, float* loss, void* state, size_t state_bytes,
                      void* stream);
int iron_ssim_backward(const float* x, const float* y, int32_t b, int32_t c, int32_t h, int32_t w, const float* win, int32_t win_size,
                       double c1, double c2, int32_t masked, const float* d_loss, const void* state, size_t state_bytes, void* scratch,
                       size_t scratch_bytes, float* dx, float* dy, void* stream);

/* gaussian_filter (inference): the "valid" separable blur with `win` (HOST [win_size]) of n_planes planes of h x w; out is
 * [n_planes, h', w'], h' = h - win_size + 1 when h >= win_size, else h (that axis is passed through); same for w. */
int iron_gaussian_filter(const float* x, int64_t n_planes, int32_t h, int32_t w, const float* win, int32_t win_size, float* out,
                         void* stream);

/* Multi-tensor Adam (csrc/optim.hip): torch.optim.Adam without weight decay or amsgrad over a HOST table of tensors,
 *     m <- m + (1 - beta1)(g - m);  v <- beta2 v + (1 - beta2) g^2;  p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with t = `step` (>= 1: the count AFTER this update, as torch keeps it) per tensor and both bias corrections formed in fp64.  All
 * four buffers of a tensor are fp32, `numel` long, 4-byte aligned (nothing more is assumed) and must not overlap another entry's.
 * zero_grad != 0: every gradient is left exactly 0, in the same pass.  The table is cut into chunks of IRON_ADAM_CHUNK elements
 * and travels in the kernels' argument block, IRON_ADAM_MAX_TENSORS tensors per launch: ceil(n_tensors / IRON_ADAM_MAX_TENSORS)
 * launches, no upload, no allocation, no host synchronisation.  IRON_ERR_BAD_ARG: a null pointer (with numel > 0), a negative
 * numel, step < 1, a beta outside [0, 1), a negative eps; nothing is enqueued then. */
#define IRON_ADAM_CHUNK 2048
#define IRON_ADAM_MAX_TENSORS 80
typedef struct iron_adam_tensor {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int64_t step;
    double lr;
} iron_adam_tensor;
int iron_adam_multi(const iron_adam_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps, int32_t zero_grad,
                    void* stream);

/* The regularisers of the stage-2 step (render_surface.py:580-613, 639), csrc/optim.hip.  Three sets of 3-vectors -- eik_grad
 * [m,3] (the uniform eikonal gradients), normal [n_pix,3] where mask [n_pix] (uint8, non-zero = kept) holds, edge_normal [e,3]
 * (NULL with e = 0) -- and roughness [n_pix]:
 *     eik_loss        = eik_weight * sum over the sets of (|g| - 1)^2 / cnt,  cnt = m + n_mask + e
 *     roughrange_loss = roughrange_weight * mean(r - 0.5 over masked r > 0.5), 0 when nothing is selected
 * As in the reference, the masked and the edge set enter only when the mask keeps at least one pixel (cnt = m otherwise).  Both
 * losses are DEVICE scalars; counts (DEVICE int64 [3]) = cnt, n_mask, number of selected roughness values; state (DEVICE double
 * [4]) carries the backward's scales.  Sums are per-workgroup partials in `workspace`, added in a fixed order in fp64 (no
 * atomics: bitwise reproducible).  The backward reads the upstream gradients d_eik / d_roughrange from DEVICE scalars (NULL =
 * zero) and WRITES every element of each non-NULL output: 2 (|g| - 1) g / |g| * eik_weight / cnt * d_eik on the vectors that
 * entered (0 for a zero vector and outside the mask), roughrange_weight / n * d_roughrange on the selected roughness values (r
 * == 0.5 is not selected), 0 elsewhere. */
typedef struct iron_surface_reg_args {
    const float* eik_grad;
    const float* normal;
    const uint8_t* mask;
    const float* roughness;
    const float* edge_normal;
    int64_t m, n_pix, e;
    float eik_weight, roughrange_weight;
} iron_surface_reg_args;
size_t iron_surface_reg_workspace_bytes(int64_t m, int64_t n_pix, int64_t e);
int iron_surface_reg(const iron_surface_reg_args* a, float* eik_loss, float* roughrange_loss, int64_t* counts, double* state,
                     void* workspace, size_t workspace_bytes, void* stream);
int iron_surface_reg_backward(const iron_surface_reg_args* a, const double* state, const float* d_eik, const float* d_roughrange,
                              float* d_eik_grad, float* d_normal, float* d_roughness, float* d_edge_normal, void* stream);

/* The loss of the stage-1 step (render_volume.py:458-496) and the statistics it logs (:507-510), csrc/volume_loss.hip.  Per ray
 * i < b: color_fine [b,3]; true_rgb (rows of rgb_stride >= 3 floats) and the RAW mask (rows of mask_stride >= 1 floats; NULL is
 * allowed when mask_weight <= 0) -- both may point into the [b,10] batch; weight_sum [b]; weight_max [b]; cdf_fine (first
 * column, rows of cdf_stride floats); gradient_error: DEVICE scalar (the renderer's eikonal statistic).
 *     m = raw > 0.5 when mask_weight > 0, else 1;  mask_sum = sum m + 1e-5
 *     color_fine_loss = sum |(c - t) m| / mask_sum;  psnr = 20 log10(1 / sqrt(sum (c - t)^2 m / (3 mask_sum)))  (+inf at c == t)
 *     mask_loss = mean over b of BCE(clip(weight_sum, 1e-3, 1 - 1e-3), m)  (torch's binary_cross_entropy)
 *     loss = color_fine_loss + igr_weight gradient_error + mask_weight mask_loss
 * `loss` is a DEVICE scalar; `record` (DEVICE fp32 [IRON_VL_RECORD]) holds the scalars at the IRON_VL_* indices; `state` (DEVICE
 * double [4]) carries the backward's scales.  Per-ray values are fp32, formed as torch forms them; the sums are per-workgroup
 * partials in `workspace`, added in a fixed order in fp64 by one final workgroup (no atomics: bitwise reproducible, and the cut
 * into workgroups depends on b alone).  The backward reads the upstream gradient from the DEVICE scalar d_loss (NULL = 1) and
 * WRITES every element of each non-NULL output:
 *     d_color [b,3]      = sign((c - t) m) m / mask_sum * d_loss            (sign(0) = 0)
 *     d_weight_sum [b]   = mask_weight / b * (-m / w + (1 - m) / (1 - w)) * d_loss where 1e-3 <= w <= 1 - 1e-3 (both fp32), else 0
 *     d_gradient_error   = igr_weight * d_loss
 * IRON_ERR_BAD_ARG: a null pointer, b < 1 or a stride too small; nothing is enqueued then. */
enum {
    IRON_VL_LOSS = 0, IRON_VL_COLOR = 1, IRON_VL_EIKONAL = 2, IRON_VL_MASK = 3, IRON_VL_PSNR = 4, IRON_VL_CDF = 5,
    IRON_VL_WEIGHT_MAX = 6, IRON_VL_MASK_SUM = 7, IRON_VL_RECORD = 8
};
typedef struct iron_volume_loss_args {
    const float* color_fine;
    const float* true_rgb;
    const float* mask;
    const float* weight_sum;
    const float* weight_max;
    const float* cdf_fine;
    const float* gradient_error;
    int64_t b, rgb_stride, mask_stride, cdf_stride;
    float igr_weight, mask_weight;
} iron_volume_loss_args;
size_t iron_volume_loss_workspace_bytes(int64_t b);
int iron_volume_loss(const iron_volume_loss_args* a, float* loss, float* record, double* state, void* workspace,
                     size_t workspace_bytes, void* stream);
int iron_volume_loss_backward(const iron_volume_loss_args* a, const double* state, const float* d_loss, float* d_color,
                              float* d_weight_sum, float* d_gradient_error, void* stream);

/* Gradients of the hash-grid encoding (iron_hip.h, iron_hashgrid_* block), csrc/hashgrid_train.hip.  x [n,3], dy [n, L F],
 * table and d_table [n_params, F], all fp32.
 *   iron_hashgrid_backward           d_table[idx_o][l-th level, f] = sum over points and corners of wgt_o dy[l,f]  (may be NULL);
 *                                    d_x [n,3] = sum_{l,f} dy[l,f] J[l,f,:]  (may be NULL; needs `table`, else it may be NULL).
 *   iron_hashgrid_backward_backward  the backward of d_x as a function of (dy, table), for the gradient g [n,3] arriving at d_x:
 *                                    d_dy[n,l,f] = sum_d J[l,f,d] g_d  (may be NULL), and the table term (may be NULL), which
 *                                    scatters dy[l,f] sum_d g_d live_d scale_l dw_o,d to corner o.  The second derivative with
 *                                    respect to x (the mixed terms of the trilinear form) is not built.
 * d_table is WRITTEN whole: an entry no corner touches is +0.0 whatever the buffer held.  It is bitwise reproducible and bitwise
 * invariant under a permutation of the points: contributions are rounded in fp64 to a multiple of a power-of-two unit and summed
 * as 64-bit integers in `workspace`; the unit's exponent is iron_hashgrid_grad_unit_exp(bound, n) with bound = max |dy| (first
 * order) or fl(fl(fl(3 max |g|) scale_l) max |dy|) (second order, per level), so that 8 n contributions stay inside 63 bits.  A
 * non-finite dy (or g) makes every entry NaN.  The per-point outputs (d_x, d_dy) are fixed-order fp32 sums that do not depend on
 * the other points.  The workspace is needed for d_table only; *_workspace_bytes returns 0 for a descriptor the layout refuses.
 * IRON_ERR_WORKSPACE: workspace too small.
 *   iron_hashgrid_backward_pair      d_table of iron_hashgrid_backward(dy1) plus d_table of iron_hashgrid_backward_backward(dy2, g)
 *                                    in ONE pass over the corners: per (corner, feature) the contribution wgt_o dy1[l,f] +
 *                                    c_o dy2[l,f] (c_o = sum_d g_d live_d scale_l dw_o,d, the second-order coefficient bit for
 *                                    bit) is formed in fp64, rounded once to the unit and added with one integer atomic, where
 *                                    the two calls round and add twice.  The unit's exponent per level is
 *                                    iron_hashgrid_grad_unit_exp(fl(max |dy1| + fl(fl(fl(3 max |g|) scale_l) max |dy2|)), n): the
 *                                    sum of the two bounds above.  d_table and the workspace are required; written whole, bitwise
 *                                    reproducible and permutation invariant as above; a non-finite dy1, dy2 or g makes every entry
 *                                    NaN; n = 0 writes zeros.  `table` is not read and may be NULL. */
size_t iron_hashgrid_backward_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n);
int iron_hashgrid_backward(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table_or_null, const float* dy,
                           float* d_table_or_null, float* d_x_or_null, void* workspace, size_t workspace_bytes, void* stream);
size_t iron_hashgrid_backward_backward_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n);
int iron_hashgrid_backward_backward(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table, const float* dy,
                                    const float* g, float* d_dy_or_null, float* d_table_or_null, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t iron_hashgrid_backward_pair_workspace_bytes(const iron_hashgrid_desc* desc, int64_t n);
int iron_hashgrid_backward_pair(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table_or_null,
                                const float* dy1, const float* dy2, const float* g, float* d_table, void* workspace,
                                size_t workspace_bytes, void* stream);
int iron_hashgrid_grad_unit_exp(float bound, int64_t n);   /* HOST: log2 of the fixed-point unit */

/* Fused training backward of the hash-grid field (iron_hip.h, iron_hashgrid_field_* block), csrc/hashgrid_field_train.hip;
 * definition and orders: DESIGN.md §29.  The forward of a training step IS iron_hashgrid_field_eval (out [n, n_out] and, when asked,
 * g [n, 3] = d out[:,0] / dp); nothing is kept but p.  For the adjoints d_out [n, n_out] and d_g [n, 3] (either may be NULL: zero)
 *   iron_hashgrid_field_backward   recomputes the forward per tile of points and writes
 *       d_weights [n_weights] fp32, flat in iron_hashgrid_field_pack's weight order: the first-order term sum_n delta_l h_{l-1}^T plus
 *                   the second-order (eikonal) term sum_n d_l hdot_{l-1}^T;
 *       d_table [n_params, F] (may be NULL): iron_hashgrid_backward_pair(x = a p + b, dy1 = ybar, dy2 = e, g = a d_g on live axes);
 *       ybar, e [n, L F] (may be NULL): the adjoint of the features and the chain vector W_0^T d_0, per point.
 *     No gradient reaches p.  ybar and e of a point depend on that point alone.  d_weights is bitwise reproducible: the points are
 *     cut into slots of iron_hashgrid_field_train_slot(n) consecutive points (HOST; a function of n alone), a slot's sum is an fp32
 *     accumulation over its points in ascending order (per pair of points the first-order product, then the second-order one), and
 *     the slots are added in fp64 in a fixed order and rounded to fp32 once.  n = 0: IRON_OK, d_weights and d_table zeros.
 *   iron_hashgrid_field_train_check   HOST.  IRON_OK for a shape the backward is built for: whatever iron_hashgrid_field_check
 *     accepts with n_neurons <= 64 whose stages fit the 160 KiB of LDS at 32 points: with r(v) = v rounded up to 32, the stages take
 *     3 r(n_neurons) rows per hidden layer (4 with Softplus) plus 2 r(L F) + 32 rows, of 4 (P + 1) bytes each at P points per tile
 *     (132 bytes at P = 32, the size the check uses; 260 at P = 64, taken where it fits).  IRON_ERR_RANGE otherwise (n_neurons = 128
 *     always).
 *   iron_hashgrid_field_train_pack    `packed` is iron_hashgrid_field_pack's blob, unchanged; `train_packed` holds the transposed
 *     fragments of the output layer, which the adjoint chain needs and the inference blob lacks.  Repack both when a weight changes.
 * workspace: 256-byte aligned, *_workspace_bytes(desc, n) bytes (0 for a refused descriptor); IRON_ERR_WORKSPACE if too small. */
int iron_hashgrid_field_train_check(const iron_hashgrid_field_desc* desc);
int64_t iron_hashgrid_field_train_slot(int64_t n);
size_t iron_hashgrid_field_train_pack_bytes(const iron_hashgrid_field_desc* desc);
int iron_hashgrid_field_train_pack(const iron_hashgrid_field_desc* desc, const float* weights, void* train_packed, void* stream);
size_t iron_hashgrid_field_backward_workspace_bytes(const iron_hashgrid_field_desc* desc, int64_t n);
int iron_hashgrid_field_backward(const iron_hashgrid_field_desc* desc, const float* p, int64_t n, const float* map_a3_or_null,
                                 const float* map_b3_or_null, const float* table, const void* packed, const void* train_packed,
                                 const float* d_out_or_null, const float* d_g_or_null, float* d_weights, float* d_table_or_null,
                                 float* ybar_out_or_null, float* e_out_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostics: last hipError_t seen by this library on the calling thread (iron_train_last_blas_status: kept for ABI
 * stability, always 0: the library links no BLAS). */
int iron_train_last_hip_error(void);
int iron_train_last_blas_status(void);

#ifdef __cplusplus
}
#endif
#endif
