/*
 * iron_hip.h -- C ABI of libiron_hip.so, the MI355X (gfx950) implementation of IRON's
 * stage-2 forward render path (sphere-trace + normal/material MLPs + co-located GGX).
 *
 * The reference (arthurlirui/IRON) has no FFI layer: its boundary for this path is the Python
 * operator surface of models/raytracer.py, models/renderer_ggx.py, models/rendering_func.py
 * and models/fields.py.  Each entry point below names the reference function it replaces
 * (file:line, relative to the reference root); iron_amd/*.py binds them with ctypes and
 * re-exposes the reference's names.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer unless marked HOST.
 *   - all arrays are contiguous row-major fp32 unless noted; masks are uint8 (0/1), i.e. the
 *     storage of a torch.bool tensor.
 *   - all buffers are caller-allocated and caller-owned; the library keeps nothing past the call
 *     except the packed weight copy made by iron_net_create().
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     the host, nothing allocates (graph-capturable) except iron_net_create/destroy.
 *   - return value: IRON_OK (0) or a negative iron_status; no exceptions / aborts cross the ABI.
 *   - handles are immutable after create and may be shared between host threads.
 */
#ifndef IRON_HIP_H
#define IRON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRON_ABI_VERSION 1

typedef enum iron_status {
    IRON_OK = 0,
    IRON_ERR_BAD_ARG = -1,      /* null pointer, negative size, misaligned buffer;
                                   iron_bvh_boxes, iron_mesh_components, iron_uv_projections: a face indexes
                                   outside the vertices or has a non-finite vertex */
    IRON_ERR_UNSUPPORTED = -2,  /* network shape / mode the kernels are not built for          */
    IRON_ERR_HIP = -3,          /* a HIP runtime call failed; see iron_last_hip_error()        */
    IRON_ERR_NO_DEVICE = -4,    /* no gfx950 device visible                                    */
    IRON_ERR_WORKSPACE = -5,    /* workspace too small                                         */
    IRON_ERR_RANGE = -6         /* IRON_H2_OVERFLOW=error: the previous call on this network left the fp16 range of the h2 core
                                   (returned by every entry on that handle until iron_net_force_exact(net, 1));
                                   iron_mc_count: a vertex or triangle count reaches 2^31;
                                   iron_bake_*: see that block */
} iron_status;

int iron_version(void);
const char* iron_strerror(int status);
/* hipError_t (as int) of the last failing HIP call on this host thread, 0 if none. */
int iron_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------
 * Networks.  Replaces the parameter side of models/fields.py:9-98 (SDFNetwork) and :141-239
 * (RenderingNetwork).  Input format = the reference state_dict: per linear layer `weight_v`
 * [out,in], `weight_g` [out] (old-style weight_norm, fields.py:75-76; NULL for a plain layer,
 * then weight_v is the weight itself) and `bias` [out].  The library folds the weight norm
 * (W = v * g/||v||_row) and re-packs into its MFMA fragment layout on the device.
 * ------------------------------------------------------------------------------------------- */
typedef struct iron_net iron_net_t; /* opaque */

typedef struct iron_linear {
    const float* weight_v; /* [out_dim, in_dim] */
    const float* weight_g; /* [out_dim] or NULL  */
    const float* bias;     /* [out_dim]          */
    int32_t out_dim;
    int32_t in_dim;
} iron_linear;

enum { IRON_NET_SDF = 0, IRON_NET_RENDER = 1, IRON_NET_NERF = 2 };
enum { IRON_MODE_IDR = 0, IRON_MODE_NO_VIEW_DIR = 1, IRON_MODE_NO_NORMAL = 2, IRON_MODE_POINTS_ONLY = 3 };

typedef struct iron_net_desc {
    int32_t kind;          /* IRON_NET_SDF | IRON_NET_RENDER | IRON_NET_NERF                        */
    int32_t n_linear;      /* number of linear layers (= n_layers + 1)                              */
    int32_t d_hidden;      /* hidden width (256)                                                    */
    int32_t d_out;         /* SDF: 1 (sdf only) or 257 (sdf + feature); RENDER: 1..3; NERF: 4        */
    int32_t multires;      /* PE levels on points (SDF: 6)                                          */
    int32_t multires_view; /* RENDER: PE levels on view_dirs (<=0: none)                            */
    int32_t skip_layer;    /* index of the skip-concat layer, -1 if none (SDF: 4)                   */
    int32_t mode;          /* RENDER: IRON_MODE_*                                                   */
    int32_t d_feature;     /* RENDER: width of the feature vector input (256)                       */
    int32_t squeeze_out;   /* RENDER: apply squeeze_out_scale*sigmoid()                             */
    float squeeze_out_scale;
    float output_bias;     /* RENDER: x = output_scale * (x + output_bias)                          */
    float output_scale;
    float scale;           /* SDF: input scale (fields.py:83,98)                                    */
} iron_net_desc;

/* Accepted shapes (d_hidden = 256 throughout; tests/test_gpu_net_shapes.py computes each family against an fp64 oracle):
 *   SDF:    n_linear 3..17, multires 6, skip_layer -1 or 2..n_linear-2, d_out 1 or 257, scale > 0, weight_g or NULL.
 *           n_linear 9 with skip 4 runs on the default (h2) core, every other shape on the exact-fp32 core.
 *           The backward (include/iron_train.h) covers every accepted shape with scale = 1.
 *   RENDER: n_linear 2..17, d_feature 256, d_out 1..3, squeeze / bias / scale any, weight_g or NULL; skip_layer -1 or
 *           1..n_linear-2 (idr, PE 10 points / 4 views only; n_linear 9 with skip 4 on the h2 core).  The (mode, PE) pairs with a
 *           kernel: idr 0/4, no_view_dir 6, points_only 6 (h2 core at an even number of hidden layers <= 8), idr 10/4 with a skip.
 *           Any other pair (no_normal among them) is created but refused by the first evaluation (IRON_ERR_UNSUPPORTED).
 *   NERF:   D = n_linear - 4 in 2..14, skip -1..D-2, PE 10 / 4 (other levels are created but refused by iron_nerf_forward);
 *           D 8 with skip 4 on the h2 core.
 * Anything else fails here with IRON_ERR_UNSUPPORTED. */

/* Build a packed network on the current device.  `layers` is a HOST array of n_linear entries
 * whose pointers are DEVICE pointers.  Synchronises `stream` before returning (the source
 * tensors may be freed afterwards).  Must be re-run when parameters change. */
int iron_net_create(iron_net_t** out, const iron_net_desc* desc, const iron_linear* layers, void* stream);
int iron_net_destroy(iron_net_t* net);

/* Numeric envelope of the default ("h2", split-fp16) core: weights are checked at create (a network with a folded |w| >= 65 504
 * runs on the exact-fp32 core); activations and features are guarded at run time: every entry that ran a network on the h2 core
 * scans the values it returns, a non-finite one raises the network's flag, and the NEXT entry on that handle moves the network to
 * the exact-fp32 MFMA core for good (IRON_H2_OVERFLOW=error: returns IRON_ERR_RANGE instead, and keeps returning it until
 * iron_net_force_exact(net, 1) has pinned the handle to the exact core).  The reference is plain fp32
 * (models/fields.py:82-98, 203-239), which the exact core reproduces over the whole fp32 range.  The call that overflowed is loud
 * row by row: a returned row that an out-of-range operand reached is non-finite (the tracer and the edge walk write NaN into
 * sdf_out / dist / points of such a ray or candidate), never a plausible number.  Not covered: IRON_MLP_CORE=w16 (opt-in, per
 * process) and iron_sdf_screen_forward (a debug entry with a guard word of its own).
 *   iron_net_numeric_status: synchronises `stream`; *status_out = bit 0: an overflow was seen, bit 1: the network runs on the exact
 *                            core, bit 2: a flag is pending (the call just finished overflowed),
 *                            bit 3: the dense sampler's screen guard has turned the screen off for this network (iron_set_sampler_screen),
 *                            bit 4: the slope guard has put the screen's adaptive march on stride 1 for this network (iron_set_sampler_stride).
 *   iron_net_force_exact:    on != 0 pins the network to the exact core and answers a pending flag (bit 2 falls, bit 0 records it);
 *                            0 returns it to the default core and clears the status (bits 0-4). */
int iron_net_numeric_status(const iron_net_t* net, int32_t* status_out, void* stream);
int iron_net_force_exact(iron_net_t* net, int32_t on);

/* ---------------------------------------------------------------------------------------------
 * Batched field queries
 * ------------------------------------------------------------------------------------------- */
/* SDFNetwork.forward / .sdf (models/fields.py:82-104).  x [n,3] -> out [n,out_cols],
 * out_cols = 1 (sdf only) or d_out (sdf + feature). */
int iron_sdf_forward(const iron_net_t* sdf, const float* x, int64_t n, float* out, int32_t out_cols, void* stream);

/* SDFNetwork.get_all(x, is_training=False) (models/fields.py:120-137): sdf [n], feature
 * [n,d_out-1], grad = d sdf/dx [n,3] (closed form, no autograd graph).  Any output may be NULL.
 * `workspace` (iron_sdf_get_all_workspace_bytes(sdf, n) bytes, 16-byte aligned, caller-owned, contents undefined afterwards) is
 * the tape of the reverse-mode kernel: forward pass, then ONE reverse sweep over transposed weights (csrc/getall_rev.hip) -- what
 * autograd.grad does in the reference.  The query returns 0 for a network that has no reverse stream (any shape other than the
 * reference's 8 x 256 / skip 4 / PE-6 / 257 outputs, or IRON_GETALL=fwd); with workspace == NULL the gradient is evaluated as
 * three forward-mode tangents instead (same results to rounding, 2.3x the matrix work). */
size_t iron_sdf_get_all_workspace_bytes(const iron_net_t* sdf, int64_t n);
int iron_sdf_get_all(const iron_net_t* sdf, const float* x, int64_t n, float* sdf_out, float* feature,
                     float* grad, void* workspace, size_t workspace_bytes, void* stream);

/* RenderingNetwork.forward (models/fields.py:203-239).  view_dirs may be NULL for modes that do
 * not read it.  out [n,d_out].
 * A net with a skip connection (skip_layer >= 1: the stage-1 colour net) parks the skip layer's partial sums in a scratch buffer
 * owned by the handle: calls on ONE such handle must be ordered on one stream (different handles are independent). */
int iron_render_forward(const iron_net_t* net, const float* points, const float* normals,
                        const float* view_dirs, const float* features, int64_t n, float* out, void* stream);

/* NeRF.forward (models/fields.py:299-327, use_viewdirs=True): pts [n,4] (the stage-1 background
 * parametrisation (x/r, 1/r)), view_dirs [n,3] -> alpha [n] (raw density), rgb [n,3] (raw).  The net is created with
 * kind IRON_NET_NERF, d_hidden 256, multires / multires_view = PE levels, skip_layer = the layer after which the input is
 * concatenated again (4), n_linear = D + 4 layers in the order pts_linears[0..D-1], alpha_linear, feature_linear,
 * views_linears[0], rgb_linear (plain nn.Linear: weight_g = NULL). */
int iron_nerf_forward(const iron_net_t* nerf, const float* pts4, const float* view_dirs, int64_t n, float* alpha, float* rgb,
                      void* stream);

/* Per-ray stages of NeuSRenderer.render (models/renderer.py:346-453; rows of at most 192 samples, one thread per ray):
 *   iron_neus_linspace    z = near + (far - near) * linspace(0,1,m)                              (:357-358)
 *   iron_neus_outside_z   z = far / rev[j] + offset: depths of the n_outside background samples            (:380-381)
 *   iron_neus_points      pts = o + d * z                                                        (:389, :236)
 *   iron_neus_up_sample   up_sample (:189-232) + sample_pdf(det=True) (:45-75): n_importance new depths per ray
 *   iron_neus_merge       the sort of cat([z, new_z]) as a merge of two ascending rows, sdf carried along (:238-246)
 *   iron_neus_mid_points  section lengths, mid points and per-sample dirs of render_core (:265-277); outside != 0: the
 *                         (x/r, 1/r) parametrisation of render_core_outside (:163-172), pts [n*m,4]
 *   iron_neus_need_background  which samples of the fed row the compositing takes from the background field: all outside samples
 *                         and the inside samples whose mid point lies outside the unit sphere (the rest are multiplied by
 *                         (1 - inside_sphere) = 0, :300-312); lets the caller evaluate the NeRF field on those only
 *   iron_neus_composite   render_core's alpha (logistic CDF), inside-sphere blend with the NeRF background, weights,
 *                         colour, weight_sum / weight_max, cdf, inside_sphere, eikonal statistics (:279-344, :174-178). */
/* extract_fields' lattice (models/renderer.py:9-31): pts [nx*ny*nz,3] = meshgrid(xs, ys, zs) in 'ij' order; the field values
 * are then one iron_sdf_forward (or any other batched query) over pts. */
int iron_grid_points(const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* pts, void* stream);
/* Marching cubes over such a lattice (the mcubes.marching_cubes of models/renderer.py:34-42), csrc/mcubes.hip.
 *   u: fp32 [nx][ny][nz], z fastest (extract_fields' 'ij' order).  Any dim < 2 gives an empty mesh.  A corner is above when
 *   u > threshold (strict; NaN is below).  Case table: csrc/mc_table.h, generated by iron_amd/mc_table.py; on a face with two
 *   diagonal above corners the above corners are separated, so the mesh is watertight; it stays open where it leaves the grid.
 *   Vertices: one per crossed lattice edge, owned by the edge's lower lattice point p and axis a, at p + t e_a in index
 *   coordinates with t = (threshold - u(p)) / (u(p + e_a) - u(p)) in fp32, clamped to [0, 1]; ordered by (linear index of p, a).
 *   Triangles: int32 vertex indices, ordered by (cell = its min lattice point, table order); right-hand normals point from
 *   u > threshold toward u < threshold.  Orders come from prefix sums: the output is bitwise deterministic.
 * Two calls, as the output sizes depend on the data:
 *   iron_mc_count  leaves the crossing pattern and the scanned per-block offsets in `workspace` and returns the counts in
 *                  HOST *n_verts / *n_tris: it synchronises `stream` once (the one entry of this ABI that waits on the device).
 *                  IRON_ERR_RANGE when either count reaches 2^31.
 *   iron_mc_emit   writes verts [n_verts,3] and tris [n_tris,3] from that workspace; same u, dims and threshold, nothing else
 *                  may have touched the workspace in between. */
int iron_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes);
int iron_mc_count(const float* u, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, int64_t* n_verts,
                  int64_t* n_tris, void* stream);
int iron_mc_emit(const float* u, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, float* verts, int32_t* tris,
                 void* stream);
/* Material texture baking (models/export_materials.py: sample_surface :13-55, accumulate_splat_material :77-140 and the
 * normalisation of export_materials :206-207), csrc/texbake.hip.
 *   Mesh: verts fp32 [n_verts,3], faces int32 [n_faces,3]; uvs fp32 [n_uvs,2], face_uvs int32 [n_faces,3].
 *   Surface sampling, two calls as the sample total depends on the data:
 *     iron_bake_count   fp32 areas |cross(v0 - v2, v1 - v2)|, normalised by their sum (fp64, rounded to fp32); per-face count
 *                       ceil(n_samples * a_f) in fp32; then sum(count) - n_samples draws with replacement among the faces with
 *                       count > 0, each distinct drawn face losing one sample (numpy's `count[idx] -= 1`).  Draws come from
 *                       Philox4x32-10 keyed by seed, counter (draw index, round, 0).  Leaves the per-face sample offsets in
 *                       `workspace` (iron_bake_workspace_bytes(n_faces)), copies the counts before and after the removal to
 *                       `ceil_counts` and `counts` [n_faces] (device, int32, either may be NULL) and returns the total in
 *                       HOST *n_total: it synchronises `stream` once.  IRON_ERR_BAD_ARG
 *                       if a face indexes outside verts or uvs; IRON_ERR_RANGE when n_samples > 2^24 (the count rule is fp32).
 *     iron_bake_sample  n_total samples ordered by face; r1, r2 from Philox counter (sample index, round, 1), 53-bit uniform;
 *                       P = (1 - sqrt(r1)) A + sqrt(r1) (1 - r2) B + sqrt(r1) r2 C in fp64, rounded to fp32, for the point
 *                       [n_total,3] and, with the same weights, the uv [n_total,2]; face_idx [n_total] may be NULL.  Same mesh,
 *                       seed and round as the count, nothing else may have touched the workspace in between.
 *   iron_bake_sample_explicit: the same point rule for caller-given face_idx [n] and fp64 r1, r2 [n] (a sample whose face or
 *                       indices are out of range comes out NaN).
 *   Splat: acc is int64 [H*W][c_a + c_b + 1] in units of 2^-24, the last channel the weight; zero it before the first call.
 *     iron_bake_splat   per sample: u = uv_x * W, v = H - uv_y * H (fp32); taps centre, (0,-1), (+1,0), (0,+1), (-1,0) shift
 *                       (u, v) before floor; label = row * W + col (fp32) is kept iff 0 <= label < H*W (so a tap off the left
 *                       edge wraps to the row above); weight exp(-((u - col - 1/2)^2 + (v - row - 1/2)^2) / 2) in fp32 from the
 *                       shifted coordinates.  Adds round(w * value * 2^24) for values_a [n,c_a], values_b [n,c_b] (c_a + c_b
 *                       <= 16) and round(w * 2^24).  A term above term_bound units, or not finite, is not added and sets
 *                       *flag (device int32, sticky; zero it with acc).  Bitwise reproducible.  H*W <= 2^24.
 *     iron_bake_resolve out [H*W][c] = fp32(acc) / (fp32(w) + 1e-10) in fp32, weight [H*W] = fp32(w); synchronises `stream`
 *                       once and returns IRON_ERR_RANGE if *flag is set. */
int iron_bake_workspace_bytes(int64_t n_faces, size_t* bytes);
int iron_bake_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_uvs, const int32_t* face_uvs, int64_t n_faces,
                    int64_t n_samples, uint64_t seed, uint32_t round, void* workspace, int32_t* ceil_counts, int32_t* counts,
                    int64_t* n_total, void* stream);
int iron_bake_sample(const float* verts, const int32_t* faces, const float* uvs, const int32_t* face_uvs, int64_t n_faces, uint64_t seed,
                     uint32_t round, const void* workspace, int64_t n_total, float* points, float* uv, int32_t* face_idx, void* stream);
int iron_bake_sample_explicit(const float* verts, int64_t n_verts, const int32_t* faces, const float* uvs, int64_t n_uvs,
                              const int32_t* face_uvs, int64_t n_faces, const int32_t* face_idx, const double* r1, const double* r2,
                              int64_t n, float* points, float* uv, void* stream);
int iron_bake_splat(const float* uv, const float* values_a, int32_t c_a, const float* values_b, int32_t c_b, int64_t n, int32_t H,
                    int32_t W, int64_t term_bound, int64_t* acc, int32_t* flag, void* stream);
int iron_bake_resolve(const int64_t* acc, int32_t c, int32_t H, int32_t W, const int32_t* flag, float* out, float* weight, void* stream);
/* Point-to-mesh distance over a linear BVH (evaluation/eval_mesh.py's igl.point_mesh_squared_distance), csrc/meshdist.hip.
 *   Mesh: verts fp32 [n_verts,3], faces int32 [n_faces,3], 0 < n_faces < 2^31 - 1; vertices no face references are ignored.
 *   Build, four steps on one stream; `workspace` (iron_bvh_workspace_bytes(n_faces)) then holds the tree and the triangles:
 *     iron_bvh_keys     zeroes the workspace; box of the face centroids; keys [n_faces] (device uint64) = 30-bit Morton code of
 *                       the centroid in that box << 32 | face index (all distinct).  A face index outside [0, n_verts) or a
 *                       non-finite coordinate of a referenced vertex sets a device flag in the workspace.
 *     (caller)          sorts the keys ascending into sorted_keys (any device sort: the keys are unique).
 *     iron_bvh_hierarchy  Karras' construction over the sorted keys: n_faces - 1 internal nodes, children and parent links.
 *     iron_bvh_boxes    the triangles copied in leaf order, the boxes bottom-up (per-node arrival counters, zeroed here; unions
 *                       are min/max, so the workspace is bitwise reproducible).  Synchronises `stream` once; IRON_ERR_BAD_ARG if
 *                       the flag is set.
 *   iron_point_mesh_distance  per point [n_points,3]: the nearest face's squared distance sqr_dist (fp32), index face_idx (int32)
 *                       and closest point closest [n_points,3] (fp32), in the caller's point order; ties in the fp32 distance go
 *                       to the smallest face index.  A point equal to a vertex of a face gets sqr_dist 0 and that vertex bitwise.
 *                       A non-finite point gets NaN, -1, NaN.  Same workspace and n_faces as the build; no host wait. */
int iron_bvh_workspace_bytes(int64_t n_faces, size_t* bytes);
int iron_bvh_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* workspace, uint64_t* keys, void* stream);
int iron_bvh_hierarchy(const uint64_t* sorted_keys, int64_t n_faces, void* workspace, void* stream);
int iron_bvh_boxes(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const uint64_t* sorted_keys, void* workspace,
                   void* stream);
int iron_point_mesh_distance(const void* workspace, int64_t n_faces, const float* points, int64_t n_points, float* sqr_dist,
                             int32_t* face_idx, float* closest, void* stream);
/* Flash render of an exported asset (mesh + baked material textures), csrc/meshrender.hip; DESIGN.md §15.  Every entry enqueues on
 * `stream`; only iron_mesh_vertex_normals waits.
 *   iron_mesh_raycast  per ray (ray_o, ray_d [n_rays,3]; directions need not be unit length) the closest hit with t in
 *                       (t_min, t_max] over the BVH of iron_bvh_* (same workspace and n_faces): t [n_rays] along ray_d, face_idx
 *                       [n_rays] int32, bary [n_rays,2] = the weights of the face's second and third vertex.  Faces are two-sided.
 *                       A miss gives t = +inf, face -1, bary 0; so does a ray with a non-finite component or a zero direction.
 *                       Watertight: a ray through an edge or a vertex shared by faces of a closed mesh hits one of them (ray-space
 *                       edge functions, exact zeros re-decided in fp64 and counted as inside).  Among equal t the smallest face
 *                       index wins, so for a fixed ray t does not depend on the order of the faces or on the tree.  The box test
 *                       only errs towards visiting; zero direction components are allowed.
 *   iron_mesh_vertex_normals  normals [n_verts,3]: per vertex the sum of its faces' un-normalised cross products (B-A) x (C-A)
 *                       (area weighting; this project's choice), normalised; the zero vector where the sum is zero or no face
 *                       references the vertex.  Faces with an index outside [0, n_verts) or a non-finite product are skipped.  The
 *                       sums are int64 in units of 2^-40 of the mesh's largest product component: bitwise reproducible whatever the
 *                       order of faces and atomics.  Allocates that accumulator (24 B per vertex), synchronises `stream` once and
 *                       frees it.
 *   iron_texture_fetch  values [n,C] (C <= 8) of tex [H,W,C] at uv [n,2] in the bake's convention: texel (row, col) covers
 *                       [col, col+1) x [row, row+1) of (uv_x W, H - uv_y H).  IRON_TEX_BILINEAR: four taps around
 *                       (uv_x W - 1/2, H - uv_y H - 1/2), clamped to the edge; IRON_TEX_NEAREST: the covering texel (clamped).
 *                       The coordinates are formed in fp64 (exact for fp32 uv).  With `weight` [H,W] (the bake's weight image, may
 *                       be NULL) taps whose weight is not > 0 are dropped and the others renormalised; with none left the value is
 *                       0 and hole [n] (uint8, may be NULL) is 1.  A non-finite uv is a hole.  H * W <= 2^24.
 *   iron_asset_shade_ggx  one lane per ray from iron_mesh_raycast's t / face_idx / bary (ray_d unit): point = o + t d, distance =
 *                       |point - o|, uv interpolated through the face's own face_uvs, normal = the normalised interpolation of
 *                       mesh->normals (NULL, or a zero result: the face's geometric normal (B-A) x (C-A); never flipped towards
 *                       the viewer), material = the bilinear fetch of mesh->material [tex_h,tex_w,7] (kd 3, ks 3, roughness) with
 *                       mesh->weight, colours = ggx_colocated_point (the function behind iron_ggx_colocated) with view = -ray_d.
 *                       Every output pointer may be NULL; a miss (or a face with an index out of range) writes zeros. */
enum { IRON_TEX_BILINEAR = 0, IRON_TEX_NEAREST = 1 };
typedef struct iron_asset_mesh {
    const float* verts; int64_t n_verts;       /* [n_verts,3] */
    const int32_t* faces; int64_t n_faces;     /* [n_faces,3] */
    const float* uvs; int64_t n_uvs;           /* [n_uvs,2] */
    const int32_t* face_uvs;                   /* [n_faces,3] into uvs */
    const float* normals;                      /* [n_verts,3] or NULL */
    const float* material;                     /* [tex_h,tex_w,7] */
    const float* weight;                       /* [tex_h,tex_w] or NULL */
    int32_t tex_h, tex_w;
} iron_asset_mesh;
typedef struct iron_asset_out {
    float *color, *diffuse_color, *specular_color, *normal, *points, *diffuse_albedo, *specular_albedo;  /* [n_rays,3] */
    float *distance, *specular_roughness;      /* [n_rays] */
    float* uv;                                 /* [n_rays,2] */
    uint8_t* hole;                             /* [n_rays] */
} iron_asset_out;
int iron_mesh_raycast(const void* workspace, int64_t n_faces, const float* ray_o, const float* ray_d, int64_t n_rays, float t_min,
                      float t_max, float* t, int32_t* face_idx, float* bary, void* stream);
int iron_mesh_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float* normals, void* stream);
int iron_texture_fetch(const float* tex, const float* weight, int32_t H, int32_t W, int32_t C, const float* uv, int64_t n, int32_t mode,
                       float* values, uint8_t* hole, void* stream);
int iron_asset_shade_ggx(const iron_asset_mesh* mesh, float light, const float* tab_trans, const float* tab_diff_trans, const float* ray_o,
                         const float* ray_d, const float* t, const int32_t* face_idx, const float* bary, int64_t n_rays,
                         const iron_asset_out* out, void* stream);
/* Environment-map relighting of an exported asset, csrc/envlight.hip; DESIGN.md §16, §17.  iron_asset_shade_env is direct
 * illumination only; iron_asset_shade_env_indirect adds the interreflections.  Every entry enqueues on `stream`; none waits.
 *   iron_mesh_occluded  per ray occluded [n_rays] (uint8) = 1 when any face is met with t in (t_min, t_max], over the BVH of
 *                       iron_bvh_* (same workspace and n_faces).  skip_face [n_rays] int32 (may be NULL): that face is ignored for
 *                       that ray, -1 ignores none.  A non-finite ray or a zero direction gives 0.  The walk uses the triangle and
 *                       box tests of iron_mesh_raycast (one header, csrc/ray_core.h) and leaves at the first accepted face, so
 *                       occluded == (iron_mesh_raycast(...).face_idx >= 0) for the same window, exactly: there is no tolerance.
 *   Environment map     image [h,w,3] fp32 linear radiance, finite and >= 0 (the caller checks), lat-long in Mitsuba 0.6's
 *                       convention: with local = to_world^T world, u = atan2(local.x, -local.z) / 2 pi wrapped to [0,1), v =
 *                       acos(local.y) / pi, texel (floor(v h), floor(u w)) clamped.  to_world: row-major rotation.  Radiance is
 *                       constant per texel (Mitsuba interpolates).  h * w <= 2^24.
 *   iron_envmap_build   the sampling distribution into `workspace` (iron_envmap_workspace_bytes): texel weight (0.2126 R + 0.7152 G
 *                       + 0.0722 B) sin(pi (row + 1/2) / h), fp64 row CDFs and the marginal CDF by block scans in a fixed order
 *                       (bitwise reproducible), and P(texel) in fp32.  iron_envmap.dist is this workspace.
 *   iron_envmap_sample  u [n,2] in (0,1): u[:,0] picks the column through the row's CDF, u[:,1] the row through the marginal; the
 *                       direction is uniform in (u, v) inside the texel.  texel [n,2] int32 (row, col), dir [n,3] world, pdf [n] =
 *                       P(texel) w h / (2 pi^2 sin theta(dir)), the solid-angle density.  A texel of weight 0 is never returned; an
 *                       all-black map returns texel (0,0) with pdf 0.
 *   iron_envmap_pdf     that density at dir [n,3] (need not be unit length; 0 in a texel of weight 0 and for a zero direction).
 *   iron_envmap_lookup  the radiance rgb [n,3] at dir.
 *   iron_roughplastic   (diffuse, specular) [count,3] = roughplastic_point (csrc/ggx_core.h): the rough-plastic BRDF times cos_i for
 *                       normal n, view v and light direction l [count,3] (unit), kd, ks [count,3], rough [count].
 *   iron_asset_shade_env  per primary hit (the point, normal and material of iron_asset_shade_ggx, one shared function) the sum
 *                       over n_light environment samples and n_brdf BRDF samples (u2 < 1/2: cosine-weighted about the normal, else
 *                       a GGX half vector with density D cos_h, reflected) of
 *                         L(w) roughplastic_point(n, v, w) V(w) / (n_light p_light(w) + n_brdf p_brdf(w)),
 *                       the multi-sample balance heuristic; a count of 0 drops its term.  p_brdf = (n.w / pi + D(h) n.h / (4 v.h))
 *                       / 2.  V(w) = 1 when n.w > 0, (n_g.w)(n_g.v) > 0 (n_g the face's unit geometric normal) and the shadow ray
 *                       from x + sign(n_g.w) shadow_eps D n_g (D the diagonal of the BVH's root box) along w meets no face other
 *                       than the primary one with t in (0, inf]; the walk is iron_mesh_occluded's, inside this kernel.  Random
 *                       numbers are a pure function of (seed, pixel_idx[ray] (NULL: the ray's position), sample, dimension) on the
 *                       odd points of the 24-bit grid; sums run in an order fixed by the sample index: a pixel's result depends on
 *                       no other pixel, on no launch geometry and on no run.  bvh_workspace: the mesh's iron_bvh_* workspace.  out:
 *                       as iron_asset_shade_ggx (color = diffuse_color + specular_color, linear radiance).  dump (may be NULL, and
 *                       each pointer in it) for tests, N = n_light + n_brdf, environment samples first: dir [n_rays,N,3] (zero for
 *                       a BRDF sample with v.h <= 0), denom [n_rays,N] the denominator above, vis [n_rays,N] uint8 V(w), contrib
 *                       [n_rays,N,3] the sample's term; zeros on a miss.
 *   iron_asset_shade_env_indirect  the light that leaves a primary hit after at least one interreflection, by n_paths (1 .. 2^16)
 *                       paths per ray of at most max_depth (2 .. 8, else IRON_ERR_BAD_ARG) surface vertices, the primary hit (vertex
 *                       0) included; no Russian roulette.  The arguments up to shadow_eps are iron_asset_shade_env's.  At vertex j
 *                       (surface record, view v_j, alpha and n_g as there) with the random numbers of (seed, pixel, sample = path,
 *                       dimension 8 (j + 1) + c):
 *                         c = 3, 4, j >= 1: an environment sample w_l adds T L(w_l) f_j(w_l) V(w_l) / (p_light(w_l) + p_brdf(w_l)),
 *                                 V and the densities as in iron_asset_shade_env with both counts 1, f = roughplastic_point's
 *                                 diffuse + specular;
 *                         c = 0, 1, 2: a BRDF sample w_b; unless it is a sample with n.w_b > 0 and (n_g.w_b)(n_g.v_j) > 0 the path
 *                                 ends.  Its ray from x_j + sign(n_g.w_b) shadow_eps D n_g is iron_mesh_raycast's walk (one
 *                                 function) over t in (0, inf], the vertex's own face ignored.  It escapes: for j >= 1 add
 *                                 T L(w_b) f_j(w_b) / (p_light(w_b) + p_brdf(w_b)), and the path ends.  It meets a face from behind
 *                                 (n_g'.w_b >= 0): the path ends.  Else the hit is vertex j + 1, v_(j+1) = -w_b, and for j >= 1
 *                                 T <- T (f_d + f_s)(w_b) / p_brdf(w_b) per channel (T = 1 at vertex 1); at j = 0 the primary's two
 *                                 lobe weights b_d = f_d / p_brdf and b_s = f_s / p_brdf are kept apart.
 *                       The last vertex j = max_depth - 1 runs the same steps and hands the path to nobody, so the first D' vertices
 *                       of a run with max_depth = D are those of a run with max_depth = D', bitwise.  With C the sum of a path's
 *                       terms, indirect_diffuse [n_rays,3] = sum over paths of b_d C / n_paths and indirect_specular likewise with
 *                       b_s (either may be NULL); zeros on a miss.  Sums run in an order fixed by the path index, as in
 *                       iron_asset_shade_env: bitwise reproducible, for any subset of the rays with their own pixel_idx.  dump (may
 *                       be NULL, and each pointer in it) for tests, per (ray, path, vertex) [n_rays,n_paths,max_depth,...]:
 *                       bounce_dir [..,3] w_b (zero: no sample), bounce_org [..,3] its ray's origin, face int32 the face it reached
 *                       (-1: escaped, -2: no ray cast), t, light_dir [..,3] w_l, light_vis uint8 V(w_l), denom_light and denom_brdf
 *                       the two denominators, light_term and escape_term [..,3] the two terms above, throughput [..,3] T after the
 *                       vertex (ones after vertex 0; zeros where the path ended); per (ray, path) lobe_diffuse, lobe_specular
 *                       [n_rays,n_paths,3] = b_d, b_s.  A vertex a path never reached has face -2 and zeros. */
typedef struct iron_envmap {
    const float* image;                        /* [h,w,3] */
    const void* dist;                          /* iron_envmap_build's workspace */
    int32_t h, w;
    float to_world[9];
} iron_envmap;
typedef struct iron_env_dump {
    float* dir; float* denom; uint8_t* vis; float* contrib;
} iron_env_dump;
typedef struct iron_env_path_dump {
    float* bounce_dir; float* bounce_org; int32_t* face; float* t; float* light_dir; uint8_t* light_vis; float* denom_light;
    float* denom_brdf; float* light_term; float* escape_term; float* throughput;  /* per (ray, path, vertex) */
    float* lobe_diffuse; float* lobe_specular;                                     /* per (ray, path) */
} iron_env_path_dump;
int iron_mesh_occluded(const void* workspace, int64_t n_faces, const float* ray_o, const float* ray_d, int64_t n_rays, float t_min,
                       float t_max, const int32_t* skip_face, uint8_t* occluded, void* stream);
int iron_envmap_workspace_bytes(int32_t h, int32_t w, size_t* bytes);
int iron_envmap_build(const float* image, int32_t h, int32_t w, void* workspace, void* stream);
int iron_envmap_sample(const iron_envmap* env, const float* u, int64_t n, int32_t* texel, float* dir, float* pdf, void* stream);
int iron_envmap_pdf(const iron_envmap* env, const float* dir, int64_t n, float* pdf, void* stream);
int iron_envmap_lookup(const iron_envmap* env, const float* dir, int64_t n, float* rgb, void* stream);
int iron_roughplastic(const float* n, const float* v, const float* l, const float* kd, const float* ks, const float* rough,
                      const float* tab_trans, const float* tab_diff_trans, int64_t count, float* diffuse, float* specular, void* stream);
int iron_asset_shade_env(const iron_asset_mesh* mesh, const void* bvh_workspace, const iron_envmap* env, const float* tab_trans,
                         const float* tab_diff_trans, const float* ray_o, const float* ray_d, const float* t, const int32_t* face_idx,
                         const float* bary, const int32_t* pixel_idx, int64_t n_rays, int32_t n_light, int32_t n_brdf, uint32_t seed,
                         float shadow_eps, const iron_asset_out* out, const iron_env_dump* dump, void* stream);
int iron_asset_shade_env_indirect(const iron_asset_mesh* mesh, const void* bvh_workspace, const iron_envmap* env, const float* tab_trans,
                                  const float* tab_diff_trans, const float* ray_o, const float* ray_d, const float* t,
                                  const int32_t* face_idx, const float* bary, const int32_t* pixel_idx, int64_t n_rays, int32_t n_paths,
                                  int32_t max_depth, uint32_t seed, float shadow_eps, float* indirect_diffuse, float* indirect_specular,
                                  const iron_env_path_dump* dump, void* stream);
/* Environment-map relighting of the neural scene, csrc/envlight.hip; DESIGN.md §19.  iron_asset_shade_env's integrator on a
 * G-buffer of n pixels -- hit [n] uint8, points, normal (unit), ray_d, diffuse_albedo, specular_albedo [n,3], specular_roughness
 * [n], pixel_idx [n] int32 (may be NULL: the pixel's position) -- with the shadow rays answered by iron_trace_occluded.  The
 * samples, random numbers, densities, denominator, terms and the order of every sum are iron_asset_shade_env's, with v = -ray_d
 * and the shading normal in the geometric normal's place: a sample counts when n.w > 0, n.v > 0 and w is finite.  One block of
 * pixels [p0, p0 + nb) per call pair, nb (n_light + n_brdf) <= capacity, the number of samples `workspace`
 * (iron_neural_env_workspace_bytes(capacity)) was sized for; all work goes on `stream`, no entry waits.
 *   iron_neural_env_emit     the shadow rays of the block's counting samples with a denominator > 0, in ascending (pixel, sample)
 *                            order: ray_o [capacity,3] = x + shadow_eps n (each product and sum rounded on its own), ray_d
 *                            [capacity,3] = w, sample_idx [capacity] int32 = (pixel - p0) N + sample, count [1] int64 (DEVICE)
 *                            their number.  Entries behind count are not written.
 *   iron_neural_env_resolve  occluded [n_rays] uint8 for the first n_rays = count listed rays (the caller: iron_intersect_sphere
 *                            with r = 1, then iron_trace_occluded; a ray that misses the sphere is not occluded) -> color,
 *                            diffuse_color, specular_color [n,3] at the block's pixels (any may be NULL; zeros on a miss), and
 *                            `dump` as in iron_asset_shade_env, [n,N(,3)].  The same seed, counts and workspace as the emit. */
typedef struct iron_neural_gbuffer {
    const uint8_t* hit;
    const float *points, *normal, *ray_d, *diffuse_albedo, *specular_albedo, *specular_roughness;
    const int32_t* pixel_idx;
    int64_t n;
} iron_neural_gbuffer;
int iron_neural_env_workspace_bytes(int64_t capacity, size_t* bytes);
int iron_neural_env_emit(const iron_neural_gbuffer* g, const iron_envmap* env, int64_t p0, int64_t nb, int32_t n_light, int32_t n_brdf,
                         uint32_t seed, float shadow_eps, int64_t capacity, void* workspace, size_t workspace_bytes, float* ray_o,
                         float* ray_d, int32_t* sample_idx, int64_t* count, void* stream);
int iron_neural_env_resolve(const iron_neural_gbuffer* g, const iron_envmap* env, const float* tab_trans, const float* tab_diff_trans,
                            int64_t p0, int64_t nb, int32_t n_light, int32_t n_brdf, uint32_t seed, int64_t capacity, void* workspace,
                            size_t workspace_bytes, const uint8_t* occluded, const int32_t* sample_idx, int64_t n_rays, float* color,
                            float* diffuse_color, float* specular_color, const iron_env_dump* dump, void* stream);
/* Interreflections on the neural scene, csrc/envlight.hip; DESIGN.md §20.  iron_asset_shade_env_indirect's paths (vertex, samples,
 * random numbers env_rand(seed, pixel, path, 8 (j + 1) + c), terms, lobe weights, the order of every sum) on the G-buffer above,
 * with the shading normal in the geometric normal's place, both rays of a vertex leaving x + shadow_eps n (each product and sum
 * rounded on its own), shadow rays answered by iron_trace_occluded and bounce rays by iron_trace with chunk = 1.  A wavefront over
 * depth: one block of pixels [p0, p0 + nb) at a time, slot = (pixel - p0) n_paths + path, nb n_paths <= capacity, the number of
 * slots `workspace` (iron_neural_path_workspace_bytes(capacity), about 150 bytes per slot) was sized for; the workspace carries the
 * paths' state from call to call.  n_paths 1 .. 2^16, max_depth 2 .. 8, else IRON_ERR_BAD_ARG.  All work goes on `stream`, no entry
 * waits.  Per block: begin, then for depth = 0 .. max_depth - 1 emit and resolve, then finish.
 *   iron_neural_path_begin    every slot's state from the G-buffer: alive on a hit, vertex 0, T = 1, C = b_d = b_s = 0.
 *   iron_neural_path_emit     the two samples of every alive slot at vertex `depth`.  Lists in ascending slot order: the shadow rays
 *                             of the environment samples that count with dl > 0 (depth >= 1) in shadow_o, shadow_d [capacity,3],
 *                             shadow_idx [capacity] int32 (the slot); the bounce rays of the BRDF samples that count and whose ray is
 *                             valid in bounce_o, bounce_d, bounce_idx likewise.  counts [3] int64 (DEVICE): shadow rays, bounce
 *                             rays, alive slots.  Entries behind a count are not written.
 *   iron_neural_path_resolve  occluded [n_shadow] uint8 for the listed shadow rays (iron_intersect_sphere with r = 1, then
 *                             iron_trace_occluded; a ray that misses the sphere is not occluded) and `bounce`, one row per listed
 *                             bounce ray [n_bounce]: hit uint8 (the tracer converged inside the sphere), distance, points, and the
 *                             surface record there -- normal (unit), diffuse_albedo, specular_albedo [.,3], specular_roughness;
 *                             rows without a hit are not read.  n_shadow and n_bounce are the emit's counts, the other arguments the
 *                             emit's.  Adds T L (f_d + f_s) / dl for a visible environment sample, then, for a bounce ray that
 *                             does not hit, T L(w_b) (f_d + f_s) / db (depth >= 1).  A hit with n'.(-w_b) > 0 and p_brdf > 0 becomes
 *                             vertex depth + 1 with v = -w_b and T <- T (f_d + f_s) / p_brdf (at depth 0: b_d = f_d / p_brdf,
 *                             b_s = f_s / p_brdf, T stays 1); anything else ends the path.
 *   iron_neural_path_finish   indirect_diffuse, indirect_specular [n,3] at the block's pixels (either may be NULL; zeros on a
 *                             miss): the sum over paths of b_d C / n_paths and b_s C / n_paths in iron_asset_shade_env_indirect's order.
 *   dump (may be NULL, and each pointer in it), per (pixel, path, vertex) [n,n_paths,max_depth,...] written by the resolve of that
 *   depth for every slot of the block: iron_env_path_dump's fields with `reached` int32 (1 hit, -1 escaped, -2 no ray) for face and
 *   `distance` (the tracer's; inf when escaped) for t, and the surface record of a hit, vertex_*; a slot that is not alive writes
 *   -2 and zeros.  Per (pixel, path) [n,n_paths,3], written by the finish: lobe_diffuse, lobe_specular, path_value = (b_d + b_s) C. */
typedef struct iron_neural_path_dump {
    float* bounce_dir; float* bounce_org; int32_t* reached; float* distance;
    float* vertex_points; float* vertex_normal; float* vertex_diffuse_albedo; float* vertex_specular_albedo; float* vertex_roughness;
    float* light_dir; uint8_t* light_vis; float* denom_light; float* denom_brdf; float* light_term; float* escape_term;
    float* throughput;                                                            /* per (pixel, path, vertex) */
    float* lobe_diffuse; float* lobe_specular; float* path_value;                  /* per (pixel, path) */
} iron_neural_path_dump;
typedef struct iron_neural_bounce {
    const uint8_t* hit;
    const float *distance, *points, *normal, *diffuse_albedo, *specular_albedo, *specular_roughness;
} iron_neural_bounce;
int iron_neural_path_workspace_bytes(int64_t capacity, size_t* bytes);
int iron_neural_path_begin(const iron_neural_gbuffer* g, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int64_t capacity,
                           void* workspace, size_t workspace_bytes, void* stream);
int iron_neural_path_emit(const iron_neural_gbuffer* g, const iron_envmap* env, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth,
                          int32_t depth, uint32_t seed, float shadow_eps, int64_t capacity, void* workspace, size_t workspace_bytes,
                          float* shadow_o, float* shadow_d, int32_t* shadow_idx, float* bounce_o, float* bounce_d, int32_t* bounce_idx,
                          int64_t* counts, void* stream);
int iron_neural_path_resolve(const iron_neural_gbuffer* g, const iron_envmap* env, const float* tab_trans, const float* tab_diff_trans,
                             int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int32_t depth, uint32_t seed, float shadow_eps,
                             int64_t capacity, void* workspace, size_t workspace_bytes, const uint8_t* occluded, int64_t n_shadow,
                             const iron_neural_bounce* bounce, int64_t n_bounce, const iron_neural_path_dump* dump, void* stream);
int iron_neural_path_finish(const iron_neural_gbuffer* g, int64_t p0, int64_t nb, int32_t n_paths, int32_t max_depth, int64_t capacity,
                            void* workspace, size_t workspace_bytes, float* indirect_diffuse, float* indirect_specular,
                            const iron_neural_path_dump* dump, void* stream);
/* Face connectivity and Smart UV project (models/export_mesh.py's largest component, models/export_uv.py's Blender smart_project),
 * csrc/uvunwrap.hip; the algorithm and its contract are in iron_amd/uv_unwrap.py and DESIGN.md §13.
 *   Mesh: verts fp32 [n_verts,3], faces int32 [n_faces,3], 0 < n_faces < 2^31 - 1.  `state` is 16 bytes of device scratch (8-byte
 *   aligned), zeroed by the caller before the first call of a sequence: it carries an argmin word, the bad-input flag and a round's
 *   "changed" word.  A face index outside [0, n_verts) or a non-finite coordinate of a referenced vertex sets the flag; the first
 *   host wait after it (iron_mesh_components or iron_uv_projections) returns IRON_ERR_BAD_ARG.
 *   iron_mesh_edge_keys   keys [3*n_faces] (device uint64): record 3f+e is edge e = (v_e, v_(e+1)%3) of face f, key min << 32 | max;
 *                         an edge whose two indices are equal (and every edge of a bad face) gets 2^63 - 1, which sorts last.
 *   (caller)              sorts the keys ascending into sorted_keys with the permutation perm [3*n_faces] (int64, record index).
 *   iron_mesh_components  union-find over the faces: faces whose records share a key and whose group [n_faces] (int32; NULL = all 0)
 *                         is equal are joined, every pair of a longer run included; a degenerate edge joins nothing.  parent
 *                         [n_faces] (int32) receives each face's component root = its smallest face index.  Rounds of a hook launch
 *                         (integer atomicMin of the larger root onto the smaller) and a pointer-jumping launch; one host wait per
 *                         round, *rounds (HOST) counts them; IRON_ERR_RANGE if max_rounds pass without convergence (parent is then
 *                         not a labelling).  Bitwise deterministic.
 *   iron_uv_workspace_bytes / iron_uv_projections  per-face unit normals and areas a = |cross(v1 - v0, v2 - v0)| in fp32 (a == 0:
 *                         degenerate); projection normals P [*n_normals,3] (at most max_normals, else IRON_ERR_RANGE): seed = the
 *                         largest face (ties: smallest index); tag the untagged non-degenerate faces with n.seed > cos_half, append
 *                         the normalised sum of their normals (fixed-order reduction); the untagged face with the smallest max_p n.p
 *                         (ties: smallest index) seeds the next normal unless none is left or that value is >= cos_limit.  One host
 *                         wait per normal (*n_waits, HOST).  Then group [n_faces] = argmax_p n.p (ties: smallest p), 0 for degenerate
 *                         faces; normals_out [n_faces,3] (may be NULL) receives the face normals (zeros for degenerate faces).
 *   iron_uv_project       xy [n_vt,2] = (x.t, x.b) of vertex vt_vertex[i] in the right-handed basis (t, b, p) of p = P[island_group[
 *                         vt_island[i]]]: t = normalize(e x p), e the axis of the smallest |p_i| (ties: lowest i), b = p x t.
 *   iron_uv_rotation_search  per island and candidate angle (cs [n_angles,2] = cos, sin, or per_island != 0: [n_islands,n_angles,2]),
 *                         the box of (x c - y s, x s + y c) over the island's vts: boxes [n_islands,n_angles,4] (uint32) =
 *                         ord(-min x), ord(-min y), ord(max x), ord(max y), ord the order-preserving encoding of fp32 (x >= 0:
 *                         bits | 2^31, else ~bits); the caller picks the angle.  vt_island sorted (the wave pre-reduction uses runs).
 *   iron_uv_apply         uv [n_vt,2]: rotate by params[k] = {cos, sin, min x, min y, max x, max y, offset u, offset v} of island k,
 *                         subtract the box minimum (swap[k] != 0: first turn by +90 degrees, (x, y) -> (-y, x)), add the offset,
 *                         multiply by scale, clamp to [0, 1]. */
int iron_mesh_edge_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, uint64_t* keys, void* state, void* stream);
int iron_mesh_components(const uint64_t* sorted_keys, const int64_t* perm, int64_t n_records, const int32_t* group, int64_t n_faces,
                         int32_t* parent, void* state, int32_t max_rounds, int32_t* rounds, void* stream);
int iron_uv_workspace_bytes(int64_t n_faces, size_t* bytes);
int iron_uv_projections(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float cos_half, float cos_limit,
                        int32_t max_normals, void* workspace, void* state, float* normals_out, float* P, int32_t* group, int32_t* n_normals,
                        int32_t* n_waits, void* stream);
int iron_uv_project(const float* verts, const int32_t* vt_vertex, const int32_t* vt_island, int64_t n_vt, const int32_t* island_group,
                    const float* P, float* xy, void* stream);
int iron_uv_rotation_search(const float* xy, const int32_t* vt_island, int64_t n_vt, int64_t n_islands, const float* cs, int32_t n_angles,
                            int32_t per_island, uint32_t* boxes, void* stream);
int iron_uv_apply(const float* xy, const int32_t* vt_island, int64_t n_vt, const float* params, const int32_t* swap, float scale, float* uv,
                  void* stream);
/* Image evaluation metrics (evaluation/eval_image_folder.py: PSNR, skimage's uniform-window SSIM, LPIPS-AlexNet), csrc/imgmetrics.hip;
 * DESIGN.md §14.  Images are [H,W,3], both uint8 (is_f32 = 0) or both fp32 (is_f32 = 1), device memory.  Every entry enqueues on
 * `stream`, allocates nothing and does not wait; every reduction is a fixed-order sum of fp64 partials kept in the caller's
 * workspace (no float atomics), so every output is bitwise reproducible.  Bad shapes or null pointers: IRON_ERR_BAD_ARG.
 *   iron_img_sqerr        out[0] (DEVICE, fp64) = sum over `count` elements of (a - b)^2 in the units of images in [0,1], out[1] =
 *                         count.  uint8: the integer differences are summed exactly and divided by 255^2 once; fp32: difference and
 *                         square in fp32 (numpy's (a - b) ** 2), accumulated in fp64.  0 < count < 2^31.
 *   iron_img_ssim         skimage.metrics.structural_similarity(data_range=1, win_size=11, use_sample_covariance=False) per channel:
 *                         uniform 11x11 means, C1 = 0.01^2, C2 = 0.03^2, S evaluated where the whole window lies inside the image.
 *                         sums[3] (DEVICE, fp64) = per channel the sum of S over (H-10) x (W-10); s_map (may be NULL) [3,H-10,W-10]
 *                         fp64 receives S.  uint8: the five window sums are exact integers (121 * 255^2 < 2^24), S is fp64 of
 *                         them; fp32: products and window sums in fp64 (the product of two fp32 values is exact there), left
 *                         to right then top to bottom.  H, W in [11, 16384].
 *   LPIPS (AlexNet, v0.1), evaluation only.  Activations are NHWC fp32; a convolution weight is [Cout, k, k, Cin] fp32 (the
 *   checkpoint's [Cout, Cin, k, k] permuted once by the caller).
 *     iron_lpips_prepare  out [2,H,W,3] = ((2 x - 1) - shift) / scale of pred (image 0) and trgt (image 1); uint8 k is float(k) / 255.
 *     iron_conv2d_relu    out [B,Ho,Wo,Cout] = relu(conv(in [B,H,W,Cin], weight, stride, zero padding pad) + bias), Ho = (H + 2 pad -
 *                         ksize) / stride + 1.  An implicit GEMM on the matrix pipe at fp32 accuracy: both operands split into fp16
 *                         hi / lo pieces, three MFMA products, fp32 accumulation (the split of csrc/gemm_h2.h).  An operand element
 *                         beyond fp16's range (|x| > 65504, or not finite) has no split: it ORs 1 into *range_flag (DEVICE int32,
 *                         zeroed by the caller) and the output is then meaningless.  in, weight, out 16-byte aligned.
 *     iron_maxpool3s2     3x3 max-pool, stride 2, no padding: out [B,(H-3)/2+1,(W-3)/2+1,C].
 *     iron_lpips_tap      feat [2,H,W,C] (C a multiple of 64, <= 384), lin [C]: per pixel sum_c lin[c] (f0[c] / (|f0| + 1e-10) -
 *                         f1[c] / (|f1| + 1e-10))^2 in fp64; partials [1024] (DEVICE, fp64) receive fixed per-wave sums over the
 *                         pixels (their sum / (H W) is the layer's term).
 *     iron_lpips_forward  the whole metric for one pair: prepare, the five convolutions with their taps, the two pools, the final
 *                         sum.  out[0] (DEVICE, fp64) = LPIPS, out[1] = 0; if any operand left fp16's range out[0] = NaN and
 *                         out[1] = 1, which the caller reports as IRON_ERR_RANGE after its own read (this entry does not wait).
 *                         workspace: iron_lpips_workspace_bytes(H, W), 16-byte aligned.  The stack needs H, W >= 31. */
typedef struct iron_lpips_weights {
    const float* conv_weight[5]; /* [64,11,11,3] [192,5,5,64] [384,3,3,192] [256,3,3,384] [256,3,3,256] */
    const float* conv_bias[5];
    const float* lin[5];         /* [64] [192] [384] [256] [256] */
} iron_lpips_weights;
int iron_img_sqerr_workspace_bytes(int64_t count, size_t* bytes);
int iron_img_sqerr(const void* a, const void* b, int64_t count, int32_t is_f32, void* workspace, double* out, void* stream);
int iron_img_ssim_workspace_bytes(int32_t H, int32_t W, size_t* bytes);
int iron_img_ssim(const void* x, const void* y, int32_t H, int32_t W, int32_t is_f32, void* workspace, double* sums, double* s_map,
                  void* stream);
int iron_lpips_prepare(const void* pred, const void* trgt, int32_t H, int32_t W, int32_t is_f32, float* out, void* stream);
int iron_conv2d_relu(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* weight, const float* bias, int32_t Cout,
                     int32_t ksize, int32_t stride, int32_t pad, float* out, int32_t* range_flag, void* stream);
int iron_maxpool3s2(const float* in, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream);
int iron_lpips_tap(const float* feat, int32_t H, int32_t W, int32_t C, const float* lin, double* partials, void* stream);
int iron_lpips_workspace_bytes(int32_t H, int32_t W, size_t* bytes);
int iron_lpips_forward(const void* pred, const void* trgt, int32_t H, int32_t W, int32_t is_f32, const iron_lpips_weights* w,
                       void* workspace, double* out, void* stream);
int iron_neus_linspace(const float* near, const float* far, const float* lin, int64_t n, int32_t m, float* z, void* stream);
int iron_neus_outside_z(const float* far, const float* rev, int64_t n, int32_t m, float offset, float* z, void* stream);
int iron_neus_points(const float* rays_o, const float* rays_d, const float* z, int64_t n, int32_t m, float* pts, void* stream);
int iron_neus_up_sample(const float* rays_o, const float* rays_d, const float* z, const float* sdf, int64_t n, int32_t m,
                        int32_t n_importance, float inv_s, float* new_z, void* stream);
int iron_neus_merge(const float* z_a, const float* s_a, int32_t m_a, const float* z_b, const float* s_b, int32_t m_b, int64_t n,
                    float* z_out, float* s_out, void* stream);
int iron_neus_mid_points(const float* rays_o, const float* rays_d, const float* z, int64_t n, int32_t m, float sample_dist,
                         int32_t outside, float* dists, float* pts, float* dirs, void* stream);
int iron_neus_need_background(const float* pts, int64_t n, int32_t m, int32_t mo, uint8_t* need, void* stream);
typedef struct iron_neus_composite_args {
    const float* dists;            /* [n,m]   section lengths of the inside samples                      */
    const float* pts;              /* [n*m,3] section mid points                                         */
    const float* dirs;             /* [n*m,3]                                                            */
    const float* sdf;              /* [n*m]                                                              */
    const float* grad;             /* [n*m,3] d sdf / dx                                                 */
    const float* color;            /* [n*m,3] colour network output                                      */
    const float* bg_dists;         /* [n,mo]  outside pass (NULL: no background model)                   */
    const float* bg_density;       /* [n*mo]  NeRF alpha output                                          */
    const float* bg_color;         /* [n*mo,3] NeRF rgb output                                           */
    const float* background_rgb;   /* [3] or NULL                                                        */
    int64_t n;
    int32_t m, mo;                 /* mo = m + n_outside when the background model is used               */
    float inv_s, cos_anneal_ratio;
    float* out_color;              /* [n,3]                                                              */
    float* weights;                /* [n, mo or m]                                                       */
    float* cdf;                    /* [n,m] or NULL                                                      */
    float* inside_sphere;          /* [n,m] or NULL                                                      */
    float* weight_sum;             /* [n]                                                                */
    float* weight_max;             /* [n]                                                                */
    float* gradient_error_acc;     /* [2]: sum(relax * (|g|-1)^2), sum(relax); or NULL                   */
} iron_neus_composite_args;
int iron_neus_composite(const iron_neus_composite_args* args, void* stream);
/* The same with the outside pass given as its ALPHA [n,mo] (what render_core itself takes, models/renderer.py:259-260,
 * 312-321) instead of the NeRF density: args->bg_density / bg_dists are ignored, args->bg_color [n*mo,3] is the outside
 * pass's sampled colour. */
int iron_neus_composite_alpha(const iron_neus_composite_args* args, const float* background_alpha, void* stream);
/* render_core_outside's compositing (models/renderer.py:174-187): density [n*mo] (the NeRF field's first output), dists
 * [n,mo], sampled_color [n*mo,3], background_rgb [3] or NULL -> alpha [n,mo] = 1 - exp(-softplus(density) dists), weights
 * [n,mo], color [n,3]. */
int iron_neus_outside_composite(const float* density, const float* dists, const float* sampled_color, const float* background_rgb,
                                int64_t n, int32_t mo, float* alpha, float* weights, float* color, void* stream);
/* sample_pdf (models/renderer.py:45-75): bins [n,n_bins], weights [n,n_bins-1] -> samples [n,n_samples] by inverting the
 * CDF of the piecewise-constant density at u [n,n_samples]; u == NULL is det=True (u = linspace(0.5/k, 1-0.5/k, k)). */
int iron_neus_sample_pdf(const float* bins, const float* weights, const float* u, int64_t n, int32_t n_bins, int32_t n_samples,
                         float* samples, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pointwise geometry
 * ------------------------------------------------------------------------------------------- */
/* Camera.get_rays (models/raytracer.py:254-286).  k_inv3 = K^-1[:3,:3], c2w34 = C2W[:3,:4], both
 * HOST row-major.  uv [n,2] -> ray_o [n,3], ray_d [n,3] (normalised), ray_d_norm [n]. */
int iron_camera_rays(const float* k_inv3, const float* c2w34, const float* uv, int64_t n, float* ray_o,
                     float* ray_d, float* ray_d_norm, void* stream);

/* intersect_sphere (models/raytracer.py:223-237). */
int iron_intersect_sphere(const float* ray_o, const float* ray_d, int64_t n, float r, uint8_t* mask,
                          float* near, float* far, void* stream);

/* GGXColocatedRenderer.forward (models/renderer_ggx.py:82-146).  distance [n], normal/viewdir
 * [n,3], albedos [n,3], roughness [n]; tab_trans [5000], tab_diff_trans [50] (models/ggx/*.txt). */
int iron_ggx_colocated(float light, const float* distance, const float* normal, const float* viewdir,
                       const float* diffuse_albedo, const float* specular_albedo, const float* roughness,
                       const float* tab_trans, const float* tab_diff_trans, int64_t n, float* diffuse_rgb,
                       float* specular_rgb, float* rgb, void* stream);

/* smithG1 (models/renderer_ggx.py:12-16) on its own: cos_theta, alpha, out all [n]. */
int iron_smith_g1(const float* cos_theta, const float* alpha, int64_t n, float* out, void* stream);

/* SURVEY 8 row f-4 -- the fork's other co-located heads.
 * CompositeRenderer.forward (models/renderer_ggx.py:781-858), quirks included: the GGX NDF is evaluated with
 * alpha := 1.48958738 (:806), the `metallic` / `dielectric` weight maps are clamped and then unused (:829-831), and
 * "diffuse_rgb" is the same tensor as "rgb" (in-place alias, :847-853) -- hence no separate diffuse output.  All
 * parameter maps are raw network outputs (the clamps of :790-797 happen inside); [n,3] albedos, [n] scalars.
 * env_light != NULL selects use_env_light=True (intensity = clamp(env_light, 1e-6, 20), `distance` unused) and
 * env_light_out (optional) receives that intensity. */
typedef struct iron_composite_params {
    const float* diffuse_albedo;
    const float* specular_albedo;
    const float* specular_roughness;
    const float* metallic_eta;
    const float* metallic_k;
    const float* dielectric_eta;
    const float* env_light; /* NULL: point light */
} iron_composite_params;
int iron_composite_colocated(float light, const float* distance, const float* normal, const float* viewdir,
                             const iron_composite_params* p, const float* tab_trans, const float* tab_diff_trans, int64_t n,
                             float* specular_rgb, float* metallic_rgb, float* dielectric_rgb, float* rgb,
                             float* env_light_out, void* stream);

/* kind 0 SmoothDielectricRenderer (:171-204), 1 ThinDielectricRenderer (:229-267), 2 SmoothConductorCoLocRenderer
 * (:299-319), 3 RoughConductorCoLocRenderer (:351-395); eta, k: the conductor's constants (ignored by kinds 0, 1);
 * roughness [n] is read by kind 3 only.  (RoughPlasticCoLocRenderer / CoLocRenderer raise TypeError in the reference
 * -- a float is indexed at :404 -- and have no entry.) */
int iron_coloc_head(int32_t kind, float light, float eta, float k, const float* distance, const float* normal,
                    const float* viewdir, const float* diffuse_albedo, const float* specular_albedo, const float* roughness,
                    int64_t n, float* diffuse_rgb, float* specular_rgb, float* rgb, void* stream);

/* Image-space passes of raytrace_camera's silhouette handling (models/raytracer.py:554-570), [H,W] fp32:
 * iron_morph_closing3x3 = kornia.morphology.closing(depth, ones(3,3)) (erosion of the dilation, border never wins;
 * `tmp` is an [H,W] scratch image); iron_sobel_magnitude = kornia.filters.sobel(depth) (kernels / 8, replicate
 * border, sqrt(gx^2+gy^2+1e-6)).  kornia is not installable offline: both are restated from its documented
 * semantics and are parity-unpinned. */
int iron_morph_closing3x3(const float* depth, int32_t H, int32_t W, float* tmp, float* out, void* stream);
int iron_sobel_magnitude(const float* depth, int32_t H, int32_t W, float* out, void* stream);

/* Tail of locate_edge_points (models/raytracer.py:481-500) in one launch: points [n,3] are projected like Camera.project
 * (w2c16 = W2C, k16 = K, both 4x4 row-major HOST floats) into uv [n,2]; for every point with found[i] != 0 whose pixel index
 * floor(v) * W + floor(u) lies in [0, H*W) the pixel's entry of first [H*W] (int32, pre-set by the caller to INT32_MAX) is
 * lowered to i: afterwards first[p] is the first found candidate of pixel p -- the one unique() keeps -- or INT32_MAX. */
int iron_edge_pixels(const float* points, const uint8_t* found, int64_t n, const float* w2c16, const float* k16, int32_t H, int32_t W,
                     float* uv, int32_t* first, void* stream);

/* The fill_holes update of raytrace_camera (models/raytracer.py:558-564) on the device: where the closed depth image
 * `depth_closed` (iron_morph_closing3x3) makes a hit of a non-convergent pixel, the reference rewrites depth at those
 * pixels, sets the mask to depth_closed > 1e-2 and recomputes distance = depth * ray_d_norm and points = ray_o + ray_d *
 * distance for EVERY pixel -- and does nothing at all when no pixel changes.  `flag` (device int32, scratch) carries that
 * any() between the two launches, so there is no host synchronisation.  All arrays [n] / [n,3]; conv is uint8. */
int iron_fill_holes(const float* depth_closed, const float* ray_o, const float* ray_d, const float* ray_d_norm, int64_t n,
                    float* depth, uint8_t* conv, float* distance, float* points, int32_t* flag, void* stream);

/* render_edge_pixels (models/raytracer.py:665-729), inference form, as two launches around the side-ray trace + shade:
 * iron_edge_sides: edge point gradients [n,3] and projections edge_uv [n,2], w2c_rot9 = W2C[:3,:3] row-major (HOST
 * float[9]) -> side_uv [2n,2] (the n positive-side samples centre - 0.707 n2d first, then the n negative-side ones) and
 * pos_weight [n] = 1 - (a - sin a) / 2pi, a = 2 acos(clamp(((uv - centre) . n2d) / 0.707, 0, 1)) (:680-698).
 * iron_edge_blend: side_color [2n,3] (same order) -> color[p] = pos * w + neg * (1 - w), normal[p] = edge_grad,
 * uv[p] = edge_uv, points[p] = edge_points at p = pixel_idx[i] (int64, flat pixel index; out-of-range entries skipped)
 * of the [n_pixels, .] image buffers (:706-729). */
int iron_edge_sides(const float* edge_uv, const float* edge_grad, const float* w2c_rot9, int64_t n, float* side_uv,
                    float* pos_weight, void* stream);
int iron_edge_blend(const float* side_color, const float* pos_weight, const float* edge_grad, const float* edge_uv,
                    const float* edge_points, const int64_t* pixel_idx, int64_t n, int64_t n_pixels, float* color, float* normal,
                    float* uv, float* points, void* stream);

/* The surface walk of locate_edge_points (models/raytracer.py:441-478) in one launch: every start point walks along
 * the surface (step_size per step, at most max_step steps) until |n.v| <= dot_threshold seen from cam_origin3 (HOST
 * float[3]); points [n,3] receives the final positions, found [n] whether the silhouette was reached.  Needs the h2
 * core for this network (IRON_ERR_UNSUPPORTED otherwise: walk with iron_sdf_get_all instead). */
int iron_edge_walk(const iron_net_t* sdf, const float* start, int64_t n, const float* cam_origin3, int32_t max_step,
                   float step_size, float dot_threshold, float* points, uint8_t* found, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sphere tracer.  Replaces RayTracer.forward = sphere_tracing + ray_sampler + rootfind
 * (models/raytracer.py:45-220) for a batch of n rays, with the per-call chunking of
 * raytrace_pixels (:378-392) expressed as `chunk`: rays [k*chunk, (k+1)*chunk) share the
 * bisection iteration count exactly as one reference RayTracer.forward call does.
 * ------------------------------------------------------------------------------------------- */
typedef struct iron_trace_params {
    float sdf_threshold;          /* 5e-5 */
    int32_t sphere_tracing_iters; /* 16   */
    int32_t n_steps;              /* 128  */
    int64_t chunk;                /* rays per reference call (<=0: all n in one chunk) */
} iron_trace_params;

typedef struct iron_trace_stats { /* written to DEVICE memory, all int64 */
    int64_t n_evals;       /* SDF point evaluations actually performed                          */
    int64_t n_sphere_conv; /* rays convergent after sphere tracing                              */
    int64_t n_sampler;     /* rays handed to the dense sampler                                  */
    int64_t n_bisect;      /* rays bisected                                                     */
    int64_t n_conv;        /* convergent rays at the end                                        */
    int64_t n_evals_ref;   /* evaluations the REFERENCE algorithm makes on the same rays: sphere-trace
                              evals + 128 per sampled ray + (chunk count + 1) per bisected ray
                              (SURVEY 8d's E; the HIP sampler stops early, so n_evals <= n_evals_ref) */
    int64_t n_evals_sphere;/* evaluations made by the sphere-tracing kernel                     */
    int64_t reserved;          /* 0; non-zero = k_sampler workgroups that left their work queue by the poll bound (a bug: report it) */
} iron_trace_stats;

size_t iron_trace_workspace_bytes(int64_t n, const iron_trace_params* p);

/* lin_steps: n_steps floats = torch.linspace(0,1,n_steps) (raytracer.py:144-146), DEVICE.
 * Outputs: conv uint8[n], points [n,3], sdf [n], dist [n] (state of non-convergent rays as the
 * reference leaves it).  stats may be NULL.  chunk_iters_io (int32[n_chunks], DEVICE) may be NULL;
 * see iron_trace_phase for the multi-rank protocol. */
int iron_trace(const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps, const float* ray_o,
               const float* ray_d, const float* near, const float* far, const uint8_t* work, int64_t n,
               uint8_t* conv, float* points, float* sdf_out, float* dist, iron_trace_stats* stats,
               void* workspace, size_t workspace_bytes, void* stream);

/* The occlusion query: occluded [n] (uint8) is, bit for bit, the `conv` iron_trace writes for the same rays, segments and work
 * mask -- the reference tracer's answer to "does this ray meet the surface in [near, far)".  The mask is final once the dense
 * sampler has found, or not found, a first negative sample (models/raytracer.py:162-167), so the call runs iron_trace's sphere and
 * sampler kernels and no bisection, and returns no points, sdf or distance.  The screen, the stride and the deferred resolve
 * apply as in iron_trace.  `workspace`: iron_trace_occluded_workspace_bytes(n, p) (the tracer's workspace and 20 bytes per ray
 * for the state the kernels keep).  stats may be NULL; n_bisect then counts the bracketed rays, none of which was bisected. */
size_t iron_trace_occluded_workspace_bytes(int64_t n, const iron_trace_params* p);
int iron_trace_occluded(const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps, const float* ray_o,
                        const float* ray_d, const float* near, const float* far, const uint8_t* work, int64_t n,
                        uint8_t* occluded, iron_trace_stats* stats, void* workspace, size_t workspace_bytes, void* stream);

/* The three stages of RayTracer.forward as separate calls, for callers that use the reference's methods directly (models/raytracer.py
 * :105-140 sphere_tracing, :142-197 ray_sampler, :199-220 rootfind; tests/test_raytracer.py).  One call = one reference call: the
 * bisection count is global to its n rays.  `workspace` as for iron_trace (iron_trace_workspace_bytes(n, p)).
 *   stage 0 sphere_tracing: in0 = min_dis, in1 = max_dis, work  ->  mask_out = convergent, unfinished_out, points, sdf_out, dist
 *   stage 1 ray_sampler:    in0 = min_dis, in1 = max_dis        ->  mask_out = rays with a bracketed root, points, sdf_out, dist
 *                           (zeros for the others, as the reference returns them)
 *   stage 2 rootfind:       in0 = f_low, in1 = f_high, in2 = d_low, in3 = d_high  ->  points = p_mid, dist = d_mid, sdf_out = f_mid
 *                           (mask_out: scratch, n bytes; the reference's in-place update of its four bracket arguments is not made) */
int iron_trace_stage(int32_t stage, const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps, const float* ray_o,
                     const float* ray_d, const float* in0, const float* in1, const float* in2, const float* in3, const uint8_t* work,
                     int64_t n, uint8_t* mask_out, uint8_t* unfinished_out, float* points, float* sdf_out, float* dist,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Multi-rank form: rays of one reference chunk may live on several ranks, so the chunk-global
 * bisection count needs one MAX all-reduce between the two halves.  phase 0 = sphere trace +
 * sampler + per-ray bisection, writing each local chunk's own count to chunk_iters[n_chunks];
 * the caller all-reduces (MAX) that array, then phase 1 finishes the bisection with it.
 * ray_index [n] (int64, may be NULL = identity) gives each ray's position in the full image so
 * that chunk = ray_index / p->chunk. */
int iron_trace_phase(int32_t phase, const iron_net_t* sdf, const iron_trace_params* p, const float* lin_steps,
                     const float* ray_o, const float* ray_d, const float* near, const float* far,
                     const uint8_t* work, const int64_t* ray_index, int64_t n, int32_t* chunk_iters,
                     int64_t n_chunks, uint8_t* conv, float* points, float* sdf_out, float* dist,
                     iron_trace_stats* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Callable tracer (trace_any.hip).  RayTracer.forward on an SDF the library cannot evaluate itself: the caller's function
 * supplies the values, batch by batch, and these entries do everything between two evaluations -- the per-ray state machine of
 * models/raytracer.py:45-220 with the reference's formulas (one rounding per product and sum) and its own comparisons (NaN and
 * zero fall where torch puts them).  The caller drives the loop:
 *
 *   start                      -> points = o + d * near, dist = near            evaluate points [n]
 *   sphere_step(list_in = -1)  -> values land in sdf, termination tests, unfinished rays step and are listed in ascending
 *     read, evaluate pts_out      ray order (pair_scan: deterministic); pts_out [count, 3] holds their new points, word 0 the
 *     sphere_step(list_in = l)    count.  Lists alternate: a step that read list l (-1: all rays) wrote list 1 - l (0).
 *     ...                         advance = 0 (the iteration limit is reached): tests and list only, no ray moves.
 *   sphere_finish              -> conv (and, optionally, the unfinished mask) as raytracer.py:132-137
 *   sampler_interval           -> [min, max] of every listed ray (raytracer.py:56-63); list_sel = -1: a = min_dis, b = max_dis
 *                                 of rays 0..m-1 taken as given (ray_sampler as a stage)
 *   sampler_points / evaluate / sampler_reduce, for blocks [k0, k0 + nk) of the list: nk * n_steps points, row-major;
 *                                 the reduce keeps no-root / first-negative index and the bracket (z, f) pairs per ray (a NaN
 *                                 sample is neither sign there: torch.sign gives 0 for it)
 *   sampler_gather             -> rootless rays zeroed, bracketed ones listed in order (word 0: their count), their first mid
 *                                 points in pts_out, word 1: whether any bracket is open (f_low > 0 > f_high)
 *   bisect_load                -> the same start from explicit brackets of rays 0..n-1 (rootfind as a stage)
 *   evaluate / bisect_step / read, while word 1 is set: every slot moves, word 1 = any open bracket wider than 2 * threshold
 *   evaluate / finish          -> final mid point, value and distance scattered to the rays (conv = 1 when conv != NULL)
 *
 * `n` is the capacity the workspace was sized for (iron_trace_any_workspace_bytes(n)): the rays of the call; every list length
 * m, block and slot count is checked against it, pts_out against pts_capacity (points), and every kernel is bounded by the count
 * it was launched with.  `values` must hold one float per point of the batch just evaluated: the caller checks that before the
 * call.  All work goes on `stream`; only iron_trace_any_read waits for it (out2[0] = word 0, out2[1] = word 1, HOST).
 * ------------------------------------------------------------------------------------------- */
size_t iron_trace_any_workspace_bytes(int64_t n);
int iron_trace_any_start(const float* ray_o, const float* ray_d, const float* near, int64_t n, float* points, float* dist, void* stream);
int iron_trace_any_sphere_step(const float* values, int64_t m, int32_t list_in, int32_t advance, float sdf_threshold, const float* ray_d,
                               const float* far, const uint8_t* work, int64_t n, float* points, float* sdf, float* dist, float* pts_out,
                               int64_t pts_capacity, void* workspace, size_t workspace_bytes, void* stream);
int iron_trace_any_read(const void* workspace, size_t workspace_bytes, int64_t n, int64_t* out2, void* stream);
int iron_trace_any_sphere_finish(const uint8_t* work, const float* far, float sdf_threshold, int64_t n, const float* sdf, const float* dist,
                                 uint8_t* conv, uint8_t* unfinished_out, void* workspace, size_t workspace_bytes, void* stream);
int iron_trace_any_sampler_interval(int32_t list_sel, int64_t m, const float* a, const float* b, const float* sdf, const float* dist, int64_t n,
                                    void* workspace, size_t workspace_bytes, void* stream);
int iron_trace_any_sampler_points(int32_t list_sel, int64_t m, int64_t k0, int64_t nk, int32_t n_steps, const float* lin_steps,
                                  const float* ray_o, const float* ray_d, int64_t n, float* pts_out, int64_t pts_capacity, void* workspace,
                                  size_t workspace_bytes, void* stream);
int iron_trace_any_sampler_reduce(int64_t m, int64_t k0, int64_t nk, int32_t n_steps, const float* lin_steps, const float* values, int64_t n,
                                  void* workspace, size_t workspace_bytes, void* stream);
int iron_trace_any_sampler_gather(int32_t list_sel, int64_t m, const float* ray_o, const float* ray_d, int64_t n, uint8_t* conv, float* points,
                                  float* sdf, float* dist, float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes,
                                  void* stream);
int iron_trace_any_bisect_load(const float* f_low, const float* f_high, const float* d_low, const float* d_high, const float* ray_o,
                               const float* ray_d, int64_t n, float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes,
                               void* stream);
int iron_trace_any_bisect_step(const float* values, int64_t nb, float sdf_threshold, const float* ray_o, const float* ray_d, int64_t n,
                               float* pts_out, int64_t pts_capacity, void* workspace, size_t workspace_bytes, void* stream);
int iron_trace_any_finish(const float* values, int64_t nb, const float* ray_o, const float* ray_d, int64_t n, uint8_t* conv, float* points,
                          float* sdf, float* dist, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shading.  Replaces render_normal_and_color (models/raytracer.py:593-662) with the driver's GGX
 * render_fn (render_surface.py:117-156): for every ray with conv != 0: get_all -> normalise ->
 * get_materials (models/rendering_func.py:5-16) -> GGXColocatedRenderer; other rays get zeros.
 * Outputs are full-size [n,3] / [n]; any may be NULL.
 * ------------------------------------------------------------------------------------------- */
typedef struct iron_shade_nets {
    const iron_net_t* sdf;
    const iron_net_t* diffuse_albedo;
    const iron_net_t* specular_albedo;
    const iron_net_t* specular_roughness;
} iron_shade_nets;

typedef struct iron_shade_out {
    float* color;              /* [n,3] rgb                    */
    float* diffuse_color;      /* [n,3]                        */
    float* specular_color;     /* [n,3]                        */
    float* diffuse_albedo;     /* [n,3]                        */
    float* specular_albedo;    /* [n,3]                        */
    float* specular_roughness; /* [n]                          */
    float* normal;             /* [n,3] normalised             */
} iron_shade_out;

size_t iron_shade_workspace_bytes(int64_t n);

int iron_shade_ggx(const iron_shade_nets* nets, float light, int32_t is_metal, const float* tab_trans,
                   const float* tab_diff_trans, const float* ray_o, const float* ray_d, const float* points,
                   const uint8_t* conv, int64_t n, const iron_shade_out* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The same with the composite render_fn (render_surface.py:159-234): get_all -> normalise ->
 * get_materials_comp (models/rendering_func.py:19-49: eight material networks) -> CompositeRenderer.forward.
 * Scalar maps are [n]; "diffuse_color" receives the same values as "color" (the reference's in-place alias). */
typedef struct iron_shade_comp_nets {
    const iron_net_t* sdf;
    const iron_net_t* diffuse_albedo;
    const iron_net_t* specular_albedo;
    const iron_net_t* specular_roughness;
    const iron_net_t* metallic;
    const iron_net_t* dielectric;
    const iron_net_t* metallic_eta;
    const iron_net_t* metallic_k;
    const iron_net_t* dielectric_eta;
} iron_shade_comp_nets;

typedef struct iron_shade_comp_out {
    float* color;              /* [n,3] */
    float* diffuse_color;      /* [n,3] == color */
    float* specular_color;     /* [n,3] */
    float* diffuse_albedo;     /* [n,3] */
    float* specular_albedo;    /* [n,3] */
    float* specular_roughness; /* [n]   */
    float* metallic_eta;       /* [n]   */
    float* metallic_k;         /* [n]   */
    float* dielectric_eta;     /* [n]   */
    float* normal;             /* [n,3] normalised */
    float* metallic_rgb;       /* [n,3] */
    float* metallic;           /* [n]   */
    float* dielectric_rgb;     /* [n,3] */
    float* dielectric;         /* [n]   */
} iron_shade_comp_out;

size_t iron_shade_composite_workspace_bytes(int64_t n);

int iron_shade_composite(const iron_shade_comp_nets* nets, float light, const float* tab_trans, const float* tab_diff_trans,
                         const float* ray_o, const float* ray_d, const float* points, const uint8_t* conv, int64_t n,
                         const iron_shade_comp_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* CU budget of the launches that follow (all streams, process-wide): the persistent kernels fill `n_cus` compute units instead of
 * the whole device; n_cus <= 0 removes the limit.  Returns the device's CU count.  For callers that run two launch sequences side by
 * side on two streams (iron_amd.raytracer.render_camera: hit shading beside the silhouette pass; no counterpart in the reference,
 * whose render_camera, models/raytracer.py:778-814, is one sequence). */
int32_t iron_set_cu_limit(int32_t n_cus);

/* Number of independent parts (1..4) the tracer cuts the rays of a call into, each part's kernel chain on its own stream (the
 * caller's + library-owned side streams, forked / joined with events); results do not depend on it.  parts <= 0 restores the
 * default (IRON_TRACE_SPLIT, else 1: measured no faster on MI355X, csrc/trace.hip).  Returns the previous setting.  Process-wide;
 * no counterpart in the reference (RayTracer.forward, models/raytracer.py:45-103, is one sequence of masked torch ops). */
int32_t iron_set_trace_split(int32_t parts);

/* The dense sampler's screen as a batched call (diagnostics and tests; no reference counterpart): out[i] = the SDF of x[i] computed
 * with ONE fp16 product per multiply-add (fp16 weights and activations, fp32 accumulation; csrc/mlp_h2.h sdf_hidden_stack_h1).
 * NOT fp32-accurate: the tracer uses it only to decide signs far from zero (csrc/trace.hip).  IRON_ERR_UNSUPPORTED
 * unless the network runs on the h2 core (8 x 256, skip 4). */
int iron_sdf_screen_forward(const iron_net_t* net, const float* x, int64_t n, float* out, void* stream);

/* The dense sampler's screen (csrc/trace.hip k_sampler_screen; no reference counterpart; results do not depend on it).  On the h2
 * core the sampler decides sample signs on the screen where they are clear by a calibrated margin and evaluates the rest exactly;
 * outputs and iron_trace_stats are those of the unscreened sampler.  The margin is empirical: a guard (iron_net_numeric_status
 * bit 3) turns the screen off for a network whose exactly evaluated samples came within half the margin, for every call that
 * starts after the call that raised it has completed (the flag is a pinned host word; calls already queued behind it still screen).
 * The trace workspace (iron_trace_workspace_bytes) holds the screen's lists on every path: ~113 bytes per ray.
 *   iron_set_sampler_screen:   on = 1 screen, 0 don't, -1 the default (IRON_SAMPLER_SCREEN=0: off, else on).  Process-wide;
 *                              returns the previous state.
 *   iron_sampler_screen_debug: test hooks, process-wide.  what 0: value > 0 forces the margin delta (0 restores the calibrated
 *                              one); what 1: value >= 1 caps the resolve list at that many samples per part (0 restores);
 *                              what 2: value 1 makes iron_sdf_screen_forward evaluate 32 points per wave instead of the
 *                              sampler's 64 (bit-identical values; 0 restores).
 *   iron_trace_screen_counts:  synchronises `stream`; from the workspace of the last iron_trace / iron_trace_phase(0) /
 *                              iron_trace_stage(1) call: out[0] screened evaluations (speculative ones included), out[1] exactly
 *                              resolved samples, out[2] rays that overflowed the resolve list (marched unscreened), out[3] the
 *                              largest |f_screen - f_exact| / delta over the resolved samples, out[4] rays decided after the resolve. */
int32_t iron_set_sampler_screen(int32_t on);
int iron_sampler_screen_debug(int32_t what, double value);
int iron_trace_screen_counts(const void* workspace, double* out, void* stream);

/* The screen's adaptive march (csrc/trace.hip k_sampler_screen; results do not depend on it).  The screen does not evaluate samples
 * that an evaluated neighbour proves positive: f1 > delta + L * (distance along the ray), with the slope bound L = 2 x the largest
 * |grad f| over the screen's calibration points.  L is empirical like the margin, and watched from three sources: the passes that
 * run at stride 1 see the slope between adjacent screened samples; the resolve sees the exact value of every listed (uncertain)
 * sample against the screened value of the sample before it, and the exact values of adjacent listed samples.  One above 0.75 L
 * raises a guard (iron_net_numeric_status bit 4) after which the network's calls
 * march every sample -- every call that starts after the call that raised it has completed, as for the screen's guard.  Calls with
 * more than 256 steps, or too large for the sampler's continuation items, march every sample too.
 *   iron_set_sampler_stride:  on = 1 adaptive, 0 every sample, -1 the default (IRON_SAMPLER_STRIDE=0: off, else on).  Process-wide;
 *                             returns the previous state.
 *   iron_sampler_screen_debug what 3: value > 0 forces the slope bound L (0 restores the calibrated one).
 *   iron_trace_stride_counts: synchronises `stream`; from the workspace of the last traced call: out[0] ray-passes the screen executed
 *                             (8 samples of one ray), out[1] those at a stride above 1, out[2] the largest watched slope relative
 *                             to L (after an allowance of delta / 2 for the screen's own error), out[3] 1 if the call marched
 *                             adaptively, 0 if it ran stride 1 throughout.  out[2] is the largest over the guard's three sources.
 *   iron_sampler_screen_debug what 4: value != 0 keeps rays with listed samples on stride 1 (the march before such rays strode,
 *                             which chose a block's stride one-sided: what 6 is implied);
 *                             what 5: value != 0 mutes the guard's stride-1-pass source (tests of the resolve's sources);
 *                             what 6: value != 0 makes a block's stride the gap in front of it, 1 + what the previous block's last
 *                             sample certifies.  (The default is two-sided: up to twice that where the previous block's last two
 *                             values rise, since a gap inside a block has an evaluated sample at each end.)
 *   iron_trace_stride_detail: synchronises `stream`; out[9] from the workspace of the last traced call: out[0] stride-1 passes of
 *                             rays that had already listed samples and whose 8 samples were all certainly positive, out[1]
 *                             stride-1 passes of rays that had listed none when the pass began, out[2] strided blocks discarded
 *                             (restarts), out[3..5] slope observations of the guard's sources (stride-1 passes, resolve against
 *                             the screened predecessor, exact adjacent pairs), out[6..8] the largest ratio each source saw. */
int32_t iron_set_sampler_stride(int32_t on);
int iron_trace_stride_counts(const void* workspace, double* out, void* stream);
int iron_trace_stride_detail(const void* workspace, double* out, void* stream);

/* The resolve's two rounds (csrc/trace.hip k_resolve_list; results do not depend on them).  A ray's outcome uses the exact value of
 * its first listed sample that is negative and of the sample before it.  The samples a ray lists behind its first listed one with a
 * negative screened value are deferred: round 1 evaluates the others, round 2 the deferred ones that lie in front of what round 1
 * left as the ray's first negative sample (usually none).  out[1] of iron_trace_screen_counts still counts every listed sample:
 * evaluated, or settled without an evaluation.  A call that collects iron_trace_stats evaluates every listed sample (round 2 takes
 * all deferred ones), so that the counts and guard maxima read after it are those of the whole list; the guards of a call that
 * does not collect them see the evaluated samples only.
 *   iron_set_resolve_defer:   on = 1 two rounds, 0 every listed sample in one, -1 the default (IRON_RESOLVE_DEFER=0: off, else on).
 *                             Process-wide; returns the previous state.
 *   iron_trace_resolve_counts: synchronises `stream`; out[4] from the workspace of the last traced call: out[0] / out[1] exact
 *                             evaluations of listed samples made by round 1 / round 2 (deferral off: all in out[0]), out[2] / out[3]
 *                             entries on round 1's / round 2's list. */
int32_t iron_set_resolve_defer(int32_t on);
int iron_trace_resolve_counts(const void* workspace, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage-1 batches and validation frames (models/dataset.py:271-300, 335-361; render_volume.py:696-729), csrc/volume.hip.
 * kinv44 / pose44: DEVICE row-major 4x4 fp32 matrices of one view -- inverse(K) and inverse(W2C); their upper 3x3 and 3x4 are
 * read.  One thread per ray, the reference's arithmetic in its order:
 *     p = Kinv (x, y, 1);  v = p / |p|;  d = R v;  o = t;  a = sum d^2;  b = 2 sum o d;  mid = 0.5 (-b) / a;  near, far = mid -+ 1
 *   iron_volume_rays       random mode.  image: uint8 [h, w, c >= 3]; mask: uint8 [h, w, cm >= 1] or NULL (the mask is then 1);
 *                          px, py: DEVICE int64 [n] pixel columns and rows (drawn by the caller: no random numbers are made here).
 *                          Writes data [n, 10] = rays_o, rays_d, rgb / 255, mask[..., 0] / 255, and near [n], far [n].  A pixel
 *                          outside the picture is not read: its colour and mask are NaN.
 *   iron_volume_rays_grid  grid mode.  tx [cols], ty [rows]: DEVICE fp32 pixel coordinates (torch.linspace(0, W - 1, W // l) and
 *                          linspace(0, H - 1, H // l) as torch makes them); ray (row, col) looks through (tx[col], ty[row]).
 *                          Writes rays_o, rays_d [rows, cols, 3]: the reference's transpose(0, 1).  No colour gather.
 *   iron_volume_frame_u8   n rays of a frame of frame_rays rays, written at ray `offset` (offset + n <= frame_rays).  rgb_frame
 *                          (uint8 [frame_rays, 3] or NULL) = trunc(clip(color * 256, 0, 255)), color [n, 3].  normal_frame (uint8
 *                          [frame_rays, 3] or NULL) = trunc(clip(rot33 . N * 128 + 128, 0, 255)) with N = sum over the first m
 *                          columns j of gradients[r, j, :] * weights[r, j] * inside_sphere[r, j], summed in order in fp32;
 *                          gradients [n, m, 3], weights [n, mw >= m] (the outside samples' columns are skipped), inside_sphere
 *                          [n, m] or NULL, rot33: DEVICE row-major 3x3 (the inverse of the pose's rotation).
 * ------------------------------------------------------------------------------------------- */
int iron_volume_rays(const uint8_t* image, int32_t h, int32_t w, int32_t c, const uint8_t* mask, int32_t cm, const float* kinv44,
                     const float* pose44, const int64_t* px, const int64_t* py, int64_t n, float* data, float* near, float* far,
                     void* stream);
int iron_volume_rays_grid(const float* kinv44, const float* pose44, const float* tx, const float* ty, int32_t rows, int32_t cols,
                          float* rays_o, float* rays_d, void* stream);
int iron_volume_frame_u8(const float* color, const float* gradients, const float* weights, const float* inside_sphere,
                         const float* rot33, int64_t n, int32_t m, int32_t mw, int64_t offset, int64_t frame_rays, uint8_t* rgb_frame,
                         uint8_t* normal_frame, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multiresolution hash-grid encoding (the tcnn.Encoding of models/tcnn_fields.py: tiny-cuda-nn's published HashGrid with Linear
 * interpolation, 3-D input, fp32 table), csrc/hashgrid.hip; the definition is csrc/hashgrid_common.h and DESIGN.md "Hash-grid
 * encoding".  Level l: scale = exp2(l log2 per_level_scale) base_resolution - 1 (double, stored fp32), res = ceil(scale) + 1,
 * size = min(roundup8(res^3), 2^log2_hashmap_size) entries of n_features_per_level floats, dense iff res^3 <= size; the flat
 * table is the levels one after another, [n_params, F].
 *   iron_hashgrid_layout   HOST only, no device needed.  Validates the descriptor (n_levels 1..32, F in {1, 2, 4, 8},
 *                          log2_hashmap_size 1..24, base_resolution >= 1, per_level_scale >= 1, else IRON_ERR_BAD_ARG;
 *                          IRON_ERR_RANGE when a level's scale reaches 2^22) and writes n_levels records to levels_out (may be
 *                          NULL) and the number of table entries to *n_params_out (may be NULL).
 *   iron_hashgrid_encode   x [n,3] (clamped to [0,1] per axis) -> y [n, L F], level-major within a row, and, when jac is not
 *                          NULL, jac [n, L F, 3] = dy/dx (a column is zero on an axis where x lay outside [0,1]).  One thread per
 *                          (point, level); the eight corners are summed in corner order in fp32, so a row does not depend on
 *                          the other rows of the call.  `table` must hold n_params F floats.
 * ------------------------------------------------------------------------------------------- */
#define IRON_HASHGRID_MAX_LEVELS 32
typedef struct iron_hashgrid_desc {
    int32_t n_levels;
    int32_t n_features_per_level;
    int32_t log2_hashmap_size;
    int32_t base_resolution;
    double per_level_scale;
} iron_hashgrid_desc;
typedef struct iron_hashgrid_level {
    float scale;
    uint32_t res;
    uint32_t size;    /* entries */
    uint32_t dense;   /* 1: (c0 + c1 res + c2 res^2) mod size, 0: the xor hash mod size */
    int64_t offset;   /* first entry of the level in the flat table */
} iron_hashgrid_level;
int iron_hashgrid_layout(const iron_hashgrid_desc* desc, iron_hashgrid_level* levels_out, int64_t* n_params_out);
int iron_hashgrid_encode(const iron_hashgrid_desc* desc, const float* x, int64_t n, const float* table, float* y, float* jac_or_null,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused inference evaluation of the hash-grid field (TCNNSDF of models/tcnn_fields.py: the encoding above and a bias-free MLP
 * head, tiny-cuda-nn's FullyFusedMLP), csrc/hashgrid_field.hip; DESIGN.md §28.  One launch computes out [n, n_out] and, when
 * grad is not NULL, grad [n, 3] = d out[:, 0] / dp; neither the features nor their Jacobian are written to memory.
 *   head      layer 0: L F -> n_neurons, n_hidden_layers - 1 layers n_neurons -> n_neurons, last: n_neurons -> n_out; `activation`
 *             between layers, none after the last.  Weights: the flat fp32 concatenation of the [out, in] row-major matrices.
 *             Every pre-activation is one fp32 fma chain over the input index in ascending order, starting from zero.
 *   shapes    L F <= 128, n_neurons in {16, 32, 64, 128}, n_hidden_layers 1..4, n_out 1..16, else IRON_ERR_RANGE; a descriptor
 *             the encoding refuses returns the encoding's code; an unknown activation IRON_ERR_BAD_ARG.
 *   iron_hashgrid_field_check       HOST only, no device needed: validates and writes the number of weights (may be NULL).
 *   iron_hashgrid_field_pack_bytes  size of the packed blob (0 for a refused descriptor); `packed` must be 16-byte aligned.
 *   iron_hashgrid_field_pack        weights -> MFMA fragment order, both orientations; once per weight version.
 *   iron_hashgrid_field_eval        evaluates at x_d = fma(p_d, a_d, b_d) (map_a3 / map_b3: HOST pointers to 3 floats, NULL: a = 1 /
 *                                   b = 0), x clamped to [0, 1] as the encoding does; grad is with respect to p (a_d times the
 *                                   gradient at x) and exactly zero on an axis where x lay outside [0, 1].  A row's results do not
 *                                   depend on the other rows, on n or on its position; n = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
enum { IRON_FIELD_ACT_NONE = 0, IRON_FIELD_ACT_RELU = 1, IRON_FIELD_ACT_SOFTPLUS = 2 };
typedef struct iron_hashgrid_field_desc {
    iron_hashgrid_desc encoding;
    int32_t n_neurons;
    int32_t n_hidden_layers;
    int32_t n_out;
    int32_t activation;   /* IRON_FIELD_ACT_* */
} iron_hashgrid_field_desc;
int iron_hashgrid_field_check(const iron_hashgrid_field_desc* desc, int64_t* n_weights_out);
size_t iron_hashgrid_field_pack_bytes(const iron_hashgrid_field_desc* desc);
int iron_hashgrid_field_pack(const iron_hashgrid_field_desc* desc, const float* weights, void* packed, void* stream);
int iron_hashgrid_field_eval(const iron_hashgrid_field_desc* desc, const float* p, int64_t n, const float* map_a3_or_null,
                             const float* map_b3_or_null, const float* table, const void* packed, float* out, float* grad_or_null,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident sphere tracer of the hash-grid field (csrc/hashgrid_trace.hip).  RayTracer.forward on the field
 * above with the field evaluated inside the tracing kernels: a fixed launch sequence, every count left on the device.  All entries
 * ENQUEUE ONLY: no device-to-host copy, no stream synchronise.  conv / points / sdf_out / dist are, bit for bit and NaN payloads
 * included, what the callable tracer (iron_trace_any_*) computes when its values come from column 0 of iron_hashgrid_field_eval
 * with the same map; `chunk` couples rays [k chunk, (k+1) chunk) through the bisection count exactly as there.
 *   desc, map_a3 / map_b3 (HOST, may be NULL), table, packed     as for iron_hashgrid_field_eval
 *   p                 iron_trace_params; n_steps 2 .. 4096 else IRON_ERR_RANGE, as is a shape iron_hashgrid_field_check refuses
 *   lin_steps         n_steps floats = torch.linspace(0, 1, n_steps), DEVICE
 *   n                 0 .. INT_MAX - 1 (else IRON_ERR_BAD_ARG); n = 0 launches nothing.  Null pointers and a workspace smaller
 *                     than iron_hashgrid_trace_workspace_bytes(n, p) (0 for an n out of range): IRON_ERR_BAD_ARG
 *   stats             NULL or 8 int64 words on the DEVICE, which the caller zeroes and the entries add to:
 *                     [0] lane evaluations issued (64 per wave evaluation)   [1] evaluations that belonged to a live ray
 *                     [2] sampled rays   [3] bisected rays   [4] the sum over chunks of the bisection count T
 *                     [5] incomplete: a bracket was still open after 256 iterations (a NaN inside an open bracket); the chunk
 *                         stopped there and its results are not the reference's (which would not end)   [6], [7] reserved
 *   iron_hashgrid_trace_occluded   the same `conv` alone: final once the sampler has found, or not found, a first negative sample
 *   iron_hashgrid_trace_stage      the three reference stages on their own, arguments as for iron_trace_stage (stage 0 sphere
 *                                  tracing, 1 ray_sampler with its bisection on the intervals given, 2 rootfind of the brackets
 *                                  given); the bisection count is global to the call
 * ------------------------------------------------------------------------------------------- */
size_t iron_hashgrid_trace_workspace_bytes(int64_t n, const iron_trace_params* p);
int iron_hashgrid_trace(const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3, const float* map_b3,
                        const float* table, const void* packed, const float* lin_steps, const float* ray_o, const float* ray_d,
                        const float* near, const float* far, const uint8_t* work, int64_t n, uint8_t* conv, float* points, float* sdf_out,
                        float* dist, int64_t* stats_or_null, void* workspace, size_t workspace_bytes, void* stream);
int iron_hashgrid_trace_occluded(const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3, const float* map_b3,
                                 const float* table, const void* packed, const float* lin_steps, const float* ray_o, const float* ray_d,
                                 const float* near, const float* far, const uint8_t* work, int64_t n, uint8_t* occluded,
                                 int64_t* stats_or_null, void* workspace, size_t workspace_bytes, void* stream);
int iron_hashgrid_trace_stage(int32_t stage, const iron_hashgrid_field_desc* desc, const iron_trace_params* p, const float* map_a3,
                              const float* map_b3, const float* table, const void* packed, const float* lin_steps, const float* ray_o,
                              const float* ray_d, const float* in0, const float* in1, const float* in2, const float* in3,
                              const uint8_t* work, int64_t n, uint8_t* mask_out, uint8_t* unfinished_out, float* points, float* sdf_out,
                              float* dist, int64_t* stats_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (no reference counterpart): per-kernel device time from hipEvents recorded on the
 * caller's stream around each compute kernel.  Off by default.  iron_profile_read blocks on the
 * recorded events, adds their elapsed milliseconds / launch counts into the caller's arrays
 * (IRON_PROF_KINDS entries each) and clears the pending list.
 * ------------------------------------------------------------------------------------------- */
enum {
    IRON_PROF_SPHERE = 0, IRON_PROF_SAMPLER = 1, IRON_PROF_BISECT_A = 2, IRON_PROF_BISECT_B = 3,
    IRON_PROF_SDF_GRAD = 4, IRON_PROF_MATERIAL = 5, IRON_PROF_GGX = 6, IRON_PROF_SDF_FORWARD = 7,
    IRON_PROF_KINDS = 8
};
int iron_profile_enable(int32_t on);
int iron_profile_read(double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* IRON_HIP_H */
