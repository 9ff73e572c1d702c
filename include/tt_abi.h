/*
 * tt_abi.h -- C ABI of libtt_hip.so: the MI355X (gfx950) triplane volume-render hot path.
 *
 * This is the drop-in boundary of triplaneturbo_amd.  Every entry point is plain C:
 * raw DEVICE pointers (fp32 unless noted), explicit sizes, a config struct, a hipStream_t
 * passed as void*.  The caller (PyTorch-ROCm host code, or any FFI) allocates every output
 * and workspace; the library itself keeps one 266 KB device scratch per GPU (work-queue counters of the per-sample
 * kernels: one 64-byte slot per stream, zeroed on the stream (by a one-wave kernel) in front of every launch, and a never-reused slot per
 * launch recorded under stream capture, so a launch can be captured in a hipGraph; allocated at the first launch,
 * which therefore must not be inside a capture); no environment variable is read; re-entrant; safe from one
 * host thread per device.  Return 0 on success, a negative tt_status on error (no C++
 * exceptions cross the boundary).  tt_strerror() maps codes to text.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *
 *   tt_planes_pack          few_step_triplane_dual_stable_diffusion.py:212-239 (rotate_planes "v1" copy)
 *                           + geometry/utils.py:131 (view as N*n_planes,C,H,W); produces the channels-last,
 *                           rotation-folded plane image the kernels gather from.
 *   tt_planes_unpack_grad   the autograd transpose of the above (d loss / d space_cache, NCHW).
 *   tt_query_points         StableDiffusionTriplaneDualAttention.forward   few_step...:273-351
 *                           (= sample_from_planes geometry/utils.py:127-145 -> aten grid_sampler_2d,
 *                            VanillaMLP networks.py:67-104, get_shifted_sdf :131-154, analytic normal :329-335
 *                            -> aten grid_sampler_2d_backward via cuda_gridsample.py:55-58)
 *                           and forward_sdf :353-373 (flags without TT_Q_TEX / TT_Q_NORMAL).
 *   tt_query_field          forward_field :375-394 (sdf + deformation head; mesh renderer / exporter grid query)
 *   tt_decode_rays          the geometry call of prop_sigma_fn (renderer :243-299 -> few_step...:273-306, sdf only)
 *   tt_sample_uniform       ImportanceEstimator.sampling level 0 (threestudio/models/estimators.py:61-79 with
 *                           _transform_stot "uniform" :104-118): n equal / stratified intervals on [near, far].
 *   tt_sample_importance    the rest of ImportanceEstimator.sampling (estimators.py:72-101) with prop_sigma_fn's
 *                           fixed-step NeuS density (renderer :288-297): nerfacc render_transmittance_from_density,
 *                           importance_sampling (inverse-CDF resample) and the merge + sort of the edges (:317-324).
 *   tt_render_fwd           GenerativeSpaceSDFVolumeRenderer._forward
 *                           generative_space_sdf_volume_renderer.py:326-431,467-472 (positions, geometry,
 *                           NoMaterial no_material.py:41-54, get_alpha neus_volume_renderer.py:93-117,
 *                           nerfacc.render_weight_from_alpha, nerfacc.accumulate_along_rays x5).
 *   tt_render_eval          the same in eval mode (per-ray outputs only): decode + march fused per ray tile with
 *                           wave-ballot early termination / texture-decode skipping
 *   tt_march_fwd / _bwd     the ray march alone (second half of tt_render_fwd / first half of tt_render_bwd_geo):
 *                           get_alpha neus_volume_renderer.py:93-117 + nerfacc.render_weight_from_alpha +
 *                           nerfacc.accumulate_along_rays x5 (renderer :407-431,467-472) on given per-sample
 *                           sdf / sdf_grad / features, and its backward.  Bandwidth-bound.
 *   tt_render_bwd_geo /     the autograd backward of the same, incl. the second-order terms the reference
 *   tt_render_bwd_tex       obtains from gridsample_cuda.cu:27-210 (grad2_2d, cuda_gridsample.py:68-79),
 *                           aten grid_sampler_2d_backward and the transposed cuBLAS GEMMs.
 *   tt_points_bwd_x         the same backward w.r.t. the query points themselves (grad_grid of both grid_sample
 *                           backwards + K1's grad_grid, gridsample_cuda.cu:196-208)
 *   tt_points_bwd_geo /     the autograd backward of tt_query_points / tt_query_field w.r.t. planes and MLP weights
 *   tt_points_bwd_tex       (training-time callers: generative_space_mesh_rasterize_renderer.py:428-452 field
 *                           query, :321-376 per-pixel geometry decode); same kernels as tt_render_bwd_*.
 *   tt_composite_fwd/_bwd   the renderer's per-ray composite: comp_rgb, disparity, comp_normal, camera-space normal
 *                           maps (generative_space_sdf_volume_renderer.py:433-530)
 *   tt_patch_composite_*    PatchRenderer.forward's upsample + paste per output key (patch_renderer.py:74-88)
 *   tt_hashgrid_fwd / _bwd  tiny-cuda-nn's `HashGrid` encoding as used by the background
 *                           (multi_prompt_neural_environment_hashgrid_map_background.py:25-34,54,104-105 via
 *                           threestudio/models/networks.py:17-26,54-64); tcnn is CUDA-only and un-vendored.
 *   tt_grid_sample_2d_grad2 gridsample_cuda.cpp:26-37 `grad2_2d` itself (operator-level drop-in; _typed: half / float /
 *   (_typed)                double, zeros / border padding, either align_corners, as gridsample_cuda.cu:560-594).
 *   tt_mc_*                 marching cubes with a backward pass: the `diso.DiffMC` call of DiffMarchingCubeHelper
 *                           (triplaneturbo_executable/utils/mesh_exporter.py:29-75, isosurface() :78-141;
 *                           threestudio/models/isosurface.py:18-65); diso is a CUDA-only, un-vendored extension.
 *   tt_mt_*                 marching tetrahedra with a backward pass: MarchingTetrahedraHelper._forward
 *                           (threestudio/models/isosurface.py:231-301) without its per-call torch.unique.
 *   tt_mesh_*               Mesh.normal_consistency / laplacian and their backward, Mesh.remove_outlier's connected
 *                           components and compaction (threestudio/models/mesh.py:31-95,255-308; trimesh on the host
 *                           in the reference).
 *   tt_uv_* / tt_tex_fill   the mesh exporter's xatlas UV unwrap (threestudio/models/mesh.py:207-249) and cv2.inpaint
 *                           texture padding (multiprompt_mesh_exporter.py:96-107): axis-projection charts, shelf
 *                           packing, an overlap guard, nearest-texel fill.
 *   tt_uv_lscm_*            the opt-in conformal flattening of those charts (least-squares conformal maps, an fp64
 *                           conjugate-gradient solve per chart); xatlas's own charts are not reproduced.
 *   tt_tex_fwd / _bwd       nvdiffrast's 2-D `texture` without mipmaps (CUDA-only, un-vendored): sampling map_Kd at
 *                           interpolated UVs, the step the reference's export render (evaluation/mesh_visualize.py)
 *                           leaves to external tools.
 *   tt_simplify_*           mesh simplification for export: vertex clustering with quadric-error placement.  The
 *                           reference exports the raw marching-cubes mesh; this step has no counterpart there.
 *   tt_decimate_*           mesh decimation for export: manifold-preserving parallel quadric edge collapse.  No
 *                           counterpart in the reference either.
 *   tt_remesh_*             isotropic remeshing (split, collapse, flip, relax) of an extracted mesh.  The reference
 *                           hands the raw extraction to xatlas; no counterpart there.
 *   tt_bake_*               Mesh.v_tng (threestudio/models/mesh.py:162-205) and the tangent-space normal map (map_Bump)
 *                           the exporter bakes for a simplified mesh from the field's analytic normals.
 *   tt_dist_*               closest point on a triangle mesh with a backward pass, and a surface sampler: what
 *                           Mesh.distance_to and Mesh.simplify(max_error=) measure a simplified export with.  No
 *                           counterpart in the reference.
 */
#ifndef TT_ABI_H
#define TT_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_ABI_VERSION 17
#define TT_CHANNELS 32 /* feature channels per plane (space_generator output_dim/2, yaml :95) */
#define TT_HIDDEN 64   /* mlp_network_config.n_neurons */

typedef enum {
    TT_OK = 0,
    TT_ERR_BAD_ARG = -1,     /* null pointer / non-positive size / unsupported shape */
    TT_ERR_UNSUPPORTED = -2, /* e.g. non-square planes */
    TT_ERR_LAUNCH = -3,      /* hipLaunch / hipGetLastError failure */
    TT_ERR_DEVICE = -4       /* not a gfx950 device / attribute query failed */
} tt_status;

/* MLP weights exactly as torch stores nn.Linear(bias=False).weight: row-major (out, in).
 * sdf net  : w1 (64,32)  w2 (64,64)  w3 (1,64)     few_step...:101-105
 * feat net : v1 (64,96)  v2 (64,64)  v3 (3,64)     few_step...:106-112  (tex_interpolate v2 => 96 inputs) */
typedef struct {
    const float* w1;
    const float* w2;
    const float* w3;
    const float* v1;
    const float* v2;
    const float* v3;
} tt_mlp_weights;

typedef struct {
    float* w1;
    float* w2;
    float* w3;
    float* v1;
    float* v2;
    float* v3;
} tt_mlp_grads; /* accumulated into (+=) with fp32 atomics; caller zero-initialises */

typedef struct {
    int32_t n_prompts;         /* P: planes are (P,6,H,W,32) packed */
    int32_t views_per_prompt;  /* view b samples prompt b / views_per_prompt  (renderer :120-143) */
    int32_t plane_h, plane_w;  /* must be equal (rotation v1 transposes) */
    int32_t rays_per_view;     /* Hh*Ww; ray r belongs to view r / rays_per_view */
    int32_t n_samples;         /* S samples per ray (dense layout, renderer :317-324) */
    int64_t n_rays;            /* total rays = views * rays_per_view */
    float radius;              /* geometry.radius: bbox = [-radius, radius]^3 */
    float sdf_bias_radius;     /* sdf_bias "sphere", sdf_bias_params (yaml :78-79) */
    float inv_std;             /* LearnedVariance.inv_std, clamped to [1e-6,1e6] (renderer :29-35) */
    float cos_anneal_ratio;    /* neus_volume_renderer.py:101-104 */
    float rgb_grad_shrink;     /* renderer :397-400 (backward only) */
    int32_t flags;             /* TT_R_* */
    int32_t image_w;           /* rays of a view form an image_w x (rays_per_view/image_w) image (pixel-block tiles);
                                  0 = unknown: tiles are runs of consecutive rays */
    int32_t tile_sb;           /* consecutive samples of one ray per 32-sample tile: 1, 2, 4, ... 32; 0 = default (2).
                                  1-2 suit evenly spaced samples; 8 suits importance sampling, where consecutive samples
                                  of a ray share texels and are then combined inside the tile (performance only:
                                  results do not depend on it beyond fp32 summation order) */
    int32_t grad_copies;       /* backward: grad_packed holds this many privatised copies (copies,P,6,H,W,32), each
                                  workgroup scatters into one of them and tt_planes_unpack_grad sums them; spreads
                                  same-texel atomics.  0/1 = a single copy */
    int32_t tile_chunk;        /* samples of a ray block per work item of the dynamic queue; 0 = automatic (performance
                                  only, like tile_sb) */
    float skip_eps_tex;        /* backward, OPT-IN approximation (0 = exact, the default): a 32-sample tile whose upstream
                                  colour gradients all satisfy |cbar|_1 <= skip_eps_tex is skipped by tt_render_bwd_tex
                                  (cbar = d loss / d raw feature = shrink w g_rgb 1.002 s (1 - s) + g_features: samples in
                                  empty space carry weights ~1e-5 and almost no gradient).  Induced error of d/d texture
                                  planes and d/d feature net: at most skip_eps_tex x (skipped samples) x the local
                                  sensitivity; measured at the training shapes in tests/test_gpu_skip.py. */
    float skip_eps_geo;        /* the same for tt_render_bwd_geo on |d loss/d sdf| + |d loss/d sdf_grad|_1 per sample (dense
                                  under an eikonal loss, so usually nothing to skip there) */
    const float* inv_std_dev;  /* null, or a DEVICE pointer to one float that replaces `inv_std` (clamped to [1e-6,1e6] in the
                                  kernels like LearnedVariance.forward, renderer :34-35): trainable_variance=True
                                  (renderer :53,82; neus_volume_renderer.py:26-37) without a host read-back per step.  Read
                                  by tt_render_fwd / _bwd_geo, tt_march_fwd / _bwd and tt_render_eval */
    uint64_t* stats;           /* null, or a DEVICE pointer to 4 x uint64 the caller zero-fills: work accounting of the decode
                                  kernel of tt_render_fwd / tt_decode_rays / tt_render_bwd_geo / tt_render_bwd_tex, added to
                                  with one atomic per wave: [0] 32-sample tile steps visited, [1] tile steps EXECUTED (those
                                  that pass the exact skip tests: some texel in bounds -- a tile without one decodes to exact
                                  zeros --, and in the backward some non-zero upstream gradient), [2] (plane, sample) pairs
                                  with an in-bounds texel over the gathers that ran (3 planes per sample; the samples a launch
                                  visits are exactly n_rays * n_samples), [3] executed tile steps that took the single-plane path
                                  (exactly one plane had an in-bounds texel in the tile: the other two planes' products and
                                  scatter passes are left out; forward: counted in the texture decode).  Measurement only
                                  (bench.py: live_tile_frac, inbounds_plane_frac) */
} tt_render_cfg;

#define TT_R_PER_SAMPLE 1 /* also write per-sample sdf / sdf_grad / features (training extras, renderer :532-545) */
/* ---- precision of the matrix products (the per-point MLPs; everything else is plain fp32 in every mode) ----
 * The reference multiplies in fp32 (threestudio/models/networks.py:91-97: nn.Linear with autocast disabled; trainer
 * precision 32, configs/TriplaneTurbo_v1.yaml:254).  Three modes; at most one of the three bits may be set, none = the
 * default = TT_R_SPLIT3:
 *   TT_R_SPLIT3     fp32-GRADE products on the fp16 matrix pipe: every operand is split EXACTLY in three fp16 pieces
 *                   (hi + mid + lo = v), the six product terms above 2^-33 are accumulated in fp32 (6 x
 *                   v_mfma_f32_32x32x16_f16 per k-step).  Product error <= 2^-24 of sum |a b| (tools/mfma16_probe.hip):
 *                   the reference's precision at ~1/3 of the fp32 MFMA's matrix-pipe time.  SCOPE: the mat-vec chains of
 *                   every kernel (forward, recompute, both gradient chains, per-point queries, eval, d/d points) are
 *                   three-piece; the REDUCTIONS OVER SAMPLES of the backward -- the weight-gradient outer products and
 *                   the scatter's combine GEMM -- use TWO-piece operands (hi + lo, per-launch / per-sample power-of-two
 *                   scales).  The outer products form all four cross terms; the combine GEMM forms three (hh, hl, lh):
 *                   its dropped lo x lo term is at most 2^-22 |a b| per product (|lo| <= 2^-11 |v|: half an ulp of
 *                   fp16's 11-bit significand).  Each operand is represented to 2^-23 and the round-to-nearest
 *                   errors average over the thousands to millions of samples such a sum runs over (measured: weight
 *                   and plane gradients 4e-7 ... 1e-6 from the fp32 oracle in all three modes).
 *   TT_R_EXACT_F32  every product on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  The A/B
 *                   reference of the split modes.
 *   TT_R_SPLIT2     the FAST mode (the default of rounds 2-4): two fp16 pieces per operand, three product terms, ~2^-21.5
 *                   per product -- a tolerance-bounded approximation (gradients within 1e-4 of the fp32 math on
 *                   well-conditioned scenes, not on every scene: DESIGN.md section 6). */
#define TT_R_EXACT_F32 2
#define TT_R_SPLIT2 32
#define TT_R_SPLIT3 64

/* use_volsdf = True of the reference (threestudio/models/renderers/neus_volume_renderer.py:19-23,:95-96 and
 * generative_space_sdf_volume_renderer.py:286-287): alpha = |t_end - t_start| x density(sdf), density = k (0.5 + 0.5
 * sign(sdf) expm1(-|sdf| k)) with k = inv_std clamped to [0, 80]; NOT clipped to [0,1] and independent of the normal and of
 * cos_anneal_ratio.  Honoured by tt_render_forward / _backward, the march entry points and the fused eval render. */
#define TT_R_VOLSDF 128

#define TT_R_WGRAD_F32 4  /* RESERVED, always TT_ERR_UNSUPPORTED: selected the round-2 backward kernels with their weight-gradient
                             outer products on the fp32-input MFMA (an A/B variant of TT_R_SPLIT2; removed from the tree) */
#define TT_R_BWD_SOLO 8   /* backward: force the one-wave-per-tile decode kernels (the default) */
#define TT_R_BWD_PAIR 16  /* RESERVED, always TT_ERR_UNSUPPORTED: selected the experimental wave-pair texture kernel of round 4
                             (two waves per SIMD; correct and 1.4x slower; removed from the tree in round 6) */

/* tt_query_points / tt_query_field / tt_decode_rays / tt_points_bwd_* flags */
#define TT_Q_NORMAL 1    /* output sdf_grad (analytic normal path) */
#define TT_Q_TEX 2       /* output features (texture planes + feature net) */
#define TT_Q_EXACT_F32 4 /* as TT_R_EXACT_F32 */
#define TT_Q_SPLIT2 8    /* as TT_R_SPLIT2 */
#define TT_Q_SPLIT3 16   /* as TT_R_SPLIT3 (the default) */

const char* tt_strerror(int status);
int tt_abi_version(void);
/* sha256 (hex) of the sources and build flags the library was built from ("unknown" for a hand-made build): the host
 * side rebuilds when it differs from the tree (triplaneturbo_amd/_lib.py), whatever the file times say. */
const char* tt_source_hash(void);
/* Test hook: leaves the work-queue counters of `stream` dirty, as a faulted kernel would; the next launch on that
 * stream must be unaffected (the counters are zeroed on the stream in front of every launch). */
int tt_debug_poison_queue(void* stream);

/* space_cache (P,6,32,H,W) NCHW  ->  packed (P,6,H,W,32), planes re-oriented per rotate_planes "v1". */
int tt_planes_pack(const float* space_cache, float* packed, int32_t n_prompts, int32_t plane_h, int32_t plane_w,
                   void* stream);
/* grad wrt packed, n_copies privatised copies (n_copies,P,6,H,W,32) -> their sum as grad wrt space_cache
 * (P,6,32,H,W); overwrites dst. */
int tt_planes_unpack_grad(const float* grad_packed, float* grad_space_cache, int32_t n_prompts, int32_t plane_h,
                          int32_t plane_w, int32_t n_copies, void* stream);

/* Per-point decode.  points (n_batch, n_points, 3) world units; batch b reads prompt b / views_per_prompt.
 * out_sdf (n_batch*n_points), out_sdf_grad (n_batch*n_points,3) [if TT_Q_NORMAL], out_features (.,3) [if TT_Q_TEX].
 * Null outputs are skipped. */
int tt_query_points(const float* packed, const tt_mlp_weights* w, const float* points, int32_t n_batch,
                    int64_t n_points, int32_t n_prompts, int32_t views_per_prompt, int32_t plane_h, int32_t plane_w,
                    float radius, float sdf_bias_radius, int32_t flags, float* out_sdf, float* out_sdf_grad,
                    float* out_features, void* stream);

/* Implicit-field query for isosurface extraction (forward_field, few_step...:375-394; callers
 * generative_space_mesh_rasterize_renderer.py:428-452 and triplaneturbo_executable/utils/mesh_exporter.py:78-105):
 * sdf (n_batch*n_points) and deformation (n_batch*n_points,3) from the geometry planes only.
 * `w`: sdf net in w1..w3, DEFORMATION net (32->64->64->3, few_step...:113-122) in v1..v3.  flags: TT_Q_EXACT_F32 or 0. */
int tt_query_field(const float* packed, const tt_mlp_weights* w, const float* points, int32_t n_batch,
                   int64_t n_points, int32_t n_prompts, int32_t views_per_prompt, int32_t plane_h, int32_t plane_w,
                   float radius, float sdf_bias_radius, int32_t flags, float* out_sdf, float* out_deformation,
                   void* stream);

/* Decode only, along rays: sdf [+ sdf_grad if TT_Q_NORMAL] [+ features if TT_Q_TEX] at the mid-points of the
 * intervals (n_rays,S).  The importance sampler's proposal pass (prop_sigma_fn, renderer :243-299) uses flags = 0. */
int tt_decode_rays(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                   const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, int32_t flags, float* sdf,
                   float* sdf_grad, float* features, void* stream);

/* Where the n + 1 edges of a level are placed in cdf space (u in [0,1]) before going through the inverse cdf.  The
 * reference draws both levels with nerfacc v0.5.2 `importance_sampling(intervals, cdfs, n, stratified)`
 * (threestudio/models/estimators.py:72-90); nerfacc is un-vendored and its pdf.cu is not available here, so its exact
 * convention is UNVERIFIABLE in this build and the choice is an explicit, switchable contract:
 *   TT_PLACE_TT     (default) u_j = j / n, j = 0..n: first / last edge pinned to near / far.  Stratified: level-0
 *                   interior edges -+ half a cell ((jitter - 0.5) / n), fine level u_j + jitter_j / n clamped to [0,1].
 *   TT_PLACE_CENTER u_j = (j + 0.5) / (n + 1): the centres of n + 1 equal cells, nothing pinned to 0 or 1.
 *                   Stratified: u_j = (j + jitter_j) / (n + 1), one uniform draw per cell.
 * Under either one the empirical distribution of the resampled edges follows the proposal cdf within one cell
 * (tests/test_gpu_sampler.py checks that against the cdf itself, not against a restatement of the kernel). */
enum tt_sample_placement { TT_PLACE_TT = 0, TT_PLACE_CENTER = 1 };
/* OR-ed into tt_sample_importance's `placement`: the proposal density is the VolSDF density of TT_R_VOLSDF (renderer
 * :286-287) instead of the fixed-step NeuS density (:288-297) */
#define TT_PLACE_VOLSDF 0x100

/* Level-0 sample intervals from the uniform cdf: edges s_k = u_k of `placement` (jitter (n_rays, n+1), U[0,1), or
 * null = deterministic), t = s*far + (1-s)*near (_transform_stot "uniform", estimators.py:104-118);
 * t_starts/t_ends (n_rays, n). */
int tt_sample_uniform(int64_t n_rays, int32_t n_samples, float near_plane, float far_plane, const float* jitter,
                      int32_t placement, float* t_starts, float* t_ends, void* stream);

/* Importance resampling of one proposal level.  In: proposal intervals t_starts/t_ends (n_rays, K) and the sdf
 * (n_rays, K) at their mid-points (tt_decode_rays, flags = 0).  sigma = NeuS alpha over a fixed step / step (or the
 * VolSDF density: placement | TT_PLACE_VOLSDF),
 * T = exp(-exclusive_cumsum(sigma dt)), cdf = 1 - [T, 0]; F + 1 fine edges at the u_j of `placement` (u_jitter
 * (n_rays, F+1), U[0,1), or null = deterministic) through the piecewise-linear inverse cdf; out = the K + F + 2
 * edges merged in increasing order as out_t_starts/out_t_ends (n_rays, K + F + 1).  inv_std_dev: null, or a device scalar
 * that replaces inv_std (as tt_render_cfg.inv_std_dev). */
int tt_sample_importance(const float* t_starts, const float* t_ends, const float* sdf, int64_t n_rays,
                         int32_t n_proposal, int32_t n_fine, float inv_std, const float* inv_std_dev,
                         float render_step_size, const float* u_jitter, int32_t placement, float* out_t_starts,
                         float* out_t_ends, void* stream);

/* Forward render for explicit sample intervals.
 * rays_o, rays_d (n_rays,3); t_starts, t_ends (n_rays,S).
 * Per-ray outputs: opacity (n_rays), depth (n_rays), rgb_fg (n_rays,3), z_variance (n_rays),
 *                  normal_acc (n_rays,3) = sum_i w_i n_i (NOT normalised).
 * Per-sample outputs (n_rays*S), all required: weights, trans, sdf, sdf_grad (.,3), features (.,3).  The decode
 *   kernel writes sdf/sdf_grad/features, the march kernel reads them back (they are also the renderer's
 *   training extras, renderer :532-545, and the saved state of the backward). */
int tt_render_fwd(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                  const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, float* opacity, float* depth,
                  float* rgb_fg, float* z_variance, float* normal_acc, float* weights, float* trans, float* sdf,
                  float* sdf_grad, float* features, void* stream);

/* tt_render_fwd that also writes h2_mask (n_rays*S, 2) uint32: the signs of the sdf net's last hidden layer,
 * h2 = relu(W2 relu(W1 f)), as the forward computed them.  Dword 2*sample + hi (hi = 0, 1) holds bit r =
 * (h2[(r & 3) + 8 * (r >> 2) + 4 * hi] > 0), r = 0..31 -- the register layout both decode kernels keep h2 in.  Every
 * sample's two dwords are written (0 where the tile step had no in-bounds texel).  Same arithmetic and outputs as
 * tt_render_fwd; the mask is the extra saved state of tt_render_bwd_geo_h2mask. */
int tt_render_fwd_h2mask(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                         const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, float* opacity,
                         float* depth, float* rgb_fg, float* z_variance, float* normal_acc, float* weights, float* trans,
                         float* sdf, float* sdf_grad, float* features, uint32_t* h2_mask, void* stream);

/* tt_render_fwd_h2mask that also writes h1_mask (n_rays*S, 2) uint32: the signs of the sdf net's FIRST hidden layer,
 * h1 = relu(W1 f), in the bit layout of h2_mask (bit r of dword 2*sample + hi = (h1[(r & 3) + 8 * (r >> 2) + 4 * hi] > 0);
 * 0 where the tile step had no in-bounds texel).  8 more bytes of saved state per sample; same arithmetic and outputs;
 * h2_mask is bit for bit the one of tt_render_fwd_h2mask.  Both masks are the saved state of tt_render_bwd_geo_masks. */
int tt_render_fwd_masks(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                        const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, float* opacity,
                        float* depth, float* rgb_fg, float* z_variance, float* normal_acc, float* weights, float* trans,
                        float* sdf, float* sdf_grad, float* features, uint32_t* h2_mask, uint32_t* h1_mask, void* stream);

/* Eval-mode render (the renderer returns no per-sample tensors outside training, renderer :532-545): the per-ray outputs
 * of tt_render_fwd from ONE kernel that decodes and marches each 8x4-pixel ray tile front to back.
 * transmittance_eps > 0: a ray stops contributing once its transmittance is below it and a tile stops when all its rays
 * have (wave ballot); weight_eps > 0: the texture decode of a tile step is skipped unless some ray has a larger weight,
 * and runs for those rays only.  Induced error: opacity / rgb < transmittance_eps + S * weight_eps per ray (depth: x far).
 * Both 0: no approximation (the skips that remain are exact).  stats (device, 2 x uint64, may be null; caller zero-fills):
 * += wave tile steps with a geometry decode / with a texture decode.  No gradients: eval only. */
int tt_render_eval(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                   const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, float transmittance_eps,
                   float weight_eps, float* opacity, float* depth, float* rgb_fg, float* z_variance, float* normal_acc,
                   uint64_t* stats, void* stream);

/* The ray march alone, on per-sample sdf (n_rays*S), sdf_grad (.,3), features (.,3) that the caller already has
 * (tt_decode_rays / tt_query_points): per-ray and per-sample outputs as in tt_render_fwd. */
int tt_march_fwd(const float* rays_d, const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                 const float* sdf, const float* sdf_grad, const float* features, float* opacity, float* depth,
                 float* rgb_fg, float* z_variance, float* normal_acc, float* weights, float* trans, void* stream);

/* Backward of tt_march_fwd down to the per-sample quantities: out_grad (n_rays*S,4) = (d/d sdf, d/d sdf_grad xyz),
 * upstream grads as in tt_render_bwd_geo (null = 0).  (d/d features = weights * g_rgb_fg * d sigmoid is formed inside
 * tt_render_bwd_tex.)  This is the `workspace` tt_render_bwd_geo fills for its decode backward.
 * g_inv_std_rays (n_rays, may be null; overwritten): d loss / d inv_std PER RAY (both logistic arguments of get_alpha are
 * sdf estimates times inv_std, neus_volume_renderer.py:108-109); the caller sums the rays (fixed order: reproducible) and
 * chains through its own parametrisation (LearnedVariance: inv_std = exp(10 p) clamped).  trainable_variance=True. */
int tt_march_bwd(const float* rays_d, const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                 const float* opacity, const float* depth, const float* trans, const float* sdf,
                 const float* sdf_grad, const float* features, const float* g_opacity, const float* g_depth,
                 const float* g_rgb_fg, const float* g_z_variance, const float* g_normal_acc, const float* g_weights,
                 const float* g_sdf, const float* g_sdf_grad, float* g_inv_std_rays, float* out_grad, void* stream);

/* Backward, geometry half: d/d(geometry planes 0..2) and d/d(sdf net).
 * Per-ray upstream grads (any may be null = 0): g_opacity, g_depth, g_rgb_fg(3), g_z_variance, g_normal_acc(3).
 * Per-sample upstream grads (null = 0): g_weights, g_sdf, g_sdf_grad(3).
 * Saved forward state: opacity, depth (per ray), trans, sdf, sdf_grad, features (per sample).
 * g_inv_std_rays: as in tt_march_bwd (null unless the variance is trained).
 * workspace: n_rays*S*4 floats (written by the march backward, read by the decode backward).
 * grad_packed (P,6,H,W,32) and mlp grads are accumulated into (caller zero-fills).  The packed planes (= one copy of
 * grad_packed) must be smaller than 4 GB - 256 B (85 prompts of 256^2 planes), else TT_ERR_UNSUPPORTED -- the limit
 * applies to every entry point that takes a tt_render_cfg or a packed-planes pointer (32-bit texel byte offsets). */
int tt_render_bwd_geo(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                      const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, const float* opacity,
                      const float* depth, const float* trans, const float* sdf, const float* sdf_grad,
                      const float* features, const float* g_opacity, const float* g_depth, const float* g_rgb_fg,
                      const float* g_z_variance, const float* g_normal_acc, const float* g_weights,
                      const float* g_sdf, const float* g_sdf_grad, float* g_inv_std_rays, float* workspace,
                      float* grad_packed, const tt_mlp_grads* grads, void* stream);

/* tt_render_bwd_geo with the h2 sign mask of tt_render_fwd_h2mask (same planes, weights, rays and intervals as that
 * call): the decode backward reads the signs instead of recomputing W2 h1 for them.  Gradients agree with
 * tt_render_bwd_geo up to the rounding of a pre-activation within an ulp of zero. */
int tt_render_bwd_geo_h2mask(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                             const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                             const float* opacity, const float* depth, const float* trans, const float* sdf,
                             const float* sdf_grad, const float* features, const float* g_opacity,
                             const float* g_depth, const float* g_rgb_fg, const float* g_z_variance,
                             const float* g_normal_acc, const float* g_weights, const float* g_sdf,
                             const float* g_sdf_grad, float* g_inv_std_rays, float* workspace, float* grad_packed,
                             const tt_mlp_grads* grads, const uint32_t* h2_mask, void* stream);

/* tt_render_bwd_geo with both sign masks of tt_render_fwd_masks.  In the split precisions nothing reads the values of h1
 * any more: with u = sbar f + J gbar (gathered directly) the kernel forms v = m1 . (W1 u) from ONE product with W1, where the
 * other entries form sbar relu(W1 f) + m1 . W1 (J gbar) from two, and it gathers u alone.  d/d planes and d/d w1 are computed
 * as by tt_render_bwd_geo_h2mask; d/d w2 and d/d w3 differ from it by the rounding of v.  The fp32-MFMA precision ignores
 * h1_mask and runs tt_render_bwd_geo_h2mask's kernel. */
int tt_render_bwd_geo_masks(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                            const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                            const float* opacity, const float* depth, const float* trans, const float* sdf,
                            const float* sdf_grad, const float* features, const float* g_opacity,
                            const float* g_depth, const float* g_rgb_fg, const float* g_z_variance,
                            const float* g_normal_acc, const float* g_weights, const float* g_sdf,
                            const float* g_sdf_grad, float* g_inv_std_rays, float* workspace, float* grad_packed,
                            const tt_mlp_grads* grads, const uint32_t* h2_mask, const uint32_t* h1_mask, void* stream);

/* Backward, texture half: d/d(texture planes 3..5) and d/d(feature net).
 * Needs saved weights (per sample) and features; g_rgb_fg (per ray), g_features (per sample; null = 0). */
int tt_render_bwd_tex(const float* packed, const tt_mlp_weights* w, const float* rays_o, const float* rays_d,
                      const float* t_starts, const float* t_ends, const tt_render_cfg* cfg, const float* weights,
                      const float* features, const float* g_rgb_fg, const float* g_features, float* grad_packed,
                      const tt_mlp_grads* grads, void* stream);

/* Backward of the per-point queries.  points (n_batch, n_points, 3) as in tt_query_points
 * (constants here: the gradient w.r.t. the points is tt_points_bwd_x)
 * _geo: upstream g_sdf (n) and/or g_sdf_grad (n,3) (one may be null) -> d/d geometry planes 0..2 (accumulated into
 *       grad_packed, caller zero-fills) and d/d sdf net (grads->w1..w3).  workspace: n*4 floats.
 * _tex: upstream g_features (n,3) of a 96->64->64->3 net in w->v1..v3 reading planes plane_base..plane_base+2 of
 *       each prompt: plane_base = 3 is the feature net on the texture planes (tt_query_points with TT_Q_TEX);
 *       plane_base = 0 with v1 = [U1 U1 U1] is a 32->64->64->3 net on the SUM of the geometry planes, i.e. the
 *       deformation head of tt_query_field (d/d U1 = the sum of the three 64x32 column blocks of grads->v1). */
int tt_points_bwd_geo(const float* packed, const tt_mlp_weights* w, const float* points, int32_t n_batch,
                      int64_t n_points, int32_t n_prompts, int32_t views_per_prompt, int32_t plane_h, int32_t plane_w,
                      float radius, float sdf_bias_radius, int32_t flags, const float* g_sdf, const float* g_sdf_grad,
                      float* workspace, float* grad_packed, const tt_mlp_grads* grads, void* stream);
int tt_points_bwd_tex(const float* packed, const tt_mlp_weights* w, const float* points, int32_t n_batch,
                      int64_t n_points, int32_t n_prompts, int32_t views_per_prompt, int32_t plane_h, int32_t plane_w,
                      float radius, int32_t plane_base, int32_t flags, const float* g_features, float* grad_packed,
                      const tt_mlp_grads* grads, void* stream);

/* Gradient of the per-point decode w.r.t. the QUERY POINTS (the reference keeps `points` in the autograd graph:
 * few_step...:283-286,329-335; caller generative_space_mesh_rasterize_renderer.py:307-331): for upstream g_sdf (n),
 * g_sdf_grad (n,3), g_features (n,3) (any may be null = 0)
 *   grad_points (n,3) = g_sdf d sdf/dx + d (g_sdf_grad . sdf_grad)/dx + (d features/dx)^T g_features,
 * i.e. aten grid_sampler_2d_backward's grad_grid for sdf / features and K1's `grad_grid` output
 * (gridsample_cuda.cu:196-208: the cross derivative of the bilinear interpolation) plus the sphere bias's Hessian for the
 * second-order term.  Overwrites grad_points.  flags: TT_Q_EXACT_F32 or 0.  (d/d planes and d/d weights of the same
 * upstream come from tt_points_bwd_geo / _tex.) */
int tt_points_bwd_x(const float* packed, const tt_mlp_weights* w, const float* points, int32_t n_batch,
                    int64_t n_points, int32_t n_prompts, int32_t views_per_prompt, int32_t plane_h, int32_t plane_w,
                    float radius, int32_t flags, const float* g_sdf, const float* g_sdf_grad, const float* g_features,
                    float* grad_points, void* stream);

/* Multiresolution hash encoding of 3-D points in [0,1]^3 (tcnn "HashGrid", Linear interpolation, fp32).
 * params: flat table, level-major, entry-major, feature-minor (tcnn's `params` layout), tt_hashgrid_n_params floats
 * (negative tt_status on a bad config); x (n,3); out / g_out (n, n_levels*n_features_per_level) row-major.
 * _bwd accumulates d/d params into grad_params (caller zero-fills); no gradient w.r.t. x. */
typedef struct {
    int32_t n_levels;             /* <= 16 */
    int32_t n_features_per_level; /* 1, 2, 4 or 8 */
    int32_t log2_hashmap_size;
    int32_t base_resolution;
    float per_level_scale;
} tt_hashgrid_cfg;
int64_t tt_hashgrid_n_params(const tt_hashgrid_cfg* cfg);
int tt_hashgrid_fwd(const float* x, int64_t n, const float* params, const tt_hashgrid_cfg* cfg, float* out,
                    void* stream);
int tt_hashgrid_bwd(const float* x, int64_t n, const float* g_out, const tt_hashgrid_cfg* cfg, float* grad_params,
                    void* stream);

/* PatchRenderer's per-key composite (threestudio/models/renderers/patch_renderer.py:74-88): out (B,H,W,C) = bilinear
 * upsample (F.interpolate, align_corners=False) of low (B,h,w,C) with patch (B,PS,PS,C) pasted at rows py.., columns
 * px..  _bwd: g_patch = the pasted region of g_out; g_low = the adjoint of the upsample over the pixels the patch did
 * not overwrite (null = global_detach: skipped).  Both overwrite their outputs. */
int tt_patch_composite_fwd(const float* low, const float* patch, float* out, int32_t B, int32_t h, int32_t w, int32_t H,
                           int32_t W, int32_t C, int32_t PS, int32_t py, int32_t px, void* stream);
int tt_patch_composite_bwd(const float* g_out, float* g_low, float* g_patch, int32_t B, int32_t h, int32_t w, int32_t H,
                           int32_t W, int32_t C, int32_t PS, int32_t py, int32_t px, void* stream);

/* Eikonal regulariser of the training loop on the renderer's per-sample `sdf_grad` output (n,3):
 *   loss[0] = mean((||sdf_grad||_2 - 1)^2)      (multiprompt_dual_renderer_multistep_generator.py:696-699)
 * one pass each way instead of ~10 torch kernels over the per-sample tensor.  _fwd overwrites loss[0] (device);
 * _bwd: g_sdf_grad (n,3) = g_loss[0] * 2 (||g|| - 1) / (n ||g||) * g (0 where ||g|| = 0), g_loss a DEVICE scalar. */
int tt_eikonal_fwd(const float* sdf_grad, int64_t n, float* loss, void* stream);
int tt_eikonal_bwd(const float* sdf_grad, const float* g_loss, int64_t n, float* g_sdf_grad, void* stream);

/* The renderer's per-ray composite (generative_space_sdf_volume_renderer.py:433-530) as one kernel each way:
 *   comp_rgb = rgb_fg + bg (1 - opacity)                                   bg: (3) with bg_stride 0, or (n,3) with 3
 *   disparity = clamp((far - (depth opacity + (1 - opacity) far)) / (far - near), 0, 1), far/near = d_cam +- sqrt(3)
 *   comp_normal = normalize(normal_acc)
 *   mode 1 ("camera"): n_cam = comp_normal @ inverse(c2w)[:3,:3]^T @ diag(-1,1,1);
 *                      normal_cam_vis = (n_cam+1)/2 opacity + (1-opacity) (0.5,0.5,1), _white with (1,1,1)
 *   mode 2 ("front") : the camera of view (v / view_group) * view_group, no flip, _white only;  mode 0 ("world"): neither.
 * _bwd: gradients w.r.t. opacity, depth, rgb_fg, normal_acc and, if g_bg is given, the PER-RAY background colour (n,3)
 * (a constant colour's gradient is its sum over rays), all overwritten, from the upstream gradients (null = 0). */
int tt_composite_fwd(const float* opacity, const float* depth, const float* rgb_fg, const float* normal_acc,
                     const float* bg, int32_t bg_stride, const float* camera_distances, const float* c2w, int64_t n_rays,
                     int32_t rays_per_view, int32_t mode, int32_t view_group, float* comp_rgb, float* disparity,
                     float* comp_normal, float* normal_cam_vis, float* normal_cam_vis_white, void* stream);
int tt_composite_bwd(const float* opacity, const float* depth, const float* rgb_fg, const float* normal_acc,
                     const float* bg, int32_t bg_stride, const float* camera_distances, const float* c2w, int64_t n_rays,
                     int32_t rays_per_view, int32_t mode, int32_t view_group, const float* g_comp_rgb,
                     const float* g_disparity, const float* g_comp_normal, const float* g_normal_cam_vis,
                     const float* g_normal_cam_vis_white, float* g_opacity, float* g_depth, float* g_rgb_fg,
                     float* g_normal_acc, float* g_bg, void* stream);

/* Operator-level drop-in for the reference's pybind op `gridsample_grad2.grad2_2d`
 * (gridsample_cuda.cpp:26-37; dispatch gridsample_cuda.cu:560-594): backward of aten::grid_sampler_2d_backward,
 * bilinear.  Contiguous tensors of one dtype: input / grad2_grad_input / grad_input (n,c,h,w); grid / grad2_grad_grid /
 * grad_grid (n,Ho,Wo,2); grad_output / grad_grad_output (n,c,Ho,Wo); n_points_per_batch = Ho*Wo.
 * padding_mode 0 = zeros, 1 = border (the reference passes it as a bool); align_corners 0 / 1; dtype TT_DTYPE_*
 * (half computes in fp32).  Reflection padding and the 3-D variant are TT_ERR_UNSUPPORTED / not exported (the
 * reference never calls them).  grad_input is zero-filled inside (like the reference).
 * A point with a non-finite grid coordinate (NaN or +-inf on either axis) is inert, as in the reference, whose
 * within_bounds_2d skips its taps: its rows of grad_grad_output and grad_grid are exactly 0 and it adds 0 to
 * grad_input (the same contract as tt_texture_* for non-finite UVs).  The sizes are the caller's to get right:
 * nothing here can check a pointer against n, c, h, w or n_points_per_batch (grid_sample_gradfix.grad2_2d does).
 * tt_grid_sample_2d_grad2 is the fp32 entry point. */
#define TT_DTYPE_F32 0
#define TT_DTYPE_F16 1
#define TT_DTYPE_F64 2
int tt_grid_sample_2d_grad2_typed(int32_t dtype, const void* grad2_grad_input, const void* grad2_grad_grid,
                                  const void* grad_output, const void* input, const void* grid, int32_t n, int32_t c,
                                  int32_t h, int32_t w, int64_t n_points_per_batch, int32_t padding_mode,
                                  int32_t align_corners, void* grad_grad_output, void* grad_input, void* grad_grid,
                                  void* stream);
int tt_grid_sample_2d_grad2(const float* grad2_grad_input, const float* grad2_grad_grid, const float* grad_output,
                            const float* input, const float* grid, int32_t n, int32_t c, int32_t h, int32_t w,
                            int64_t n_points_per_batch, int32_t padding_mode, int32_t align_corners,
                            float* grad_grad_output, float* grad_input, float* grad_grid, void* stream);

/* ---- marching cubes (tt_isosurface.hip): the drop-in for diso.DiffMC ----
 * Replaces `DiffMC(dtype=torch.float32)(level, deformation, isovalue=...)` as DiffMarchingCubeHelper.forward calls it
 * (triplaneturbo_executable/utils/mesh_exporter.py:65-75; grid query :78-105 = tt_query_field).  diso's own
 * conventions are not available to pin, so this is the library's contract; what the reference itself fixes is marked (ref).
 *   input       level (R,R,R) fp32, indexed [i][j][k] = level.view(R,R,R) of the helper's grid_vertices
 *               (torch.meshgrid(..., indexing="ij"), k fastest) (ref); deformation (R,R,R,3) fp32 or NULL; isovalue.
 *               2 <= R <= TT_MC_MAX_RES, anything else is TT_ERR_BAD_ARG.
 *   inside      a grid point is inside iff level < isovalue (strict); an edge crosses iff exactly one end is inside.
 *   vertex      on the crossing edge p0 -> p1 (p = integer grid index, d = deformation IN GRID-CELL UNITS -- an
 *               assumption about diso, not verifiable here):  t = (iso - s0) / (s1 - s0),
 *               v = ((p0 + d0) + t * ((p1 + d1) - (p0 + d0))) / (R - 1), i.e. [0,1] coordinates like the reference's
 *               CPU helper (isosurface.py:122); the caller maps them to its points_range (mesh_exporter.py:73) (ref).
 *   sharing     one vertex per crossing edge; grid point p owns its +x, +y, +z edges.
 *   order       vertices by (owner point linear index, axis x < y < z); triangles by (cell linear index, table order),
 *               the cell of origin (i,j,k) having linear index i*R*R + j*R + k.  Deterministic: no atomics, identical
 *               launches give bit-identical outputs and gradients.
 *   orientation cross(v1 - v0, v2 - v0) points toward increasing level (outward for an SDF), as Mesh.v_nrm
 *               (mesh.py:114-140) expects.  The case tables (csrc/tt_mc_tables.h, generated by tools/gen_mc_tables.py)
 *               cut every face from its own 4 bits (an ambiguous face cuts its two inside corners off separately), so
 *               the mesh is watertight inside the box.
 *   boundary    no padding: a surface that leaves the box is open there (like the reference's mcubes helper).
 *   outputs     v_pos fp32 (V,3); t_pos_idx int32 (T,3) (the type nvdiffrast consumes).
 *   gradients   tt_mc_bwd: from d loss / d v_pos to level and deformation (as DiffMC); t_pos_idx has none.
 * Use: bytes = tt_mc_workspace_bytes(R); tt_mc_count(...) writes (V, T) to out_totals (2 int32 in DEVICE memory; read
 * them back -- the only host round trip); allocate v_pos / t_pos_idx; tt_mc_emit(...) with the SAME level / isovalue /
 * workspace; the backward reads the crossing masks and vertex offsets the count left in the workspace, so keep it.
 * Every kernel write is bounded by the totals the count itself computed (whatever the level values); NaN levels are
 * outside.  tt_mc_workspace_bytes returns TT_ERR_BAD_ARG for an unsupported R. */
#define TT_MC_MAX_RES 512
int64_t tt_mc_workspace_bytes(int32_t res);
int tt_mc_count(const float* level, int32_t res, float isovalue, void* workspace, int32_t* out_totals, void* stream);
int tt_mc_emit(const float* level, const float* deformation, int32_t res, float isovalue, void* workspace, float* v_pos,
               int32_t* t_pos_idx, void* stream);
/* grad_v (V,3) -> grad_level (R,R,R) and, iff deformation is given, grad_deformation (R,R,R,3): dense, every element
 * written (zero off the surface); a gather over each point's 6 incident edges. */
int tt_mc_bwd(const float* level, const float* deformation, int32_t res, float isovalue, void* workspace,
              const float* grad_v, float* grad_level, float* grad_deformation, void* stream);

/* ---- marching tetrahedra (tt_tets.hip): the drop-in for MarchingTetrahedraHelper._forward ----
 * Replaces the extraction of threestudio/models/isosurface.py:231-301 (DMTet) and reproduces its outputs: same vertices,
 * same faces, same order.  The reference finds the unique edges of the surface tets with torch.unique(dim=0) on every
 * call; the tet grid is static, so here the tables are built once per grid (ops.TetGrid) and passed in:
 *   tets        (Nt,4) int32: the grid's tetrahedra, vertex ids in [0, Nv).
 *   edges       (Ne,2) int32: the unique vertex pairs (a < b) of the six base edges 01 02 03 12 13 23 of every tet, in
 *               lexicographic order (the helper's all_edges, isosurface.py:206-219).
 *   tet_edge    (Nt,6) int32: the row of `edges` of each base edge of each tet, in that base order.
 *   vert_ptr    (Nv+1) int32, vert_col int32: vertex -> incident rows of `edges` (CSR, each row ascending).
 * The entry points TRUST these tables (ops.TetGrid validates them once: every id in range, counts within
 * TT_MESH_MAX_ITEMS); with valid tables no kernel indexes out of range whatever the level values.
 *   occupied    a grid vertex is occupied iff level > 0 (isosurface.py:236; NOT marching cubes' level < iso); a NaN
 *               level is unoccupied.  An edge crosses iff exactly one end is occupied; a tet's case is
 *               sum_k occupied[v_k] << k into the 16-row triangle table of isosurface.py:141-169.
 *   vertex      vertex i is the i-th crossing edge in `edges` order.  On the edge (a < b), with s = level, p = pos:
 *               D = s_a - s_b,  w_a = (-s_b) / D,  w_b = s_a / D,  v = p_a * w_a + p_b * w_b, evaluated in fp32 in that
 *               order without contraction (isosurface.py:269-276).  D adds like-signed magnitudes: it never cancels.
 *   faces       the faces of the one-triangle tets in tet order, then two rows per two-triangle tet in tet order
 *               (isosurface.py:285-299); vertex ids through tet_edge and the triangle table.
 *   outputs     v_pos fp32 (V,3); t_pos_idx int32 (T1 + 2 T2, 3).  pos (Nv,3) fp32 is the (deformed) grid.
 *   gradients   tt_mt_bwd: from d loss / d v_pos to level (Nv) and pos (Nv,3), dense, every element written (exact
 *               zeros off the crossing edges): a gather over each vertex's CSR row in ascending edge order.
 *               dv/ds_a = (p_b - p_a)(-s_b)/D^2, dv/ds_b = (p_b - p_a) s_a/D^2, dv/dp_a = w_a, dv/dp_b = w_b.
 * Use: bytes = tt_mt_workspace_bytes(Ne, Nt); tt_mt_count(...) writes (V, T1, T2) to out_totals (3 int32 in DEVICE
 * memory; read them back -- the only host round trip); allocate v_pos (V,3) and t_pos_idx (T1 + 2 T2, 3); tt_mt_emit
 * with the SAME tables / workspace; the backward reads the crossing flags and vertex offsets the count left in the
 * workspace, so keep it.  Every kernel write is bounded by the totals the count itself computed.  No atomics:
 * identical launches give bit-identical outputs and gradients.  1 <= Ne, Nt, Nv <= TT_MESH_MAX_ITEMS, anything else
 * is TT_ERR_BAD_ARG. */
int64_t tt_mt_workspace_bytes(int32_t n_edges, int32_t n_tets);
int tt_mt_count(const float* level, const int32_t* edges, const int32_t* tets, int32_t n_edges, int32_t n_tets,
                void* workspace, int32_t* out_totals, void* stream);
int tt_mt_emit(const float* pos, const float* level, const int32_t* edges, const int32_t* tet_edge, int32_t n_edges,
               int32_t n_tets, void* workspace, float* v_pos, int32_t* t_pos_idx, void* stream);
int tt_mt_bwd(const float* pos, const float* level, const int32_t* edges, const int32_t* vert_ptr,
              const int32_t* vert_col, int32_t n_vertices, int32_t n_edges, int32_t n_tets, void* workspace,
              const float* grad_v, float* grad_level, float* grad_pos, void* stream);

/* ---- rasterize / interpolate / antialias (tt_raster.hip): the drop-in for nvdiffrast ----
 * Replaces dr.rasterize, dr.interpolate and dr.antialias as NVDiffRasterizerContext calls them
 * (threestudio/utils/rasterize.py; generative_space_mesh_rasterize_renderer.py:137-295).  Instance mode: one
 * topology tri (T,3) int32 shared by B >= 1 views of clip-space positions pos (B,V,4); every tensor contiguous, fp32.
 * Range mode (the tt_*_range_* entries, below) renders different meshes in one call.
 * T = 0 and V = 0 are legal (zero outputs, zero gradients).  T >= TT_RAST_MAX_TRIS is TT_ERR_BAD_ARG (tri + 1 is
 * stored as a float).  A pointer may be NULL only where the count it is indexed by is 0 (pos: V, tri / topology: T).
 * A triangle with an index outside [0, V) or a repeated index is never rasterized, and interpolate / antialias treat
 * a pixel whose id is not in [1, T] as empty.  nvdiffrast's source is not available to pin, so this is the contract:
 *   rasterize   rast (B,H,W,4) = (u, v, z/w, tri + 1); an empty pixel is all zeros.
 *     pixel     (px, py) samples NDC x = (2 px + 1) / W - 1, y = (2 py + 1) / H - 1 (row 0 at y = -1).
 *     bary      u, v perspective-correct barycentrics of vertices tri[t,0], tri[t,1] (tri[t,2] gets 1 - u - v).
 *     coverage  the pixel centre is inside by the homogeneous 2-D edge functions (Olano-Greer) over (x, y, w), with
 *               e_k = (v_i x v_j) . (x, y, 1), (i, j, k) cyclic, each multiplied by sign(det[v0, v1, v2]); the
 *               interpolated w > 0; -1 <= z/w <= 1 (near / far clipping).  No face is culled; zero-area triangles
 *               (det = 0) never produce fragments.  When all three w > 0 the same test runs on screen-space edge
 *               functions (x/w, y/w differences, with their rounding residuals) for accuracy on pixel-sized triangles.
 *     edges     every edge function is evaluated from its endpoints in canonical order (lower vertex index first), so
 *               two triangles sharing an edge see exactly negated values.  Tie (value exactly 0): the triangle owns
 *               the pixel iff its inward edge normal (sign * (n.x, n.y)) has n.x > 0, or n.x = 0 and n.y > 0 -- one
 *               of the two triangles of a shared edge.  The form is chosen per EDGE where it decides coverage: an edge
 *               whose two endpoints both have w > 0 takes its sign and its tie from the screen-space form, also in a
 *               triangle whose third vertex has w <= 0 (its neighbour across that edge may have every w > 0, and the
 *               two forms are not each other's negation in float); such a triangle still computes (u, v, z/w) from
 *               the homogeneous values of all three edges, that edge's clamped at 0 where the two forms disagree in
 *               sign.  An edge with an endpoint at w <= 0 uses the homogeneous form in both of its triangles.
 *     depth     the smallest z/w wins; on equal z/w the smaller triangle id.  z/w = -0 is stored, and compared, as
 *               +0: the two zeros are equal depths.  64-bit atomicMin of (order-preserving bits of z/w + 0 << 32 |
 *               tri) per pixel: bit-identical across launches.
 *     gradient  tt_rast_bwd: grad_rast (B,H,W,4) -> grad_pos (B,V,4) through u, v only (z/w and the id carry none;
 *               pos[...,2] receives nothing: u, v do not depend on clip z).
 *   interpolate out (B,H,W,C) = u a0 + v a1 + (1-u-v) a2, 0 on empty pixels; attr (attr_batch,V,C), attr_batch = B or
 *               1 (broadcast over views).  Backward: grad_attr (attr_batch,V,C) (batch summed out when broadcast) and
 *               grad_rast (B,H,W,4) in the u, v channels (z/w, id zero); either output may be NULL, not both.  No
 *               rast_db / diff_attrs.
 *   antialias   analytic silhouette antialiasing (Laine et al. 2020, "Modular Primitives for High-Performance
 *               Differentiable Rendering", section 4.3):
 *     pairs     every horizontally or vertically adjacent pixel pair (p, q) whose triangle ids differ.
 *     occluder  t = the triangle of the covered pixel; both covered: the smaller z/w, on a tie the smaller id.  a =
 *               t's pixel, b = the other.
 *     silhouette an edge of t is a silhouette edge in this view if no other triangle shares it, or a triangle sharing
 *               it has the opposite screen-space orientation (sign of det[[x,y,w]_0, [x,y,w]_1, [x,y,w]_2]).  Edges
 *               with an endpoint at w <= 0 are skipped.
 *     crossing  among the silhouette edges whose screen projection crosses the segment from a's centre to b's
 *               centre, the crossing nearest a; half-open in the perpendicular axis (an edge crosses the scanline q
 *               iff (q_0 > q) != (q_1 > q)); s in [0, 1) its distance from a's centre in pixels.  A vertex projects
 *               to pixel coordinates ((x/w + 1) W - 1) / 2, ((y/w + 1) H - 1) / 2.
 *     blend     out = color; per pair, if s < 0.5: out[a] += (0.5 - s)(color[b] - color[a]), else
 *               out[b] += (s - 0.5)(color[a] - color[b]).  Each pair changes at most one pixel; coverage moves
 *               one-for-one with the edge.
 *     gradient  tt_aa_bwd: grad_color, and through s to the two edge vertices' clip x, y, w (grad_pos, may be NULL);
 *               none to rast.
 *     topology  edge_ofs (3T,2) int32 = (first, count) of the group of triangle edge 3t + k (vertices k, (k+1)%3)
 *               in the list of the 3T edges sorted by (lower, higher) vertex index; edge_tri (3T) int32 = the
 *               triangle of each sorted entry.  It depends on tri only: build it once per mesh (raster.py).
 *   range mode  nvdiffrast's second batching mode: one vertex buffer pos (V,4) shared by all images, tri (T,3), and
 *               ranges (B,2) int32 = (first triangle, triangle count) per image.  Image b rasterizes exactly the
 *               triangles first_b .. first_b + count_b - 1 by the rules above; the id channel holds the GLOBAL
 *               triangle index + 1 (an index into the whole tri), so depth ties go to the smaller global index.
 *               count = 0 is legal (an all-zero image, no gradient); ranges may overlap, repeat and come in any
 *               order; first < 0, count < 0 or first + count > T is TT_ERR_BAD_ARG.  The caller passes the ranges
 *               twice: ranges_dev (read by the kernels) and ranges_host, the same values in host memory, from which
 *               the entry point validates them and sizes the work list (n_slots = the sum of the counts) without a
 *               device round trip.  tt_rast_range_bwd, tt_aa_range_fwd / _bwd read pos (V,4) for every image and
 *               write grad_pos (V,4), summed over the images.  Interpolation needs no entry of its own: tt_interp_fwd
 *               / _bwd with attr_batch = 1 on a range-mode rast (global ids) is range-mode interpolation.  Antialias
 *               takes the topology of the whole tri, and the silhouette test looks at every triangle sharing an edge,
 *               whatever range it is in (nvdiffrast builds its topology on the whole tri too): meshes that share no
 *               vertices never interact, meshes that share an edge see each other there.
 * Determinism: rast, interpolate's output, antialias's output and grad_color are gathers (or an order-independent
 * min): bit-identical across launches.  grad_pos (tt_rast_bwd, tt_aa_bwd) and grad_attr use fp32 atomic adds and are
 * NOT bit-reproducible.  Every gradient output is overwritten (zeroed inside).
 * Use: bytes = tt_rast_workspace_bytes(B, T, H, W) (device workspace of tt_rast_fwd: bounding boxes, the int64
 * candidate scan, per-pixel depth keys); no host round trip (the candidate total is read on the device), so the
 * forward is capturable.  Range mode: bytes = tt_rast_range_workspace_bytes(B, n_slots, H, W); tt_rast_range_fwd reads
 * ranges_host during the call (it may be freed or changed afterwards) and makes no device round trip either. */
#define TT_RAST_MAX_TRIS (1 << 24)
int64_t tt_rast_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W);
int tt_rast_fwd(const float* pos, const int32_t* tri, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W,
                void* workspace, float* rast, void* stream);
int tt_rast_bwd(const float* pos, const int32_t* tri, const float* rast, const float* grad_rast, int32_t B, int32_t V,
                int32_t T, int32_t H, int32_t W, float* grad_pos, void* stream);
int tt_interp_fwd(const float* attr, int32_t attr_batch, const float* rast, const int32_t* tri, int32_t B, int32_t V,
                  int32_t T, int32_t H, int32_t W, int32_t C, float* out, void* stream);
int tt_interp_bwd(const float* attr, int32_t attr_batch, const float* rast, const int32_t* tri, const float* grad_out,
                  int32_t B, int32_t V, int32_t T, int32_t H, int32_t W, int32_t C, float* grad_attr, float* grad_rast,
                  void* stream);
int tt_aa_fwd(const float* color, const float* rast, const float* pos, const int32_t* tri, const int32_t* edge_ofs,
              const int32_t* edge_tri, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W, int32_t C, float* out,
              void* stream);
int tt_aa_bwd(const float* color, const float* rast, const float* pos, const int32_t* tri, const int32_t* edge_ofs,
              const int32_t* edge_tri, const float* grad_out, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W,
              int32_t C, float* grad_color, float* grad_pos, void* stream);
int64_t tt_rast_range_workspace_bytes(int32_t B, int64_t n_slots, int32_t H, int32_t W);
int tt_rast_range_fwd(const float* pos, const int32_t* tri, const int32_t* ranges_dev, const int32_t* ranges_host,
                      int32_t B, int32_t V, int32_t T, int32_t H, int32_t W, void* workspace, float* rast,
                      void* stream);
int tt_rast_range_bwd(const float* pos, const int32_t* tri, const float* rast, const float* grad_rast, int32_t B,
                      int32_t V, int32_t T, int32_t H, int32_t W, float* grad_pos, void* stream);
int tt_aa_range_fwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                    const int32_t* edge_ofs, const int32_t* edge_tri, int32_t B, int32_t V, int32_t T, int32_t H,
                    int32_t W, int32_t C, float* out, void* stream);
int tt_aa_range_bwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                    const int32_t* edge_ofs, const int32_t* edge_tri, const float* grad_out, int32_t B, int32_t V,
                    int32_t T, int32_t H, int32_t W, int32_t C, float* grad_color, float* grad_pos, void* stream);

/* ---- texture sampling (tt_texture.hip): the drop-in for nvdiffrast's 2-D `texture`, without mipmaps ----
 * Replaces dr.texture(tex, uv, filter_mode = "nearest" | "linear", boundary_mode = "wrap" | "clamp" | "zero"): with
 * rasterize, interpolate and antialias above, what a consumer of an exported OBJ + map_Kd needs to put the texture
 * back on the mesh (triplaneturbo_amd/viewer.py; the reference renders its exports with CUDA-only tools,
 * evaluation/mesh_visualize.py).  No mip levels, no uv_da / mip_level_bias, no cube maps: minification is the caller's
 * (the viewer supersamples).  Every tensor contiguous fp32.
 *   shapes      tex (tex_batch,TH,TW,C), tex_batch = B or 1 (one texture shared by all images); uv (B,H,W,2);
 *               out (B,H,W,C).  u runs along the width, v along the height; row 0 is at v = 0; texel (i, j) has its
 *               centre at ((i + 0.5) / TW, (j + 0.5) / TH).
 *   linear      x = u TW - 0.5, y = v TH - 0.5 (fp32, multiply then subtract); taps floor(x), floor(x) + 1 with weights
 *               1 - f, f, f = x - floor(x); the same in y; out = the sum over the four taps of wy wx tex.
 *   nearest     the texel floor(u TW), floor(v TH), weight 1.
 *   boundary    wrap: tap indices modulo the size (a negative index wraps to the far side; u is first reduced
 *               to u - trunc(u), which is exact in fp32 and the same sample); clamp: tap indices clamped to
 *               [0, size - 1]; zero: a tap outside [0, size - 1] has weight 0.
 *   non-finite  a pixel whose u or v is NaN or +-inf gets out = 0 and contributes no gradient.
 *   addresses   tap indices are formed as floats (floor, a floating-point modulo for wrap), clamped to [0, size - 1]
 *               by fmin / fmax and only then converted to integers: no uv value produces an address outside tex.  They
 *               are exact integers below 2^24, hence TT_TEX_MAX_SIZE.  Element offsets are 64-bit.
 *   gradient    tt_tex_bwd: grad_out (B,H,W,C) -> grad_tex (tex_batch,TH,TW,C) (summed over the images when tex_batch
 *               = 1) and grad_uv (B,H,W,2) = (TW d out/dx, TH d out/dy) . grad_out with the tap weights' derivatives
 *               (-1, +1, times the zero boundary's in-range factors); exactly 0 under nearest.  Either may be NULL.  Every
 *               element of a given output is written (grad_tex is zeroed inside): the caller does not pre-clear.
 *   sizes       B H W = 0 is legal and does nothing (tt_tex_bwd still zeroes grad_tex).  TH, TW or C < 1, TH or TW >
 *               TT_TEX_MAX_SIZE, tex_batch other than 1 or B, an unknown filter or boundary: TT_ERR_BAD_ARG.
 * Determinism: out and grad_uv are per-pixel gathers, bit-identical across launches; grad_tex uses fp32 atomic adds
 * (like grad_attr and grad_pos above) and is NOT bit-reproducible.  No workspace, no host round trip: capturable. */
#define TT_TEX_FILTER_NEAREST 0
#define TT_TEX_FILTER_LINEAR 1
#define TT_TEX_BOUNDARY_WRAP 0
#define TT_TEX_BOUNDARY_CLAMP 1
#define TT_TEX_BOUNDARY_ZERO 2
#define TT_TEX_MAX_SIZE 16777216
int tt_tex_fwd(const float* tex, int32_t tex_batch, const float* uv, int32_t B, int32_t H, int32_t W, int32_t TH,
               int32_t TW, int32_t C, int32_t filter, int32_t boundary, float* out, void* stream);
int tt_tex_bwd(const float* tex, int32_t tex_batch, const float* uv, const float* grad_out, int32_t B, int32_t H,
               int32_t W, int32_t TH, int32_t TW, int32_t C, int32_t filter, int32_t boundary, float* grad_tex,
               float* grad_uv, void* stream);

/* ---- mesh regularisers and outlier removal (tt_mesh.hip): threestudio Mesh.normal_consistency / laplacian /
 * remove_outlier (threestudio/models/mesh.py:31-95,255-308) ----
 * A mesh is v_pos (V,3) fp32 and t_pos_idx (T,3) int32 with every index in [0, V) (the host checks it when it builds
 * the topology; a face with an index outside [0, V) is never kept and never read through).
 *   topology    built once per mesh on the host side with torch sorts (ops.mesh_topology), from t_pos_idx alone:
 *               edges (E,2) int32 = the unique rows of sort(each face's (0,1), (1,2), (2,0) pair), ascending
 *               lexicographic, self pairs (a,a) of degenerate faces included (Mesh._compute_edges);
 *               face_pairs (P,2) int32 = for every edge that EXACTLY TWO of the 3T face edges use, the two faces;
 *               the vertex -> neighbour CSR nbr_ptr (V+1), nbr_col (2E) int32 = both directions of every edge, each
 *               row in ascending column order (a self edge appears twice in its row); nbr_col (and edges) may be
 *               NULL for a mesh without edges.
 *   adjacency   two faces are joined iff they share an edge used by exactly two face edges (trimesh's
 *               face_adjacency rule, group_rows(..., require_count=2)); an edge used once, or three or more times
 *               (non-manifold), joins nothing.  On an edge-manifold mesh (every tt_mc_* mesh) any rule agrees.
 *   components  tt_mesh_components: labels (T) int32, label[f] = the smallest face index of f's component
 *               (independent of scheduling); the workspace keeps the face count per component and the largest count.
 *   threshold   tt_mesh_compact_count after tt_mesh_components with the same workspace: frac_mode = 1 -> thr =
 *               (int64)((double)max_faces * frac) (Python's int(max * t)); frac_mode = 0 -> thr = threshold.  A
 *               face is kept iff its component has >= thr faces; a vertex is kept iff a kept face references it.
 *   order       kept vertices and kept faces keep their original relative order; t_out holds the new vertex ids.
 *               (V', T') go to out_totals (2 int32, DEVICE memory, read back: the only host round trip); allocate;
 *               tt_mesh_compact_emit with the same workspace.  Every write is bounded by those totals.
 *   empty       T = 0: tt_mesh_components does nothing; the compaction needs T >= 1 (the host returns an empty mesh
 *               unchanged).
 *   laplacian   r_i = sum over the neighbours j != i of (v_i - v_j); loss = (1/V) sum_i |r_i| (unreferenced vertices
 *               count in V with r_i = 0; V = 0 gives NaN like torch's mean).  Backward: g_k = sum over the neighbours
 *               j != k of (w_k - w_j), w_i = (grad_loss / V) r_i / |r_i| (0 where r_i = 0, torch's subgradient).
 *   normal c.   loss = (1/E) sum over the edges (a,b) of (1 - cos(n_a, n_b)) with torch.cosine_similarity(dim=-1,
 *               eps=1e-8): cos = sum_c (x_c / max(|x|, eps)) (y_c / max(|y|, eps)); E = 0 gives NaN.  Backward to
 *               v_nrm per vertex over its CSR row: d cos / d x = y/(max(|y|,eps) max(|x|,eps)) - cos x/(max(|x|,eps)
 *               |x|) (the last factor 0 for x = 0), times -grad_loss / E.  The gradient to v_pos is the caller's
 *               (autograd through its vertex normals).
 * Determinism: the labels, counts and the compaction use integer atomics only (order-independent); the losses are
 * fixed-order block partials plus a one-block sum, the gradients CSR gathers: forward values and gradients are
 * bit-identical from launch to launch.  The losses take no host round trip and allocate nothing (grad_loss is read
 * on the device), so they are capturable given the topology and workspace.  Every gradient output is overwritten.
 * Use: bytes = tt_mesh_workspace_bytes(V, T) (one workspace serves all entry points of one mesh); every entry point
 * validates its arguments before any HIP call (TT_ERR_BAD_ARG). */
#define TT_MESH_MAX_ITEMS (1 << 28)
#define TT_MESH_COS_EPS 1e-8f
int64_t tt_mesh_workspace_bytes(int32_t V, int32_t T);
int tt_mesh_components(const int32_t* face_pairs, int32_t P, int32_t T, void* workspace, int32_t* labels,
                       void* stream);
int tt_mesh_compact_count(const int32_t* t_pos_idx, const int32_t* labels, int32_t V, int32_t T, int32_t frac_mode,
                          double frac, int64_t threshold, void* workspace, int32_t* out_totals, void* stream);
int tt_mesh_compact_emit(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, void* workspace,
                         float* v_out, int32_t* t_out, void* stream);
int tt_mesh_laplacian_fwd(const float* v_pos, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V, int32_t T,
                          void* workspace, float* loss, void* stream);
int tt_mesh_laplacian_bwd(const float* v_pos, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V, int32_t T,
                          const float* grad_loss, void* workspace, float* grad_v, void* stream);
int tt_mesh_nc_fwd(const float* v_nrm, const int32_t* edges, int32_t V, int32_t T, int32_t E, void* workspace,
                   float* loss, void* stream);
int tt_mesh_nc_bwd(const float* v_nrm, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V, int32_t E,
                   const float* grad_loss, float* grad_nrm, void* stream);

/* ---- UV atlas and texture fill (tt_uv.hip; tt_uv_pack in tt_host.cpp): the stand-ins for xatlas and cv2.inpaint
 * in the mesh exporter (multiprompt_mesh_exporter.py:72-134, threestudio/models/mesh.py:207-249) ----
 * An axis-projection atlas for marching-cubes meshes, NOT an xatlas clone.  A mesh is v_pos (V,3) fp32, t_pos_idx
 * (T,3) int32 and its face_pairs (P,2) int32 (the topology of the mesh regularisers above, ops.mesh_topology).
 *   labels      l in {0: +x, 1: -x, 2: +y, 3: -y, 4: +z, 5: -z}.  n = (p1 - p0) x (p2 - p0) in double from the fp32
 *               positions (n_x = e1y e2z - e1z e2y, n_y = e1z e2x - e1x e2z, n_z = e1x e2y - e1y e2x, |n|^2 =
 *               (n_x^2 + n_y^2) + n_z^2, in that order, no fused operations); the score of l is +-n_axis.  The
 *               initial label is the first argmax of the six scores.  l is admissible iff copysign(s^2, s) >=
 *               tau^2 |n|^2 (tau^2 = (double)tau * (double)tau), i.e. n_hat . a_l >= tau.  A face with |n|^2 = 0
 *               (or an index outside [0, V)) is zero-area: no admissible label, initial label +x.
 *   smoothing   `rounds` Jacobi rounds (TT_UV_DEFAULT_ROUNDS = 8, tau = TT_UV_DEFAULT_TAU = 0.3; 0 < tau <=
 *               TT_UV_MAX_TAU < 1/sqrt(3), so the argmax is always admissible).  The neighbours of f are the other
 *               faces of the face_pairs rows (a, b), a != b, that hold f (at most 3).  Votes: 1 for f's current label
 *               and 1 per neighbour's.  The new label is the admissible label with the most votes; on a tie the
 *               current label (always admissible) stays, else the smallest wins.  A zero-area face takes the smallest
 *               neighbour label of the previous round, +x without neighbours.
 *   charts      the connected components (tt_mesh_components) of the face_pairs rows whose faces have the same label
 *               and are not marked in `singleton` (T uint8, may be NULL); dense ids 0..C-1 in order of each chart's
 *               smallest face.  C goes to out_totals[0] (DEVICE memory).
 *   projection  a chart of label l maps a position p to (u, v) = +x (y,z), -x (z,y), +y (z,x), -y (x,z), +z (x,y),
 *               -z (y,x): u x v = +a_l, so a non-degenerate face has positive signed UV area, at least tau times its
 *               3-D area.  chart_box (T,4) fp32, rows 0..C-1 = (umin, vmin, umax, vmax) of the chart's vertices.
 *   packing     tt_uv_pack, HOST memory: w = (double)umax - (double)umin, h the same in v.  At density s (texels per
 *               world unit) a chart's box is bw = ceil(w s) + 2 pad + 1 by bh = ceil(h s) + 2 pad + 1 texels.  Boxes
 *               sorted by (bh desc, bw desc, chart asc) go left to right onto shelves of width N; a box that does not
 *               fit on the current shelf opens a new one at y += the shelf's height (its first box's).  s fits iff
 *               every box lands inside N x N.  s = the largest fitting value found by bisection on [0, (N - 2 pad) /
 *               max(w, h)], every probe rounded to float, until hi - lo <= TT_UV_PACK_REL_PREC * hi (s = 1 when every
 *               chart is a point); offsets (C,2) int32 = (x, y) of each box at s.  TT_ERR_UNSUPPORTED when no s > 0
 *               fits (too many charts for N).
 *   emit        one UV vertex per distinct (chart, vertex) pair of the face corners, numbered in order of the pair's
 *               first corner 3f + k.  In fp32: U = ((float)(x + pad) + 0.5f) + (u - umin) * s, V' = the same with y,
 *               v, vmin; v_tex = (U / N, V' / N), in [0, 1].  t_tex_idx (T,3) int32: row f is face f of t_pos_idx.
 *               tt_uv_emit_count leaves Vt in out_totals[0] (DEVICE); tt_uv_emit, with the same workspace, writes
 *               v_tex (Vt,2) and t_tex_idx.
 *   overlap     tt_uv_overlap: per texel centre of the N x N texture, the UV triangles that cover it under the
 *               rasterizer's rules above (clip (2u - 1, 2v - 1, 0, 1): coverage, canonical edges, tie rule), so a
 *               shared edge counts once; flags (T) uint8 = 1 for the faces that cover a texel counted twice;
 *               out_totals = (flagged faces, covered texels).  The caller (ops.uv_atlas) makes flagged faces singletons
 *               and redoes charts .. overlap; after TT_UV_MAX_OVERLAP_ROUNDS such rounds every face of a chart that
 *               still has a flagged face becomes a singleton.  A flagged face is never a singleton (singletons sit in
 *               disjoint boxes), so every round adds singletons and the loop ends.  Result: no texel centre lies in
 *               two UV triangles.
 *   fill        tt_tex_fill: out (H,W,C) fp32 = img where mask (H,W) uint8 != 0, bit for bit; elsewhere img at the
 *               nearest masked texel by jump flooding (steps 2^k .. 1, then 2, 1) of the keys (squared distance << 32
 *               | texel id), the smaller key wins; 0 when nothing is masked.  Nearest up to JFA's rare misses.
 * Determinism: labels, charts, UVs, flags and the fill use integer atomics and fixed-order gathers only: bit-identical
 * from launch to launch.  Counts are read back through out_totals; every entry point validates its arguments before
 * any HIP call (TT_ERR_BAD_ARG).  Use: bytes = tt_uv_workspace_bytes(V, T, N) (one workspace for every tt_uv_* call of
 * one mesh and texture size), tt_tex_fill_workspace_bytes(H, W). */
#define TT_UV_DEFAULT_ROUNDS 8
#define TT_UV_DEFAULT_TAU 0.3f
#define TT_UV_MAX_TAU 0.577f
#define TT_UV_MAX_SMOOTH_ROUNDS 1024
#define TT_UV_MAX_FACES ((1 << 24) - 1)
#define TT_UV_MAX_TEX 16384
#define TT_UV_MAX_PADDING 256
#define TT_UV_MAX_CHANNELS 64
#define TT_UV_MAX_OVERLAP_ROUNDS 4
#define TT_UV_PACK_REL_PREC 1e-4
int64_t tt_uv_workspace_bytes(int32_t V, int32_t T, int32_t N);
int tt_uv_labels(const float* v_pos, const int32_t* t_pos_idx, const int32_t* face_pairs, int32_t V, int32_t T,
                 int32_t P, int32_t rounds, float tau, int32_t N, void* workspace, int32_t* labels, void* stream);
int tt_uv_charts(const float* v_pos, const int32_t* t_pos_idx, const int32_t* face_pairs, const int32_t* labels,
                 const uint8_t* singleton, int32_t V, int32_t T, int32_t P, int32_t N, void* workspace, int32_t* chart,
                 float* chart_box, int32_t* out_totals, void* stream);
int tt_uv_pack(const float* chart_box, int32_t C, int32_t N, int32_t padding, int32_t* offsets, float* scale);
int tt_uv_emit_count(const int32_t* t_pos_idx, const int32_t* chart, int32_t V, int32_t T, int32_t N, void* workspace,
                     int32_t* out_totals, void* stream);
int tt_uv_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* labels, const int32_t* chart,
               const float* chart_box, const int32_t* offsets, int32_t C, float scale, int32_t V, int32_t T, int32_t N,
               int32_t padding, void* workspace, float* v_tex, int32_t* t_tex_idx, void* stream);
int tt_uv_overlap(const float* v_tex, const int32_t* t_tex_idx, int32_t Vt, int32_t V, int32_t T, int32_t N,
                  void* workspace, uint8_t* flags, int32_t* out_totals, void* stream);
int64_t tt_tex_fill_workspace_bytes(int32_t H, int32_t W);
int tt_tex_fill(const float* img, const uint8_t* mask, int32_t H, int32_t W, int32_t C, void* workspace, float* out,
                void* stream);

/* ---- conformal UV charts (tt_uv_lscm.hip; tt_uv_lscm_index in tt_uv.hip): least-squares conformal maps (Levy et al.
 * 2002, "Least squares conformal maps for automatic texture atlas generation") of the charts above ----
 * The opt-in second flattening of the atlas (ops.uv_atlas(method="lscm")): labels, charts, packing, the overlap guard
 * and the fill are the ones above; only the map of a chart's vertices into its box changes.  A chart is the set of
 * faces with one id in chart (T) int32; every solver number is fp64.
 *   unknowns    one UV vertex per distinct (chart, vertex) pair, tt_uv_emit's numbering: tt_uv_lscm_index writes
 *               t_tex_idx (T,3) from the workspace tt_uv_emit_count has just left (Vt = its out_totals[0]).
 *   tables      the solver works on the UV vertices in CHART ORDER: sorted by chart, then by UV-vertex id (a stable
 *               sort, the caller's), position i.  `tables` is ONE int32 array of tt_uv_lscm_table_ints(T, Vt, C, NT)
 *               ints: fc [3T] position of corner 3f + k | ccol [3T] the corners of every position, each row ascending
 *               | vmesh [Vt] mesh vertex of position i | vchart [Vt] its chart | vperm [Vt] its UV-vertex id | cptr
 *               [Vt+1] rows of ccol | vptr [C+1] positions of chart c | tptr [C+1] tiles of chart c | tchart [NT] chart
 *               of tile t | tbegin [NT] its first position.  A chart of n vertices has ceil(n / TT_UV_LSCM_TILE) tiles,
 *               in order.  Every entry is clamped into range before it is used as an index.
 *   energy      per face f with n = (p1 - p0) x (p2 - p0), |n|^2 as in "labels" above: local frame x along p1 - p0, y =
 *               n x x, so p0 = (0,0), p1 = (x1,0), p2 = (x2,y2), x1 = |p1 - p0|, x2 = (p2 - p0).(p1 - p0) / x1, y2 = |n|
 *               / x1 > 0, A_f = |n| / 2, all in double from the fp32 positions.  With W_k = (y_{k+1} - y_{k+2}, x_{k+2}
 *               - x_{k+1}), grad u = (1 / 2 A_f) sum_k u_k W_k, and E = sum_f A_f |grad v - J grad u|^2, J = rotation
 *               by +90 degrees in that frame: the minimiser keeps orientation.  A face with |n|^2 = 0 has no term.
 *   pins        p0 = the chart's UV vertex farthest from the middle 0.5 (min + max) of the chart's 3-D box, squared
 *               distance (dx^2 + dy^2) + dz^2 in double, no fused operations; on a tie the smallest UV-vertex id.  p1 =
 *               the one farthest from p0, same rule.  Pinned at (0, 0) and (|p1 - p0|, 0).  A chart whose vertices all
 *               coincide has no pins: it fails.
 *   solve       the normal equations M^T M x = -M^T M x_pin of E on the free entries, conjugate gradients with the
 *               Jacobi preconditioner, x_0 = 0, all charts in lock step with their own alpha, beta and residual
 *               (alpha = r.z / p.Ap, or 0 when p.Ap <= 0; beta likewise).  An entry whose diagonal is 0 (only zero-area
 *               faces use the vertex) stays 0.  After each iteration a chart with |r|^2 <= tol^2 |b|^2 is converged
 *               and changes no more; without an iteration nothing is converged.  tt_uv_lscm_iterate runs n_iters
 *               iterations (at most TT_UV_LSCM_MAX_BATCH) and leaves the number of charts still iterating in
 *               out_totals[0] (DEVICE): the caller reads it back every TT_UV_LSCM_CHECK_EVERY iterations, never per
 *               iteration.  M is applied matrix-free: a face pass writes the three corner terms, a vertex gather sums
 *               them in ascending corner order.  Per-chart sums: a wave per tile (4 positions per lane ascending, then
 *               a fixed shuffle tree), then a wave per chart over its tiles, the same way.  No float atomics.
 *   normalise   k = sqrt(sum A_f / sum UV area) over the chart's faces with A_f > 0; the chart fails unless both
 *               sums and k^2 are positive and finite.
 *   orient      theta = atan2(2 s_uv, s_uu - s_vv) / 2 from the sums of squares of the chart's UV vertices about their
 *               mean (atan2(0, 0) = 0: no rotation on a tie); final (u, v) = k R(-theta) (u, v), rounded to fp32.
 *               rotation = -theta, scale = k.  The chart's box is the min / max of the fp32 values.
 *   accept      a chart keeps its map iff it converged, did not fail above, and every face with A_f > 0 has UV area
 *               > 0 and k^2 UV area / A_f in [tau, 1 / tau] (double; tau the (double) of the float): the projection's
 *               own worst case.  Every other chart falls back: fallback = 1, box = its chart_box row of tt_uv_charts
 *               (zeros when chart_box is NULL), rotation 0, scale 1.
 *   emit        tt_uv_lscm_emit: tt_uv_emit's fp32 formula on (u, v) = the final coordinates, or, for a fallback chart,
 *               the projection of its label: with every chart fallen back, v_tex is bit-identical to tt_uv_emit's.
 *   outputs     tt_uv_lscm_finish: uv (Vt,2) fp64 the raw solution (before normalise / orient; the partial iterate of a
 *               chart that did not converge), uv_final (Vt,2) fp32 (0 for fallback charts), box_out (C,4), fallback (C)
 *               uint8, pins (C,2) int32 UV-vertex ids, iterations (C) int32, residual (C) |r| / |b| (0 when b = 0, 1
 *               before the first iteration), rotation, scale (C) fp64.
 * Determinism: integer atomics (boxes, pins, flags) and fixed-order sums only: bit-identical from launch to launch.
 * Use: tt_uv_emit_count; tt_uv_lscm_index; the caller's tables; tt_uv_lscm_setup; tt_uv_lscm_iterate until 0 charts
 * iterate or the caller's limit; tt_uv_lscm_finish; tt_uv_pack on box_out; tt_uv_lscm_emit.  One workspace of
 * tt_uv_lscm_workspace_bytes(T, Vt, C, NT) for setup .. finish.  C <= Vt, C <= NT <= Vt, Vt <= 3T. */
#define TT_UV_LSCM_TILE 256
#define TT_UV_LSCM_CHECK_EVERY 32
#define TT_UV_LSCM_MAX_BATCH 4096
#define TT_UV_LSCM_DEFAULT_TOL 1e-8
#define TT_UV_LSCM_DEFAULT_MAX_ITERS 20000
int64_t tt_uv_lscm_workspace_bytes(int32_t T, int32_t Vt, int32_t C, int32_t NT);
int64_t tt_uv_lscm_table_ints(int32_t T, int32_t Vt, int32_t C, int32_t NT);
int tt_uv_lscm_index(int32_t V, int32_t T, int32_t N, void* workspace, int32_t* t_tex_idx, void* stream);
int tt_uv_lscm_setup(const float* v_pos, const int32_t* tables, int32_t V, int32_t T, int32_t Vt, int32_t C, int32_t NT,
                     void* workspace, void* stream);
int tt_uv_lscm_iterate(const int32_t* tables, int32_t T, int32_t Vt, int32_t C, int32_t NT, int32_t n_iters, double tol,
                       void* workspace, int32_t* out_totals, void* stream);
int tt_uv_lscm_finish(const int32_t* tables, const float* chart_box, int32_t T, int32_t Vt, int32_t C, int32_t NT,
                      float tau, void* workspace, double* uv, float* uv_final, float* box_out, uint8_t* fallback,
                      int32_t* pins, int32_t* iterations, double* residual, double* rotation, double* scale,
                      void* stream);
int tt_uv_lscm_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* labels, const int32_t* chart,
                    const int32_t* t_tex_idx, const float* uv_final, const uint8_t* fallback, const float* chart_box,
                    const int32_t* offsets, int32_t C, float scale, int32_t V, int32_t T, int32_t Vt, int32_t N,
                    int32_t padding, float* v_tex, void* stream);

/* ---- mesh simplification (tt_simplify.hip): vertex clustering with quadric-error placement ----
 * Lindstrom 2000 ("Out-of-core simplification of large polygonal models") with the quadrics of Garland & Heckbert
 * 1997.  The reference has no such step; it makes the low-poly mesh the exporter's baked texture is meant for.  A mesh
 * is v_pos (V,3) fp32 and t_pos_idx (T,3) int32 with every index in [0, V) (the host checks it; a face with an index
 * outside takes part in nothing).  Inputs besides: grid G, TT_SIMPLIFY_MIN_GRID <= G <= TT_SIMPLIFY_MAX_GRID, and
 * lam >= 0 (the host's default is 1e-3).
 *   box         in fp32: lo_a = min over the vertices of v_a; ext = the largest of the three extents max v_a - lo_a;
 *               h = ext / (float)G; inv_h = (float)G / ext (two IEEE divisions).  ext == 0, V == 0 or T == 0: the host
 *               returns the mesh as it is and calls nothing here.
 *   cell        of EVERY vertex, referenced or not: c_a = min(G-1, max(0, floorf((v_a - lo_a) * inv_h))), the
 *               subtraction and the product each rounded to fp32 (tri_cell of csrc/tt_trigrid.h; it has no sum behind
 *               its product, so nothing contracts into an FMA and a float32 restatement gets bit-identical keys);
 *               key = (c_x G + c_y) G + c_z.
 *               tt_simplify_keys writes keys (V) int64.
 *   clusters    the distinct keys, ranked by ascending key; C of them.  The host sorts the keys (stable, so a cluster's
 *               vertices are in ascending vertex index); tt_simplify_ranks, from the sorted keys and the permutation,
 *               writes rank (V) int32 and leaves the cluster keys and member segments in the workspace; C goes to
 *               out_totals[0] (DEVICE memory, read back).  centre_a = lo_a + ((float)c_a + 0.5f) * h, product and sum
 *               each rounded to fp32.  C > TT_SIMPLIFY_MAX_CLUSTERS (three ranks must fit one 63-bit key) is
 *               TT_ERR_UNSUPPORTED in every entry point that takes C (the host raises ValueError before it calls one).
 *   quadric     corner k (k = 0, 1, 2) of face f contributes to the cluster r_k of that corner iff r_k differs from r_j
 *               for all j < k: a face counts once per distinct cluster it touches.  tt_simplify_pairs writes pair_keys
 *               (3T) int64 = r_k << 32 | 3f + k, INT64_MAX for a corner that does not contribute; the host sorts them.
 *               n = (p1 - p0) x (p2 - p0), l = |n|; l == 0 contributes nothing; else n^ = n / l, area = l / 2,
 *               d = -n^ . (p0 - centre); A += area n^ n^T, b += area d n^, w += area.  Everything relative to the cell
 *               centre, for fp32 conditioning.
 *   mean        m = mean of (v - centre) over the cluster's vertices.
 *   placement   x solves (A + lam w I) x = lam w m - b, symmetric positive definite whenever w > 0 and lam > 0;
 *               w == 0 (or a solve that is not finite: lam == 0 on a rank-deficient A): x = m.  Each component of x is
 *               clamped to [-h/2, h/2]; the cluster's vertex is centre + x.  tt_simplify_solve: sums in fp32, the 3x3
 *               Cholesky solve in double, cluster_pos (C,3) fp32.
 *   faces       r = rank[face].  A face with two equal corners is dropped; the rest are rotated so that the smallest
 *               rank comes first (orientation kept: (a,b,c) and (a,c,b) are different faces).  tt_simplify_faces writes
 *               face_keys (T) int64 = r0 << 42 | r1 << 21 | r2 of the rotated triple, INT64_MAX for a dropped face; the
 *               host sorts them (stable).  Among the faces with the same rotated triple the one with the smallest
 *               original index stays; survivors keep their original order and hold the rotated triple.
 *   output      the output vertices are the clusters a surviving face references, in ascending key order, renumbered
 *               densely.  tt_simplify_emit_count leaves (V', T') in out_totals (2 int32, DEVICE memory, read back);
 *               tt_simplify_emit, with the same workspace, writes v_out (V',3) fp32, t_out (T',3) int32 and
 *               vertex_map (V) int32 = the output vertex of each input vertex's cluster, -1 when that cluster is not
 *               kept.  Every write is bounded by those totals.  T' == 0: the host returns empty tensors.
 * Guarantees: every input vertex lies within sqrt(3) h of its cluster's vertex (both are in the same cell of side h).
 * Identical inputs give bit-identical outputs: no float atomics (the pair counts are integer atomics), and the sums
 * run in a fixed order -- a cluster's pairs in ascending (f, k) and its members in ascending vertex index are dealt
 * to the 64 lanes of one wave round-robin, each lane adds its share in ascending order, a fixed shuffle tree adds the
 * lanes.  NOT guaranteed: that the output is manifold (a cell that holds two sheets of the surface welds them), free
 * of self-intersections, or of the input's genus; faces may flip where the surface folds inside one cell.
 * Use: bytes = tt_simplify_workspace_bytes(V, T) (V, T >= 1; one workspace for every call of one run), in the order
 * keys, ranks, pairs, solve, faces, emit_count, emit.  Every entry point validates its arguments before any HIP call
 * (TT_ERR_BAD_ARG); V, T <= TT_MESH_MAX_ITEMS. */
#define TT_SIMPLIFY_MIN_GRID 2
#define TT_SIMPLIFY_MAX_GRID 1024
#define TT_SIMPLIFY_MAX_CLUSTERS 2097151
int64_t tt_simplify_workspace_bytes(int32_t V, int32_t T);
int tt_simplify_keys(const float* v_pos, int32_t V, int32_t grid, float lo_x, float lo_y, float lo_z, float inv_h,
                     int64_t* keys, void* stream);
int tt_simplify_ranks(const int64_t* sorted_keys, const int64_t* perm, int32_t V, int32_t T, int32_t grid,
                      void* workspace, int32_t* rank, int32_t* out_totals, void* stream);
int tt_simplify_pairs(const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T, int32_t C, void* workspace,
                      int64_t* pair_keys, void* stream);
int tt_simplify_solve(const float* v_pos, const int32_t* t_pos_idx, const int64_t* sorted_pair_keys,
                      const int64_t* perm, int32_t V, int32_t T, int32_t C, int32_t grid, float lo_x, float lo_y,
                      float lo_z, float h, double lam, void* workspace, float* cluster_pos, void* stream);
int tt_simplify_faces(const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T, int32_t C,
                      int64_t* face_keys, void* stream);
int tt_simplify_emit_count(const int64_t* sorted_face_keys, const int64_t* face_perm, const int32_t* t_pos_idx,
                           const int32_t* rank, int32_t V, int32_t T, int32_t C, void* workspace, int32_t* out_totals,
                           void* stream);
int tt_simplify_emit(const float* cluster_pos, const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T,
                     int32_t C, void* workspace, float* v_out, int32_t* t_out, int32_t* vertex_map, void* stream);

/* ---- mesh decimation (tt_decimate.hip): manifold-preserving, round-based parallel quadric edge collapse ----
 * Garland & Heckbert 1997 with the collapses of one round chosen so that their closed neighbourhoods are pairwise
 * disjoint: they can then be applied together and every validity check made for one of them still holds.  The
 * reference has no such step.  A mesh is v_pos (V,3) fp32 and t_pos_idx (T,3) int32 with every index in [0, V) (the
 * host checks it; every kernel skips an index outside).  target_faces >= 4.
 *   state       v_pos (V,3) fp32, the live faces tri (T,3) int32, one symmetric 4x4 quadric per vertex as 10 doubles
 *               (a00 a01 a02 a11 a12 a22 b0 b1 b2 c: error(x) = x^T A x + 2 b^T x + c), root (V) int32 = the current
 *               representative of every input vertex, remap (V) int32 = the identity between rounds.  Vertices are
 *               never renumbered during the rounds.
 *   quadrics    once, from the INPUT mesh, in fp64 (tt_decimate_quadrics, one thread per vertex): for the faces of the
 *               vertex in ascending face order (the vertex -> face CSR: vf_ptr (V+1), vf_col = face corners 3f + k
 *               ascending inside a row), n = (p1 - p0) x (p2 - p0), l = |n|; l == 0 contributes nothing; else
 *               n^ = n / l, area = l / 2, d = -n^ . p0; A += area n^ n^T, b += area d n^, c += area d d.
 *   topology    of a round (host): the unique edges (a, b), a <= b, in lexicographic order with the number of face
 *               edges that use each (edges (E,2), counts (E) int32), the vertex -> neighbour CSR with ascending rows
 *               (nbr_ptr (V+1), nbr_col (2E)) and the vertex -> face CSR of the live faces.
 *   locking     tt_decimate_lock, one thread per edge: locked (V) uint8 = 1 for both endpoints of an edge with
 *               counts != 2 (boundary, non-manifold) or a == b, else 0.  A locked vertex never moves or merges.
 *   cost        tt_decimate_edges, one thread per edge, Qe = Qa + Qb, fp64: det and the cofactors of A;
 *               |det| > 1e-9 (trace A / 3)^3: x = -A^-1 b; else x = the cheapest of v_a, v_b, (v_a + v_b) / 2, ties in
 *               that order.  cost = max(error(x), 0) at the fp64 x, rounded to fp32; x is rounded to fp32.
 *   validity    neither endpoint locked, a != b; deg a + deg b - 4 >= 3 (deg = row length of the neighbour CSR);
 *               |N(a) n N(b)| == 2 by a merge of the two rows (the link condition) and both common neighbours have
 *               deg >= 4; every face of star(a) u star(b) that does not hold both endpoints, with its corner a or b
 *               moved to the fp32 x, has n_new != 0 and n_old . n_new > 0.2 |n_old| |n_new| (fp64).
 *               cost_bits (E) = the bit pattern of the fp32 cost (unsigned order = cost order), 0xffffffff for an
 *               invalid edge; xopt (E,3) fp32, zero for an invalid edge.
 *   threshold   (host, on the device) tau = the cost_bits at rank floor(TT_DECIMATE_QUANTILE n_valid) of the valid
 *               edges' ascending cost_bits, as one int64 in DEVICE memory; the candidates are the valid edges with
 *               cost_bits <= tau.
 *   priorities  key = (uint64) hash32(a, b, round) << 32 | edge index, with (all uint32, wrapping)
 *                   h = (a * 0x9E3779B1) ^ ((b + 0x7F4A7C15) * 0x85EBCA77) ^ ((round + 1) * 0xC2B2AE3D);
 *                   h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16.
 *   selection   TT_DECIMATE_SELECT_PASSES passes of tt_decimate_mark, tt_decimate_select over state (E) uint8 (0 no
 *               candidate, 1 candidate, 2 selected, 3 blocked), taken (V) uint8 (host: zero before pass 0) and owner
 *               (V) uint64 (host: all ones before every pass).  The closed neighbourhood of an edge is {a, b} u N(a)
 *               u N(b).  mark: pass 0 writes every state from cost_bits and tau; a candidate whose neighbourhood
 *               holds a taken vertex becomes blocked; every other candidate does a 64-bit atomicMin of its key into
 *               owner[w] for every w of its neighbourhood.  select: a candidate that owns every such w becomes selected
 *               and sets taken[w] for all of them.  Selected edges have pairwise disjoint closed neighbourhoods; the
 *               candidate with the smallest key is always selected in pass 0.
 *   budget      (host) need = ceil((T - target_faces) / 2); of more than `need` selected edges the `need` smallest by
 *               (cost_bits, edge index) are kept, listed in ascending edge index.
 *   apply       tt_decimate_apply for the K kept edges: v_pos[a] = xopt, Q[a] += Q[b], remap[b] = a; every face is
 *               remapped, one with two equal corners is dropped, the survivors are written to t_out (room for T rows)
 *               in their order (the two-counter compaction of tt_compact.h); root[v] = remap[root[v]]; remap returns
 *               to the identity.  out_totals[1] (2 int32, DEVICE memory, read back) = the number of faces written.
 *   rounds      stop when T <= target_faces, when a round has no valid edge (stalled), or after max_rounds.
 *   output      tt_decimate_emit_count leaves (V', 0) in out_totals; tt_decimate_emit, with the same workspace and T,
 *               writes the vertices a live face references in index order (v_out (V',3)), the faces renumbered (t_out
 *               (T,3)) and vertex_map (V) int32 = the output vertex of each input vertex's root, -1 for a vertex no
 *               face referenced.
 * Guarantees: identical inputs give bit-identical outputs (no float atomics, fixed summation orders, the one atomic is
 * an integer min).  A closed 2-manifold input gives a closed 2-manifold with the same Euler characteristic and number
 * of components; no collapse flips a face past the 0.2 bound; locked vertices keep their position bit for bit and are
 * all present; a closed manifold input that does not stall ends with target_faces - 1 <= T' <= target_faces.  NOT
 * guaranteed: freedom from self-intersection between parts of the surface that are far apart on the mesh, and any
 * particular accuracy.
 * Use: bytes = tt_decimate_workspace_bytes(V, T) for the INPUT sizes (one workspace for every call of one run, T only
 * falls); quadrics once; per round lock, edges, (mark, select) per pass, apply; at the end emit_count, emit.  Every
 * entry point validates its arguments before any HIP call (TT_ERR_BAD_ARG); V, T <= TT_MESH_MAX_ITEMS, 1 <= E <= 3 T,
 * 1 <= K <= T. */
#define TT_DECIMATE_QUANTILE 0.25f
#define TT_DECIMATE_SELECT_PASSES 2
#define TT_DECIMATE_MIN_FACES 4
#define TT_DECIMATE_DEFAULT_ROUNDS 1024
int64_t tt_decimate_workspace_bytes(int32_t V, int32_t T);
int tt_decimate_quadrics(const float* v_pos, const int32_t* t_pos_idx, const int32_t* vf_ptr, const int32_t* vf_col,
                         int32_t V, int32_t T, double* quadrics, void* stream);
int tt_decimate_lock(const int32_t* edges, const int32_t* counts, int32_t V, int32_t E, uint8_t* locked, void* stream);
int tt_decimate_edges(const float* v_pos, const double* quadrics, const int32_t* t_pos_idx, const int32_t* edges,
                      const int32_t* nbr_ptr, const int32_t* nbr_col, const int32_t* vf_ptr, const int32_t* vf_col,
                      const uint8_t* locked, int32_t V, int32_t T, int32_t E, int32_t* cost_bits, float* xopt,
                      void* stream);
int tt_decimate_mark(const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr_col, const int32_t* cost_bits,
                     const int64_t* tau, int32_t V, int32_t T, int32_t E, int32_t round, int32_t pass, uint8_t* state,
                     const uint8_t* taken, int64_t* owner, void* stream);
int tt_decimate_select(const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V, int32_t T,
                       int32_t E, int32_t round, uint8_t* state, uint8_t* taken, const int64_t* owner, void* stream);
int tt_decimate_apply(const int32_t* kept_edges, const float* kept_xopt, const int32_t* t_pos_idx, int32_t V, int32_t T,
                      int32_t K, void* workspace, float* v_pos, double* quadrics, int32_t* remap, int32_t* root,
                      int32_t* t_out, int32_t* out_totals, void* stream);
int tt_decimate_emit_count(const int32_t* t_pos_idx, int32_t V, int32_t T, void* workspace, int32_t* out_totals,
                           void* stream);
int tt_decimate_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* root, int32_t V, int32_t T,
                     void* workspace, float* v_out, int32_t* t_out, int32_t* vertex_map, void* stream);

/* ---- isotropic remeshing (tt_remesh.hip): split, collapse, flip, relax (Botsch & Kobbelt 2004) ----
 * Brings the edges of a mesh towards one length L and its vertices towards valence 6 on the surface of the INPUT mesh.
 * The reference has no such step.  A mesh is v_pos (V,3) fp32 and t_pos_idx (T,3) int32 with every index in [0, V)
 * (the host checks it; every kernel skips an index outside).  edge_length L > 0, iterations >= 0.
 *   thresholds  h = (float)((4.0 / 3.0) * L), l = (float)(0.8 * L) (the products in double, L a double), hi2 = h * h,
 *               lo2 = l * l in fp32 (host).  len2(p, q) = (dx dx + dy dy) + dz dz with d = q - p, every operation
 *               rounded to fp32, no fused multiply-add; the midpoint of p, q is 0.5f * (p + q) per component in fp32.
 *               Every length comparison below is len2 against hi2 or lo2.
 *   topology    of a pass or round (host), as decimation's: the unique edges (a, b), a <= b, lexicographic, with their
 *               counts, the two CSR tables with ascending rows, locked (tt_decimate_lock; recomputed every round);
 *               for the split face_edge (3T) int32 = the unique edge of face edge 3f + k (corners k, (k+1) % 3); for
 *               the flip edge_fe (E,2) int32 = the two face edges 3f + k of an edge with counts == 2 in ascending
 *               order, -1 -1 for any other edge.
 *   iteration   split, collapse, flip, move; after the last iteration one more split.
 *   split       passes until no edge has len2 > hi2, at most TT_REMESH_MAX_SPLIT_PASSES (then split_capped).  A pass
 *               marks every edge with a != b and len2 > hi2, boundary and non-manifold ones included; marked edge e
 *               gets vertex V + rank(e), rank among the marked edges in ascending edge order, at the midpoint.
 *               tt_remesh_split_count leaves (marked edges, child faces) in out_totals (read back; the host refuses
 *               a result beyond TT_MESH_MAX_ITEMS before it emits); tt_remesh_split_emit writes the midpoints to
 *               v_new (M,3) (the host appends them to v_pos), the marked edges to marked (M,2) and the children to
 *               t_out (Tn,3) in parent order, then template order.  With m_k the midpoint vertex of edge k of face
 *               (c0, c1, c2):
 *                 none marked   (c0, c1, c2)
 *                 edge k only   a = c_k, b = c_k+1, c = c_k+2:  (a, m_k, c), (m_k, b, c)
 *                 all but k     a, b, c as above, mb = m_k+1, mc = m_k+2:  (mb, c, mc), then the quad a, b, mb, mc cut
 *                               by the diagonal a-mb if len2(a, mb) < len2(b, mc), or if they are equal and a < b:
 *                               (a, b, mb), (a, mb, mc); else by b-mc: (a, b, mc), (b, mb, mc)
 *                 all three     (c0, m0, m2), (c1, m1, m0), (c2, m2, m1), (m0, m1, m2)
 *               Orientation is kept, the templates of two faces agree on their shared edge by construction (no
 *               selection), no existing vertex moves: surface and topology are kept exactly.
 *   collapse    rounds until a round has no candidate, at most TT_REMESH_MAX_ROUNDS (then rounds_capped).
 *               tt_remesh_collapse_candidates, one thread per edge: neither endpoint locked (so the edge has two
 *               faces); len2(a, b) < lo2; decimation's link condition (deg a + deg b - 4 >= 3, exactly two common
 *               neighbours, both of deg >= 4); with x = the midpoint, len2(w, x) <= hi2 for every w of N(a) u N(b)
 *               other than a, b; decimation's flip test of star(a) u star(b) at x.  cost_bits = 0 for a candidate,
 *               0xffffffff else; xopt = x.  Selection is one pass of tt_decimate_mark (tau = 0: every candidate is
 *               eligible) and tt_decimate_select with the keys hash32(a, b, round) << 32 | edge index; every selected
 *               edge is applied by tt_decimate_apply (b -> a at x; the quadrics it sums are not read).
 *   flip        rounds as for collapse.  Edge (a, b), a < b, with the face that runs a -> b, (a, b, c), and the face
 *               that runs b -> a, (b, a, d), becomes edge (c, d): the first face becomes (a, d, c), the second
 *               (d, b, c).  tt_remesh_flip_select, one thread per edge.  Candidate: counts == 2 with the two faces in
 *               opposite directions; a, b unlocked; c != d and d not in N(c); with val = deg and target = 6 (4 for a
 *               locked vertex), the sum of |val - target| over a, b, c, d strictly falls for val a, val b - 1 and
 *               val c, val d + 1; len2(c, d) <= hi2; each of (d - a) x (c - a), (b - d) x (c - d) has a positive dot
 *               product with each of (b - a) x (c - a), (a - b) x (d - b) (fp64).  state (E) uint8: 0 no candidate, 1
 *               candidate, 2 selected; cd (E,2) = (c, d), faces (E,2) = the two faces.  A candidate does a 64-bit
 *               atomicMin of its key into owner[] of a, b, c, d (owner (V) uint64, set to all ones by the call) and is
 *               selected iff it owns the four: selected flips share no vertex, so they share no face, cannot create
 *               one edge twice and leave each other's checks valid.  tt_remesh_flip_apply rewrites the two faces of
 *               every selected edge in place.
 *   move        one Jacobi step.  tt_remesh_relax, one thread per vertex: movable = not locked, in a face and with a
 *               neighbour; q = p + (g - p) - ((g - p) . n) n in fp64, rounded to fp32, with g the mean of the
 *               neighbours (ascending) and n the normalised sum of (p1 - p0) x (p2 - p0) over its faces in ascending
 *               face order (zero when the sum is); q = p for any other vertex.  q is sent to the closest point of the
 *               INPUT mesh (tt_dist_query on a grid of the input built once per call); tt_remesh_place puts a movable
 *               vertex at (b0 s0 + b1 s1) + b2 s2 of that face's corners in fp32 and leaves every other one.  The fold
 *               guard: tt_remesh_fold_flag is one Jacobi step over the faces (positions: old where rev_in is set,
 *               else new): a face whose old normal is not zero and whose new normal has a non-positive dot product
 *               with it (fp64) sets rev_out of its three corners and adds one to count; rev_out starts as a copy of
 *               rev_in.  The host repeats with the two arrays swapped until count == 0 (the reverted set only grows,
 *               and with every vertex reverted no face fails); tt_remesh_revert puts the old position back.
 *   output      tt_decimate_emit_count / tt_decimate_emit: the referenced vertices in ascending index, the faces in
 *               order.  One more tt_dist_query gives every output vertex its closest input face and barycentrics.
 * Guarantees: identical inputs give bit-identical outputs (no float atomics; the atomics are the integer min of the
 * selections, the integer add of the guard's count and flag stores).  A closed 2-manifold input stays one with the same
 * Euler characteristic and number of components; no operation flips a face; locked vertices of the input keep their
 * position bit for bit; unless split_capped, no edge of the result has len2 > hi2; every vertex the last move left
 * unreverted lies on the input surface (to the fp32 evaluation of its barycentrics).  NOT guaranteed: a lower bound on
 * edge length (blocked collapses remain; the share of short edges is what tools report), sharp features, vertices of
 * the closing split on the surface (they lie on chords), differentiability.
 * TT_REMESH_MAX_ROUNDS / _SPLIT_PASSES bound a phase; every phase measured so far ended by exhaustion.  Measured maxima
 * (profiles/mesh_remesh.json, the two 160^3 scenes, 84 k and 473 k faces): 151 collapse rounds (L = 4.6 x the mean edge;
 * 47 at 1.9 x, 31 at 1.0 x), 10 flip rounds, 1 split pass; the numpy restatement on the meshes of
 * tests/test_remesh_reference.py (1 000 to 3 000 faces): 25 rounds, 2 passes.  The rounds grow with L / mean edge.
 * Use: per pass bytes = tt_remesh_workspace_bytes(T, E).  Every entry point validates its arguments before any HIP call
 * (TT_ERR_BAD_ARG); V, T <= TT_MESH_MAX_ITEMS, 1 <= E <= 3 T, 1 <= M <= E, T <= Tn <= 4 T. */
#define TT_REMESH_MAX_ROUNDS 1024
#define TT_REMESH_MAX_SPLIT_PASSES 32
#define TT_REMESH_DEFAULT_ITERATIONS 5
int64_t tt_remesh_workspace_bytes(int32_t T, int32_t E);
int tt_remesh_split_count(const float* v_pos, const int32_t* edges, const int32_t* face_edge, int32_t V, int32_t T,
                          int32_t E, float hi2, void* workspace, int32_t* out_totals, void* stream);
int tt_remesh_split_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges, const int32_t* face_edge,
                         int32_t V, int32_t T, int32_t E, int32_t M, int32_t Tn, void* workspace, float* v_new,
                         int32_t* marked, int32_t* t_out, void* stream);
int tt_remesh_collapse_candidates(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges,
                                  const int32_t* nbr_ptr, const int32_t* nbr_col, const int32_t* vf_ptr,
                                  const int32_t* vf_col, const uint8_t* locked, int32_t V, int32_t T, int32_t E,
                                  float hi2, float lo2, int32_t* cost_bits, float* xopt, void* stream);
int tt_remesh_flip_select(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges, const int32_t* edge_fe,
                          const int32_t* nbr_ptr, const int32_t* nbr_col, const uint8_t* locked, int32_t V, int32_t T,
                          int32_t E, float hi2, int32_t round, uint8_t* state, int32_t* cd, int32_t* faces,
                          int64_t* owner, void* stream);
int tt_remesh_flip_apply(const int32_t* edges, const int32_t* cd, const int32_t* faces, const uint8_t* state, int32_t V,
                         int32_t T, int32_t E, int32_t* t_pos_idx, void* stream);
int tt_remesh_relax(const float* v_pos, const int32_t* t_pos_idx, const int32_t* nbr_ptr, const int32_t* nbr_col,
                    const int32_t* vf_ptr, const int32_t* vf_col, const uint8_t* locked, int32_t V, int32_t T, int32_t E,
                    float* q, uint8_t* movable, void* stream);
int tt_remesh_place(const float* v_old, const int32_t* face, const float* bary, const float* src_pos,
                    const int32_t* src_tri, const uint8_t* movable, int32_t V, int32_t V0, int32_t T0, float* v_new,
                    void* stream);
int tt_remesh_fold_flag(const float* v_old, const float* v_new, const int32_t* t_pos_idx, const uint8_t* rev_in,
                        int32_t V, int32_t T, uint8_t* rev_out, int32_t* count, void* stream);
int tt_remesh_revert(const float* v_old, const uint8_t* rev, int32_t V, float* v_new, void* stream);

/* ---- tangents and normal-map baking (tt_bake.hip): Mesh.v_tng (threestudio/models/mesh.py:162-205) and the
 * exporter's map_Bump ----
 * A mesh is v_pos (V,3) fp32, t_pos_idx (T,3) int32, its UVs v_tex (Vt,2) fp32, t_tex_idx (T,3) int32 (row f is face f)
 * and its unit vertex normals v_nrm (V,3).  Corner 3f + k is corner k of face f.  In this file nothing contracts into a
 * fused multiply-add: every product, quotient and sum is rounded to fp32 on its own, in the order written, and a dot
 * product is (a_x b_x + a_y b_y) + a_z b_z.
 *   face tangent  pe_j = p_j - p_0, uve_j = uv_j - uv_0 (j = 1, 2); denom = uve1.x uve2.y - uve1.y uve2.x;
 *               d = denom > 0 ? max(denom, 1e-6) : min(denom, -1e-6) (the reference's sign test; denom = 0 and NaN
 *               take the negative branch); tang_f = (pe1 uve2.y - pe2 uve1.y) / d, per component.
 *   groups      tt_bake_tangents writes one tangent per group: TT_BAKE_GROUP_POS, the V position vertices (a corner
 *               belongs to t_pos_idx[f,k]; the reference's v_tng), or TT_BAKE_GROUP_TEX, the Vt UV vertices (a corner
 *               belongs to t_tex_idx[f,k]; tangents that split at chart seams).  The host passes the group -> corner CSR:
 *               group_ptr (G+1) int32 and group_corner (3T) int32, the corner ids ordered by (group, corner id) -- one
 *               stable sort of the flattened index array.  A corner whose face has an index outside [0, V) / [0, Vt)
 *               contributes nothing.
 *   normal      n of a POS group = v_nrm of that vertex.  n of a TEX group = v_nrm of the position vertex of the group's
 *               smallest contributing corner id ((0,0,1) for a group without one).
 *   tangent     s = the sum of tang_f over the group's contributing corners in ascending corner id (a face adds its
 *               tangent once per corner it has in the group); t = s / sqrt(s.s); r = t - (t.n) n; out = r / sqrt(r.r).
 *               (The reference divides s by the corner count first, which normalising undoes.)
 *   degenerate  a group with no contributing corner, with s.s <= 1e-20 or not finite, or with r.r <= 1e-12 or not finite
 *               (a tangent parallel to the normal) gets perp(n) instead, where the reference yields NaN:
 *               perp(n) = q / sqrt(q.q), q = e_a - n_a n, a = the first of x, y, z with the smallest |n_a| (q.q >= 2/3
 *               for a unit n); (1,0,0) if q.q <= 0.25 or is not finite (n not a unit vector).
 *   project     tt_bake_project, one step of pulling points (M,3) (in place) onto the iso-surface given the field's
 *               sdf (M) and sdf_grad (M,3) there: gg = g.g; a = min(max(sdf / max(gg, 1e-12), -1), 1);
 *               len = |a| sqrt(gg); c = len > max_step ? a (max_step / len) : a; p_k -= c g_k.  So a step is the Newton
 *               step -sdf g / |g|^2, its factor clamped to [-1, 1] and its length limited to max_step (>= 0, finite).
 *               A point whose sdf or gradient (|sdf| + g.g) is not finite stays; so does point i when mask (M) uint8,
 *               which may be NULL, has mask[i] = 0 (an uncovered texel).
 *   encode      tt_bake_encode, per texel p of rast (H,W,4) = (u, v, z/w, face + 1) of the UV-space rasterisation
 *               (the rasterizer's layout above): a texel whose id is not in [1, T], or whose face has an index outside
 *               its range, is uncovered and gets (0.5, 0.5, 1).  Else, with interpolate's weights, x = (u x_0 + v x_1) +
 *               (1 - u - v) x_2: n from v_nrm through t_pos_idx, t from tng_tex (Vt,3) through t_tex_idx;
 *               n^ = unit(n) ((0,0,1) where n.n <= 1e-20); t^ = unit(t - (t.n^) n^) (perp(n^) where that is <= 1e-20);
 *               b^ = t^ x n^; m^ = unit(field_nrm[p]) (n^ where it is <= 1e-20 or not finite: a flat texel);
 *               out[p] = 0.5 + 0.5 (m^.t^, m^.b^, m^.n^).  b^ = t^ x n^ is the direction of increasing OBJ v (green
 *               up, the OpenGL convention): the atlas gives every UV triangle positive area in (u, v), so dP/dv is
 *               parallel to n^ x t^, and the OBJ writer flips v.  out_counts (2 int32, DEVICE memory) = (covered texels,
 *               covered texels with m^.n^ <= 0: the field normal points into the face; stored as computed).
 * Determinism: gathers in a fixed order and integer atomics only; identical inputs give bit-identical outputs.  No
 * workspace, no host round trip.  Every entry point validates its arguments before any HIP call (TT_ERR_BAD_ARG); G, M
 * or H W = 0 does nothing (tt_bake_encode still zeroes out_counts). */
#define TT_BAKE_GROUP_POS 0
#define TT_BAKE_GROUP_TEX 1
#define TT_BAKE_MAX_POINTS 268435456
int tt_bake_tangents(const float* v_pos, const int32_t* t_pos_idx, const float* v_tex, const int32_t* t_tex_idx,
                     const float* v_nrm, const int32_t* group_ptr, const int32_t* group_corner, int32_t V, int32_t Vt,
                     int32_t T, int32_t group, float* out, void* stream);
int tt_bake_project(float* points, const float* sdf, const float* sdf_grad, const uint8_t* mask, int64_t M,
                    float max_step, void* stream);
int tt_bake_encode(const float* rast, const float* v_nrm, const int32_t* t_pos_idx, const float* tng_tex,
                   const int32_t* t_tex_idx, const float* field_nrm, int32_t V, int32_t Vt, int32_t T, int32_t H,
                   int32_t W, float* out, int32_t* out_counts, void* stream);

/* ---- point-to-mesh distance (tt_dist.hip): closest point on a triangle mesh, its backward, a surface sampler ----
 * The geometric query the export chain measures itself with (Mesh.distance_to, Mesh.simplify(max_error=)) and a
 * point-to-surface loss stands on.  The reference has no such step.  A mesh is v_pos (V,3) fp32 and t_pos_idx (T,3)
 * int32, T >= 1, every index in [0, V) and every coordinate finite (the host checks both); query points are (N,3) fp32.
 *   pair        the closest point on triangle f = (a, b, c) to p, in fp32, by ONE device function (dist_closest) with
 *               one call site: Voronoi regions (Ericson, Real-Time Collision Detection 5.1.5).  The vertex regions
 *               come from the six projections d1..d6 of p - a, p - b, p - c on ab and ac; the edge and face regions
 *               from the signed areas taken as n . (ab x ap), n . (ap x ac), n . (bc x bp) with n = ab x ac (the
 *               book's differences of products of d1..d6 cancel to noise once |p - a| is a few hundred edge lengths).
 *               Edge parameters are t = clamp(num / den, 0, 1), 0 where den <= 0.  A triangle with
 *               n.n <= 1e-12 (ab.ab) (ac.ac) -- zero area, equal vertices, collinear -- is the union of its three edge
 *               segments: the nearest of ab, ac, bc, in that order at equal distance.  Never NaN for finite input.
 *               Yields v, w (barycentrics b = (max(1 - v - w, 0), v, w), each >= 0, sum 1 to rounding), the point
 *               c = a + v ab + w ac and d2 = |p - c|^2.
 *   answer      per point the lexicographic minimum of (d2, f) over ALL T triangles: equal distance goes to the smaller
 *               face index.  d2 (N) fp32, face (N) int32, bary (N,3) fp32.  It does not depend on the grid, on the order
 *               of triangles inside a cell, on the order of the points or on the launch, bit for bit.  A point with a
 *               coordinate that is not finite gives d2 = NaN, face = -1, bary = 0 and leaves the kernel before the
 *               search.
 *   grid        G^3 cells over the mesh's bounding cube, 1 <= G <= TT_DIST_MAX_GRID: lo_a = min v_a, ext = the largest
 *               of the three extents, h = ext / (float)G, inv_h = (float)G / ext (ext == 0: h = inv_h = 0, everything
 *               is in cell 0).  cell(x) = min(G-1, max(0, floorf((x - lo_a) * inv_h))), difference and product each
 *               rounded to fp32, the clamp taken before the conversion to int: ONE device function, tri_cell of
 *               csrc/tt_trigrid.h, which every stage below shares along with the cube, the record and the view of
 *               the tables; key = (c_x G + c_y) G + c_z, so consecutive cells along z are consecutive rows.
 *               tt_dist_build_count packs every triangle into a 48-byte record (three float4: a, b, c, w unused),
 *               counts per cell the triangles whose axis-aligned box overlaps it (cells of the box's two corners,
 *               integer atomics) and scans (tt_scan.h): cell_ptr (G^3 + 1) int32; M = the number of (cell, triangle)
 *               pairs goes to out_total (int64, DEVICE memory, read back: the one host round trip of the build).  M and
 *               G^3 + 1 must not exceed TT_MESH_MAX_ITEMS (the host raises ValueError before the fill).
 *               tt_dist_build_fill writes cell_tri (M) int32; the order inside a row is arrival order and means
 *               nothing.  G = 1 is brute force and runs the same code.  A triangle is binned by its box, so one that
 *               spans the cube is a member of every cell.
 *   default G   clamp(ceil(sqrt(T) / 8), 1, 256), the host's rule when the caller names no grid.  A surface occupies
 *               about G^2 cells; the first rule, sqrt(T) / 2 (a few triangles per occupied cell, M / T = 8), lost to
 *               coarser grids on the GPU: at T = 84 k a query of 100 k points near the surface took 11.0 / 5.2 / 4.0 ms at
 *               sqrt(T) / 2, / 4, / 8 and one of 100 k points uniform in the box 786 / 265 / 157 ms -- a thread walks its
 *               empty cells one dependent load at a time, so empty rings cost more than spare triangles
 *               (profiles/mesh_distance.json).  A point far from the surface in units of h visits O((d / h)^3) cells:
 *               the grid suits points near the surface; far ones want a coarser grid.
 *   search      one thread per point.  q = p clamped to the cube [lo, lo + ext]^3, c0 = cell(q).  Rings r = 0, 1, 2, ...
 *               of cells at Chebyshev distance r from c0, clipped to the grid; a triangle met in several cells is
 *               evaluated again.  After ring r every triangle not yet seen lies inside the cube and outside the block of
 *               rings <= r, hence (projection onto the convex cube) at squared distance >= |p - q|^2 + (r h)^2.  The
 *               search stops when the best d2 is STRICTLY below (1 - 2^-16) |p - q|^2 + (max(r - 1/64, 0) h)^2: equality
 *               goes on, or a smaller face index at equal distance would be lost; the two factors keep the bound
 *               conservative under the fp32 rounding of the cell assignment of points and boxes (h >= ext / 256 is far
 *               above an ulp of ext) and of d2 itself for a far point.  It ends at the latest when the block covers the
 *               grid.  Every loop is bounded by G or a CSR row clamped to [0, M]; no spin wait, no dependence between
 *               workgroups.  tt_dist_keys writes key(c0) (N) int64 (-1 for a point that is not finite): the host may
 *               sort it (stable) and pass the permutation as `order` (N) int64 -- thread t then serves point order[t]
 *               and writes row order[t]; order = NULL serves point t.
 *   backward    tt_dist_bwd, the face and its barycentrics fixed (envelope theorem): with c = sum b_k v_k,
 *               grad_points[i] = 2 g_i (p - c) is written, grad_v_pos[t_pos_idx[face, k]] += -2 g_i b_k (p - c) by float
 *               atomicAdd (the caller zeroes grad_v_pos; the sum's last bits depend on arrival order).  Either output
 *               may be NULL.  A row with face outside [0, T) writes zeros and adds nothing.
 *   sampler     a deterministic sample set with every point of the surface within `spacing` of a sample: face f with
 *               fp32 longest edge L_f (squares, sums and the root each rounded to fp32) gets k_f = max(1,
 *               ceil(L_f / spacing)) and the samples a + (i/k)(b - a) + (j/k)(c - a), i, j >= 0, i + j <= k:
 *               (k+1)(k+2)/2 of them, ordered face-major, then i, then j (a sub-triangle has edges <= spacing).
 *               tt_dist_sample_count writes offsets (T+1) int64, the exclusive scan of the counts with the total S at
 *               [T] (DEVICE memory, read back once; a face's k is capped at 2^17, whose count alone exceeds the limit);
 *               S > TT_DIST_MAX_SAMPLES is the host's ValueError before anything is allocated.  tt_dist_sample_emit,
 *               one thread per sample: points (S,3) fp32, face (S) int32.  Shared edges and vertices are sampled more
 *               than once.
 * Use: ws = tt_dist_workspace_bytes(G); build_count, read M, build_fill with the same workspace; then any number of
 * tt_dist_query / tt_dist_bwd.  tt_dist_sample_workspace_bytes(T) sizes the sampler's scan scratch.  Every entry point
 * validates its arguments before any HIP call (TT_ERR_BAD_ARG); N = 0 does nothing; N, V, T, M <= TT_MESH_MAX_ITEMS.
 * Out of scope: a BVH, area weighting.  The sign of the distance comes from "winding number" below, rays from "ray
 * casting". */
#define TT_DIST_MAX_GRID 256
#define TT_DIST_MAX_SAMPLES (1 << 26)
int64_t tt_dist_workspace_bytes(int32_t grid);
int tt_dist_build_count(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, int32_t grid, float lo_x,
                        float lo_y, float lo_z, float ext, float inv_h, void* workspace, float* records,
                        int32_t* cell_ptr, int64_t* out_total, void* stream);
int tt_dist_build_fill(const float* records, int32_t T, int32_t grid, float lo_x, float lo_y, float lo_z, float ext,
                       float inv_h, void* workspace, const int32_t* cell_ptr, int32_t M, int32_t* cell_tri,
                       void* stream);
int tt_dist_keys(const float* points, int32_t N, int32_t grid, float lo_x, float lo_y, float lo_z, float ext,
                 float inv_h, int64_t* keys, void* stream);
int tt_dist_query(const float* points, const int64_t* order, int32_t N, const float* records, const int32_t* cell_ptr,
                  const int32_t* cell_tri, int32_t T, int32_t M, int32_t grid, float lo_x, float lo_y, float lo_z,
                  float ext, float h, float inv_h, float* d2, int32_t* face, float* bary, void* stream);
int tt_dist_bwd(const float* points, const float* v_pos, const int32_t* t_pos_idx, const int32_t* face,
                const float* bary, const float* g_d2, int32_t N, int32_t V, int32_t T, float* grad_points,
                float* grad_v_pos, void* stream);
int64_t tt_dist_sample_workspace_bytes(int32_t T);
int tt_dist_sample_count(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, float spacing,
                         void* workspace, int64_t* offsets, void* stream);
int tt_dist_sample_emit(const float* v_pos, const int32_t* t_pos_idx, const int64_t* offsets, int32_t V, int32_t T,
                        float spacing, int32_t S, float* points, int32_t* face, void* stream);

/* ---- winding number (tt_wind.hip): generalized winding number of a triangle mesh, exact and by a dipole tree ----
 * The inside test the distance above lacks (ops.mesh_winding_number, mesh_contains, mesh_signed_distance; shape.MeshOBJ
 * and ShapeLoss, the reference's libigl-based threestudio/utils/ops.py:482-584).  A mesh is v_pos (V,3) fp32 and
 * t_pos_idx (T,3) int32 as for the distance; query points are (N,3) fp32; the answer is w (N) fp32.
 *   pair        the signed solid angle of triangle (a, b, c) seen from p (Van Oosterom-Strackee), in fp32, by ONE device
 *               function (wind_pair) with one call site per query kernel.  With A = a - p, B = b - p, C = c - p:
 *               num = A . (B x C), den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|, Omega = 2 atan2(num, den); the atan2
 *               is the file's own (wind_atan2, about 2 ulp, every select on a single compare: tt_mask.h).
 *               num == 0 (either sign) contributes exactly 0: a triangle without area, a point in the triangle's plane;
 *               the sign of a zero never picks +-pi.  Never NaN for finite input (coordinate differences beyond 2^40
 *               overflow the products; such a pair counts 0).
 *   w           w(p) = sum_f Omega_f / 4 pi: 1 inside and 0 outside an outward-oriented closed surface (the orientation
 *               of the marching-cubes, marching-tetrahedra and simplify outputs), fractional near an open one.
 *   exact       tt_wind_exact: per point the sum over ALL T faces in ascending face order; the pairs fp32, the running
 *               sum a double, converted to fp32 after the division by 4 pi.  Bit for bit independent of the launch and
 *               of the order of the points.  One thread per point; the block stages tiles of TT_ITEM_BLOCK 48-byte
 *               records (three float4: a, b, c, w unused -- the distance grid's layout) in LDS.  A point with a
 *               coordinate that is not finite gives NaN and takes no part in the pair loop.
 *   tree        a dense octree over the bounding cube (lo_a = min v_a, ext = the largest extent, as the distance grid)
 *               with L levels below the root, 0 <= L <= TT_WIND_MAX_LEVELS; G = 2^L leaf cells per axis, inv_h = G / ext
 *               (0 where ext == 0).  A face belongs to the leaf cell of its centroid ((a + b) + c) * (1/3 in fp32), every
 *               operation rounded to fp32, cell(x) the distance grid's own function (tri_cell).  The Morton key of cell
 *               (c_x, c_y, c_z) puts bit b of c_x, c_y, c_z at bits 3b+2, 3b+1, 3b.  tt_wind_face_keys writes the
 *               records in face order and keys (T) int64; the host sorts (key, face) (one stable sort) and gathers the
 *               records into that order: sorted_records, and leaf_ptr (8^L + 1) int32, the CSR of the leaves.  The
 *               faces under node (l, m) are then the range leaf_ptr[m 8^(L-l)] .. leaf_ptr[(m+1) 8^(L-l)] of the sorted list.
 *   node table  level l holds its 8^l nodes in Morton order from node (8^l - 1) / 7 on; tt_wind_node_count(L) =
 *               (8^(L+1) - 1) / 7 nodes of 8 floats: N_x, N_y, N_z, r, c_x, c_y, c_z, A.  N = sum 1/2 (b-a) x (c-a), the
 *               sum of the area vectors; A = sum of the areas |1/2 (b-a) x (c-a)|; c the area-weighted centroid
 *               sum A_f cen_f / A (the plain mean where A == 0); r a bounding radius about the STORED c.  r = -1 marks an
 *               empty node.  A leaf (one thread per leaf, tt_wind_build's first launch) sums its faces in sorted
 *               order, r = the largest distance from c to a vertex of its faces.  An inner node (one launch per level,
 *               bottom up) combines its eight children in child order: N and A summed, c = sum A_k c_k / A, r =
 *               max_k (|c - c_k| + r_k) over the occupied children.  Per-face terms are fp32, every sum a double rounded
 *               to fp32 when stored.  No float atomics: two builds give the same bits.
 *   fast        tt_wind_fast (Barnes-Hut; Barill et al. 2018, the dipole term only), one thread per point, depth first
 *               from the root: an empty node is skipped; a node with |c-p|^2 > (beta r)^2 (fp32) contributes
 *               N . (c-p) / |c-p|^3; any other inner node is descended; any other leaf is summed pair by pair over its
 *               faces in sorted order.  w = sum / 4 pi, accumulated in double in walk order: for a given (L, beta) bit
 *               for bit independent of the launch and the order of the points.  The walk keeps no stack, its state is
 *               (l, m): descend (l+1, 8m); advance: while (l > 0 && (m & 7) == 7) { m >>= 3; --l; }, stop at l == 0,
 *               else ++m.  It visits a node at most once.  beta > 0; a beta whose (beta r)^2 overflows (1e30, inf)
 *               never takes the far branch and gives the pair sum in sorted order.  tt_wind_point_keys writes the Morton
 *               key of the leaf cell of every point clamped to the cube (-1 for a point that is not finite): the host
 *               may sort it and pass the permutation as `order` (N) int64, as for tt_dist_query.
 *   default L   ops.wind_default_levels(T) = the smallest L with 6 * 4^L >= T, at most 6 (clamp(ceil(log4(T / 6)), 0, 6)):
 *               about two faces per occupied leaf.  The first rule, 8 faces per occupied leaf, lost to deeper trees on
 *               every mesh measured, 1.8 k to 473 k faces: 100 k points near the surface of a 28 k-face mesh took 6.1 /
 *               1.94 / 1.06 ms at L = 4 / 5 / 6, of a 3 040-face torus 3.26 / 1.58 / 0.92 / 0.99 ms at L = 3 .. 6 -- the walk
 *               waits for one node's 32 bytes at a time and its lanes diverge in the leaves' pair loops, so small leaves
 *               win until they hold a face or two (profiles/mesh_winding.json).
 * Every entry point validates its arguments before any HIP call (TT_ERR_BAD_ARG); N = 0 does nothing; N, V, T <=
 * TT_MESH_MAX_ITEMS; leaf_ptr values are clamped to [0, T] where they are read.
 * Out of scope: the quadrupole terms, a gradient of w, watertightness repair. */
#define TT_WIND_MAX_LEVELS 6
int64_t tt_wind_node_count(int32_t levels);
int tt_wind_face_keys(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, int32_t levels, float lo_x,
                      float lo_y, float lo_z, float ext, float inv_h, float* records, int64_t* keys, void* stream);
int tt_wind_build(const float* sorted_records, const int32_t* leaf_ptr, int32_t T, int32_t levels, float* nodes,
                  void* stream);
int tt_wind_point_keys(const float* points, int32_t N, int32_t levels, float lo_x, float lo_y, float lo_z, float ext,
                       float inv_h, int64_t* keys, void* stream);
int tt_wind_exact(const float* points, int32_t N, const float* records, int32_t T, float* out, void* stream);
int tt_wind_fast(const float* points, const int64_t* order, int32_t N, const float* sorted_records,
                 const int32_t* leaf_ptr, const float* nodes, int32_t T, int32_t levels, float beta, float* out,
                 void* stream);

/* ---- ray casting (tt_ray.hip): closest hit and any hit of rays with a triangle mesh, an ambient-occlusion count ----
 * The query behind ops.mesh_ray_cast / mesh_ray_occluded / ray_mesh_depth, Mesh.ray_cast and the ambient-occlusion map
 * of a simplified export (ops.bake_ambient_occlusion, map_Ka).  The reference has no such step.  The mesh is the
 * TriangleGrid of "point-to-mesh distance" above, unchanged: records (T,3,4), cell_ptr (G^3 + 1), cell_tri (M), lo, ext,
 * h, inv_h, G (the kernels take it as the TriGridView of csrc/tt_trigrid.h).  A ray is a row o of origins (N,3) and a
 * row d of dirs (N,3), fp32; d has any length, t is in units of d;
 * t_max is one fp32 per call, >= 0, +inf allowed.  Hits have 0 <= t <= t_max.
 *   pair        ONE device function (ray_pair) with one call site (ray_walk), shared by the three kernels: the
 *               watertight test of Woop, Benthin and Wald (JCGT 2013) in fp32.  kz = argmax |d| (the lowest index at
 *               equal magnitude), kx, ky the next two axes cyclically, swapped when d[kz] < 0; Sx = d[kx] / d[kz],
 *               Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Per vertex A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz],
 *               likewise B, C.  U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax, each of the six products and three
 *               differences rounded on its own (a contracted a b - c d is not antisymmetric; watertightness rests on the
 *               two triangles of an edge seeing the same magnitude with opposite sign; the file rounds every operation
 *               of the pair on its own, so an fp32 restatement gives the same bits).  If any of U, V, W is exactly 0 all
 *               three are recomputed from the same fp32 operands in double and rounded to fp32.  A miss when some of
 *               U, V, W are < 0 and some > 0; a miss when det = (U + V) + W == 0 (a ray in the triangle's plane, a
 *               triangle without area) or is not finite (overflow).  t = ((U Az + V Bz) + W Cz) / det with Az = Sz A[kz];
 *               a miss unless 0 <= t <= t_max.  A pair accepted so far is still a miss when the face's fp32 edge vectors
 *               b - a and c - a are exactly parallel (their cross product, the products taken exactly in double, is
 *               (0, 0, 0): equal vertices, exactly collinear ones): det is rounding noise on such a face, and a ray that
 *               passes within rounding of its line would hit it.  Barycentrics (U, V, W) / det, each >= 0.  Both sides
 *               of a triangle are hit.  Finite input never gives NaN: every NaN on the way is a miss.
 *   answer      per ray the lexicographic minimum of (t, face) over ALL T triangles: equal t goes to the smaller face
 *               index.  t (N) fp32, face (N) int32, bary (N,3) fp32; a miss is (+inf, -1, 0).  It does not depend on
 *               the grid, on the order inside a cell, on the order of the rays or on the launch, bit for bit.  A row
 *               with a coordinate that is not finite, or whose largest |d| component is below FLT_MIN (d == 0, and a
 *               denormal direction, whose reciprocal overflows), is (NaN, -1, 0) and leaves the kernel before the walk.
 *   walk        one thread per ray, no stack, no incremental DDA state: slices of cells along the dominant axis
 *               ka = kz.  S = ext + max_a |o_a - centre_a| + max_a |centre_a| (centre = lo + ext / 2) is the scale of
 *               every coordinate the walk forms; tol = 2^-16 S.  The ray's span [t_lo, t_hi] is [0, t_max] cut by the
 *               three slabs [lo_a - tol, lo_a + ext + tol] (each bound (plane - o_a) / d_a moved outward by 2^-16 |t|;
 *               an axis with d_a == 0 only decides whether the ray is outside, which ends the ray).  For j = 0 .. G-1,
 *               k = j (d[ka] > 0) or G-1-j: the planes lo[ka] + k h and lo[ka] + (k+1) h, their parameters ordered as
 *               [ta, tb], dilated to s = ta - (2^-16 |ta| + tol / |d[ka]|), e = tb + (2^-16 |tb| + tol / |d[ka]|); the
 *               first slice has s = -inf, the last e = +inf (inf - inf opens likewise).  s > t_hi ends the walk.
 *               [t0, t1] = [s, e] cut by the span; if it is not empty, on each lateral axis b the ray's coordinates
 *               o_b + t0 d_b and o_b + t1 d_b (o_b itself where d_b == 0), their minimum lowered and their maximum
 *               raised by tol, go through the grid's own cell() -- tri_cell of csrc/tt_trigrid.h, the monotone function
 *               the triangles were binned with (its clamp is taken before the conversion, so that an infinity lands on
 *               a cell) -- and give the cell range.  Every triangle of every cell of that rectangle is tested against
 *               the ray; a hit is accepted whatever cell it falls in; (t, face) is minimised.  After a slice the walk
 *               stops when the best t is STRICTLY below s: equality goes on.  tt_ray_any and tt_ray_ao leave at the
 *               first accepted pair instead.  G = 1 is brute force through the same code.
 *   why it is   Let the pair accept triangle f at the fp32 value t.  P = the point of f nearest to R(t) = o + t d (in
 *   conservative exact arithmetic).  The pair's t is within 2^-20 (L + |o|) / |d| of the exact parameter (measured 2.4e-7 of
 *               that scale, tests/ray_reference.py), so |R(t) - P| <= eps = 2^-19 S.  P lies in f's box, so by the
 *               monotonicity of cell() f is a member of cell(P) on every axis.  Slice: with kk = cell(P_ka), P_ka lies
 *               between the planes of kk up to delta, the disagreement of lo + k h with the boundary cell() implies:
 *               a few ulp of |lo| + ext, delta <= 2^-21 S.  Then t lies within (delta + eps) / |d[ka]| of the exact
 *               [ta, tb]; the fp32 ta, tb carry three roundings (2^-22 |t|) and the rounding of plane - o
 *               (2^-23 S / |d[ka]|): all inside the dilation 2^-16 |t| + 2^-16 S / |d[ka]|, by a factor of four.
 *               t is in [0, t_max] as an fp32 fact, and in the span since R(t) is within eps < tol of the cube.
 *               Lateral: t in [t0, t1] puts the exact o_b + t d_b between the two end values; the fp32 end values are
 *               off by at most 2^-23 (|o_b| + |t d_b|) <= 2^-21 S (|t d_b| <= |t d_ka| <= |o_ka| + |centre| + ext inside
 *               the span), and P_b is within eps of it: 2^-21 S + 2^-19 S < tol, so cell(min - tol) <= cell(P_b) <=
 *               cell(max + tol).  Order: s does not decrease with j (every operation on the way is monotone), so a
 *               pair first met in a later slice has t >= that slice's s >= this slice's s.  The first constant
 *               tried, 2^-18 in tol, left a factor below two against eps; extra cells cost time only.
 *   loops       bounded by G (slices, the two lateral ranges) or by a CSR row clamped to [0, M]; cell ids come from
 *               clamped coordinates; no spin wait, no float atomics, no dependence between workgroups, no scratch.
 *   tt_ray_cast   origins, dirs, order (N) int64 or NULL as for tt_dist_query (the host may sort tt_dist_keys of the
 *               origins), N, t_max, the grid; writes t, face, bary.
 *   tt_ray_any    the same inputs; hit (N) uint8 = 1 where some triangle is hit in [0, t_max], which does not depend on
 *               the grid; a row that is not usable gives 0.
 *   tt_ray_ao     points (N,3), normals (N,3) of any non-zero length, dirs_local (K,3) fp32, 1 <= K <= TT_RAY_MAX_DIRS,
 *               bias (finite), max_distance (>= 0, +inf allowed), the grid; hits (N) int32.  n^ = the normal divided by
 *               its largest |component|, then by its length.  Ray (i, k) starts at p_i + bias n^_i and runs along
 *               x T + y B + z n^ with (x, y, z) = dirs_local[k] and (T, B) the branch-free orthonormal basis of Duff et
 *               al. 2017 about n^ (every operation fp32, rounded on its own); t_max = max_distance.  hits[i] = the
 *               number of the K rays with any hit: ray r = i K + k is thread r, so the rays of a point sit in adjacent
 *               lanes, and the count is by integer atomicAdd onto a zero written by a launch in front -- an integer, so
 *               the order of arrival cannot show.  The directions are a table from the host: no device sin / cos
 *               enters the answer.  A point or normal that is not finite, or a zero normal, gives -1.
 * Every entry point validates its arguments before any HIP call (TT_ERR_BAD_ARG); N = 0 does nothing; N, T <=
 * TT_MESH_MAX_ITEMS, 1 <= G <= TT_DIST_MAX_GRID.
 * Out of scope: a BVH, per-ray t_max, bent normals, a backward kernel (ops.ray_mesh_depth differentiates the plane
 * formula of the hit face in torch: the query is the hot path). */
#define TT_RAY_MAX_DIRS 1024
int tt_ray_cast(const float* origins, const float* dirs, const int64_t* order, int32_t N, float t_max,
                const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T, int32_t M,
                int32_t grid, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h, float* t,
                int32_t* face, float* bary, void* stream);
int tt_ray_any(const float* origins, const float* dirs, const int64_t* order, int32_t N, float t_max,
               const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T, int32_t M,
               int32_t grid, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h, uint8_t* hit,
               void* stream);
int tt_ray_ao(const float* points, const float* normals, const float* dirs_local, int32_t N, int32_t K, float bias,
              float max_distance, const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T,
              int32_t M, int32_t grid, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h,
              int32_t* hits, void* stream);

/* ---- mesh to SDF grid (tt_dist.hip): the signed distance of a triangle mesh on a regular grid, clamped to a band ----
 * The field of a mesh, for ops.marching_cubes (ops.mesh_sdf_grid, Mesh.sdf_grid, Mesh.solidify): level (R,R,R) fp32 in
 * the layout tt_mc_* reads, level[(i R + j) R + k] at the corner with position (x, y, z)_a = fl(lo_a + fl(idx_a * h)),
 * idx = (i, j, k) -- the product and the sum each rounded to fp32, never fused: the values torch computes for
 * lo + idx.float() * h.  New symbols only: TT_ABI_VERSION is unchanged.
 *   value       tau = fl(band * h) (the host's), (d2, face) = tt_dist_query's answer at the corner, BIT FOR BIT, d =
 *               sqrt(d2) correctly rounded.  A corner with d < tau is a BAND corner: level = sgn d, face = its face.
 *               Every other corner: level = sgn tau, face = -1.
 *   sign        a corner with d < sign_tau (>= tau, the host's) is a SIGN corner: sgn = -1 where its winding number w >
 *               0.5, else +1 (NaN: +1), the rule of ops.mesh_signed_distance.  Any other corner takes the sign of the
 *               nearest sign corner BELOW it along the last axis in its (i, j) row, and + when there is none.  With
 *               sign_tau = tau the sign corners are the band corners.  ops.mesh_sdf_grid passes sign_tau = max(band,
 *               1 + 2^-10) h: along a row the distance to a closed surface changes by at most h per corner, so the first
 *               corner behind a crossing has d <= h and is a sign corner itself -- a band narrower than a cell would
 *               otherwise carry the outside sign through the interior whenever the crossing's inner corner is not in
 *               the band.  For band >= 1 + 2^-10 the two sets coincide.
 *   scatter     tt_sdfgrid_scatter finds the CANDIDATES, the corners within reach of some triangle.  Work item =
 *               (triangle, one i-plane x 4 rows of its box): the triangle's bounding box in corner indices, grown by
 *               reach = sign_tau / h + 1/100 + 2^-18 m / h cells (double), m the largest |coordinate| of the triangle
 *               and of the grid's corners, and clipped to the grid.  tt_exclusive_scan of the item counts (int64, the
 *               total stays on the device), a grid-stride loop over items, a binary search for the item's triangle: a
 *               thread loops over at most 4 R corners however large the triangle.  A corner whose squared distance to
 *               the triangle's BOX exceeds 1.001 (reach h)^2 is skipped; else dist_closest, the query's device
 *               function, gives the pair's d2, and d2 <= (reach h)^2 goes to atomicMin (uint64) on (bits of d2) << 32 |
 *               face -- d2 >= 0 orders as its bits do.  Integer atomics only: the candidate set does not depend on the
 *               launch or on the order of the triangles.  A triangle with a vertex that is not finite reaches no
 *               corner (the query never lets it win either).  Every index is clamped to [0, R) before it addresses a
 *               key.
 *   why two     The scatter's d2 is the query's up to the LAST BIT only: dist_closest is inlined into both kernels,
 *   passes      under the same contraction setting, and the compiler fuses products and sums differently in the two
 *               (measured on a 32^3 sphere at R = 33: 30 % of the band corners differ in the last bit of sqrt(d2), 1 %
 *               in the face of a tie; a barrier that hides the loop invariants from the optimiser changed neither).
 *               So the scatter's keys only select: the slack above exceeds that bit by three orders of magnitude, every
 *               sign corner is a candidate, and the host runs tt_dist_query on the candidates -- near points, which
 *               the ring search is built for -- and tt_wind_fast next to it.  Their answers are what the grid holds.
 *   compaction  tt_compact.h over the keys that are not empty: out_count (2) int32, both the number of candidates,
 *               DEVICE memory, read back once.  tt_sdfgrid_corners writes them in ascending corner id: corner (n_cand)
 *               int32, points (n_cand,3) fp32.
 *   finish      tt_sdfgrid_finish takes d2 (n_cand), nearest (n_cand) int32 (tt_dist_query's) and winding (n_cand) of the
 *               candidates: k_sdf_keys replaces their keys by the query's (nearest = -1: empty) and writes sgn into
 *               level; then k_sdf_finish, one wave per (i, j) row over 64 corners of the last axis at a time (ballots
 *               of sign / inside, the highest set bit below a lane, a carry between chunks), writes level and face of
 *               every corner.  A candidate beyond sign_tau is an ordinary far corner.
 * Use: ws = tt_sdfgrid_workspace_bytes(R, T) = 12 R^3 bytes (keys, compaction offsets) + 8 T (item offsets) + block
 * sums; scatter, read out_count, corners, tt_dist_query and tt_wind_fast on points, finish -- all with the same
 * workspace.  2 <= R <= TT_SDFGRID_MAX_RES, 0 < tau <= sign_tau <= (TT_SDFGRID_MAX_BAND + 1) h, h > 0, 1 <= T <=
 * TT_MESH_MAX_ITEMS, 0 <= n_cand <= R^3; every entry point validates before any HIP call (TT_ERR_BAD_ARG).  No float
 * atomics, no scratch, no spin wait.  Not differentiable.
 * Out of scope: a gradient, adaptive or sparse grids, dual contouring of sharp features, a ShapeLoss on the grid. */
#define TT_SDFGRID_MAX_RES 512
#define TT_SDFGRID_MAX_BAND 16
int64_t tt_sdfgrid_workspace_bytes(int32_t resolution, int32_t T);
int tt_sdfgrid_scatter(const float* records, int32_t T, int32_t resolution, float lo_x, float lo_y, float lo_z, float h,
                       float tau, float sign_tau, void* workspace, int32_t* out_count, void* stream);
int tt_sdfgrid_corners(int32_t resolution, int32_t T, float lo_x, float lo_y, float lo_z, float h, float tau,
                       float sign_tau, const void* workspace, int32_t n_cand, int32_t* corner, float* points,
                       void* stream);
int tt_sdfgrid_finish(int32_t resolution, int32_t T, float tau, float sign_tau, void* workspace, const int32_t* corner,
                      const float* d2, const int32_t* nearest, const float* winding, int32_t n_cand, float* level,
                      int32_t* face, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TT_ABI_H */
