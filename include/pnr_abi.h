/*
 * pnr_abi.h — C ABI of the MI355X (gfx950) pixelNeRF ray-march library (libpnr.so).
 *
 * The library replaces the per-ray hot path of the reference (etiiiR/pixel-nerf) and the mesh
 * step of its evaluation script:
 *   src/render/nerf.py      NeRFRenderer.forward / sample_* / composite  (nerf.py:98-303)
 *   src/model/models.py     PixelNeRFNet.forward                         (models.py:146-266)
 *   src/model/resnetfc.py   ResnetFC / ResnetBlockFC                     (resnetfc.py:10-184)
 *   src/model/code.py       PositionalEncoding                           (code.py:30-42)
 *   src/model/encoder.py    SpatialEncoder.index (grid_sample)           (encoder.py:80-109)
 *   eval/eval.py            skimage.measure.marching_cubes               (eval.py:105)
 *   src/util/recon.py       mcubes.marching_cubes                        (recon.py:71)
 *   eval/calc_metrics.py    skimage compare_ssim / compare_psnr          (calc_metrics.py:188-191)
 *   eval/eval_approx.py     the same two scores per rendered view
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller, except the struct
 *     arguments themselves (host memory, read during the call only).
 *   - All tensors are fp32, C-contiguous, row-major, in the shapes given below (exceptions:
 *     the float64 `out` of pnr_image_metrics and pnr_mesh_distance_reduce, the float64
 *     `total_area` of pnr_mesh_sample, the float64 `w` of pnr_winding, the float64 `out` and int64
 *     `order` / `seg_start` of pnr_mesh_component_sums, and the int32 index tensors named as such).
 *     The `lo` / `hi` of pnr_box_sample and the `launches` of pnr_mesh_components are host memory.
 *   - Calls are asynchronous and stream-ordered on `stream` (a hipStream_t; NULL
 *     = the default stream).  The library never allocates device memory: scratch
 *     comes from a caller-provided workspace sized by the *_workspace_bytes query.
 *     Three calls wait for their stream before they return: pnr_mc_emit, which reads the two
 *     counted totals back to check the caller's capacities, pnr_mesh_sample, which reads its
 *     face-index flag and the total area back before it samples, and pnr_mesh_components, which
 *     reads its face-index flag back.  pnr_mc_case_table is host-only.
 *   - Functions return PNR_OK (0) or a negative pnr_status; pnr_last_error()
 *     returns a thread-local message for the last failing call on that thread.
 *     No C++ exception crosses this boundary.
 *   - Re-entrant: no mutable global state; callers may use one thread per GPU.
 */
#ifndef PNR_ABI_H
#define PNR_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_ABI_VERSION 8   /* 4: pnr_weight_grad_arith (per-call weight-gradient arithmetic);
                               5: pnr_latent_channels_last_nhwc;
                               6: pnr_fold_batchnorm;
                               7: pnr_latent_channels_last_backward,
                                  pnr_points_input_backward_masked;
                               8: pnr_render_cfg.ray_order */

typedef enum pnr_status {
    PNR_OK = 0,
    PNR_ERR_INVALID = -1,     /* bad argument / shape / null pointer               */
    PNR_ERR_UNSUPPORTED = -2, /* configuration the kernels do not implement        */
    PNR_ERR_HIP = -3,         /* HIP runtime error (launch or device query)        */
    PNR_ERR_WORKSPACE = -4    /* workspace missing or too small                    */
} pnr_status;

typedef void *pnr_stream_t; /* hipStream_t */

/* Encoded source views: what PixelNeRFNet.encode() leaves in the model
 * (models.py:111-141) plus the encoder feature map (encoder.py:160-163). */
typedef struct pnr_scene {
    const float *latent; /* (n_obj*n_views, latent_h, latent_w, latent_c), channels-LAST  */
    const float *cams;   /* (n_obj*n_views, 16): R_wc[3][3] row-major, t_wc[3],
                            fx, fy (already negated as models.py:130 does), cx, cy         */
    int32_t n_obj;       /* SB: objects in the super-batch                                 */
    int32_t n_views;     /* NS: source views per object                                    */
    int32_t latent_h, latent_w, latent_c;
    float image_w, image_h; /* PixelNeRFNet.image_shape = [W, H] (models.py:116-117)       */
} pnr_scene;

/* Shape of a ResnetFC (resnetfc.py:65-130) + positional encoding (code.py). */
typedef struct pnr_mlp_desc {
    int32_t d_in;          /* 42 for the shipped conf (xyz PE 39 + viewdir 3)             */
    int32_t d_latent;      /* 512                                                          */
    int32_t d_hidden;      /* 512                                                          */
    int32_t d_out;         /* 4                                                            */
    int32_t n_blocks;      /* 5                                                            */
    int32_t combine_layer; /* 3 (>= n_blocks means never combine; requires n_views == 1)  */
    int32_t pe_n;          /* entries of code._freqs / code._phases (2*num_freqs = 12)    */
    int32_t precision;     /* PNR_PREC_*: arithmetic of the 512-wide layers (see below)  */
} pnr_mlp_desc;

/* Arithmetic of the ResnetFC GEMMs (fp32 in, fp32 out, fp32 accumulation in all modes):
 *   PNR_PREC_F32    v_mfma_f32_16x16x4_f32 — fp32 products, fp32 accumulation.
 *   PNR_PREC_BF16X9 both operands split EXACTLY into three bf16 parts (x = x0+x1+x2),
 *                   all 9 part-products on v_mfma_f32_16x16x32_bf16: every product exact,
 *                   only the fp32 accumulation rounds (numerically an fp32 GEMM).
 *   PNR_PREC_BF16X6 the 6 largest of those products (drops x1*y2, x2*y1, x2*y2, each
 *                   < 2^-24 |x y|): error at the fp32 unit roundoff.
 *   PNR_PREC_F16X3  W (per layer) and every activation column scaled by a power of two
 *                   (max <= 2^14), each split into two fp16 parts x = x0 + x1 (|x - x0 - x1|
 *                   <= 2^-22 |x|); 3 exact products x0 y0 + x0 y1 + x1 y0 on
 *                   v_mfma_f32_16x16x32_f16, fp32 accumulation, scales undone exactly.
 *                   Error at the fp32 level (tools/precision_study.py).
 *   PNR_PREC_F16    half precision, INFERENCE ONLY (additive in ABI 8).  The same scaling as
 *                   F16X3 (W per layer and every activation column by a power of two, max
 *                   <= 2^14, so the mode is safe at any dynamic range), but each operand of the
 *                   512 -> 512 layers is rounded ONCE to fp16 (round to nearest even): one
 *                   product per k-step on v_mfma_f32_16x16x32_f16, fp32 accumulation, scales
 *                   undone exactly.  The pack of those layers holds one fp16 part (half of
 *                   F16X3's layer bytes).  lin_in (d_in <= 64), the lin_z contribution (the
 *                   fp32 projected latent), the multi-view mean and the head keep F16X3's /
 *                   fp32 arithmetic.  Error: one fp16 rounding (2^-11 relative) per operand
 *                   and layer; on the pixelNeRF fixtures max |d rgb| 6e-4 per point and 4e-4
 *                   per ray, max |d sigma| 2.6e-3, against an 8-bit step of 3.9e-3
 *                   (tests/f16_emul.py).  It runs on the projected-latent path
 *                   only: pnr_point_query_proj / pnr_render_forward_proj with the latent
 *                   projections; a call without them, the training forward (activation save),
 *                   pnr_mlp_packed_t_bytes / pnr_mlp_pack_t and pnr_mlp_backward refuse it
 *                   (PNR_ERR_UNSUPPORTED, 0 bytes). */
#define PNR_PREC_F32 0
#define PNR_PREC_F16 1
#define PNR_PREC_F16X3 3
#define PNR_PREC_BF16X6 6
#define PNR_PREC_BF16X9 9

/* Unpacked weights in torch nn.Linear layout: weight (out, in), bias (out). */
typedef struct pnr_mlp_weights {
    pnr_mlp_desc desc;
    const float *lin_in_w, *lin_in_b;
    const float *lin_z_w[8], *lin_z_b[8];  /* min(combine_layer, n_blocks) entries  */
    const float *fc0_w[8], *fc0_b[8];      /* blocks[i].fc_0, n_blocks entries       */
    const float *fc1_w[8], *fc1_b[8];      /* blocks[i].fc_1                         */
    const float *lin_out_w, *lin_out_b;
    const float *pe_freqs, *pe_phases;     /* code._freqs, code._phases (pe_n each)  */
} pnr_mlp_weights;

/* Rays, (n_rays, 8) = [ox, oy, oz, dx, dy, dz, near, far] (nerf.py:101).  Rays are
 * object-major: ray b belongs to object b / rays_per_obj (nerf.py:191-196). */
typedef struct pnr_rays {
    const float *rays;
    int64_t n_rays;
    int64_t rays_per_obj;
} pnr_rays;

/* Random draws of the march (nerf.py:111, 135, 141, 158), in one of two modes:
 *   injected  the four streams below, drawn by the caller in the reference's order (tests
 *             and fixtures: the reference's own torch.rand draws replayed exactly);
 *   counter   every stream pointer NULL: the kernels draw on device from {seed, offset}
 *             with Philox4x32-10.  Draw k of ray b of stream s uses the counter
 *             (lo32 e, hi32 e, s, 0), e = (offset + b) * width_s + k, key (lo32 seed,
 *             hi32 seed); U[0,1) = (word0 >> 8) * 2^-24; N(0,1) = Box-Muller on
 *             u1 = ((word0 >> 8) + 1) * 2^-24, u2 = (word1 >> 8) * 2^-24.  A ray's draws
 *             depend on its global index (offset + b) only, so chunking a batch with
 *             offset = the chunk's first ray gives the same samples as one call.
 *             No HBM streams are written or read.  pnr_rng_fill materialises a stream. */
#define PNR_RNG_U_COARSE 0   /* width n_coarse                      */
#define PNR_RNG_U_FINE 1     /* width n_fine - n_fine_depth         */
#define PNR_RNG_U_FINE_JIT 2 /* width n_fine - n_fine_depth         */
#define PNR_RNG_N_DEPTH 3    /* width n_fine_depth, normal          */
typedef struct pnr_rng {
    const float *u_coarse;   /* (n_rays, n_coarse)          U[0,1)  */
    const float *u_fine;     /* (n_rays, n_fine - n_fine_depth)     */
    const float *u_fine_jit; /* (n_rays, n_fine - n_fine_depth)     */
    const float *n_depth;    /* (n_rays, n_fine_depth)      N(0,1)  */
    uint64_t seed;           /* counter mode (all four pointers NULL) */
    uint64_t offset;         /* global index of ray 0 of this call    */
} pnr_rng;

typedef struct pnr_render_cfg {
    int32_t n_coarse;     /* Kc                          (nerf.py:75)       */
    int32_t n_fine;       /* Kf incl. depth samples       (nerf.py:76)       */
    int32_t n_fine_depth; /* Kfd                          (nerf.py:77)       */
    float depth_std;      /*                              (nerf.py:80)       */
    int32_t white_bkgd;   /*                              (nerf.py:83)       */
    int32_t lindisp;      /*                              (nerf.py:84)       */
    /* ABI 3: ray-march schedule of THIS call (no process state is read or written):
     *   3  coarse and fine pass in ONE launch (n_coarse = 64, n_coarse + n_fine = 128,
     *      projected latents; other shapes run mode 2),
     *   2  fused passes + fine-draw kernel, 1  fine draws in the coarse epilogue too,
     *   0  separate sample / MLP / composite kernels (see pnr_render_set_fused);
     *  -1  the process default set by pnr_render_set_fused (initially 2).
     * All modes give bit-identical results. */
    int32_t march_mode;
    /* ABI 8: the order in which the fused march (modes 1-3) takes the rays, or NULL (input
     * order).  ray_order[i] is the index of the i-th ray to process; it should be a permutation
     * of 0 .. n_rays - 1 (an entry out of range processes ray i instead).  Every draw and every
     * output stays at the ray's own index, so the results are bit-identical to NULL's; only the
     * schedule -- which rays share an XCD's L2 at a time -- changes (NeRFRenderer.ray_order:
     * pixel blocks of 16 x 16 rays). */
    const int32_t *ray_order;
} pnr_render_cfg;

/* Outputs; any pointer may be NULL except the rgb/depth of each pass that runs. */
typedef struct pnr_render_out {
    float *coarse_rgb;     /* (n_rays, 3)                              */
    float *coarse_depth;   /* (n_rays)                                 */
    float *coarse_weights; /* (n_rays, n_coarse)                       */
    float *fine_rgb;       /* (n_rays, 3)           if n_fine > 0      */
    float *fine_depth;     /* (n_rays)                                 */
    float *fine_weights;   /* (n_rays, n_coarse + n_fine)              */
    float *z_coarse;       /* (n_rays, n_coarse)    sample depths      */
    float *z_fine;         /* (n_rays, n_coarse + n_fine), sorted      */
} pnr_render_out;

/* ---- library ---------------------------------------------------------------- */
int pnr_abi_version(void);
const char *pnr_last_error(void);

/* ---- MLP weight packing (ResnetFC -> MFMA fragment order) ------------------- */
/* Replaces: the nn.Linear parameters of ResnetFC (resnetfc.py:88-112) as the hot
 * path consumes them.  Pack once per weight version; the packed buffer is what
 * pnr_point_query / pnr_render_forward read. */
size_t pnr_mlp_packed_bytes(const pnr_mlp_desc *desc);
int pnr_mlp_pack(const pnr_mlp_weights *w, void *packed, size_t packed_bytes,
                 pnr_stream_t stream);

/* ---- per-point model query ---------------------------------------------------- */
/* Replaces: PixelNeRFNet.forward(xyz, coarse, viewdirs) (models.py:146-266):
 * world->camera transform, PE, projection + bilinear latent gather, ResnetFC with
 * the multi-view mean, sigmoid/relu head.  xyz/viewdirs (n_obj*points_per_obj, 3);
 * viewdirs may be NULL (zeros).  out (n_obj*points_per_obj, 4). */
size_t pnr_point_query_workspace_bytes(const pnr_scene *scene, int64_t n_points);
int pnr_point_query(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                    const float *xyz, const float *viewdirs, int64_t points_per_obj,
                    float *out, void *workspace, size_t workspace_bytes,
                    pnr_stream_t stream);

/* ---- full coarse + fine render ------------------------------------------------ */
/* Replaces: NeRFRenderer.forward(model, rays, want_weights) (nerf.py:251-303)
 * with model = PixelNeRFNet (mlp_coarse / mlp_fine; pass the coarse pack twice when
 * mlp_fine is None, models.py:242).  pnr_render_forward* take ONE `desc`: both packs (and
 * both projections) must come from the same pnr_mlp_desc, since the fine pack is read under
 * that descriptor's layout (a smaller fine pack would be read past its end).  A model whose
 * mlp_fine has another n_blocks or min(combine_layer, n_blocks) cannot use these calls. */
size_t pnr_render_workspace_bytes(const pnr_scene *scene, const pnr_render_cfg *cfg,
                                  int64_t n_rays);
int pnr_render_forward(const pnr_scene *scene, const pnr_mlp_desc *desc,
                       const void *coarse_packed, const void *fine_packed,
                       const pnr_rays *rays, const pnr_rng *rng,
                       const pnr_render_cfg *cfg, const pnr_render_out *out,
                       void *workspace, size_t workspace_bytes, pnr_stream_t stream);

/* Same as pnr_render_forward, plus hipEventRecord of caller-created events on
 * `stream` around every launch: events[0] before sample_coarse, [1] after it
 * (= before the coarse point MLP), [2] after the coarse MLP, [3] after the coarse
 * composite, [4] after sample_fine, [5] after the fine MLP, [6] after the fine
 * composite (entries 4-6 unused when n_fine == 0).  `events` holds 7 hipEvent_t;
 * no host synchronization is added.  Used by bench.py for per-kernel timing.
 * With the fused ray march (pnr_render_set_fused) a pass is one launch: [1]-[2] and
 * [4]-[5] then time the whole coarse / fine pass (sampling and composite included),
 * and the other intervals are empty; with march_mode 3 the single launch is [1]-[2]. */
int pnr_render_forward_events(const pnr_scene *scene, const pnr_mlp_desc *desc,
                              const void *coarse_packed, const void *fine_packed,
                              const pnr_rays *rays, const pnr_rng *rng,
                              const pnr_render_cfg *cfg, const pnr_render_out *out,
                              void *workspace, size_t workspace_bytes, pnr_stream_t stream,
                              void *const *events);

/* ---- projected latent (lin_z folded into the latent, inference) --------------- */
/* Floats-as-bytes of one model's projected latent for `scene`: n_linz x (n_obj * n_views)
 * x latent_h x latent_w x 512 fp32, n_linz = min(combine_layer, n_blocks); 0 if invalid. */
size_t pnr_latent_project_bytes(const pnr_scene *scene, const pnr_mlp_desc *desc);

/* Replaces: the per-point lin_z GEMMs of ResnetFC (resnetfc.py:160-163) on the bilinearly
 * sampled latent (encoder.py:102-108).  grid_sample's output is a blend of four latent
 * pixels and lin_z is linear, so lin_z[b](z) = blend of the rows of
 *   proj[b][image][y][x][:] = lin_z[b].weight . latent[image][y][x][:]      (no bias)
 * computed here once per (scene, weight version) with fp32 products and accumulation.
 * The *_proj entry points below blend four rows per point instead of the lin_z GEMM
 * (same results up to fp32 reassociation).  Forward (inference) only. */
int pnr_latent_project(const pnr_scene *scene, const pnr_mlp_weights *w, float *proj, size_t proj_bytes,
                       pnr_stream_t stream);

/* pnr_point_query / pnr_render_forward_events with the projected latent of the model(s):
 * `proj` (point query), `coarse_proj` / `fine_proj` (render; pass the coarse projection
 * twice when mlp_fine is None) from pnr_latent_project on the same scene and weights.
 * NULL projections select the latent gather + lin_z GEMM path.  `events` may be NULL.
 * When fine_packed == coarse_packed and fine_proj == coarse_proj (mlp_fine is None), the fine
 * pass evaluates only the n_fine new samples and reuses the coarse pass's outputs for the
 * n_coarse coarse samples (bit-identical: a point's output does not depend on the others). */
int pnr_point_query_proj(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                         const float *proj, const float *xyz, const float *viewdirs,
                         int64_t points_per_obj, float *out, void *workspace,
                         size_t workspace_bytes, pnr_stream_t stream);
int pnr_render_forward_proj(const pnr_scene *scene, const pnr_mlp_desc *desc,
                            const void *coarse_packed, const void *fine_packed,
                            const float *coarse_proj, const float *fine_proj,
                            const pnr_rays *rays, const pnr_rng *rng,
                            const pnr_render_cfg *cfg, const pnr_render_out *out,
                            void *workspace, size_t workspace_bytes, pnr_stream_t stream,
                            void *const *events);

/* Fused ray march.  3: the whole march is ONE k_point_mlp launch -- a workgroup takes a ray's
 * coarse tile, composites it and draws its fine samples in the epilogue into LDS, then runs the
 * ray's two fine tiles with the fine MLP and composites them (nerf.py:273-301 per ray; the fine
 * depths never reach HBM unless pnr_render_out.z_fine asks for them).  It applies to
 * n_coarse = 64, n_coarse + n_fine = 128 with both projected latents (the headline shape) and
 * falls back to mode 2 otherwise.  2 (the default): each pass of pnr_render_forward* is one
 * k_point_mlp launch
 * that draws the coarse depths in its prologue and composites each ray from LDS in its
 * epilogue (the per-point rgb/sigma never reach HBM); the fine draws (inverse CDF + sort) run
 * in their own small kernel between the passes.  1: the coarse epilogue draws the fine samples
 * too (one launch per pass; measured 0.3-0.5 % slower on MI355X, since one wave runs them while
 * the workgroup's other seven wait).  0: the separate sample / MLP / composite kernels.  The
 * fusion applies when a pass's samples per ray are 64 or 128 (and kc + kf <= 128 for the fine
 * draws) and mlp_fine is not None; other shapes take the separate kernels.  All modes run the
 * same device code and give bit-identical results.  This only sets the DEFAULT that calls with
 * pnr_render_cfg.march_mode = -1 use (ABI 3); a call that names its mode reads no process state,
 * so host threads (DataParallel replicas, nerf.py:370) may render with different modes at once.
 * Returns the previous default. */
int32_t pnr_render_set_fused(int32_t on);

/* The fused point model (k_point_mlp) has a lean instantiation for the launches of a render of ONE
 * source view on the projected latent by a per-pass fused march (march modes 1 and 2), without an
 * activation save, in precision f16x3 or f16: the paths such a launch never takes are compiled
 * out, and the tile index, the ray and the camera row are scalar registers.  Its outputs are
 * bit-identical to the general kernel's.  pnr_mlp_set_lean(0) makes every launch of the process
 * take the general kernel (tests, A/B runs); nonzero restores the default (on).  Returns the
 * previous setting.  pnr_mlp_last_kernel: the kernel the process's last point-model launch took
 * (any thread), PNR_MLP_KERNEL_NONE before the first.  Additive in ABI 8. */
#define PNR_MLP_KERNEL_NONE 0
#define PNR_MLP_KERNEL_GENERAL 1
#define PNR_MLP_KERNEL_LEAN 2
int32_t pnr_mlp_set_lean(int32_t on);
int32_t pnr_mlp_last_kernel(void);

/* ---- building blocks (also the generic model-callback path) ------------------ */
/* Replaces: NeRFRenderer.sample_coarse (nerf.py:98-118).  z (n_rays, n_coarse). */
int pnr_sample_coarse(const float *rays, int64_t n_rays, int32_t n_coarse,
                      const float *u_coarse, int32_t lindisp, float *z,
                      pnr_stream_t stream);

/* Replaces: sample_fine + sample_fine_depth + cat + sort (nerf.py:120-161, 284-295).
 * weights/depth of the coarse pass; z_fine (n_rays, n_coarse + n_fine) sorted. */
int pnr_sample_fine(const float *rays, int64_t n_rays, int32_t n_coarse,
                    const float *z_coarse, const float *coarse_weights,
                    const float *coarse_depth, int32_t n_fine, int32_t n_fine_depth,
                    float depth_std, const float *u_fine, const float *u_fine_jit,
                    const float *n_depth, int32_t lindisp, float *z_fine,
                    pnr_stream_t stream);

/* Replaces: NeRFRenderer.composite's alpha compositing (nerf.py:176-249).
 * z (n_rays, K), raw (n_rays, K, 4) = model output [r, g, b, sigma];
 * weights (n_rays, K) may be NULL; rgb (n_rays, 3); depth (n_rays).
 * Any k >= 1 is supported (k <= 256 runs the register-resident kernels, larger k the chunked
 * one).  raw must be 16-byte aligned (PNR_ERR_INVALID otherwise); z and weights need only float
 * alignment. */
int pnr_composite(const float *z, const float *raw, const float *rays, int64_t n_rays,
                  int32_t k, int32_t white_bkgd, float *weights, float *rgb, float *depth,
                  pnr_stream_t stream);

/* ---- counter-mode draws --------------------------------------------------------- */
/* Replaces: the torch.rand / torch.randn draws of the march (nerf.py:111, 135, 141, 158) in
 * counter mode: writes out (n_rays, width) = the draws of `stream` (PNR_RNG_*) for rays
 * offset .. offset + n_rays - 1 exactly as the render kernels draw them (uniform for
 * streams 0-2, normal for 3). */
int pnr_rng_fill(uint64_t seed, uint64_t offset, int32_t stream, int64_t n_rays, int32_t width, float *out,
                 pnr_stream_t stream_h);

/* ---- ray generation ------------------------------------------------------------ */
/* Replaces: util.gen_rays (util.py:238-276) with unproj_map (util.py:113-143), ndc=False.
 * poses (n_images, pose_rows, 4) row-major camera-to-world (pose_rows 3 or 4); focal
 * (fx, fy) and principal point (cx, cy) in pixels, as the reference's float(f[0]) etc.;
 * rays (n_images, height, width, 8) = [o, d (unit), near, far]. */
int pnr_gen_rays(const float *poses, int64_t n_images, int32_t pose_rows, int32_t width,
                 int32_t height, float fx, float fy, float cx, float cy, float z_near,
                 float z_far, float *rays, pnr_stream_t stream);

/* ---- encoder latent, channels-last --------------------------- */
/* Replaces: the upsample + concat tail of SpatialEncoder.forward (encoder.py:150-160):
 * n_maps (<= 8) trunk feature maps, maps[k] (n_images, channels[k], heights[k], widths[k])
 * NCHW fp32 device pointers (the pointer arrays themselves are host memory), bilinearly
 * upsampled with align_corners = True to (out_h, out_w) and concatenated along channels,
 * written channels-LAST: latent_cl (n_images, out_h, out_w, sum channels). */
int pnr_latent_channels_last(const float *const *maps, const int32_t *channels,
                             const int32_t *heights, const int32_t *widths, int32_t n_maps,
                             int32_t n_images, float *latent_cl, int32_t out_h, int32_t out_w,
                             pnr_stream_t stream);

/* pnr_latent_channels_last with every maps[k] channels-last, (n_images, heights[k], widths[k],
 * channels[k]) (the trunk's maps when its convolutions run in channels-last memory format):
 * the same arithmetic and output (ABI 5). */
int pnr_latent_channels_last_nhwc(const float *const *maps, const int32_t *channels,
                                  const int32_t *heights, const int32_t *widths, int32_t n_maps,
                                  int32_t n_images, float *latent_cl, int32_t out_h, int32_t out_w,
                                  pnr_stream_t stream);

/* Backward of pnr_latent_channels_last_nhwc: d_maps[k] (n_images, heights[k], widths[k], channels[k],
 * channels-last) = the adjoint of map k's bilinear upsample (align_corners = True) applied to its
 * channel slice of g (n_images, out_h, out_w, sum channels) -- what autograd of encoder.py:150-160's
 * F.interpolate + torch.cat computes (upsample_bilinear2d_backward).  Gathered per source element in
 * a fixed order (deterministic; torch scatters with atomics); one launch for all maps (ABI 7). */
int pnr_latent_channels_last_backward(const float *g, float *const *d_maps, const int32_t *channels,
                                      const int32_t *heights, const int32_t *widths, int32_t n_maps,
                                      int32_t n_images, int32_t out_h, int32_t out_w, pnr_stream_t stream);

/* One (convolution, BatchNorm) pair of the eval-mode encoder trunk (encoder.py:135-149 with the
 * BatchNorms on their running statistics).  conv_w / w_out: n_out blocks of per_out contiguous
 * floats (OIHW or channels-last OHWI weights: the output channel is outermost in both); gamma /
 * beta NULL for a BatchNorm without affine parameters. */
typedef struct pnr_bn_fold {
    const float *conv_w;
    const float *gamma, *beta, *mean, *var;
    float *w_out, *b_out;
    int64_t n_out, per_out;
    float eps;
    int32_t pad_;
} pnr_bn_fold;

/* Fold every pair: w_out[o, :] = conv_w[o, :] s[o], b_out[o] = beta[o] - mean[o] s[o] with
 * s = gamma[o] / sqrt(var[o] + eps) (correctly rounded sqrt and divide).  `folds` is a DEVICE
 * array of n_folds records (the kernel reads it; a HIP graph that captured this call keeps
 * reading the same array); max_elems = max n_out * per_out.  Replaces the per-encode BatchNorm
 * arithmetic of SpatialEncoder.forward in eval mode (encoder.py:135-149); ABI 6. */
int pnr_fold_batchnorm(const pnr_bn_fold *folds, int32_t n_folds, int64_t max_elems, pnr_stream_t stream);

/* ---- training (autograd over the ray march) ------------ */
/* Floats of the activation save of pnr_render_points for n_points rows; call it with
 * n_points = n_rays * k * n_views.  Regions, each [row][width] with R = n_rays * k *
 * n_views rows: features (64) | z (512) | relu(x) into fc_0 of each block (512 each) |
 * relu(h) of each block (512 each) | relu(x) into lin_out (512), then the relu sign masks
 * of the 2 n_blocks + 1 relu regions (same order), each [row][64 bytes], [activation n > 0]
 * of n = 64 w + 16 r + 4 g + e (w, r, g, e = 0..7, 0..3, 0..3, 0..3) at bit 4 (r & 1) + e
 * of byte 8 w + 2 g + (r >> 1).  Row v * (n_rays * k) + p holds (source view v, point p)
 * for the per-view stages (features, z, the blocks before combine_layer); the blocks from
 * combine_layer on and lin_out use rows p < n_rays * k (the view mean). */
size_t pnr_point_save_floats(const pnr_mlp_desc *desc, int64_t n_points);

/* Replaces: the model call of NeRFRenderer.composite (nerf.py:182-216) under autograd:
 * PixelNeRFNet.forward at the points o + z d of every ray (z (n_rays, k)), writing
 * out (n_rays * k, 4) and, when `save` is not NULL, the activations the backward needs
 * (pnr_point_save_floats(desc, n_rays * k * n_views) floats).  Workspace as pnr_point_query. */
int pnr_render_points(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                      const pnr_rays *rays, const float *z, int32_t k, float *out, float *save,
                      void *workspace, size_t workspace_bytes, pnr_stream_t stream);

/* Replaces: autograd of NeRFRenderer.composite (nerf.py:225-247).  Given d_rgb (n_rays, 3),
 * d_depth (n_rays, may be NULL) and d_weights (n_rays, k, may be NULL): d_raw (n_rays, k, 4)
 * = d [rgb, sigma] and d_z (n_rays, k, may be NULL).  k <= 256. */
int pnr_composite_backward(const float *z, const float *raw, const float *rays, int64_t n_rays,
                           int32_t k, int32_t white_bkgd, const float *d_rgb, const float *d_depth,
                           const float *d_weights, float *d_raw, float *d_z, pnr_stream_t stream);

/* Replaces: autograd of the input stage of PixelNeRFNet.forward (models.py:156-221,
 * code.py:30-42, encoder.py:80-109).  d_feat (n_views * n_rays * k, 64): gradient of the
 * lin_in input; d_zlat (n_views * n_rays * k, 512): gradient of the sampled latent feature,
 * rows as the activation save (view-major).  Accumulates d_latent (channels-last, like
 * scene->latent; may be NULL) and writes d_z (n_rays * k, may be NULL) = dL / d z_sample,
 * summed over the views in view order.  `packed` supplies the PE buffers. */
int pnr_points_input_backward(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                              const pnr_rays *rays, const float *z, int32_t k, const float *d_feat,
                              const float *d_zlat, float *d_latent, float *d_z, pnr_stream_t stream);

/* pnr_points_input_backward with z_mask (n_rays * k bytes, may be NULL = every point): d_z is
 * computed only where z_mask is nonzero and written 0 elsewhere.  The fine pass's depths are the
 * sort of [importance samples (no gradient), depth samples (gradient to the coarse depth)]
 * (nerf.py:150-161, 292), so only the depth samples' dL/dz reaches the graph; the mask skips the
 * latent-corner reads of the others (ABI 7). */
int pnr_points_input_backward_masked(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                                     const pnr_rays *rays, const float *z, int32_t k, const float *d_feat,
                                     const float *d_zlat, float *d_latent, float *d_z, const uint8_t *z_mask,
                                     pnr_stream_t stream);

/* Bytes of the transposed (backward) weight pack of an f16x3 model (precision
 * PNR_PREC_F16X3); 0 for an invalid desc or another precision. */
size_t pnr_mlp_packed_t_bytes(const pnr_mlp_desc *desc);

/* Pack W^T of every 512-wide ResnetFC layer for pnr_mlp_backward.  `packed` is the model's
 * pnr_mlp_pack output (same weights, same stream order): its header holds the scales. */
int pnr_mlp_pack_t(const pnr_mlp_weights *w, const void *packed, void *packed_t, size_t packed_t_bytes,
                   pnr_stream_t stream);

/* Replaces: autograd of ResnetFC.forward (resnetfc.py:132-184, n_views == 1) up to the
 * weight GEMMs, for an f16x3 model.  Given the forward's activation save (pnr_render_points)
 * and d_o (n_points, 4) = dL / d lin_out output, writes the gradient of every layer's output:
 *   dy ((2 n_blocks + 1), n_points, 512): [b] fc_0 of block b, [n_blocks] lin_in,
 *       [n_blocks + 1 + b] fc_1 of block b; the lin_z of block b takes dy[n_blocks + b];
 *   d_zlat (n_points, 512): dL / d (sampled latent), summed over the lin_z layers
 *       (required when the model has lin_z layers).
 * Weight and bias gradients are then dy^T . (saved layer input) and column sums of dy.
 *
 * Accuracy of pnr_mlp_backward* (tests/test_gpu_mlp_bwd_inputs.py holds the kernels to it).  The
 * chain runs on the forward's f16x3 GEMM with the gradient image scaled by a power of two PER
 * POINT (per image column: 2^e with max|column| 2^e in (2^13, 2^14], e clamped to [-64, 40]), so
 * the bound is per point, relative to the point's OWN gradient scale and not to the tensor's:
 * for a point p and an output T (dy: every slot and view row of p; d_zlat; and d_feat = dy[n_blocks]
 * W_in computed from it), with s_p(T) = max |exact value| over p's rows of T,
 *   every row of p is within 2e-5 max(s_p(T), s_clamp(T)) of the exact (fp64) backward of the
 *   saved activations.
 * Range: column maxima from 2^-26 (below it the clamp e <= 40, not the data, sets the exponent:
 * s_clamp(dy) = 2^-26) up to 2^78 (e >= -64 keeps max|column| 2^e <= 2^14; above it the fp16 image
 * overflows: not supported; tested with d_o up to 2^60).  For d_zlat and d_feat the threshold is
 * carried through the layer, s_clamp = 2^-26 K A summed over the layers that produce T (K = the
 * layer's input width, A = the power of two above its largest |weight|, the pack's weight scale).
 * Below s_clamp the bound is absolute, 2e-5 s_clamp(T) (a clamped column is stored with the fixed
 * quantum 2^-64; fp32 denormals in d_o are inside this range).
 * A zero d_o row gives exactly zero rows in dy, d_zlat and d_feat (whole zero tiles included).
 * A NaN / Inf in d_o row p stays in point p's rows (every view); d_bias sums over the points and
 * is not confined.  A point's rows do not depend on its position in the launch, on n_points or
 * on the other points (bit for bit), and a repeated call returns the same bits, d_bias included.
 * d_bias is the fp32 sum of the returned dy rows: within n_rows 2^-24 sum |dy| per column.
 * An activation of exactly 0 passes no gradient (the mask bit is [n > 0], torch's relu backward). */
int pnr_mlp_backward(const pnr_mlp_desc *desc, const void *packed, const void *packed_t,
                     const float *lin_out_w, const float *save, const float *d_o, int64_t n_points,
                     float *dy, float *d_zlat, pnr_stream_t stream);

/* Workspace bytes of pnr_mlp_backward_bias for n_points points (0 if n_points <= 0). */
size_t pnr_mlp_backward_workspace_bytes(const pnr_mlp_desc *desc, int64_t n_points);

/* pnr_mlp_backward plus the ResnetFC bias gradients (resnetfc.py:132-184: the column sums of
 * the dy slots over the points) in the same pass: d_bias ((2 n_blocks + 1), 512) in dy's slot
 * order, summed per workgroup over its tiles and then over the workgroups, both in a fixed
 * order (deterministic).  d_bias NULL = pnr_mlp_backward; otherwise `workspace` holds
 * pnr_mlp_backward_workspace_bytes. */
int pnr_mlp_backward_bias(const pnr_mlp_desc *desc, const void *packed, const void *packed_t,
                          const float *lin_out_w, const float *save, const float *d_o, int64_t n_points,
                          float *dy, float *d_zlat, float *d_bias, void *workspace, size_t workspace_bytes,
                          pnr_stream_t stream);

/* pnr_mlp_backward_bias for n_views >= 1 source views per point (resnetfc.py:151-172 with
 * util.combine_interleaved's mean): `save` from pnr_render_points with n_views views (its
 * regions have n_views * n_points rows, row v * n_points + p for the blocks before
 * combine_layer); dy is (2 n_blocks + 1) x (n_views * n_points) x 512, the slots of the blocks
 * from combine_layer on (and lin_out's input) using their first n_points rows, the others the
 * view rows; d_zlat is (n_views * n_points, 512); d_bias sums every slot over all its rows.
 * The blocks after the mean run once per point; dL/d(mean) / n_views then enters the chain of
 * the blocks before it once per view.  n_views == 1 is pnr_mlp_backward_bias. */
int pnr_mlp_backward_views(const pnr_mlp_desc *desc, const void *packed, const void *packed_t,
                           const float *lin_out_w, const float *save, const float *d_o, int64_t n_points,
                           int32_t n_views, float *dy, float *d_zlat, float *d_bias, void *workspace,
                           size_t workspace_bytes, pnr_stream_t stream);

/* Workspace bytes of pnr_weight_grad (n_layers in 1..16); 0 if the sizes are invalid. */
size_t pnr_weight_grad_workspace_bytes(int32_t n_layers, int64_t n_points);

/* Arithmetic of pnr_weight_grad_arith (ABI 4).  fp32 in, fp32 out, fp32 accumulation in both.
 *   PNR_WGRAD_F16X3  (the default of pnr_weight_grad) every operand scaled by a power of two per
 *       (point chunk, channel) that follows the data, split into two fp16 parts, 3 products on
 *       v_mfma_f32_16x16x32_f16.  Error bound PER VALUE, relative to M = the running maximum of
 *       its channel in its chunk (not to the value itself): 22 significand bits down to 2^-8 M,
 *       an absolute error below ~2^-30 M beneath that (subnormal fp16 parts), zero below
 *       ~2^-31 M.  So an output element G_ij is fp32-accurate relative to
 *       sum_p |dy_pi| M_j + M_i |x_pj| (the scale of its channel pair), and an element built
 *       ONLY from values far below their channels' maxima (x_j nonzero only where dy_i is
 *       2^-20 M_i) can carry a large RELATIVE error.  Measured on training-step data at the
 *       fp32 GEMM error scale (DESIGN.md §3 training path).
 *   PNR_WGRAD_BF16X6 three exact bf16 parts per operand (fp32's exponent range, no scales), the
 *       6 largest products on v_mfma_f32_16x16x32_bf16 (dropped terms < 2^-24 |x y|): fp32-level
 *       error PER ELEMENT relative to sum_p |dy_pi x_pj|, whatever the dynamic range.
 *       ~1.4x the kernel time of F16X3. */
#define PNR_WGRAD_F16X3 0
#define PNR_WGRAD_BF16X6 1

/* Replaces: the weight-gradient GEMMs autograd runs for the 512 x 512 nn.Linear layers of
 * ResnetFC (resnetfc.py:132-184): for each layer j,
 *   d_weight[j] (512 x 512, [out][in]) = dy[j]^T x[j],
 * dy[j] (n_points x 512) the layer's output gradient (pnr_mlp_backward's slots), x[j]
 * (n_points x 512) its input (the activation save).  dy, x, d_weight are host arrays of
 * n_layers device pointers (16-byte aligned).  PNR_WGRAD_F16X3 arithmetic (bound above);
 * deterministic (fixed reduction order). */
int pnr_weight_grad(const float *const *dy, const float *const *x, float *const *d_weight, int32_t n_layers,
                    int64_t n_points, void *workspace, size_t workspace_bytes, pnr_stream_t stream);

/* pnr_weight_grad with the arithmetic named per call (PNR_WGRAD_*; another value is
 * PNR_ERR_INVALID); the same workspace. */
int pnr_weight_grad_arith(const float *const *dy, const float *const *x, float *const *d_weight,
                          int32_t n_layers, int64_t n_points, int32_t arith, void *workspace,
                          size_t workspace_bytes, pnr_stream_t stream);

/* ---- Isosurface extraction (marching cubes; additive in ABI 8) ------------------------------
 * Replaces: skimage.measure.marching_cubes in eval/eval.py:105 and mcubes.marching_cubes in
 * src/util/recon.py:71, on a grid that is already on the device.  The output is an INDEXED
 * mesh, verts (V, 3) float32 and faces (T, 3) int32, every shared vertex once.
 *
 *   Grid      (nx, ny, nz) fp32, contiguous, [x][y][z] with z fastest; 1 .. 1024 per axis (larger:
 *             PNR_ERR_UNSUPPORTED).  Grid point p = (x * ny + y) * nz + z.  A grid with a
 *             dimension of 1 has no cells: V = T = 0.
 *   Inside    a corner is inside iff value > level.  NaN compares false: outside, never a fault.
 *   Vertices  one per grid edge whose two ends differ in that predicate, in index units (as skimage
 *             returns them).  With a the value at the lower-index end and b at the higher,
 *             t = (level - a) / (b - a); t = t > 0 ? t : 0 (NaN -> 0); t = t < 1 ? t : 1; the
 *             coordinate along the edge's axis is index + t, the two others are the indices.  Each
 *             operation is rounded once to nearest (no contraction), so every cell sharing the
 *             edge sees the same bits.
 *   Ownership a grid point owns the three edges leaving it towards +x (axis 0), +y (1), +z (2).
 *   Order     vertices by (owner grid point, axis); faces by (cell = its minimum corner's grid
 *             point, position in the case table).  Count pass, exclusive scan, emit pass, no
 *             atomics: the outputs are bit-identical from run to run.
 *   Cases     corner k of a cell is (dx, dy, dz) = (k & 1, (k >> 1) & 1, (k >> 2) & 1) and sets bit
 *             k of the case when inside; edge e = 4 * axis + j runs along `axis` from the corner
 *             whose two other coordinates (in increasing axis order) are (j & 1, j >> 1).  The
 *             256-case table is generated (tools/gen_mc_table.py) from the marching-squares
 *             segments of the six faces; an ambiguous face (two diagonal inside corners) always
 *             separates its inside corners, a rule of that face's four signs alone, so adjacent
 *             cells agree and a surface that does not leave the grid is closed.
 *   Winding   by the right-hand rule a face's normal points towards lower values (skimage's
 *             gradient_direction = "descent"): a blob of high values has positive signed volume.
 *   Empty     a surface that leaves the grid is left open at the boundary; a level above the
 *             maximum or below the minimum gives V = T = 0 and PNR_OK.
 *
 * Call order: pnr_mc_count, read the two counts, size verts / faces, pnr_mc_emit with the SAME
 * grid, dimensions, level and workspace. */

/* Workspace bytes for an (nx, ny, nz) grid: the per-workgroup counts, their scan, the totals and
 * the edge map (one int32 per (grid point, axis): 12 nx ny nz bytes, 201 MB at 256^3).  0 if a
 * dimension is outside 1 .. 1024. */
size_t pnr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);

/* Count pass and scan.  counts_dev: 2 x int64 on the device, {V, T}, valid once the stream
 * reaches this point.  Stream-ordered, no host sync. */
int pnr_mc_count(const float *grid, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                 size_t workspace_bytes, int64_t *counts_dev, pnr_stream_t stream);

/* Emit pass after pnr_mc_count on the same arguments: verts (verts_cap, 3) float32, faces
 * (faces_cap, 3) int32 (NULL allowed with a capacity of 0).  Nothing is stored at or past a
 * capacity.  After its launches the call waits for the stream and compares the counted totals
 * with the capacities: smaller ones return PNR_ERR_INVALID (the outputs are then truncated; a
 * face may hold -1 for a vertex that did not fit). */
int pnr_mc_emit(const float *grid, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                size_t workspace_bytes, float *verts, int64_t verts_cap, int32_t *faces, int64_t faces_cap,
                pnr_stream_t stream);

/* The case table the kernels use (HOST memory, no device needed): out[case] = up to 5 triangles
 * as edge triples, -1 padded. */
int pnr_mc_case_table(int8_t out[256][16]);

/* ---- Image metrics (per-image MSE and mean SSIM; additive in ABI 8) --------------------------
 * Replaces: skimage.measure.compare_ssim(multichannel=True) / compare_psnr in
 * eval/calc_metrics.py:188-191 and eval/eval_approx.py, on images that are already on the device.
 *
 *   Inputs    x, y (n, h, w, c) fp32, contiguous, channels last (what the renderer returns);
 *             n >= 1, c in 1 .. 4, h and w in 7 .. 8192 (larger: PNR_ERR_UNSUPPORTED, as is a
 *             batch that needs 2^24 or more workgroups: n * c * ceil((h - 6) / T) *
 *             ceil((w - 6) / T) with T = PNR_IMAGE_METRICS_TILE).
 *   SSIM      skimage's defaults: 7 x 7 uniform window, sample covariance (cov_norm = 49 / 48),
 *             C1 = (k1 R)^2, C2 = (k2 R)^2 with R = data_range; the map is evaluated at the
 *             (h - 6) x (w - 6) pixels whose window lies inside the image (no boundary mode enters),
 *             averaged per channel, then over the channels.
 *   MSE       the mean over all h * w * c elements.  PSNR = 10 log10(R^2 / mse) is left to the
 *             caller (+inf at mse = 0).
 *   Numerics  the fp32 inputs are widened exactly; window moments, the SSIM expression and every
 *             sum are fp64.  data_range, k1 and k2 are each read as the shortest decimal that
 *             rounds to the float passed (0.03f means 0.03, not 0.0299999993...): C2 enters the
 *             result at full fp64 precision.
 *   Order     one partial per (image, channel, tile), summed per channel in ascending tile order,
 *             then over the channels; no atomics.  A row of `out` is bit-identical from run to run
 *             and whether its image is scored alone or inside a batch.
 *   NaN       a NaN anywhere in image i of x or y makes row i of `out` NaN and no other row.
 *
 * out: (n, 2) FLOAT64 on the device, {mse, ssim} per image, 8-byte aligned like the workspace.
 * Two launches, stream-ordered, no host sync. */
#define PNR_IMAGE_METRICS_TILE 16 /* edge of the SSIM-map tile of one workgroup */

/* Workspace bytes (the per-workgroup partials), 0 for any shape pnr_image_metrics would refuse. */
size_t pnr_image_metrics_workspace_bytes(int64_t n, int32_t h, int32_t w, int32_t c);

int pnr_image_metrics(const float *x, const float *y, int64_t n, int32_t h, int32_t w, int32_t c,
                      float data_range, float k1, float k2, void *workspace, size_t workspace_bytes,
                      double *out, pnr_stream_t stream);

/* ---- Mesh metrics (surface sampling, nearest neighbour, score sums; additive in ABI 8) --------
 * The reference has no counterpart: its eval/eval.py stops at the STL.  These three steps score an
 * extracted mesh against a ground-truth mesh the way Occupancy Networks' eval_pointcloud does
 * (Chamfer-L1 / L2, accuracy / completeness, F-score at a distance tau, normal consistency), on
 * the tensors pnr_mc_emit leaves on the device.
 *
 * Surface sampling (pnr_mesh_sample): verts (n_verts, 3) fp32, faces (n_faces, 3) int32.
 *   Area      area[t] = 0.5 * |(b - a) x (c - a)| of face t = (a, b, c), in fp64 from the fp32
 *             vertices: the differences, the cross product (x = uy vz - uz vy, ...), the squares
 *             summed x, y, z, the root and the half, each operation rounded once.
 *   Indices   a face with an index outside [0, n_verts) is detected in the area pass (its
 *             vertices are never read) and the call returns PNR_ERR_INVALID before sampling.
 *   CDF       the inclusive fp64 sum of the areas in a fixed blocked-sequential order.  With
 *             C = PNR_MESH_SCAN_CHUNK: local[t] = the areas of t's chunk of C faces up to t, added
 *             one by one from 0; mid[t] = off[chunk] + local[t], off = the totals (local of the
 *             chunk's last face) of the earlier chunks of t's group of C chunks, added one by one
 *             from 0; cdf[t] = goff[group] + mid[t], goff = the totals (mid of the group's last
 *             face) of the earlier groups, added one by one from 0.  The CDF is non-decreasing,
 *             cdf[t] == cdf[t - 1] bit for bit where area[t] == 0, and total = cdf[n_faces - 1].
 *             A total that is 0, infinite or NaN returns PNR_ERR_INVALID.
 *   Draws     sample s uses (u0, u1, u2) = draws k = 0, 1, 2 of ray s of the counter-mode stream
 *             PNR_RNG_MESH with width 3, offset 0 and key = seed (pnr_rng above): a sample
 *             depends on (seed, s) only, so the first rows of a longer call equal a shorter one.
 *   Face      the first t with cdf[t] > (double)u0 * total (binary search): a face of area 0 is
 *             never picked.
 *   Point     if u1 + u2 > 1 (the fp32 sum): u1 = 1 - u1, u2 = 1 - u2.  Per coordinate
 *             (a + u1 * (b - a)) + u2 * (c - a) in fp32, each operation rounded once.
 *   Normal    the cross product above over its length, in fp64, rounded to fp32: the unit normal
 *             by the right-hand rule.
 *   Outputs   points (n, 3) fp32; normals (n, 3) fp32 or NULL; tri (n) int32, the picked face, or
 *             NULL; total_area: one FLOAT64 on the device.  No atomics: bit-identical from run to
 *             run.  The call waits for its stream once (it reads the index flag and the total
 *             before anything is read through a face index), as pnr_mc_emit does.
 *
 * Nearest neighbour (pnr_nearest): for every row i of a (n, 3) the nearest row of b (m, 3).
 *   Distance  dx = a.x - b.x, dy, dz rounded to fp32; d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in
 *             fp32.  Never the expanded form |a|^2 + |b|^2 - 2 a.b: with D the exact squared
 *             distance of the fp32 inputs and u = 2^-24, |d2 - D| <= 6 u D whatever the
 *             coordinates' magnitude.
 *   Choice    idx[i] = the LOWEST j whose d2 equals the minimum over j of that fp32 d2; d2[i] is
 *             that minimum.  A comparison with NaN is false: a query none of whose candidates
 *             compares below +inf returns d2 = +inf, idx = 0.  Deterministic.
 *   Tiling    a workgroup scores PNR_NEAREST_QUERIES rows of a against one slice of
 *             PNR_NEAREST_SLICE rows of b, staged PNR_NEAREST_TILE rows at a time; with more than
 *             one slice the per-slice minima (the workspace) are folded in ascending slice order.
 *   Limits    n <= 2^31 - 1, m <= 65535 * PNR_NEAREST_SLICE (larger: PNR_ERR_UNSUPPORTED).
 *
 * Score sums (pnr_mesh_distance_reduce): from d2_ab / idx_ab (n; a's rows against b) and d2_ba /
 * idx_ba (m; b's rows against a), the normals of the two clouds (both, or NULL for none) and tau:
 *   out[0] = sum_i sqrt((double)d2_ab[i])       out[1] = sum_i (double)d2_ab[i]
 *   out[2] = #{i : sqrt((double)d2_ab[i]) < tau}
 *   out[3] = sum_i |normals_a[i] . normals_b[idx_ab[i]]|   (0 without normals; an index outside
 *            [0, m) contributes 0 and is not read through)
 *   out[4 .. 7] the same four for b -> a.  All fp64, summed in a fixed order (element i by thread
 *   i mod 1024 in ascending i, the threads by a fixed tree); out[0 .. 3] depend on the a -> b
 *   inputs only and equal, bit for bit, out[4 .. 7] of a call with the two clouds exchanged.  The
 *   caller divides by n and m.  One launch, no workspace, no host sync. */
#define PNR_RNG_MESH 4           /* width 3: (u0, u1, u2) of surface sample `ray` (not a pnr_rng_fill stream) */
#define PNR_MESH_SCAN_CHUNK 256  /* faces per chunk and chunks per group of the CDF */
#define PNR_NEAREST_QUERIES 1024 /* rows of a per workgroup (four per lane)          */
#define PNR_NEAREST_TILE 1024    /* rows of b in LDS at a time                       */
#define PNR_NEAREST_SLICE 4096   /* rows of b per workgroup                          */

/* Workspace bytes for a mesh of n_faces faces (the CDF, 8 bytes per face, and the group sums); 0 if
 * n_faces is outside 1 .. 2^31 - 1. */
size_t pnr_mesh_sample_workspace_bytes(int64_t n_faces);

/* n >= 1 samples of the mesh; n, n_verts <= 2^31 - 1.  workspace 16-byte aligned, total_area
 * 8-byte aligned. */
int pnr_mesh_sample(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int64_t n,
                    uint64_t seed, void *workspace, size_t workspace_bytes, float *points, float *normals,
                    int32_t *tri, double *total_area, pnr_stream_t stream);

/* Workspace bytes of pnr_nearest (the per-slice minima; 256 unused bytes where b is one slice); 0
 * for any sizes pnr_nearest would refuse. */
size_t pnr_nearest_workspace_bytes(int64_t n, int64_t m);

/* d2 (n) fp32, idx (n) int32.  Stream-ordered, no host sync. */
int pnr_nearest(const float *a, int64_t n, const float *b, int64_t m, void *workspace, size_t workspace_bytes,
                float *d2, int32_t *idx, pnr_stream_t stream);

/* out: 8 x FLOAT64 on the device, 8-byte aligned.  n, m in 1 .. 2^31 - 1; tau >= 0. */
int pnr_mesh_distance_reduce(const float *d2_ab, const int32_t *idx_ab, int64_t n, const float *d2_ba,
                             const int32_t *idx_ba, int64_t m, const float *normals_a, const float *normals_b,
                             double tau, double *out, pnr_stream_t stream);

/* ---- Mesh containment (winding number, box samples; additive in ABI 8) ------------------------
 * The reference has no counterpart.  Occupancy Networks' third headline score, volumetric IoU, needs
 * a point-in-mesh test; its own is a compiled ray caster.  Here containment is the generalized
 * winding number of the indexed mesh pnr_mc_emit leaves on the device: verts (n_verts, 3) fp32,
 * faces (n_faces, 3) int32, points (n, 3) fp32 -> w (n) FLOAT64.
 *
 * Winding number (pnr_winding): w[i] = (sum over faces t of Omega(t, p_i)) / (4 pi).
 *   Pair      face t = (A, B, C), query p, all in fp32, u . v = fma(u.z, v.z, fma(u.y, v.y, u.x * v.x)):
 *               a = A - p, b = B - p, c = C - p           each difference rounded once
 *               la = sqrt(a . a), lb = sqrt(b . b), lc = sqrt(c . c)   correctly rounded roots
 *               n = b x c: n.x = b.y * c.z - b.z * c.y, ...  two rounded products and one rounded
 *                          difference per component, NO fma: b == c gives n == 0 exactly
 *               num = a . n
 *               den = fma(c . a, lb, fma(b . c, la, fma(a . b, lc, (la * lb) * lc)))
 *               Omega = 2 * atan2f(num, den); num == 0 and den == 0 (p on a vertex) gives Omega = 0
 *             (van Oosterom & Strackee 1983).  atan2f is the device math library's, within a few
 *             ulp; everything else is fixed to the bit.
 *   Sum       (double)Omega is added in fp64 from 0 in ascending face order within a slice of
 *             PNR_WINDING_SLICE faces; the per-slice sums (the workspace) are added in ascending
 *             slice order from slice 0's; the total is divided once by 4 pi (fp64).  No atomics:
 *             w[i] depends on (p_i, the mesh) only, not on n, the row's position or the run.
 *   Sign      a closed mesh whose normals point outward by the right-hand rule (pnr_mc_emit's
 *             orientation for density blobs: towards lower density) gives w = 1 inside, 0 outside.
 *   Indices   a face with an index outside [0, n_verts) contributes exactly 0 and its vertices are
 *             never read (pnr_mesh_distance_reduce's convention).  It keeps its place in its slice,
 *             so w equals, bit for bit, that of the mesh with (0, 0, 0)-indexed faces in their
 *             places, and that of the mesh without them where it fits one slice or they come last.
 *   NaN       a query or a vertex with a NaN or infinite coordinate counts as NaN: the w of that
 *             query, or of every query if a used vertex (one of a face with good indices), is NaN.
 *   Tiling    a workgroup scores PNR_WINDING_QUERIES queries (two per lane) against one slice,
 *             staged PNR_WINDING_TILE faces at a time; a partial tile is padded with the triangle
 *             (0, 0, 0), (0, 0, 0), (0, 0, 0), which contributes exactly 0 like a bad face.
 *   Limits    n, n_verts <= 2^31 - 1, n_faces <= min(2^31 - 1, 65535 * PNR_WINDING_SLICE) (larger:
 *             PNR_ERR_UNSUPPORTED).  No host sync, nothing allocated.
 *
 * Box samples (pnr_box_sample): points (n, 3) uniform in [lo, hi].  Sample s uses u_k = draw k of
 * ray s of the counter-mode stream PNR_RNG_VOLUME with width 3, offset 0 and key = seed (pnr_rng
 * above); coordinate k = fma(u_k, fl(hi_k - lo_k), lo_k), within [lo_k, hi_k].  A sample depends on
 * (seed, s) only.  lo and hi are HOST arrays of 3, read during the call. */
#define PNR_RNG_VOLUME 5          /* width 3: (u0, u1, u2) of box sample `ray` (not a pnr_rng_fill stream) */
#define PNR_WINDING_QUERIES 512   /* queries per workgroup (two per lane)  */
#define PNR_WINDING_TILE 512      /* faces in LDS at a time                */
#define PNR_WINDING_SLICE 4096    /* faces per workgroup                   */

/* Workspace bytes of pnr_winding (the per-slice sums, 8 bytes each; 256 unused bytes where the mesh
 * is one slice); 0 for any sizes pnr_winding would refuse. */
size_t pnr_winding_workspace_bytes(int64_t n, int64_t n_faces);

/* w (n) FLOAT64, 8-byte aligned like the workspace.  Stream-ordered, no host sync. */
int pnr_winding(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *points,
                int64_t n, void *workspace, size_t workspace_bytes, double *w, pnr_stream_t stream);

/* n in 1 .. 2^31 - 1; lo, hi finite with lo_k <= hi_k (else PNR_ERR_INVALID). */
int pnr_box_sample(const float *lo, const float *hi, int64_t n, uint64_t seed, float *points, pnr_stream_t stream);

/* ---- Mesh cleanup (weld, connected components, per-component sums; additive in ABI 8) ----------
 * The reference has no counterpart; the usual host route is trimesh's split.  A density mesh carries
 * floaters, and one stray blob rescales a mesh that is normalised by its bounds before it is scored:
 * these three steps find the components of the mesh pnr_mc_emit leaves on the device (or of an STL
 * soup, once welded) so that the caller can keep the large ones.  All indices are int32.
 *
 * Weld (pnr_mesh_weld): verts (n_verts, 3) fp32 -> remap (n_verts) int32.
 *   Equality  two vertices are equal when their three coordinates compare equal as floats: -0.0
 *             equals +0.0, and a vertex with a NaN coordinate equals nothing, itself included.
 *   Result    remap[i] = the LOWEST j whose vertex equals vertex i; remap[i] = i for a NaN vertex.
 *             remap[remap[i]] == remap[i].  A function of verts alone: each class settles at its
 *             minimum whatever the order its members arrive in (integer atomicCAS / atomicMin on a
 *             hash table in the workspace; csrc/meshclean.hip).
 *   Limits    n_verts in 1 .. 2^29 (larger: PNR_ERR_UNSUPPORTED).  No host sync.
 *
 * Components (pnr_mesh_components): faces (n_faces, 3) int32 over n_verts vertices -> vert_label
 * (n_verts) int32, face_label (n_faces) int32.
 *   Connected two vertices are connected when a face names both; components are the classes of the
 *             transitive closure.  A vertex that no face names is a component of its own.
 *   Labels    vert_label[v] = the lowest vertex index of v's component; face_label[t] = the label of
 *             face t's vertices.  n_faces = 0 is allowed (faces and face_label may then be NULL).
 *   Indices   a face with an index outside [0, n_verts) is never read through; it sets a flag, its
 *             face_label is -1 and the call returns PNR_ERR_INVALID.
 *   Schedule  lock-free union-find with min-hooking in ONE pass over the faces, then one flatten
 *             pass: *launches (HOST memory, may be NULL) receives the number of kernel launches the
 *             call took (3; 2 without faces).  No fixed-point iteration, so no round ceiling.  The
 *             call waits for its stream once to read the index flag, as pnr_mesh_sample does.
 *   Limits    n_verts in 1 .. 2^31 - 1, n_faces in 0 .. 2^31 - 1.
 *
 * Sums (pnr_mesh_component_sums): per component its area and signed volume, out (n_components, 2)
 * FLOAT64 = {area, signed volume}.
 *   Input     order (n_faces) int64: the face indices grouped by component, ascending within a
 *             component (a stable sort of the faces by component id); seg_start (n_components + 1)
 *             int64: component c owns order[seg_start[c] .. seg_start[c + 1]).
 *   Terms     per face (a, b, c), in fp64 from the fp32 vertices, every operation rounded once:
 *             area = 0.5 * sqrt((nx nx + ny ny) + nz nz), n = (b - a) x (c - a) with
 *             n.x = u.y w.z - u.z w.y, ...; volume term = (a.x m.x + a.y m.y) + a.z m.z, m = b x c.
 *             A face (or an entry of order) with an index out of range contributes 0.
 *   Order     with B = 1024: position k of the component's run is added by thread k mod B, each
 *             thread in ascending k from 0; the 64 threads of a wave are folded by a butterfly
 *             (xor 32, 16, .. 1) and the 16 waves added in ascending order from wave 0's; the volume
 *             sum is divided once by 6.  A function of the component's own face sequence: bit-identical
 *             from run to run and whether the mesh is processed alone or inside a larger one.
 *   No atomics, no workspace, no host sync. */
#define PNR_MESH_CLEAN_BLOCK 256 /* threads (vertices or faces) per workgroup of the weld / component kernels */

/* Workspace bytes of pnr_mesh_weld (the table: 4 bytes x the power of two >= 2 n_verts, at least
 * 256 slots); 0 if n_verts is outside 1 .. 2^29. */
size_t pnr_mesh_weld_workspace_bytes(int64_t n_verts);

int pnr_mesh_weld(const float *verts, int64_t n_verts, void *workspace, size_t workspace_bytes, int32_t *remap,
                  pnr_stream_t stream);

/* Workspace bytes of pnr_mesh_components (the flag and one parent per vertex); 0 for sizes it refuses. */
size_t pnr_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces);

int pnr_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_verts, void *workspace,
                        size_t workspace_bytes, int32_t *vert_label, int32_t *face_label, int32_t *launches,
                        pnr_stream_t stream);

/* n_verts, n_faces, n_components in 1 .. 2^31 - 1; out 8-byte aligned. */
int pnr_mesh_component_sums(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                            const int64_t *order, const int64_t *seg_start, int64_t n_components, double *out,
                            pnr_stream_t stream);

/* ---- Mesh rendering (depth, silhouette and shaded views; additive in ABI 8) ---------------------
 * The reference renders its training views of STL meshes with Blender scripts (headless_Blender.py,
 * Blender_cli.py, newBlender.py); nothing of it runs on a device.  These calls render an indexed
 * triangle mesh, verts (n_verts, 3) fp32 and faces (n_faces, 3) int32, from nv cameras at once:
 * poses (nv, pose_rows, 4) fp32 with pose_rows 3 or 4, camera-to-world, x right, y up, the camera
 * looking down -z (what pnr_gen_rays takes), and the host scalars w, h, fx, fy, cx, cy.
 *
 * Raster (pnr_mesh_raster): face (nv, h, w) int32, depth (nv, h, w) fp32.
 *   Pixel     pixel (row j, column i) of view v is ray [v, j, i] of pnr_gen_rays: origin o = pose[:3, 3],
 *             direction R u / |u| with u = (X, -Y, -1), X = fl(fl(i - cx) / fx), Y = fl(fl(j - cy) / fy),
 *             |u| = sqrt(fl(fl(X X + Y Y) + 1)); integer pixel coordinates, no + 0.5.
 *   Output    face = the nearest face the ray hits with t > 0, -1 where it hits none; depth = the
 *             distance t along the UNIT direction (the quantity pnr_composite's depth is in), 0
 *             where face is -1.
 *   Camera    a vertex p goes to camera space as q = R^T (p - o): the three differences rounded
 *             once, q_k = fma(R[2][k], d.z, fma(R[1][k], d.y, R[0][k] * d.x)).  R is taken for a
 *             rotation: its transpose stands for its inverse, so an fp32 R that is orthonormal to
 *             one rounding moves the depth by a few 1e-7 relative against the exact ray.
 *   Edge      the edge p -> q of a face has the normal n = +-(lo x e), e = hi - lo (rounded once),
 *             n.x = lo.y e.z - lo.z e.y, ... (two rounded products and one rounded difference, NO
 *             fma), where lo is the endpoint whose WORLD coordinates come first in (x, y, z)
 *             order and the sign is - when that is q.  The order is a rule of the endpoints alone,
 *             so the face on the other side of the edge, in a welded mesh or an STL soup alike,
 *             forms the same three floats and the opposite sign.
 *   Hit       in homogeneous form, nothing is clipped.  E_k = fma(n_k.x, X, fma(n_k.y, -Y, -n_k.z))
 *             for the edges ab, bc, ca (the signed volume u . (p x q); exactly opposite for the
 *             two faces of an edge).  The ray hits the face when no two E_k have strictly opposite
 *             signs (edges and vertices are included), det = (E_ab + E_bc) + E_ca is not 0 (the
 *             face is not edge-on) and s = -(fma(E_ca, b.z, fma(E_bc, a.z, E_ab * c.z)) / det), the
 *             camera-z depth of the hit point, is positive and finite.  Both orientations count.
 *             A ray through a shared edge or vertex therefore hits at least one of the faces.  A
 *             face that straddles the camera plane needs no special case.
 *   Nearest   the smallest s wins, as computed in fp32; equal s go to the lower face index.
 *             depth = s * |u|, rounded once.
 *   Bad input a face with an index outside [0, n_verts), with a non-finite vertex or with zero area
 *             (the unfused cross product of its two world edges is (0, 0, 0)) contributes nothing and
 *             its vertices are never read through the bad index; a pose with a non-finite entry in
 *             its first three rows makes that view all -1 / 0.
 *   Result    a function of the inputs only: bit-identical from run to run, for a view alone or in
 *             a batch, and with faces appended that cover no pixel; depth and face >= 0 are
 *             bit-identical under any permutation of the faces.
 *   Schedule  one lane per (view, face) computes the camera-space vertices, the edge normals and
 *             the pixel bounds of the projected vertices (the whole image when a vertex is at or
 *             behind the camera plane).  Bounds of at most PNR_RASTER_SMALL_PIXELS pixels are
 *             scanned by the lane itself; larger faces are taken by the whole wave, PNR_RASTER_TILE
 *             x PNR_RASTER_TILE pixels a step.  Both run the same arithmetic per (pixel, face).  The
 *             workspace holds one 64-bit key (bits of s << 32 | face) per pixel, taken to its
 *             minimum with an integer atomic; no float atomics.  pnr_mesh_raster_set_small moves
 *             the threshold between the two paths for measurements (the result does not change).
 *   Limits    w, h in 1 .. 8192; nv h w, n_faces and n_verts in 1 .. 2^31 - 1 (else the workspace
 *             size is 0 and the call returns PNR_ERR_UNSUPPORTED).  No host sync, nothing allocated.
 *
 * Shading (pnr_mesh_shade): rgb (nv, h, w, 3) fp32, channels last, and optionally normal (nv, h, w, 3),
 * from the face and depth of pnr_mesh_raster.  n = the unit normal (b - a) x (c - a) of the face,
 * negated where n . d > 0 for the pixel's unit direction d (turned towards the camera, two-sided);
 * p = o + depth d; rgb = clamp(albedo * (ambient + sum_l k_l max(0, n . unit(L_l - p))), 0, 254/255), so
 * no object pixel is the 255-white a loader reads as background.  Up to PNR_RASTER_MAX_LIGHTS point
 * lights: lights (n_lights, 3) world positions and weights (n_lights) are HOST arrays, as are albedo
 * (3) and background (3), read during the call.  A pixel whose face is outside [0, n_faces) gets the
 * background triple and the normal (0, 0, 0). */
#define PNR_RASTER_BLOCK 256        /* (view, face) lanes per workgroup of the coverage kernel */
#define PNR_RASTER_TILE 8           /* the wave tests TILE x TILE pixels of a large face a step */
#define PNR_RASTER_SMALL_PIXELS 8   /* bounds of at most this many pixels are scanned by one lane */
#define PNR_RASTER_MAX_LIGHTS 8

/* Workspace bytes of pnr_mesh_raster (the keys, 8 bytes per pixel); 0 for an unsupported shape. */
size_t pnr_mesh_raster_workspace_bytes(int64_t nv, int32_t h, int32_t w, int64_t n_faces);

/* workspace 8-byte aligned.  Stream-ordered, no host sync. */
int pnr_mesh_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                    int64_t nv, int32_t pose_rows, int32_t w, int32_t h, float fx, float fy, float cx, float cy,
                    void *workspace, size_t workspace_bytes, int32_t *face_out, float *depth_out,
                    pnr_stream_t stream);

/* The largest pixel count a lane scans on its own (default PNR_RASTER_SMALL_PIXELS; negative restores
 * it); returns the previous value.  Process-wide, for measurements: outputs do not depend on it. */
int pnr_mesh_raster_set_small(int32_t pixels);

/* normal may be NULL.  lights / weights may be NULL when n_lights is 0. */
int pnr_mesh_shade(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                   int64_t nv, int32_t pose_rows, int32_t w, int32_t h, float fx, float fy, float cx, float cy,
                   const int32_t *face, const float *depth, const float *lights, const float *weights,
                   int32_t n_lights, const float *albedo, float ambient, const float *background, float *rgb,
                   float *normal, pnr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PNR_ABI_H */
