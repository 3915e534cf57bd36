// Host launchers and size helpers behind the C ABI (abi.cpp), each declared once with the parameter
// names of its definition.  Every .hip file that defines one includes this header, so a definition
// whose types drift from its declaration fails to compile.  A launcher with many buffers takes them
// as a struct of named fields (FineSampleCall, CompositeCall and CompositeBwdCall for the ray march,
// PointMlpCall for the fused MLP's forward, MlpBwdCall for its training backward); the stream is
// every launcher's last parameter.  launch_flat is the one spelling of a flat launch.
#pragma once
#include "pnr_common.h"

namespace pnr {

struct MarchCfg;   // march_dev.h

// workgroups of `threads` that cover n elements
inline unsigned blocks(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// A flat launch: nothing when n == 0, else the workgroups of `threads` that cover n items at `per_block`
// items each, `lds` bytes of dynamic LDS, and the launch status as a PNR_* code.
template <typename Kernel, typename... Args>
inline int launch_flat(const char *what, Kernel kern, int64_t n, int per_block, int threads, size_t lds,
                       hipStream_t st, Args... args) {
    if (n == 0) return PNR_OK;
    hipLaunchKernelGGL(kern, dim3(blocks((size_t)n, per_block)), dim3(threads), lds, st, args...);
    return launch_ok(what) ? PNR_OK : PNR_ERR_HIP;
}

// march.hip
int launch_sample_coarse(const float *rays, int64_t n_rays, int kc, const RngSrc &u, int lindisp, float *z,
                         hipStream_t st);
// sample_fine + sample_fine_depth + sort of n_rays rays: kc coarse samples in, kc + kf sorted depths out
struct FineSampleCall {
    const float *rays = nullptr;       // (n_rays, 8)
    int64_t n_rays = 0;
    int kc = 0;
    const float *z_coarse = nullptr;   // (n_rays, kc)
    const float *weights = nullptr;    // (n_rays, kc) coarse weights
    const float *depth = nullptr;      // (n_rays) coarse depth (read when kfd > 0)
    int kf = 0, kfd = 0;               // new samples, and how many of them are depth samples
    float depth_std = 0.f;
    RngSrc u_fine{}, u_jit{}, n_depth{};
    int lindisp = 0;
    float *z_fine = nullptr;           // (n_rays, kc + kf), sorted
    int *origin = nullptr;             // NULL, or (n_rays, kc + kf): each value's index in cat(coarse, new)
    float *z_new = nullptr;            // with origin: (n_rays, kf), the new samples in draw order
};
int launch_sample_fine(const FineSampleCall &c, hipStream_t st);
// the alpha composite of n_rays rays x K samples
struct CompositeCall {
    const float *z = nullptr;          // (n_rays, K)
    const float *raw = nullptr;        // (n_rays, K, 4) rgb, sigma
    const float *rays = nullptr;       // (n_rays, 8)
    int64_t n_rays = 0;
    int K = 0;
    int white_bkgd = 0;
    float *weights = nullptr;          // (n_rays, K), or NULL
    float *rgb = nullptr;              // (n_rays, 3)
    float *depth = nullptr;            // (n_rays)
};
int launch_composite(const CompositeCall &c, hipStream_t st);
int launch_rng_fill(const RngSrc &r, int64_t n_rays, int width, float *out, hipStream_t st);
int launch_merge_raw(const int *origin, const float *raw_c, const float *raw_new, int64_t n_rays, int kc, int kf,
                     float *raw_f, hipStream_t st);
int launch_gen_rays(const float *poses, int64_t n_images, int pose_rows, int width, int height, float fx, float fy,
                    float cx, float cy, float near, float far, float *rays, hipStream_t st);
int sort_width(int n);
// mlp_pack.hip
size_t mlp_packed_bytes(const pnr_mlp_desc &d);
int mlp_check_desc(const pnr_mlp_desc &d);
int mlp_pack(const pnr_mlp_weights &w, void *packed, size_t bytes, hipStream_t st);
size_t mlp_packed_t_bytes(const pnr_mlp_desc &d);
int mlp_pack_t(const pnr_mlp_weights &w, const void *packed, void *packed_t, size_t bytes, hipStream_t st);
// mlp.hip
size_t mlp_xsum_bytes(int ns);
int64_t mlp_save_floats(const pnr_mlp_desc &d, int64_t n_points);
// One launch of the fused point model: n_points points drawn from EITHER the render source (point
// p is sample p % K of ray p / K) OR the query source (explicit positions).
struct PointMlpCall {
    const void *packed = nullptr;      // packed weights (pnr_mlp_pack)
    const float *proj = nullptr;       // projected latent (pnr_latent_project), or NULL: the latent gather path
    // render source
    const float *rays = nullptr;       // (n_rays, 8); non-NULL selects render mode
    const float *z = nullptr;          // (n_rays, K) depths (drawn by the kernel itself under `march`)
    int K = 0;
    int64_t rays_per_obj = 1;
    // query source
    const float *xyz = nullptr;        // (n_points, 3)
    const float *dirs = nullptr;       // (n_points, 3) or NULL
    int64_t points_per_obj = 1;
    int64_t n_points = 0;
    float *out = nullptr;              // (n_points, 4) raw outputs, or NULL (a fused march composites them)
    float *save = nullptr;             // activation save of the training forward, or NULL
    const MarchCfg *march = nullptr;   // fused ray march in the kernel's prologue / epilogue, or NULL
    float *xsum = nullptr;             // workspace of mlp_xsum_bytes()
};
int launch_point_mlp(const pnr_scene &sc, const pnr_mlp_desc &d, const PointMlpCall &c, hipStream_t st);
int mlp_set_lean(int on);   // the lean instantiation's process-wide switch (returns the previous setting)
int mlp_last_kernel();      // PNR_MLP_KERNEL_* of the last launch_point_mlp
// mlp_bwd.hip
// One launch of the fused f16x3 backward chain over n_points points with n_views source views.
struct MlpBwdCall {
    const void *packed = nullptr;      // forward pack (header: weight scale exponents)
    const void *packed_t = nullptr;    // k_pack_f16_t output (pnr_mlp_pack_t)
    const float *w_out = nullptr;      // lin_out weight (4 x 512, fp32)
    const float *save = nullptr;       // forward activation save
    const float *d_o = nullptr;        // (n_points, 4) gradient of the pre-head output
    int64_t n_points = 0;
    int n_views = 1;                   // source views per point (the save's view rows)
    float *dy = nullptr;               // (2 nb + 1) x (n_views n_points) x 512 output gradients per layer
    float *dzlat = nullptr;            // (n_views n_points, 512) gradient of the sampled latent (n_linz > 0)
    float *d_bias = nullptr;           // NULL, or (2 nb + 1) x 512 column sums of each dy slot
    void *ws = nullptr;                // workspace of mlp_bwd_workspace_bytes() (d_bias only)
    size_t ws_bytes = 0;
};
int launch_mlp_bwd(const pnr_mlp_desc &d, const MlpBwdCall &c, hipStream_t st);
size_t mlp_bwd_workspace_bytes(const pnr_mlp_desc &d, int64_t n_points);
// wgrad.hip
size_t wgrad_workspace_bytes(int n_jobs, int64_t n_points);
int launch_wgrad(const float *const *dy, const float *const *x, float *const *g, int n_jobs, int64_t n_points,
                 void *ws, size_t ws_bytes, int arith, hipStream_t st);
// encoder.hip
int launch_fold_bn(const pnr_bn_fold *folds, int n_folds, int64_t max_elems, hipStream_t st);
int launch_latent_cl_bwd(const float *g, float *const *d_maps, const int32_t *channels, const int32_t *heights,
                         const int32_t *widths, int n_maps, int n_images, int out_h, int out_w, hipStream_t st);
int launch_latent_cl(const float *const *maps, const int32_t *channels, const int32_t *heights,
                     const int32_t *widths, int n_maps, int n_images, float *latent_cl, int out_h, int out_w,
                     bool nhwc, hipStream_t st);
// train.hip
// the composite's backward (K <= 256): the forward's inputs, the output gradients, the input gradients
struct CompositeBwdCall {
    const float *z = nullptr, *raw = nullptr, *rays = nullptr;   // as CompositeCall
    int64_t n_rays = 0;
    int K = 0;
    int white_bkgd = 0;
    const float *d_rgb = nullptr;      // (n_rays, 3)
    const float *d_depth = nullptr;    // (n_rays), or NULL
    const float *d_weights = nullptr;  // (n_rays, K), or NULL
    float *d_raw = nullptr;            // (n_rays, K, 4)
    float *d_z = nullptr;              // (n_rays, K), or NULL
};
int launch_composite_bwd(const CompositeBwdCall &c, hipStream_t st);
int launch_points_in_bwd(const pnr_scene &sc, const pnr_rays &rays, const float *zs, int K, const float *pe,
                         int pe_n, const float *d_feat, const float *d_zlat, float *d_latent, float *d_z,
                         const uint8_t *z_mask, hipStream_t st);
// proj.hip
int64_t latent_proj_floats(const pnr_scene &sc, const pnr_mlp_desc &d);
int launch_latent_proj(const pnr_scene &sc, const pnr_mlp_weights &w, float *proj, size_t bytes, hipStream_t st);
// mcubes.hip
size_t mc_workspace_bytes(int nx, int ny, int nz);
void mc_case_table(int8_t out[256][16]);
int launch_mc_count(const float *grid, int nx, int ny, int nz, float level, void *ws, size_t bytes,
                    int64_t *counts_dev, hipStream_t st);
int launch_mc_emit(const float *grid, int nx, int ny, int nz, float level, void *ws, size_t bytes, float *verts,
                   int64_t verts_cap, int32_t *faces, int64_t faces_cap, hipStream_t st);
// metrics.hip
size_t image_metrics_workspace_bytes(int64_t n, int h, int w, int c);
int launch_image_metrics(const float *x, const float *y, int64_t n, int h, int w, int c, float data_range, float k1,
                         float k2, void *ws, size_t ws_bytes, double *out, hipStream_t st);
// meshdist.hip
size_t mesh_sample_workspace_bytes(int64_t n_faces);
int launch_mesh_sample(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int64_t n,
                       uint64_t seed, void *ws, size_t bytes, float *points, float *normals, int32_t *tri,
                       double *total_area, hipStream_t st);
size_t nearest_workspace_bytes(int64_t n, int64_t m);
int launch_nearest(const float *a, int64_t n, const float *b, int64_t m, void *ws, size_t bytes, float *d2,
                   int32_t *idx, hipStream_t st);
int launch_mesh_distance_reduce(const float *d2_ab, const int32_t *idx_ab, int64_t n, const float *d2_ba,
                                const int32_t *idx_ba, int64_t m, const float *normals_a, const float *normals_b,
                                double tau, double *out, hipStream_t st);
// winding.hip
size_t winding_workspace_bytes(int64_t n, int64_t n_faces);
int launch_winding(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *points,
                   int64_t n, void *ws, size_t bytes, double *w, hipStream_t st);
int launch_box_sample(const float lo[3], const float ext[3], int64_t n, uint64_t seed, float *points, hipStream_t st);
// meshclean.hip
size_t mesh_weld_workspace_bytes(int64_t n_verts);
int launch_mesh_weld(const float *verts, int64_t n_verts, void *ws, size_t bytes, int32_t *remap, hipStream_t st);
size_t mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces);
int launch_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_verts, void *ws, size_t bytes,
                           int32_t *vert_label, int32_t *face_label, int32_t *launches, hipStream_t st);
int launch_mesh_component_sums(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                               const int64_t *order, const int64_t *seg_start, int64_t n_components, double *out,
                               hipStream_t st);
// meshraster.hip (small_max < 0: PNR_RASTER_SMALL_PIXELS)
size_t mesh_raster_workspace_bytes(int64_t nv, int h, int w, int64_t n_faces);
int launch_mesh_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                       int64_t nv, int pose_rows, int w, int h, float fx, float fy, float cx, float cy, void *ws,
                       size_t bytes, int32_t *face_out, float *depth_out, int small_max, hipStream_t st);
int launch_mesh_shade(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                      int64_t nv, int pose_rows, int w, int h, float fx, float fy, float cx, float cy,
                      const int32_t *face_in, const float *depth_in, const float *lights, const float *weights,
                      int n_lights, const float albedo[3], float ambient, const float background[3], float *rgb,
                      float *normal, hipStream_t st);

}  // namespace pnr
