// Host launchers and size helpers behind the C ABI (abi.cpp), each declared once with its default
// arguments.  Every .hip file that defines one includes this header, so a definition that drifts
// from its declaration fails to compile.
#pragma once
#include "pnr_common.h"

namespace pnr {

struct MarchCfg;   // march_dev.h

// march.hip
int launch_sample_coarse(const float *, int64_t, int, const RngSrc &, int, float *, hipStream_t);
int launch_sample_fine(const float *, int64_t, int, const float *, const float *, const float *,
                       int, int, float, const RngSrc &, const RngSrc &, const RngSrc &, int, float *,
                       hipStream_t, int *origin = nullptr, float *z_new = nullptr);
int launch_rng_fill(const RngSrc &, int64_t, int, float *, hipStream_t);
int launch_merge_raw(const int *, const float *, const float *, int64_t, int, int, float *, hipStream_t);
int launch_gen_rays(const float *, int64_t, int, int, int, float, float, float, float, float, float,
                    float *, hipStream_t);
int launch_composite(const float *, const float *, const float *, int64_t, int, int, float *,
                     float *, float *, hipStream_t);
int sort_width(int n);
// mlp_pack.hip
size_t mlp_packed_bytes(const pnr_mlp_desc &);
int mlp_check_desc(const pnr_mlp_desc &);
int mlp_pack(const pnr_mlp_weights &, void *, size_t, hipStream_t);
size_t mlp_packed_t_bytes(const pnr_mlp_desc &);
int mlp_pack_t(const pnr_mlp_weights &, const void *, void *, size_t, hipStream_t);
// mlp.hip
size_t mlp_xsum_bytes(int ns);
int64_t mlp_save_floats(const pnr_mlp_desc &d, int64_t n_points);
int launch_point_mlp(const pnr_scene &, const pnr_mlp_desc &, const void *, const float *,
                     const float *, int, int64_t, const float *, const float *, int64_t, int64_t,
                     float *, float *, hipStream_t, float *save = nullptr, const float *proj = nullptr,
                     const MarchCfg *march = nullptr);
int mlp_set_lean(int on);   // the lean instantiation's process-wide switch (returns the previous setting)
int mlp_last_kernel();      // PNR_MLP_KERNEL_* of the last launch_point_mlp
// mlp_bwd.hip
int launch_mlp_bwd(const pnr_mlp_desc &, const void *, const void *, const float *, const float *, const float *,
                   int64_t, float *, float *, hipStream_t, float *, void *, size_t, int n_views);
size_t mlp_bwd_workspace_bytes(const pnr_mlp_desc &, int64_t);
// wgrad.hip
size_t wgrad_workspace_bytes(int, int64_t);
int launch_wgrad(const float *const *, const float *const *, float *const *, int, int64_t, void *, size_t,
                 hipStream_t, int arith);
// encoder.hip
int launch_fold_bn(const pnr_bn_fold *, int, int64_t, hipStream_t);
int launch_latent_cl_bwd(const float *, float *const *, const int32_t *, const int32_t *, const int32_t *, int, int, int,
                         int, hipStream_t);
int launch_latent_cl(const float *const *, const int32_t *, const int32_t *, const int32_t *, int, int, float *,
                     int, int, bool, hipStream_t);
// train.hip
int launch_composite_bwd(const float *, const float *, const float *, int64_t, int, int, const float *,
                         const float *, const float *, float *, float *, hipStream_t);
int launch_points_in_bwd(const float *, const float *, int, int64_t, int64_t, int, const float *, const float *,
                         int, int, float, float, const float *, int, const float *, const float *, float *,
                         float *, const uint8_t *, hipStream_t);
// proj.hip
int64_t latent_proj_floats(const pnr_scene &, const pnr_mlp_desc &);
int launch_latent_proj(const pnr_scene &, const pnr_mlp_weights &, float *, size_t, hipStream_t);
// mcubes.hip
size_t mc_workspace_bytes(int, int, int);
void mc_case_table(int8_t out[256][16]);
int launch_mc_count(const float *, int, int, int, float, void *, size_t, int64_t *, hipStream_t);
int launch_mc_emit(const float *, int, int, int, float, void *, size_t, float *, int64_t, int32_t *, int64_t,
                   hipStream_t);
// metrics.hip
size_t image_metrics_workspace_bytes(int64_t, int, int, int);
int launch_image_metrics(const float *, const float *, int64_t, int, int, int, float, float, float, void *, size_t,
                         double *, hipStream_t);
// meshdist.hip
size_t mesh_sample_workspace_bytes(int64_t);
int launch_mesh_sample(const float *, int64_t, const int32_t *, int64_t, int64_t, uint64_t, void *, size_t, float *,
                       float *, int32_t *, double *, hipStream_t);
size_t nearest_workspace_bytes(int64_t, int64_t);
int launch_nearest(const float *, int64_t, const float *, int64_t, void *, size_t, float *, int32_t *, hipStream_t);
int launch_mesh_distance_reduce(const float *, const int32_t *, int64_t, const float *, const int32_t *, int64_t,
                                const float *, const float *, double, double *, hipStream_t);
// winding.hip
size_t winding_workspace_bytes(int64_t, int64_t);
int launch_winding(const float *, int64_t, const int32_t *, int64_t, const float *, int64_t, void *, size_t, double *,
                   hipStream_t);
int launch_box_sample(const float[3], const float[3], int64_t, uint64_t, float *, hipStream_t);   // lo, extent

}  // namespace pnr
