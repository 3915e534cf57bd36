// extern "C" entry points of libpnr.so (declared in include/pnr_abi.h):
// argument validation, workspace carving and the stream-ordered launch
// sequence of the coarse + fine ray march.  No allocation, no host sync (three calls wait for
// their stream: pnr_mc_emit, where mcubes.hip reads the counted totals back to check the
// capacities, pnr_mesh_sample, where meshdist.hip reads its index flag and the total area, and
// pnr_mesh_components, where meshclean.hip reads its index flag).
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "march_dev.h"
#include "pnr_launch.h"

namespace pnr {

static thread_local char g_err[1024];
// pnr_render_set_fused: the DEFAULT march mode of calls whose pnr_render_cfg.march_mode is -1:
// the fused ray march (2: draws + composite in the MLP passes, the fine draws in their own
// kernel; 1: those too in the coarse epilogue) or the separate sample / composite kernels (0).
// Set once at start-up by callers that want another default; a call naming its own mode never
// reads it.
static std::atomic<int> g_fused_default{2};
// pnr_mesh_raster_set_small: the largest pixel count one lane scans (-1: PNR_RASTER_SMALL_PIXELS)
static std::atomic<int> g_raster_small{-1};

int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return status;
}

int device_cu_count() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// PNR_ERR_WORKSPACE if the call `who` needs `need` bytes and the caller's workspace is absent or smaller
static int check_workspace(const char *who, const void *workspace, size_t workspace_bytes, size_t need) {
    if (need && (!workspace || workspace_bytes < need))
        return fail(PNR_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    return PNR_OK;
}

static int check_scene(const pnr_scene *sc) {
    if (!sc) return fail(PNR_ERR_INVALID, "scene is NULL");
    if (!sc->latent || !sc->cams) return fail(PNR_ERR_INVALID, "scene latent/cams NULL");
    if (sc->n_obj < 1 || sc->n_views < 1) return fail(PNR_ERR_INVALID, "n_obj/n_views < 1");
    if (sc->latent_h < 2 || sc->latent_w < 2)
        return fail(PNR_ERR_INVALID, "latent must be at least 2x2 (align_corners scaling)");
    if (sc->latent_c != 512) return fail(PNR_ERR_UNSUPPORTED, "latent_c must be 512 (got %d)", sc->latent_c);
    if (!(sc->image_w > 0.f) || !(sc->image_h > 0.f)) return fail(PNR_ERR_INVALID, "image size <= 0");
    if (misaligned(15, sc->latent)) return fail(PNR_ERR_INVALID, "latent must be 16-byte aligned");
    if ((int64_t)sc->n_obj * sc->n_views * sc->latent_h * sc->latent_w * sc->latent_c >= (1ll << 32))
        return fail(PNR_ERR_UNSUPPORTED, "latent larger than 2^32 floats (32-bit gather offsets)");
    return PNR_OK;
}

static int check_desc_for_scene(const pnr_mlp_desc *d, const pnr_scene *sc) {
    if (!d) return fail(PNR_ERR_INVALID, "mlp desc is NULL");
    int rc = mlp_check_desc(*d);
    if (rc) return rc;
    if (sc->n_views > 1 && d->combine_layer >= d->n_blocks)
        return fail(PNR_ERR_UNSUPPORTED, "n_views > 1 needs combine_layer < n_blocks");
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_abi_version(void) { return PNR_ABI_VERSION; }

const char *pnr_last_error(void) { return g_err; }

size_t pnr_mlp_packed_bytes(const pnr_mlp_desc *desc) {
    if (!desc || mlp_check_desc(*desc) != PNR_OK) return 0;
    return mlp_packed_bytes(*desc);
}

int pnr_mlp_pack(const pnr_mlp_weights *w, void *packed, size_t packed_bytes, pnr_stream_t stream) {
    if (!w || !packed) return fail(PNR_ERR_INVALID, "pnr_mlp_pack: NULL argument");
    return mlp_pack(*w, packed, packed_bytes, (hipStream_t)stream);
}

size_t pnr_point_query_workspace_bytes(const pnr_scene *scene, int64_t n_points) {
    (void)n_points;
    return scene ? align256(mlp_xsum_bytes(scene->n_views)) : 0;
}

int pnr_point_query(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                    const float *xyz, const float *viewdirs, int64_t points_per_obj, float *out,
                    void *workspace, size_t workspace_bytes, pnr_stream_t stream) {
    return pnr_point_query_proj(scene, desc, packed, nullptr, xyz, viewdirs, points_per_obj, out, workspace,
                                workspace_bytes, stream);
}

size_t pnr_latent_project_bytes(const pnr_scene *scene, const pnr_mlp_desc *desc) {
    if (!scene || !desc || check_scene(scene) != PNR_OK || mlp_check_desc(*desc) != PNR_OK) return 0;
    return sizeof(float) * (size_t)latent_proj_floats(*scene, *desc);
}

int pnr_latent_project(const pnr_scene *scene, const pnr_mlp_weights *w, float *proj, size_t proj_bytes,
                       pnr_stream_t stream) {
    int rc = check_scene(scene);
    if (rc) return rc;
    if (!w || !proj) return fail(PNR_ERR_INVALID, "pnr_latent_project: NULL argument");
    if ((rc = check_desc_for_scene(&w->desc, scene))) return rc;
    if (misaligned(15, proj)) return fail(PNR_ERR_INVALID, "pnr_latent_project: proj must be 16-byte aligned");
    return launch_latent_proj(*scene, *w, proj, proj_bytes, (hipStream_t)stream);
}

int pnr_point_query_proj(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                         const float *proj, const float *xyz, const float *viewdirs, int64_t points_per_obj,
                         float *out, void *workspace, size_t workspace_bytes, pnr_stream_t stream) {
    int rc = check_scene(scene);
    if (rc) return rc;
    if ((rc = check_desc_for_scene(desc, scene))) return rc;
    if (!packed || !xyz || !out) return fail(PNR_ERR_INVALID, "pnr_point_query: NULL pointer");
    if (points_per_obj < 0) return fail(PNR_ERR_INVALID, "points_per_obj < 0");
    const int64_t n_points = points_per_obj * scene->n_obj;
    if (n_points == 0) return PNR_OK;
    if ((rc = check_workspace("pnr_point_query", workspace, workspace_bytes,
                              pnr_point_query_workspace_bytes(scene, n_points))))
        return rc;
    if (misaligned(15, proj)) return fail(PNR_ERR_INVALID, "pnr_point_query_proj: proj must be 16-byte aligned");
    PointMlpCall c;
    c.packed = packed;
    c.proj = proj;
    c.xyz = xyz;
    c.dirs = viewdirs;
    c.points_per_obj = points_per_obj;
    c.n_points = n_points;
    c.out = out;
    c.xsum = static_cast<float *>(workspace);
    return launch_point_mlp(*scene, *desc, c, (hipStream_t)stream);
}

size_t pnr_point_save_floats(const pnr_mlp_desc *desc, int64_t n_points) {
    if (!desc || n_points < 0 || mlp_check_desc(*desc) != PNR_OK) return 0;
    return (size_t)mlp_save_floats(*desc, n_points);
}

static int check_rays_z(const pnr_scene *scene, const pnr_rays *rays, const float *z, int32_t k) {
    if (!rays || (rays->n_rays > 0 && (!rays->rays || !z))) return fail(PNR_ERR_INVALID, "rays / z NULL");
    if (rays->n_rays < 0 || k < 1) return fail(PNR_ERR_INVALID, "bad n_rays / k");
    if (rays->rays_per_obj < 1 || rays->n_rays != rays->rays_per_obj * scene->n_obj)
        return fail(PNR_ERR_INVALID, "n_rays must equal rays_per_obj * n_obj");
    return PNR_OK;
}

int pnr_render_points(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                      const pnr_rays *rays, const float *z, int32_t k, float *out, float *save,
                      void *workspace, size_t workspace_bytes, pnr_stream_t stream) {
    int rc = check_scene(scene);
    if (rc) return rc;
    if ((rc = check_desc_for_scene(desc, scene))) return rc;
    if ((rc = check_rays_z(scene, rays, z, k))) return rc;
    if (!packed || !out) return fail(PNR_ERR_INVALID, "pnr_render_points: NULL pointer");
    const int64_t n_points = rays->n_rays * k;
    if (n_points == 0) return PNR_OK;
    if ((rc = check_workspace("pnr_render_points", workspace, workspace_bytes,
                              pnr_point_query_workspace_bytes(scene, n_points))))
        return rc;
    PointMlpCall c;
    c.packed = packed;
    c.rays = rays->rays;
    c.z = z;
    c.K = k;
    c.rays_per_obj = rays->rays_per_obj;
    c.n_points = n_points;
    c.out = out;
    c.save = save;
    c.xsum = static_cast<float *>(workspace);
    return launch_point_mlp(*scene, *desc, c, (hipStream_t)stream);
}

int pnr_composite_backward(const float *z, const float *raw, const float *rays, int64_t n_rays, int32_t k,
                           int32_t white_bkgd, const float *d_rgb, const float *d_depth,
                           const float *d_weights, float *d_raw, float *d_z, pnr_stream_t stream) {
    if (n_rays < 0 || k < 1) return fail(PNR_ERR_INVALID, "pnr_composite_backward: bad sizes");
    if (k > 256) return fail(PNR_ERR_UNSUPPORTED, "pnr_composite_backward: k <= 256");
    if (n_rays == 0) return PNR_OK;
    if (!z || !raw || !rays || !d_rgb || !d_raw) return fail(PNR_ERR_INVALID, "pnr_composite_backward: NULL");
    if (misaligned(15, raw, d_raw)) return fail(PNR_ERR_INVALID, "raw / d_raw must be 16-byte aligned");
    CompositeBwdCall c;
    c.z = z; c.raw = raw; c.rays = rays; c.n_rays = n_rays; c.K = k; c.white_bkgd = white_bkgd; c.d_rgb = d_rgb;
    c.d_depth = d_depth; c.d_weights = d_weights; c.d_raw = d_raw; c.d_z = d_z;
    return launch_composite_bwd(c, (hipStream_t)stream);
}

int pnr_points_input_backward_masked(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                                     const pnr_rays *rays, const float *z, int32_t k, const float *d_feat,
                                     const float *d_zlat, float *d_latent, float *d_z, const uint8_t *z_mask,
                                     pnr_stream_t stream) {
    int rc = check_scene(scene);
    if (rc) return rc;
    if ((rc = check_desc_for_scene(desc, scene))) return rc;
    if ((rc = check_rays_z(scene, rays, z, k))) return rc;
    if (scene->latent_c != 512) return fail(PNR_ERR_UNSUPPORTED, "input backward: latent_c == 512");
    if (!packed || !d_feat || !d_zlat) return fail(PNR_ERR_INVALID, "pnr_points_input_backward: NULL");
    return launch_points_in_bwd(*scene, *rays, z, k, static_cast<const float *>(packed), desc->pe_n, d_feat, d_zlat,
                                d_latent, d_z, z_mask, (hipStream_t)stream);
}

int pnr_points_input_backward(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *packed,
                              const pnr_rays *rays, const float *z, int32_t k, const float *d_feat,
                              const float *d_zlat, float *d_latent, float *d_z, pnr_stream_t stream) {
    return pnr_points_input_backward_masked(scene, desc, packed, rays, z, k, d_feat, d_zlat, d_latent, d_z, nullptr,
                                            stream);
}

size_t pnr_mlp_packed_t_bytes(const pnr_mlp_desc *desc) {
    if (!desc) return 0;
    return mlp_packed_t_bytes(*desc);
}

int pnr_mlp_pack_t(const pnr_mlp_weights *w, const void *packed, void *packed_t, size_t packed_t_bytes,
                   pnr_stream_t stream) {
    if (!w || !packed || !packed_t) return fail(PNR_ERR_INVALID, "pnr_mlp_pack_t: NULL argument");
    return mlp_pack_t(*w, packed, packed_t, packed_t_bytes, (hipStream_t)stream);
}

int pnr_mlp_backward(const pnr_mlp_desc *desc, const void *packed, const void *packed_t, const float *lin_out_w,
                     const float *save, const float *d_o, int64_t n_points, float *dy, float *d_zlat,
                     pnr_stream_t stream) {
    return pnr_mlp_backward_bias(desc, packed, packed_t, lin_out_w, save, d_o, n_points, dy, d_zlat, nullptr,
                                 nullptr, 0, stream);
}

size_t pnr_mlp_backward_workspace_bytes(const pnr_mlp_desc *desc, int64_t n_points) {
    return desc ? mlp_bwd_workspace_bytes(*desc, n_points) : 0;
}

int pnr_mlp_backward_bias(const pnr_mlp_desc *desc, const void *packed, const void *packed_t,
                          const float *lin_out_w, const float *save, const float *d_o, int64_t n_points, float *dy,
                          float *d_zlat, float *d_bias, void *workspace, size_t workspace_bytes,
                          pnr_stream_t stream) {
    return pnr_mlp_backward_views(desc, packed, packed_t, lin_out_w, save, d_o, n_points, 1, dy, d_zlat, d_bias,
                                  workspace, workspace_bytes, stream);
}

int pnr_mlp_backward_views(const pnr_mlp_desc *desc, const void *packed, const void *packed_t,
                           const float *lin_out_w, const float *save, const float *d_o, int64_t n_points,
                           int32_t n_views, float *dy, float *d_zlat, float *d_bias, void *workspace,
                           size_t workspace_bytes, pnr_stream_t stream) {
    if (!desc || n_points < 0 || n_views < 1) return fail(PNR_ERR_INVALID, "pnr_mlp_backward: bad arguments");
    if (n_points > 0 && (!packed || !packed_t || !lin_out_w || !save || !d_o || !dy))
        return fail(PNR_ERR_INVALID, "pnr_mlp_backward: NULL argument");
    if (misaligned(15, lin_out_w, save, d_o, dy, d_zlat))
        return fail(PNR_ERR_INVALID, "pnr_mlp_backward: buffers must be 16-byte aligned");
    MlpBwdCall c;
    c.packed = packed;
    c.packed_t = packed_t;
    c.w_out = lin_out_w;
    c.save = save;
    c.d_o = d_o;
    c.n_points = n_points;
    c.n_views = n_views;
    c.dy = dy;
    c.dzlat = d_zlat;
    c.d_bias = d_bias;
    c.ws = workspace;
    c.ws_bytes = workspace_bytes;
    return launch_mlp_bwd(*desc, c, (hipStream_t)stream);
}

size_t pnr_weight_grad_workspace_bytes(int32_t n_layers, int64_t n_points) {
    return wgrad_workspace_bytes(n_layers, n_points);
}

int pnr_weight_grad(const float *const *dy, const float *const *x, float *const *d_weight, int32_t n_layers,
                    int64_t n_points, void *workspace, size_t workspace_bytes, pnr_stream_t stream) {
    if (!dy || !x || !d_weight) return fail(PNR_ERR_INVALID, "pnr_weight_grad: NULL argument");
    return launch_wgrad(dy, x, d_weight, n_layers, n_points, workspace, workspace_bytes, PNR_WGRAD_F16X3,
                        (hipStream_t)stream);
}

int pnr_weight_grad_arith(const float *const *dy, const float *const *x, float *const *d_weight, int32_t n_layers,
                          int64_t n_points, int32_t arith, void *workspace, size_t workspace_bytes,
                          pnr_stream_t stream) {
    if (!dy || !x || !d_weight) return fail(PNR_ERR_INVALID, "pnr_weight_grad_arith: NULL argument");
    return launch_wgrad(dy, x, d_weight, n_layers, n_points, workspace, workspace_bytes, arith, (hipStream_t)stream);
}

// workspace layout of pnr_render_forward
struct RenderWs {
    size_t z_c, raw_c, w_c, z_f, raw_f, xsum, origin, z_new, raw_new, total;
};

static RenderWs render_ws(const pnr_scene *sc, const pnr_render_cfg *cfg, int64_t n) {
    RenderWs w;
    const size_t kc = (size_t)cfg->n_coarse, kall = (size_t)(cfg->n_coarse + cfg->n_fine);
    size_t o = 0;
    w.z_c = o; o += align256(sizeof(float) * n * kc);
    w.raw_c = o; o += align256(sizeof(float) * n * kc * 4);
    w.w_c = o; o += align256(sizeof(float) * n * kc);
    w.z_f = o; o += cfg->n_fine > 0 ? align256(sizeof(float) * n * kall) : 0;
    w.raw_f = o; o += cfg->n_fine > 0 ? align256(sizeof(float) * n * kall * 4) : 0;
    w.xsum = o; o += align256(mlp_xsum_bytes(sc->n_views));
    // coarse-output reuse when the fine pass runs the coarse MLP (see pnr_render_forward_proj)
    const size_t kf = (size_t)cfg->n_fine;
    w.origin = o; o += kf > 0 ? align256(sizeof(int) * n * kall) : 0;
    w.z_new = o; o += kf > 0 ? align256(sizeof(float) * n * kf) : 0;
    w.raw_new = o; o += kf > 0 ? align256(sizeof(float) * n * kf * 4) : 0;
    w.total = o;
    return w;
}

size_t pnr_render_workspace_bytes(const pnr_scene *scene, const pnr_render_cfg *cfg, int64_t n_rays) {
    if (!scene || !cfg || n_rays < 0) return 0;
    return render_ws(scene, cfg, n_rays).total;
}

int pnr_render_forward(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *coarse_packed,
                       const void *fine_packed, const pnr_rays *rays, const pnr_rng *rng,
                       const pnr_render_cfg *cfg, const pnr_render_out *out, void *workspace,
                       size_t workspace_bytes, pnr_stream_t stream) {
    return pnr_render_forward_events(scene, desc, coarse_packed, fine_packed, rays, rng, cfg, out,
                                     workspace, workspace_bytes, stream, nullptr);
}

int pnr_render_forward_events(const pnr_scene *scene, const pnr_mlp_desc *desc,
                              const void *coarse_packed, const void *fine_packed,
                              const pnr_rays *rays, const pnr_rng *rng, const pnr_render_cfg *cfg,
                              const pnr_render_out *out, void *workspace, size_t workspace_bytes,
                              pnr_stream_t stream, void *const *events) {
    return pnr_render_forward_proj(scene, desc, coarse_packed, fine_packed, nullptr, nullptr, rays, rng, cfg,
                                   out, workspace, workspace_bytes, stream, events);
}

// The route of a render call.  Pure: the march mode, the sample counts, whether the fine pass runs
// the coarse model on the coarse projection, and whether both projections are present.
//
//   route                  coarse pass                              fine pass
//   single                 k_point_mlp: both passes of every ray in ONE launch
//   fuse_c                 k_point_mlp (draws z in its prologue,    see below
//                          composites in its epilogue; fuse_s:
//                          the epilogue draws the fine samples too)
//   !fuse_c                sample_coarse, k_point_mlp, composite    see below
//   kf == 0                                                         none
//   fuse_f                                                          [sample_fine unless fuse_s], k_point_mlp
//                                                                   (composites in its epilogue)
//   reuse                                                           sample_fine, k_point_mlp over the kf new
//                                                                   samples, merge_raw, composite
//   otherwise                                                       [sample_fine unless fuse_s], k_point_mlp,
//                                                                   composite
struct RenderRoute {
    bool reuse;    // mlp_fine is None: the fine pass evaluates only its new samples and merges the coarse outputs
    bool single;   // mode 3: both passes in one launch
    bool fuse_c;   // the coarse pass is one k_point_mlp launch
    bool fuse_s;   // ... whose epilogue also draws the fine samples (mode 1)
    bool fuse_f;   // the fine pass is one k_point_mlp launch
};

static RenderRoute render_route(int mode, int kc, int kf, bool fine_is_coarse, bool both_proj) {
    // Fused ray march (default): each pass is ONE k_point_mlp launch whose prologue draws the
    // coarse depths and whose epilogue composites the ray from LDS (raw never reaches HBM); the
    // coarse epilogue also draws the fine samples.  Needs rays that are whole 64-point tiles
    // (K = 64 or 128); other shapes, and the coarse-output reuse below, take the separate
    // sample / composite kernels, which run the same device code (march_dev.h).
    const int kall = kc + kf;
    RenderRoute r;
    // mlp_fine is None (the coarse pack passed twice, models.py:242-255; eval_approx.py --coarse):
    // the kc coarse samples re-enter the fine pass with the MLP that already evaluated them, so
    // only the kf new samples run through it and the coarse outputs are merged in.
    r.reuse = kf > 0 && fine_is_coarse;
    const bool fused = mode != 0;
    r.fuse_c = fused && kc % 64 == 0 && kc <= 128;
    r.fuse_s = r.fuse_c && mode == 1 && kf > 0 && !r.reuse && kc <= 64 && sort_width(kall) <= 128;
    r.fuse_f = fused && kf > 0 && !r.reuse && kall % 64 == 0 && kall <= 128;
    // mode 3: both passes in ONE launch (a ray's coarse tile, then its fine tiles; the fine depths
    // stay in LDS), for kc = 64 and kc + kf = 128 with both projections; other shapes run mode 2
    r.single = mode == 3 && r.fuse_c && kf > 0 && !r.reuse && kc == 64 && kall == 128 &&
               sort_width(kall) <= 128 && both_proj;
    return r;
}

// The draws of a render call: injected streams, or Philox counters keyed by {seed, offset}
struct RenderRng {
    RngSrc u_coarse, u_fine, u_jit, n_depth;
};

// MarchCfg of one fused pass: the fields every pass sets ...
static MarchCfg march_pass(const pnr_render_cfg *cfg, int kpt, float *weights, float *rgb, float *depth) {
    MarchCfg m = {};
    m.order = cfg->ray_order;
    m.kpt = kpt;
    m.white_bkgd = cfg->white_bkgd;
    m.weights = weights;
    m.rgb = rgb;
    m.depth = depth;
    return m;
}
// ... + the coarse draw in the prologue ...
static void add_coarse_draw(MarchCfg &m, const pnr_render_cfg *cfg, const RenderRng &g, float *z_out) {
    m.sample_coarse = 1;
    m.lindisp = cfg->lindisp;
    m.u_coarse = g.u_coarse;
    m.z_out = z_out;
}
// ... + the fine draws in the coarse epilogue
static void add_fine_draw(MarchCfg &m, const pnr_render_cfg *cfg, const RenderRng &g, float *z_fine) {
    m.kf = cfg->n_fine;
    m.kfd = cfg->n_fine_depth;
    m.n_sort = sort_width(cfg->n_coarse + cfg->n_fine);
    m.depth_std = cfg->depth_std;
    m.u_fine = g.u_fine;
    m.u_jit = g.u_jit;
    m.n_depth = g.n_depth;
    m.z_fine = z_fine;
}

// Validation of a render call, up to and including its workspace (n_rays == 0 passes early: the
// call then launches nothing).
static int check_render(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *coarse_packed,
                        const void *fine_packed, const float *coarse_proj, const float *fine_proj,
                        const pnr_rays *rays, const pnr_rng *rng, const pnr_render_cfg *cfg,
                        const pnr_render_out *out, const void *workspace, size_t workspace_bytes) {
    int rc = check_scene(scene);
    if (rc) return rc;
    if ((rc = check_desc_for_scene(desc, scene))) return rc;
    if (!rays || !rng || !cfg || !out) return fail(PNR_ERR_INVALID, "pnr_render_forward: NULL struct");
    if (!coarse_packed) return fail(PNR_ERR_INVALID, "coarse_packed is NULL");
    const int kc = cfg->n_coarse, kf = cfg->n_fine, kfd = cfg->n_fine_depth;
    if (kc < 1) return fail(PNR_ERR_INVALID, "n_coarse < 1");
    if (cfg->march_mode < -1 || cfg->march_mode > 3)
        return fail(PNR_ERR_INVALID, "march_mode must be -1 (default), 0, 1, 2 or 3 (got %d)", cfg->march_mode);
    if (kf < 0 || kfd < 0 || kfd > kf) return fail(PNR_ERR_INVALID, "need 0 <= n_fine_depth <= n_fine");
    if (kc + kf > 1024) return fail(PNR_ERR_UNSUPPORTED, "n_coarse + n_fine must be <= 1024");
    if (kf > 0 && !fine_packed) return fail(PNR_ERR_INVALID, "fine_packed is NULL");
    if (misaligned(15, coarse_proj, fine_proj))
        return fail(PNR_ERR_INVALID, "latent projections must be 16-byte aligned");
    const int64_t n = rays->n_rays;
    if (n < 0 || !rays->rays) return fail(PNR_ERR_INVALID, "bad rays");
    if (n == 0) return PNR_OK;
    if (rays->rays_per_obj <= 0 || n % rays->rays_per_obj != 0 || n / rays->rays_per_obj != scene->n_obj)
        return fail(PNR_ERR_INVALID, "n_rays (%lld) must be n_obj (%d) x rays_per_obj (%lld)",
                    (long long)n, scene->n_obj, (long long)rays->rays_per_obj);
    // injected streams, or counter mode when every stream pointer is NULL (pnr_abi.h)
    const bool counter = !rng->u_coarse && !rng->u_fine && !rng->u_fine_jit && !rng->n_depth;
    if (!counter) {
        if (!rng->u_coarse) return fail(PNR_ERR_INVALID, "u_coarse stream is NULL");
        if (kf - kfd > 0 && (!rng->u_fine || !rng->u_fine_jit)) return fail(PNR_ERR_INVALID, "fine streams NULL");
        if (kfd > 0 && !rng->n_depth) return fail(PNR_ERR_INVALID, "n_depth stream NULL");
    }
    if (!out->coarse_rgb || !out->coarse_depth) return fail(PNR_ERR_INVALID, "coarse outputs NULL");
    if (kf > 0 && (!out->fine_rgb || !out->fine_depth)) return fail(PNR_ERR_INVALID, "fine outputs NULL");
    return check_workspace("pnr_render_forward", workspace, workspace_bytes, render_ws(scene, cfg, n).total);
}

int pnr_render_forward_proj(const pnr_scene *scene, const pnr_mlp_desc *desc, const void *coarse_packed,
                            const void *fine_packed, const float *coarse_proj, const float *fine_proj,
                            const pnr_rays *rays, const pnr_rng *rng, const pnr_render_cfg *cfg,
                            const pnr_render_out *out, void *workspace, size_t workspace_bytes,
                            pnr_stream_t stream, void *const *events) {
    int rc = check_render(scene, desc, coarse_packed, fine_packed, coarse_proj, fine_proj, rays, rng, cfg, out,
                          workspace, workspace_bytes);
    if (rc || rays->n_rays == 0) return rc;
    const int64_t n = rays->n_rays;
    const int kc = cfg->n_coarse, kf = cfg->n_fine, kfd = cfg->n_fine_depth, kall = kc + kf;
    const int mode = cfg->march_mode >= 0 ? cfg->march_mode : g_fused_default.load(std::memory_order_relaxed);
    const RenderRoute route = render_route(mode, kc, kf, fine_packed == coarse_packed && fine_proj == coarse_proj,
                                           coarse_proj && fine_proj);
    const RenderRng g{{rng->u_coarse, rng->seed, rng->offset, PNR_RNG_U_COARSE},
                      {rng->u_fine, rng->seed, rng->offset, PNR_RNG_U_FINE},
                      {rng->u_fine_jit, rng->seed, rng->offset, PNR_RNG_U_FINE_JIT},
                      {rng->n_depth, rng->seed, rng->offset, PNR_RNG_N_DEPTH}};
    const RenderWs w = render_ws(scene, cfg, n);
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    float *zc = out->z_coarse ? out->z_coarse : reinterpret_cast<float *>(ws + w.z_c);
    float *rawc = reinterpret_cast<float *>(ws + w.raw_c);
    float *wc = out->coarse_weights ? out->coarse_weights : reinterpret_cast<float *>(ws + w.w_c);
    float *zf = kf > 0 ? (out->z_fine ? out->z_fine : reinterpret_cast<float *>(ws + w.z_f)) : nullptr;
    auto mark = [&](int i) -> int {   // bench.py reads all seven
        if (!events || !events[i]) return PNR_OK;
        hipError_t e = hipEventRecord((hipEvent_t)events[i], st);
        return e == hipSuccess ? PNR_OK : fail(PNR_ERR_HIP, "hipEventRecord: %s", hipGetErrorString(e));
    };
    // a k_point_mlp launch of the coarse or the fine model over K samples of every ray at the depths z
    auto pass_call = [&](bool coarse, const float *z, int K) {
        PointMlpCall c;
        c.packed = coarse ? coarse_packed : fine_packed;
        c.proj = coarse ? coarse_proj : fine_proj;
        c.rays = rays->rays;
        c.rays_per_obj = rays->rays_per_obj;
        c.z = z;
        c.K = K;
        c.n_points = n * K;
        c.xsum = reinterpret_cast<float *>(ws + w.xsum);
        return c;
    };
    auto launch = [&](const PointMlpCall &c) { return launch_point_mlp(*scene, *desc, c, st); };
    // the standalone composite of a pass: K samples at z with the MLP's raw outputs
    auto composite = [&](const float *z, const float *raw, int K, float *weights, float *rgb, float *depth) {
        CompositeCall cc;
        cc.z = z; cc.raw = raw; cc.rays = rays->rays; cc.n_rays = n; cc.K = K; cc.white_bkgd = cfg->white_bkgd;
        cc.weights = weights; cc.rgb = rgb; cc.depth = depth;
        return launch_composite(cc, st);
    };

    if (route.single) {   // events 0 1 [launch] 2 3 4 5 6
        MarchCfg m = march_pass(cfg, 1, out->coarse_weights, out->coarse_rgb, out->coarse_depth);
        add_coarse_draw(m, cfg, g, out->z_coarse);
        add_fine_draw(m, cfg, g, out->z_fine);   // NULL unless the caller wants the fine depths
        m.single = 1;
        m.kpt_f = kall / 64;
        m.packed_f = static_cast<const float *>(fine_packed);
        m.proj_f = fine_proj;
        m.weights_f = out->fine_weights;
        m.rgb_f = out->fine_rgb;
        m.depth_f = out->fine_depth;
        PointMlpCall c = pass_call(/*coarse=*/true, zc, kc);
        c.n_points = n * (kc + kall);
        c.march = &m;
        if ((rc = mark(0)) || (rc = mark(1)) || (rc = launch(c))) return rc;
        for (int i = 2; i < 6; ++i)
            if ((rc = mark(i))) return rc;
        return mark(6);
    }

    // coarse pass (nerf.py:273-276); events: fused 0 1 [mlp] 2 3, separate 0 [sample] 1 [mlp] 2 [composite] 3
    if ((rc = mark(0))) return rc;
    PointMlpCall c = pass_call(/*coarse=*/true, zc, kc);
    if (route.fuse_c) {
        const bool fs = route.fuse_s;
        MarchCfg m = march_pass(cfg, kc / 64, fs ? out->coarse_weights : wc, out->coarse_rgb, out->coarse_depth);
        add_coarse_draw(m, cfg, g, fs ? out->z_coarse : zc);
        if (fs) add_fine_draw(m, cfg, g, zf);
        if (route.reuse) c.out = rawc;
        c.march = &m;
        if ((rc = mark(1)) || (rc = launch(c)) || (rc = mark(2))) return rc;
    } else {
        c.out = rawc;
        if ((rc = launch_sample_coarse(rays->rays, n, kc, g.u_coarse, cfg->lindisp, zc, st))) return rc;
        if ((rc = mark(1)) || (rc = launch(c)) || (rc = mark(2))) return rc;
        if ((rc = composite(zc, rawc, kc, wc, out->coarse_rgb, out->coarse_depth))) return rc;
    }
    if ((rc = mark(3)) || kf == 0) return rc;

    // fine pass (nerf.py:284-301); events: fused [sample_fine unless fuse_s] 4 [mlp] 5 6,
    // separate or reuse [sample_fine] 4 [mlp (+ merge)] 5 [composite] 6
    float *rawf = reinterpret_cast<float *>(ws + w.raw_f);
    int *origin = route.reuse ? reinterpret_cast<int *>(ws + w.origin) : nullptr;
    float *z_new = route.reuse ? reinterpret_cast<float *>(ws + w.z_new) : nullptr;
    if (!route.fuse_s) {
        FineSampleCall f;
        f.rays = rays->rays; f.n_rays = n; f.kc = kc; f.z_coarse = zc; f.weights = wc; f.depth = out->coarse_depth;
        f.kf = kf; f.kfd = kfd; f.depth_std = cfg->depth_std; f.u_fine = g.u_fine; f.u_jit = g.u_jit;
        f.n_depth = g.n_depth; f.lindisp = cfg->lindisp; f.z_fine = zf; f.origin = origin; f.z_new = z_new;
        if ((rc = launch_sample_fine(f, st))) return rc;
    }
    if ((rc = mark(4))) return rc;
    if (route.fuse_f) {
        const MarchCfg m = march_pass(cfg, kall / 64, out->fine_weights, out->fine_rgb, out->fine_depth);
        c = pass_call(/*coarse=*/false, zf, kall);
        c.march = &m;
        if ((rc = launch(c)) || (rc = mark(5))) return rc;
        return mark(6);
    }
    if (route.reuse) {
        float *raw_new = reinterpret_cast<float *>(ws + w.raw_new);
        c = pass_call(/*coarse=*/false, z_new, kf);
        c.out = raw_new;
        if ((rc = launch(c)) || (rc = launch_merge_raw(origin, rawc, raw_new, n, kc, kf, rawf, st))) return rc;
    } else {
        c = pass_call(/*coarse=*/false, zf, kall);
        c.out = rawf;
        if ((rc = launch(c))) return rc;
    }
    if ((rc = mark(5))) return rc;
    if ((rc = composite(zf, rawf, kall, out->fine_weights, out->fine_rgb, out->fine_depth))) return rc;
    return mark(6);
}

int32_t pnr_render_set_fused(int32_t on) { return g_fused_default.exchange(on < 0 || on > 3 ? 2 : on); }
int32_t pnr_mlp_set_lean(int32_t on) { return pnr::mlp_set_lean(on); }
int32_t pnr_mlp_last_kernel(void) { return pnr::mlp_last_kernel(); }

int pnr_sample_coarse(const float *rays, int64_t n_rays, int32_t n_coarse, const float *u_coarse,
                      int32_t lindisp, float *z, pnr_stream_t stream) {
    if (n_rays < 0 || n_coarse < 1) return fail(PNR_ERR_INVALID, "pnr_sample_coarse: bad sizes");
    if (n_rays > 0 && (!rays || !u_coarse || !z)) return fail(PNR_ERR_INVALID, "pnr_sample_coarse: NULL");
    return launch_sample_coarse(rays, n_rays, n_coarse, RngSrc{u_coarse, 0, 0, PNR_RNG_U_COARSE}, lindisp, z,
                                (hipStream_t)stream);
}

int pnr_sample_fine(const float *rays, int64_t n_rays, int32_t n_coarse, const float *z_coarse,
                    const float *coarse_weights, const float *coarse_depth, int32_t n_fine,
                    int32_t n_fine_depth, float depth_std, const float *u_fine,
                    const float *u_fine_jit, const float *n_depth, int32_t lindisp, float *z_fine,
                    pnr_stream_t stream) {
    if (n_rays < 0 || n_coarse < 1 || n_fine < 1 || n_fine_depth < 0 || n_fine_depth > n_fine)
        return fail(PNR_ERR_INVALID, "pnr_sample_fine: bad sizes");
    if (n_coarse + n_fine > 1024) return fail(PNR_ERR_UNSUPPORTED, "n_coarse + n_fine must be <= 1024");
    if (n_rays == 0) return PNR_OK;
    if (!rays || !z_coarse || !coarse_weights || !z_fine) return fail(PNR_ERR_INVALID, "pnr_sample_fine: NULL");
    if (n_fine - n_fine_depth > 0 && (!u_fine || !u_fine_jit)) return fail(PNR_ERR_INVALID, "fine streams NULL");
    if (n_fine_depth > 0 && (!n_depth || !coarse_depth)) return fail(PNR_ERR_INVALID, "depth inputs NULL");
    FineSampleCall c;
    c.rays = rays; c.n_rays = n_rays; c.kc = n_coarse; c.z_coarse = z_coarse; c.weights = coarse_weights;
    c.depth = coarse_depth; c.kf = n_fine; c.kfd = n_fine_depth; c.depth_std = depth_std;
    c.u_fine = RngSrc{u_fine, 0, 0, PNR_RNG_U_FINE}; c.u_jit = RngSrc{u_fine_jit, 0, 0, PNR_RNG_U_FINE_JIT};
    c.n_depth = RngSrc{n_depth, 0, 0, PNR_RNG_N_DEPTH}; c.lindisp = lindisp; c.z_fine = z_fine;
    return launch_sample_fine(c, (hipStream_t)stream);
}

int pnr_rng_fill(uint64_t seed, uint64_t offset, int32_t stream, int64_t n_rays, int32_t width, float *out,
                 pnr_stream_t stream_h) {
    if (stream < PNR_RNG_U_COARSE || stream > PNR_RNG_N_DEPTH) return fail(PNR_ERR_INVALID, "pnr_rng_fill: bad stream");
    if (n_rays < 0 || width < 0) return fail(PNR_ERR_INVALID, "pnr_rng_fill: bad sizes");
    if (n_rays * (int64_t)width == 0) return PNR_OK;
    if (!out) return fail(PNR_ERR_INVALID, "pnr_rng_fill: NULL");
    return launch_rng_fill(RngSrc{nullptr, seed, offset, stream}, n_rays, width, out, (hipStream_t)stream_h);
}

int pnr_composite(const float *z, const float *raw, const float *rays, int64_t n_rays, int32_t k,
                  int32_t white_bkgd, float *weights, float *rgb, float *depth, pnr_stream_t stream) {
    if (n_rays < 0 || k < 1) return fail(PNR_ERR_INVALID, "pnr_composite: bad sizes");
    if (n_rays == 0) return PNR_OK;
    if (!z || !raw || !rays || !rgb || !depth) return fail(PNR_ERR_INVALID, "pnr_composite: NULL");
    if (misaligned(15, raw)) return fail(PNR_ERR_INVALID, "raw must be 16-byte aligned");
    CompositeCall c;
    c.z = z; c.raw = raw; c.rays = rays; c.n_rays = n_rays; c.K = k; c.white_bkgd = white_bkgd; c.weights = weights;
    c.rgb = rgb; c.depth = depth;
    return launch_composite(c, (hipStream_t)stream);
}

int pnr_latent_channels_last(const float *const *maps, const int32_t *channels, const int32_t *heights,
                             const int32_t *widths, int32_t n_maps, int32_t n_images, float *latent_cl,
                             int32_t out_h, int32_t out_w, pnr_stream_t stream) {
    if (!maps || !channels || !heights || !widths || !latent_cl)
        return fail(PNR_ERR_INVALID, "pnr_latent_channels_last: NULL");
    if (n_images < 0 || out_h < 1 || out_w < 1) return fail(PNR_ERR_INVALID, "pnr_latent_channels_last: bad sizes");
    return launch_latent_cl(maps, channels, heights, widths, n_maps, n_images, latent_cl, out_h, out_w, false,
                            (hipStream_t)stream);
}

int pnr_latent_channels_last_nhwc(const float *const *maps, const int32_t *channels, const int32_t *heights,
                                  const int32_t *widths, int32_t n_maps, int32_t n_images, float *latent_cl,
                                  int32_t out_h, int32_t out_w, pnr_stream_t stream) {
    if (!maps || !channels || !heights || !widths || !latent_cl)
        return fail(PNR_ERR_INVALID, "pnr_latent_channels_last_nhwc: NULL");
    if (n_images < 0 || out_h < 1 || out_w < 1)
        return fail(PNR_ERR_INVALID, "pnr_latent_channels_last_nhwc: bad sizes");
    return launch_latent_cl(maps, channels, heights, widths, n_maps, n_images, latent_cl, out_h, out_w, true,
                            (hipStream_t)stream);
}

int pnr_latent_channels_last_backward(const float *g, float *const *d_maps, const int32_t *channels,
                                      const int32_t *heights, const int32_t *widths, int32_t n_maps,
                                      int32_t n_images, int32_t out_h, int32_t out_w, pnr_stream_t stream) {
    if (!d_maps || !channels || !heights || !widths)
        return fail(PNR_ERR_INVALID, "pnr_latent_channels_last_backward: NULL");
    return launch_latent_cl_bwd(g, d_maps, channels, heights, widths, n_maps, n_images, out_h, out_w,
                                (hipStream_t)stream);
}

int pnr_fold_batchnorm(const pnr_bn_fold *folds, int32_t n_folds, int64_t max_elems, pnr_stream_t stream) {
    if (n_folds < 0 || n_folds > 65535 || max_elems < 0) return fail(PNR_ERR_INVALID, "pnr_fold_batchnorm: bad sizes");
    if (n_folds > 0 && !folds) return fail(PNR_ERR_INVALID, "pnr_fold_batchnorm: NULL");
    return launch_fold_bn(folds, n_folds, max_elems, (hipStream_t)stream);
}

int pnr_gen_rays(const float *poses, int64_t n_images, int32_t pose_rows, int32_t width, int32_t height,
                 float fx, float fy, float cx, float cy, float z_near, float z_far, float *rays,
                 pnr_stream_t stream) {
    if (n_images < 0 || width < 0 || height < 0) return fail(PNR_ERR_INVALID, "pnr_gen_rays: bad sizes");
    if (pose_rows != 3 && pose_rows != 4) return fail(PNR_ERR_INVALID, "pnr_gen_rays: pose_rows must be 3 or 4");
    if (n_images == 0 || width == 0 || height == 0) return PNR_OK;
    if (!poses || !rays) return fail(PNR_ERR_INVALID, "pnr_gen_rays: NULL");
    if (misaligned(15, rays)) return fail(PNR_ERR_INVALID, "rays must be 16-byte aligned");
    return launch_gen_rays(poses, n_images, pose_rows, width, height, fx, fy, cx, cy, z_near, z_far, rays,
                           (hipStream_t)stream);
}

size_t pnr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) { return mc_workspace_bytes(nx, ny, nz); }

int pnr_mc_count(const float *grid, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                 size_t workspace_bytes, int64_t *counts_dev, pnr_stream_t stream) {
    if (!grid || !workspace || !counts_dev) return fail(PNR_ERR_INVALID, "pnr_mc_count: NULL argument");
    if (misaligned(3, grid)) return fail(PNR_ERR_INVALID, "pnr_mc_count: grid must be 4-byte aligned");
    if (misaligned(15, workspace)) return fail(PNR_ERR_INVALID, "pnr_mc_count: workspace must be 16-byte aligned");
    if (misaligned(7, counts_dev))
        return fail(PNR_ERR_INVALID, "pnr_mc_count: counts_dev must be 8-byte aligned");
    return launch_mc_count(grid, nx, ny, nz, level, workspace, workspace_bytes, counts_dev, (hipStream_t)stream);
}

int pnr_mc_emit(const float *grid, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                size_t workspace_bytes, float *verts, int64_t verts_cap, int32_t *faces, int64_t faces_cap,
                pnr_stream_t stream) {
    if (!grid || !workspace) return fail(PNR_ERR_INVALID, "pnr_mc_emit: NULL argument");
    if (verts_cap < 0 || faces_cap < 0 || verts_cap > INT32_MAX || faces_cap > INT32_MAX)
        return fail(PNR_ERR_INVALID, "pnr_mc_emit: capacities must be in 0 .. 2^31 - 1 (int32 vertex indices)");
    if ((verts_cap > 0 && !verts) || (faces_cap > 0 && !faces))
        return fail(PNR_ERR_INVALID, "pnr_mc_emit: NULL output with a non-zero capacity");
    if (misaligned(3, grid, verts, faces))
        return fail(PNR_ERR_INVALID, "pnr_mc_emit: grid, verts and faces must be 4-byte aligned");
    if (misaligned(15, workspace)) return fail(PNR_ERR_INVALID, "pnr_mc_emit: workspace must be 16-byte aligned");
    return launch_mc_emit(grid, nx, ny, nz, level, workspace, workspace_bytes, verts, verts_cap, faces, faces_cap,
                          (hipStream_t)stream);
}

int pnr_mc_case_table(int8_t out[256][16]) {
    if (!out) return fail(PNR_ERR_INVALID, "pnr_mc_case_table: NULL");
    mc_case_table(out);
    return PNR_OK;
}

size_t pnr_image_metrics_workspace_bytes(int64_t n, int32_t h, int32_t w, int32_t c) {
    return image_metrics_workspace_bytes(n, h, w, c);
}

int pnr_image_metrics(const float *x, const float *y, int64_t n, int32_t h, int32_t w, int32_t c, float data_range,
                      float k1, float k2, void *workspace, size_t workspace_bytes, double *out,
                      pnr_stream_t stream) {
    if (!x || !y || !out) return fail(PNR_ERR_INVALID, "pnr_image_metrics: NULL argument");
    if (!(data_range > 0.f)) return fail(PNR_ERR_INVALID, "pnr_image_metrics: data_range must be > 0");
    if (misaligned(3, x, y)) return fail(PNR_ERR_INVALID, "pnr_image_metrics: x and y must be 4-byte aligned");
    if (misaligned(7, out, workspace))
        return fail(PNR_ERR_INVALID, "pnr_image_metrics: out and workspace must be 8-byte aligned");
    return launch_image_metrics(x, y, n, h, w, c, data_range, k1, k2, workspace, workspace_bytes, out,
                                (hipStream_t)stream);
}

size_t pnr_mesh_sample_workspace_bytes(int64_t n_faces) { return mesh_sample_workspace_bytes(n_faces); }

int pnr_mesh_sample(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int64_t n,
                    uint64_t seed, void *workspace, size_t workspace_bytes, float *points, float *normals,
                    int32_t *tri, double *total_area, pnr_stream_t stream) {
    if (n < 1 || n_faces < 1 || n_verts < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: n, n_faces and n_verts must be >= 1");
    if (!verts || !faces || !points || !total_area || !workspace)
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: NULL argument");
    if (misaligned(3, verts, faces, points, normals, tri))
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: verts, faces, points, normals and tri must be 4-byte aligned");
    if (misaligned(15, workspace) || misaligned(7, total_area))
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: workspace must be 16-byte, total_area 8-byte aligned");
    return launch_mesh_sample(verts, n_verts, faces, n_faces, n, seed, workspace, workspace_bytes, points, normals, tri,
                              total_area, (hipStream_t)stream);
}

size_t pnr_nearest_workspace_bytes(int64_t n, int64_t m) { return nearest_workspace_bytes(n, m); }

int pnr_nearest(const float *a, int64_t n, const float *b, int64_t m, void *workspace, size_t workspace_bytes,
                float *d2, int32_t *idx, pnr_stream_t stream) {
    if (n < 1 || m < 1) return fail(PNR_ERR_INVALID, "pnr_nearest: n and m must be >= 1");
    if (!a || !b || !d2 || !idx) return fail(PNR_ERR_INVALID, "pnr_nearest: NULL argument");
    if (misaligned(3, a, b, d2, idx, workspace))
        return fail(PNR_ERR_INVALID, "pnr_nearest: a, b, d2, idx and workspace must be 4-byte aligned");
    return launch_nearest(a, n, b, m, workspace, workspace_bytes, d2, idx, (hipStream_t)stream);
}

int pnr_mesh_distance_reduce(const float *d2_ab, const int32_t *idx_ab, int64_t n, const float *d2_ba,
                             const int32_t *idx_ba, int64_t m, const float *normals_a, const float *normals_b,
                             double tau, double *out, pnr_stream_t stream) {
    if (n < 1 || m < 1) return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: n and m must be >= 1");
    if (!d2_ab || !idx_ab || !d2_ba || !idx_ba || !out)
        return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: NULL argument");
    if ((normals_a == nullptr) != (normals_b == nullptr))
        return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: normals of both clouds, or of neither");
    if (!(tau >= 0.0)) return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: tau must be >= 0");
    if (misaligned(7, out)) return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: out must be 8-byte aligned");
    return launch_mesh_distance_reduce(d2_ab, idx_ab, n, d2_ba, idx_ba, m, normals_a, normals_b, tau, out,
                                       (hipStream_t)stream);
}

size_t pnr_winding_workspace_bytes(int64_t n, int64_t n_faces) { return winding_workspace_bytes(n, n_faces); }

int pnr_winding(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *points,
                int64_t n, void *workspace, size_t workspace_bytes, double *w, pnr_stream_t stream) {
    if (n < 1 || n_faces < 1 || n_verts < 1)
        return fail(PNR_ERR_INVALID, "pnr_winding: n, n_faces and n_verts must be >= 1");
    if (!verts || !faces || !points || !w) return fail(PNR_ERR_INVALID, "pnr_winding: NULL argument");
    if (misaligned(3, verts, faces, points))
        return fail(PNR_ERR_INVALID, "pnr_winding: verts, faces and points must be 4-byte aligned");
    if (misaligned(7, w, workspace))
        return fail(PNR_ERR_INVALID, "pnr_winding: w and workspace must be 8-byte aligned");
    return launch_winding(verts, n_verts, faces, n_faces, points, n, workspace, workspace_bytes, w, (hipStream_t)stream);
}

int pnr_box_sample(const float *lo, const float *hi, int64_t n, uint64_t seed, float *points, pnr_stream_t stream) {
    if (n < 1) return fail(PNR_ERR_INVALID, "pnr_box_sample: n must be >= 1");
    if (!lo || !hi || !points) return fail(PNR_ERR_INVALID, "pnr_box_sample: NULL argument");
    if (n > 0x7fffffff) return fail(PNR_ERR_UNSUPPORTED, "pnr_box_sample: n above 2^31 - 1");
    if (misaligned(3, points)) return fail(PNR_ERR_INVALID, "pnr_box_sample: points must be 4-byte aligned");
    float ext[3];
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || hi[k] < lo[k])
            return fail(PNR_ERR_INVALID, "pnr_box_sample: bounds must be finite with lo <= hi (axis %d: %g, %g)", k,
                        (double)lo[k], (double)hi[k]);
        ext[k] = hi[k] - lo[k];   // rounded once
        if (!std::isfinite(ext[k])) return fail(PNR_ERR_INVALID, "pnr_box_sample: the extent of axis %d overflows", k);
    }
    return launch_box_sample(lo, ext, n, seed, points, (hipStream_t)stream);
}

size_t pnr_mesh_weld_workspace_bytes(int64_t n_verts) { return mesh_weld_workspace_bytes(n_verts); }

int pnr_mesh_weld(const float *verts, int64_t n_verts, void *workspace, size_t workspace_bytes, int32_t *remap,
                  pnr_stream_t stream) {
    if (n_verts < 1) return fail(PNR_ERR_INVALID, "pnr_mesh_weld: n_verts must be >= 1");
    if (!verts || !remap || !workspace) return fail(PNR_ERR_INVALID, "pnr_mesh_weld: NULL argument");
    if (misaligned(3, verts, remap, workspace))
        return fail(PNR_ERR_INVALID, "pnr_mesh_weld: verts, remap and workspace must be 4-byte aligned");
    return launch_mesh_weld(verts, n_verts, workspace, workspace_bytes, remap, (hipStream_t)stream);
}

size_t pnr_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    return mesh_components_workspace_bytes(n_verts, n_faces);
}

int pnr_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_verts, void *workspace,
                        size_t workspace_bytes, int32_t *vert_label, int32_t *face_label, int32_t *launches,
                        pnr_stream_t stream) {
    if (n_verts < 1 || n_faces < 0)
        return fail(PNR_ERR_INVALID, "pnr_mesh_components: n_verts must be >= 1 and n_faces >= 0");
    if (!vert_label || !workspace || (n_faces > 0 && (!faces || !face_label)))
        return fail(PNR_ERR_INVALID, "pnr_mesh_components: NULL argument");
    if (misaligned(3, faces, vert_label, face_label, workspace))
        return fail(PNR_ERR_INVALID,
                    "pnr_mesh_components: faces, vert_label, face_label and workspace must be 4-byte aligned");
    return launch_mesh_components(faces, n_faces, n_verts, workspace, workspace_bytes, vert_label, face_label, launches,
                                  (hipStream_t)stream);
}

int pnr_mesh_component_sums(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                            const int64_t *order, const int64_t *seg_start, int64_t n_components, double *out,
                            pnr_stream_t stream) {
    if (n_verts < 1 || n_faces < 1 || n_components < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_component_sums: n_verts, n_faces and n_components must be >= 1");
    if (!verts || !faces || !order || !seg_start || !out)
        return fail(PNR_ERR_INVALID, "pnr_mesh_component_sums: NULL argument");
    if (misaligned(3, verts, faces) || misaligned(7, order, seg_start, out))
        return fail(PNR_ERR_INVALID,
                    "pnr_mesh_component_sums: verts and faces must be 4-byte, order, seg_start and out 8-byte aligned");
    return launch_mesh_component_sums(verts, n_verts, faces, n_faces, order, seg_start, n_components, out,
                                      (hipStream_t)stream);
}

size_t pnr_mesh_raster_workspace_bytes(int64_t nv, int32_t h, int32_t w, int64_t n_faces) {
    return mesh_raster_workspace_bytes(nv, h, w, n_faces);
}

int pnr_mesh_raster_set_small(int32_t pixels) {
    const int prev = g_raster_small.exchange(pixels < 0 ? -1 : pixels);
    return prev < 0 ? PNR_RASTER_SMALL_PIXELS : prev;
}

int pnr_mesh_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                    int64_t nv, int32_t pose_rows, int32_t w, int32_t h, float fx, float fy, float cx, float cy,
                    void *workspace, size_t workspace_bytes, int32_t *face_out, float *depth_out,
                    pnr_stream_t stream) {
    if (nv < 1 || n_faces < 1 || n_verts < 1 || w < 1 || h < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_raster: nv, n_faces, n_verts, w and h must be >= 1");
    if (pose_rows != 3 && pose_rows != 4)
        return fail(PNR_ERR_INVALID, "pnr_mesh_raster: pose_rows must be 3 or 4 (got %d)", pose_rows);
    if (!verts || !faces || !poses || !face_out || !depth_out)
        return fail(PNR_ERR_INVALID, "pnr_mesh_raster: NULL argument");
    if (misaligned(3, verts, faces, poses, face_out, depth_out))
        return fail(PNR_ERR_INVALID, "pnr_mesh_raster: verts, faces, poses, face and depth must be 4-byte aligned");
    if (misaligned(7, workspace)) return fail(PNR_ERR_INVALID, "pnr_mesh_raster: workspace must be 8-byte aligned");
    return launch_mesh_raster(verts, n_verts, faces, n_faces, poses, nv, pose_rows, w, h, fx, fy, cx, cy, workspace,
                              workspace_bytes, face_out, depth_out, g_raster_small.load(std::memory_order_relaxed),
                              (hipStream_t)stream);
}

int pnr_mesh_shade(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                   int64_t nv, int32_t pose_rows, int32_t w, int32_t h, float fx, float fy, float cx, float cy,
                   const int32_t *face, const float *depth, const float *lights, const float *weights,
                   int32_t n_lights, const float *albedo, float ambient, const float *background, float *rgb,
                   float *normal, pnr_stream_t stream) {
    if (nv < 1 || n_faces < 1 || n_verts < 1 || w < 1 || h < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_shade: nv, n_faces, n_verts, w and h must be >= 1");
    if (pose_rows != 3 && pose_rows != 4)
        return fail(PNR_ERR_INVALID, "pnr_mesh_shade: pose_rows must be 3 or 4 (got %d)", pose_rows);
    if (!verts || !faces || !poses || !face || !depth || !albedo || !background || !rgb ||
        (n_lights > 0 && (!lights || !weights)))
        return fail(PNR_ERR_INVALID, "pnr_mesh_shade: NULL argument");
    if (misaligned(3, verts, faces, poses, face, depth, rgb, normal))
        return fail(PNR_ERR_INVALID,
                    "pnr_mesh_shade: verts, faces, poses, face, depth, rgb and normal must be 4-byte aligned");
    return launch_mesh_shade(verts, n_verts, faces, n_faces, poses, nv, pose_rows, w, h, fx, fy, cx, cy, face, depth,
                             lights, weights, n_lights, albedo, ambient, background, rgb, normal, (hipStream_t)stream);
}

}  // extern "C"
