// Mesh rendering on the device: the nearest face and its depth for every pixel of a batch of
// cameras, and a flat-shaded colour on top (the reference renders its training views of STL meshes
// with Blender scripts; its eval/eval.py stops at the STL).  Semantics: include/pnr_abi.h, "Mesh
// rendering"; tests/raster_ref.py restates them in numpy.
//
// Rasterisation, not a ray cast against all faces: k_raster_cover has one lane per (view, face).  It
// moves the face to camera space, forms the three edge normals n_k = lo x (hi - lo) with the two
// endpoints of every edge in coordinate order (so the face on the other side of the edge computes the
// same three floats and negates them: the signed volume d . n_k of a pixel's direction d is then the
// same number with the opposite sign for the two faces, and a ray through the edge is inside at least
// one of them), and the pixel bounds of the projected vertices.  A face whose bounds hold at most
// PNR_RASTER_SMALL_PIXELS pixels is scanned by its own lane; the larger ones are found with a ballot
// over the wave's 64 faces and taken one after the other by the whole wave, coefficients broadcast
// with v_readlane, the 64 lanes testing a PNR_RASTER_TILE x PNR_RASTER_TILE block of pixels a step.
// Both paths call pixel_hit, so a (pixel, face) pair gives the same bits whichever path takes it.
//
// The depth buffer is the workspace: one 64-bit key (bits of the camera-z depth << 32 | face) per
// pixel, taken to its minimum with an integer atomic min (the depth is positive, so its bits order
// like its value; the minimum does not depend on the order of arrival, and equal depths go to the
// lower face).  A plain pre-read skips the atomic where the pixel already holds a smaller key (a
// stale read is only ever too large).  k_raster_resolve decodes the key and scales the camera-z depth
// by the length of the pixel's direction; k_raster_shade colours from face and depth.  No float
// atomics, no LDS, no host sync.
#include "mesh_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace rst {

constexpr int kThreads = PNR_RASTER_BLOCK, kTile = PNR_RASTER_TILE, kSmall = PNR_RASTER_SMALL_PIXELS;
constexpr int kMaxSide = 8192, kMaxLights = PNR_RASTER_MAX_LIGHTS;
constexpr unsigned long long kEmpty = ~0ull;
static_assert(kTile * kTile == kWave, "one pixel of the block per lane");
static_assert(kThreads % kWave == 0, "whole waves");

struct Cam {
    float r[9];   // camera-to-world rotation, row-major
    float o[3];
    bool ok;      // every entry finite
};

struct View {
    int w, h;
    float fx, fy, cx, cy;
};

struct Shading {
    float light[kMaxLights][3];
    float weight[kMaxLights];
    int n_lights;
    float albedo[3], ambient, background[3];
};

__device__ __forceinline__ Cam load_cam(const float *__restrict__ poses, int pose_rows, int64_t view) {
    const float *P = poses + view * pose_rows * 4;
    Cam c;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c.r[3 * r + k] = P[4 * r + k];
            s += c.r[3 * r + k] - c.r[3 * r + k];
        }
        c.o[r] = P[4 * r + 3];
        s += c.o[r] - c.o[r];
    }
    c.ok = s == s;
    return c;
}

// The header fixes where the per-(pixel, face) arithmetic rounds: plain operators under this pragma
// are never fused, every __builtin_fmaf is one fma.
#pragma clang fp contract(off)

// pixel (column i, row j) -> (X, -Y) of its direction (X, -Y, -1), as k_gen_rays forms them
__device__ __forceinline__ void pixel_dir(const View &v, int i, int j, float &X, float &Yn) {
    X = ((float)i - v.cx) / v.fx;
    Yn = -(((float)j - v.cy) / v.fy);
}
__device__ __forceinline__ float dir_len(float X, float Yn) { return sqrtf((X * X + Yn * Yn) + 1.0f); }

// world -> camera: R^T (p - o)
__device__ __forceinline__ void to_cam(const Cam &c, const float p[3], float q[3]) {
    const float x = p[0] - c.o[0], y = p[1] - c.o[1], z = p[2] - c.o[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __builtin_fmaf(c.r[6 + k], z, __builtin_fmaf(c.r[3 + k], y, c.r[k] * x));
}

__device__ __forceinline__ bool lex_less(const float p[3], const float q[3]) {
    if (p[0] != q[0]) return p[0] < q[0];
    if (p[1] != q[1]) return p[1] < q[1];
    return p[2] < q[2];
}

// n = +-(lo x (hi - lo)) for the edge p -> q: lo is the endpoint that comes first in the coordinate
// order of the WORLD vertices (pw, qw), the sign is that of the edge's direction in the face
__device__ __forceinline__ void edge_normal(const float pw[3], const float qw[3], const float pc[3], const float qc[3],
                                            float n[3]) {
    const bool swap = lex_less(qw, pw);
    const float *lo = swap ? qc : pc, *hi = swap ? pc : qc;
    const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    const float nx = lo[1] * ez - lo[2] * ey;
    const float ny = lo[2] * ex - lo[0] * ez;
    const float nz = lo[0] * ey - lo[1] * ex;
    n[0] = swap ? -nx : nx;
    n[1] = swap ? -ny : ny;
    n[2] = swap ? -nz : nz;
}

// The hit rule of one (pixel, face) pair.  n: the edge normals of ab, bc, ca; z: the camera z of a, b, c.
__device__ __forceinline__ bool pixel_hit(const float n[9], const float z[3], float X, float Yn, float &s) {
    const float e_ab = __builtin_fmaf(n[0], X, __builtin_fmaf(n[1], Yn, -n[2]));
    const float e_bc = __builtin_fmaf(n[3], X, __builtin_fmaf(n[4], Yn, -n[5]));
    const float e_ca = __builtin_fmaf(n[6], X, __builtin_fmaf(n[7], Yn, -n[8]));
    const bool pos = e_ab > 0.f || e_bc > 0.f || e_ca > 0.f;
    const bool neg = e_ab < 0.f || e_bc < 0.f || e_ca < 0.f;
    const float det = (e_ab + e_bc) + e_ca;               // d . face normal
    const float num = __builtin_fmaf(e_ca, z[1], __builtin_fmaf(e_bc, z[0], e_ab * z[2]));
    s = -(num / det);
    // NaNs compare false everywhere: a NaN edge value, det or depth is a miss
    return !(pos && neg) && (pos || neg) && det != 0.f && s > 0.f && s < __builtin_inff();
}

struct FaceSetup {
    float n[9], z[3];
    int x0, x1, y0, y1;   // inclusive pixel bounds; empty when x1 < x0 or y1 < y0
};

// false: the face contributes nothing (bad index, non-finite vertex, zero area, behind the camera)
__device__ __forceinline__ bool face_setup(const float *__restrict__ verts, uint32_t nv,
                                           const int32_t *__restrict__ faces, uint32_t t, const Cam &cam,
                                           const View &vw, FaceSetup &fs) {
    uint32_t idx[3];
    if (!face_indices(faces, t, nv, idx)) return false;
    float w[3][3], c[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) w[k][a] = verts[3 * (size_t)idx[k] + a];
        if (!finite3(w[k][0], w[k][1], w[k][2])) return false;
    }
    {   // zero area: the unfused cross product of the two world edges is exactly (0, 0, 0)
        const float ux = w[1][0] - w[0][0], uy = w[1][1] - w[0][1], uz = w[1][2] - w[0][2];
        const float vx = w[2][0] - w[0][0], vy = w[2][1] - w[0][1], vz = w[2][2] - w[0][2];
        const float ax = uy * vz - uz * vy, ay = uz * vx - ux * vz, az = ux * vy - uy * vx;
        if (ax == 0.f && ay == 0.f && az == 0.f) return false;
        if (!finite3(ax, ay, az)) return false;
    }
    float scale = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        to_cam(cam, w[k], c[k]);
        if (!finite3(c[k][0], c[k][1], c[k][2])) return false;
        fs.z[k] = c[k][2];
        scale = fmaxf(scale, fabsf(w[k][0]) + fabsf(w[k][1]) + fabsf(w[k][2]));
    }
    if (c[0][2] >= 0.f && c[1][2] >= 0.f && c[2][2] >= 0.f) return false;   // no point with depth > 0
    edge_normal(w[0], w[1], c[0], c[1], fs.n);
    edge_normal(w[1], w[2], c[1], c[2], fs.n + 3);
    edge_normal(w[2], w[0], c[2], c[0], fs.n + 6);
    // Pixel bounds from the projected vertices, each widened by 1/16 pixel plus the pixel's share of the
    // rounding of its projection.  A vertex at or behind the camera plane, or closer to it than 2^-10 of
    // the scene's size, projects nowhere useful: the bounds are then the whole image.
    scale += fabsf(cam.o[0]) + fabsf(cam.o[1]) + fabsf(cam.o[2]);
    const float guard = scale * 0x1p-10f;
    float xlo = __builtin_inff(), xhi = -__builtin_inff(), ylo = xlo, yhi = xhi;
    bool whole = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = -c[k][2];
        whole |= !(d > guard);
        const float inv = 1.0f / d;
        const float X = c[k][0] * inv, Y = c[k][1] * inv;
        const float slack = scale * 0x1p-20f * inv;
        const float px = __builtin_fmaf(X, vw.fx, vw.cx), py = __builtin_fmaf(-Y, vw.fy, vw.cy);
        const float mx = 0.0625f + fabsf(vw.fx) * (1.0f + fabsf(X)) * slack + fabsf(px) * 0x1p-20f;
        const float my = 0.0625f + fabsf(vw.fy) * (1.0f + fabsf(Y)) * slack + fabsf(py) * 0x1p-20f;
        xlo = fminf(xlo, px - mx);
        xhi = fmaxf(xhi, px + mx);
        ylo = fminf(ylo, py - my);
        yhi = fmaxf(yhi, py + my);
    }
    const float wmax = (float)(vw.w - 1), hmax = (float)(vw.h - 1);
    if (whole || !(xlo == xlo) || !(xhi == xhi) || !(ylo == ylo) || !(yhi == yhi)) {
        fs.x0 = 0, fs.x1 = vw.w - 1, fs.y0 = 0, fs.y1 = vw.h - 1;
        return true;
    }
    // clamped in float first: the conversions below never see a value outside [-1, side]
    fs.x0 = (int)ceilf(fminf(fmaxf(xlo, 0.f), wmax + 1.0f));
    fs.x1 = (int)floorf(fmaxf(fminf(xhi, wmax), -1.0f));
    fs.y0 = (int)ceilf(fminf(fmaxf(ylo, 0.f), hmax + 1.0f));
    fs.y1 = (int)floorf(fmaxf(fminf(yhi, hmax), -1.0f));
    return true;
}

__device__ __forceinline__ void depth_min(unsigned long long *__restrict__ keys, size_t pix, float s, uint32_t face) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 32) | face;
    unsigned long long *p = keys + pix;
    if (*p > key) __hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float lane_f(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

__global__ __launch_bounds__(kThreads) void k_raster_fill(unsigned long long *__restrict__ keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) keys[i] = kEmpty;
}

// grid (face blocks, views folded into gridDim.y); `small_max`: the largest pixel count a lane scans
__global__ __launch_bounds__(kThreads) void k_raster_cover(const float *__restrict__ verts, uint32_t n_verts,
                                                           const int32_t *__restrict__ faces, uint32_t n_faces,
                                                           const float *__restrict__ poses, int pose_rows, uint32_t nv,
                                                           View vw, int small_max,
                                                           unsigned long long *__restrict__ keys) {
    const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const size_t hw = (size_t)vw.w * vw.h;
    for (uint32_t view = blockIdx.y; view < nv; view += gridDim.y) {
        const Cam cam = load_cam(poses, pose_rows, view);
        if (!cam.ok) continue;   // block-uniform
        unsigned long long *vk = keys + view * hw;
        FaceSetup fs;
        bool live = t < n_faces && face_setup(verts, n_verts, faces, t, cam, vw, fs);
        live = live && fs.x1 >= fs.x0 && fs.y1 >= fs.y0;
        const bool big = live && (int64_t)(fs.x1 - fs.x0 + 1) * (fs.y1 - fs.y0 + 1) > small_max;
        if (live && !big) {
            for (int j = fs.y0; j <= fs.y1; ++j)
                for (int i = fs.x0; i <= fs.x1; ++i) {
                    float X, Yn, s;
                    pixel_dir(vw, i, j, X, Yn);
                    if (pixel_hit(fs.n, fs.z, X, Yn, s)) depth_min(vk, (size_t)j * vw.w + i, s, t);
                }
        }
        // the wave's large faces, one after the other, by all 64 lanes
        unsigned long long todo = __ballot(big);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            float n[9], z[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) n[k] = lane_f(big ? fs.n[k] : 0.f, src);
#pragma unroll
            for (int k = 0; k < 3; ++k) z[k] = lane_f(big ? fs.z[k] : 0.f, src);
            const int x0 = __builtin_amdgcn_readlane(big ? fs.x0 : 0, src);
            const int x1 = __builtin_amdgcn_readlane(big ? fs.x1 : -1, src);
            const int y0 = __builtin_amdgcn_readlane(big ? fs.y0 : 0, src);
            const int y1 = __builtin_amdgcn_readlane(big ? fs.y1 : -1, src);
            const uint32_t face = (t - lane) + src;
            for (int ty = y0; ty <= y1; ty += kTile)
                for (int tx = x0; tx <= x1; tx += kTile) {
                    const int i = tx + (lane & (kTile - 1)), j = ty + lane / kTile;
                    if (i <= x1 && j <= y1) {
                        float X, Yn, s;
                        pixel_dir(vw, i, j, X, Yn);
                        if (pixel_hit(n, z, X, Yn, s)) depth_min(vk, (size_t)j * vw.w + i, s, face);
                    }
                }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_raster_resolve(const unsigned long long *__restrict__ keys, size_t n,
                                                             View vw, int32_t *__restrict__ face_out,
                                                             float *__restrict__ depth_out) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = keys[p];
    const size_t pix = p % ((size_t)vw.w * vw.h);
    const int j = (int)(pix / vw.w), i = (int)(pix - (size_t)j * vw.w);
    float X, Yn;
    pixel_dir(vw, i, j, X, Yn);
    const bool hit = key != kEmpty;
    face_out[p] = hit ? (int32_t)(uint32_t)key : -1;
    depth_out[p] = hit ? __uint_as_float((uint32_t)(key >> 32)) * dir_len(X, Yn) : 0.f;
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0]));
}

// rgb (and normal) of every pixel from face and depth: the header's "Shading"
__global__ __launch_bounds__(kThreads) void k_raster_shade(const float *__restrict__ verts, uint32_t n_verts,
                                                           const int32_t *__restrict__ faces, uint32_t n_faces,
                                                           const float *__restrict__ poses, int pose_rows, size_t n,
                                                           View vw, const int32_t *__restrict__ face_in,
                                                           const float *__restrict__ depth_in, Shading sh,
                                                           float *__restrict__ rgb, float *__restrict__ normal) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const size_t hw = (size_t)vw.w * vw.h;
    const size_t view = p / hw, pix = p - view * hw;
    float col[3] = {sh.background[0], sh.background[1], sh.background[2]}, nrm[3] = {0.f, 0.f, 0.f};
    const uint32_t t = (uint32_t)face_in[p];
    if (t < n_faces) {   // -1 is a large unsigned one
        uint32_t fi[3];
        if (face_indices(faces, t, n_verts, fi)) {
            const Cam cam = load_cam(poses, pose_rows, (int64_t)view);
            const float *a = verts + 3 * (size_t)fi[0], *b = verts + 3 * (size_t)fi[1], *c = verts + 3 * (size_t)fi[2];
            const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            float g[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const float gl = sqrtf(dot3(g, g));
            const int j = (int)(pix / vw.w), i = (int)(pix - (size_t)j * vw.w);
            float X, Yn;
            pixel_dir(vw, i, j, X, Yn);
            const float len = dir_len(X, Yn);
            const float uc[3] = {X / len, Yn / len, -1.0f / len};   // k_gen_rays' unit direction
            float d[3], pt[3];
            const float depth = depth_in[p];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                d[r] = (cam.r[3 * r] * uc[0] + cam.r[3 * r + 1] * uc[1]) + cam.r[3 * r + 2] * uc[2];
                pt[r] = __builtin_fmaf(depth, d[r], cam.o[r]);
            }
            const float flip = dot3(g, d) > 0.f ? -1.0f : 1.0f;   // towards the camera
#pragma unroll
            for (int r = 0; r < 3; ++r) nrm[r] = flip * (g[r] / gl);
            float lum = sh.ambient;
            for (int l = 0; l < sh.n_lights; ++l) {
                const float v[3] = {sh.light[l][0] - pt[0], sh.light[l][1] - pt[1], sh.light[l][2] - pt[2]};
                const float c0 = dot3(nrm, v) / sqrtf(dot3(v, v));
                lum = __builtin_fmaf(sh.weight[l], fmaxf(c0, 0.f), lum);   // a NaN cosine (light at the point) adds 0
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) col[r] = fminf(fmaxf(sh.albedo[r] * lum, 0.f), 254.0f / 255.0f);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) rgb[3 * p + r] = col[r];
    if (normal) {
#pragma unroll
        for (int r = 0; r < 3; ++r) normal[3 * p + r] = nrm[r];
    }
}

struct Plan {
    size_t n_pix;   // nv * h * w
    size_t total;   // the keys
};

static bool plan(int64_t nv, int h, int w, int64_t n_faces, Plan &pl) {
    if (nv < 1 || h < 1 || w < 1 || n_faces < 1 || h > kMaxSide || w > kMaxSide || n_faces > kMaxCount) return false;
    if (nv > kMaxCount / ((int64_t)h * w)) return false;
    pl.n_pix = (size_t)nv * h * w;
    pl.total = align256(sizeof(unsigned long long) * pl.n_pix);
    return true;
}

static bool finite_view(float fx, float fy, float cx, float cy) {
    return fx - fx == 0.f && fy - fy == 0.f && cx - cx == 0.f && cy - cy == 0.f && fx != 0.f && fy != 0.f;
}

// what pnr_mesh_raster and pnr_mesh_shade (`fn`) refuse alike: the shape, the vertex count, the camera
static int check(const char *fn, int64_t nv, int h, int w, int64_t n_faces, int64_t n_verts, float fx, float fy,
                 float cx, float cy, Plan &pl) {
    if (!plan(nv, h, w, n_faces, pl))
        return fail(PNR_ERR_UNSUPPORTED,
                    "%s: %lld views of %d x %d with %lld faces not supported (sides in 1 .. %d, nv h w and "
                    "n_faces in 1 .. 2^31 - 1)", fn, (long long)nv, w, h, (long long)n_faces, kMaxSide);
    if (n_verts < 1 || n_verts > kMaxCount)
        return fail(PNR_ERR_INVALID, "%s: n_verts must be in 1 .. 2^31 - 1 (got %lld)", fn, (long long)n_verts);
    if (!finite_view(fx, fy, cx, cy))
        return fail(PNR_ERR_INVALID, "%s: fx, fy, cx, cy must be finite, fx and fy not 0", fn);
    return PNR_OK;
}

}  // namespace rst

size_t mesh_raster_workspace_bytes(int64_t nv, int h, int w, int64_t n_faces) {
    rst::Plan pl;
    return rst::plan(nv, h, w, n_faces, pl) ? pl.total : 0;
}

int launch_mesh_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                       int64_t nv, int pose_rows, int w, int h, float fx, float fy, float cx, float cy, void *ws,
                       size_t bytes, int32_t *face_out, float *depth_out, int small_max, hipStream_t st) {
    rst::Plan pl;
    const int rc = rst::check("pnr_mesh_raster", nv, h, w, n_faces, n_verts, fx, fy, cx, cy, pl);
    if (rc) return rc;
    if (!ws || bytes < pl.total)
        return fail(PNR_ERR_WORKSPACE, "pnr_mesh_raster: workspace %zu bytes, needs %zu", bytes, pl.total);
    if (small_max < 0) small_max = rst::kSmall;
    unsigned long long *keys = static_cast<unsigned long long *>(ws);
    const rst::View vw{w, h, fx, fy, cx, cy};
    const unsigned pix_blocks = blocks(pl.n_pix, rst::kThreads);
    hipLaunchKernelGGL(rst::k_raster_fill, dim3(pix_blocks), dim3(rst::kThreads), 0, st, keys, pl.n_pix);
    if (!launch_ok("raster_fill")) return PNR_ERR_HIP;
    const dim3 grid(blocks((size_t)n_faces, rst::kThreads), (unsigned)(nv < 65535 ? nv : 65535));
    hipLaunchKernelGGL(rst::k_raster_cover, grid, dim3(rst::kThreads), 0, st, verts, (uint32_t)n_verts, faces,
                       (uint32_t)n_faces, poses, pose_rows, (uint32_t)nv, vw, small_max, keys);
    if (!launch_ok("raster_cover")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(rst::k_raster_resolve, dim3(pix_blocks), dim3(rst::kThreads), 0, st, keys, pl.n_pix, vw, face_out,
                       depth_out);
    return launch_ok("raster_resolve") ? PNR_OK : PNR_ERR_HIP;
}

int launch_mesh_shade(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *poses,
                      int64_t nv, int pose_rows, int w, int h, float fx, float fy, float cx, float cy,
                      const int32_t *face_in, const float *depth_in, const float *lights, const float *weights,
                      int n_lights, const float albedo[3], float ambient, const float background[3], float *rgb,
                      float *normal, hipStream_t st) {
    rst::Plan pl;
    const int rc = rst::check("pnr_mesh_shade", nv, h, w, n_faces, n_verts, fx, fy, cx, cy, pl);
    if (rc) return rc;
    if (n_lights < 0 || n_lights > rst::kMaxLights)
        return fail(PNR_ERR_INVALID, "pnr_mesh_shade: n_lights must be in 0 .. %d (got %d)", rst::kMaxLights, n_lights);
    rst::Shading sh = {};
    sh.n_lights = n_lights;
    for (int l = 0; l < n_lights; ++l) {
        for (int k = 0; k < 3; ++k) sh.light[l][k] = lights[3 * l + k];
        sh.weight[l] = weights[l];
    }
    for (int k = 0; k < 3; ++k) sh.albedo[k] = albedo[k], sh.background[k] = background[k];
    sh.ambient = ambient;
    const rst::View vw{w, h, fx, fy, cx, cy};
    const unsigned pix_blocks = blocks(pl.n_pix, rst::kThreads);
    hipLaunchKernelGGL(rst::k_raster_shade, dim3(pix_blocks), dim3(rst::kThreads), 0, st, verts, (uint32_t)n_verts, faces,
                       (uint32_t)n_faces, poses, pose_rows, pl.n_pix, vw, face_in, depth_in, sh, rgb, normal);
    return launch_ok("raster_shade") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
