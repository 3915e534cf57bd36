// Mesh containment on the device: the generalized winding number of an indexed triangle mesh at a
// set of query points, and uniform samples of an axis-aligned box to put them at (volumetric IoU,
// Occupancy Networks' third headline score).  The reference has no counterpart: its eval/eval.py
// stops at the STL.  Semantics: include/pnr_abi.h, "Mesh containment"; tests/winding_ref.py restates
// them in numpy.
//
// The winding number is the sum over the faces of the solid angle each subtends at the query (van
// Oosterom & Strackee 1983: tan(Omega / 2) = a.(b x c) / (|a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)),
// over 4 pi.  No predicate, no ray: marching-cubes vertices lie on grid lines, where a ray from a
// grid point grazes edges and vertices all the time, and the surface is open where it meets the grid
// border, where parity means nothing and the winding number degrades to a fraction.
//
// Tiling as k_nearest (meshdist.hip): all pairs, queries in registers (kQpl per lane), triangles of
// one slice staged kTile at a time in LDS, gathered through `faces` while staging.  The tile is SoA
// in records of four triangles, {ax[4], ay[4], az[4], bx[4], ... cz[4]}: nine ds_read_b128 whose
// every lane reads the same address (a broadcast) feed four triangles.  A face with a bad index, and
// the rows that pad a partial tile, are the triangle (0, 0, 0), (0, 0, 0), (0, 0, 0): its a = b = c,
// the unfused cross product of two equal vectors is exactly 0, so num = 0 and den >= 0 and the
// angle is +0 (or the query is not finite and its w is NaN anyway).  Each lane adds (double)Omega
// to its query's fp64 sum in ascending face order; blockIdx.y indexes the slices, and with more
// than one k_winding_combine folds the per-slice sums in ascending slice order.  No atomics.
#include "mesh_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace wnk {

constexpr int kThreads = 256, kQpl = 2;
constexpr int kQ = PNR_WINDING_QUERIES, kTile = PNR_WINDING_TILE, kSlice = PNR_WINDING_SLICE;
constexpr int64_t kMaxSlices = 65535;       // gridDim.y
constexpr double kFourPi = 12.566370614359172;   // 4 pi rounded to fp64
static_assert(kQ == kThreads * kQpl, "kQpl queries per lane");
static_assert(kSlice % kTile == 0 && kTile % kThreads == 0 && kTile % 4 == 0, "whole tiles, whole records");

// The header fixes where the pair arithmetic rounds.  Plain operators under this pragma are never
// fused; hipcc's __fmul_rn / __fsub_rn are plain operators in ITS header, outside the pragma, where
// the default (fast) contraction may still fuse them after inlining: a fused b x c no longer
// vanishes for b == c.
#pragma clang fp contract(off)
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// Omega of one pair, the header's rule: every operator below is one rounding, every fmaf one fma
__device__ __forceinline__ float solid_angle(float px, float py, float pz, float Ax, float Ay, float Az, float Bx,
                                             float By, float Bz, float Cx, float Cy, float Cz) {
    const float ax = Ax - px, ay = Ay - py, az = Az - pz;
    const float bx = Bx - px, by = By - py, bz = Bz - pz;
    const float cx = Cx - px, cy = Cy - py, cz = Cz - pz;
    const float la = sqrtf(dot3(ax, ay, az, ax, ay, az));   // correctly rounded (hipcc's default)
    const float lb = sqrtf(dot3(bx, by, bz, bx, by, bz));
    const float lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
    const float ab = dot3(ax, ay, az, bx, by, bz), bc = dot3(bx, by, bz, cx, cy, cz), ca = dot3(cx, cy, cz, ax, ay, az);
    // b x c without fma: both products of a component round alike, so b == c gives exactly 0
    const float nx = by * cz - bz * cy;
    const float ny = bz * cx - bx * cz;
    const float nz = bx * cy - by * cx;
    const float num = dot3(ax, ay, az, nx, ny, nz);
    const float den = __builtin_fmaf(ca, lb, __builtin_fmaf(bc, la, __builtin_fmaf(ab, lc, (la * lb) * lc)));
    const float half = atan2f(num, den);
    return (num == 0.f && den == 0.f) ? 0.f : 2.0f * half;
}

// out = (slices, n) per-slice sums, or with `final` (one slice) w itself
__global__ __launch_bounds__(kThreads) void k_winding(const float *__restrict__ verts, uint32_t nv,
                                                      const int32_t *__restrict__ faces, uint32_t nt,
                                                      const float *__restrict__ points, uint32_t n,
                                                      double *__restrict__ out, int final) {
    __shared__ f4 s_t[kTile / 4][9];
    float *s_w = reinterpret_cast<float *>(s_t);
    const int tid = threadIdx.x;
    const uint32_t q0 = blockIdx.x * (uint32_t)kQ + tid;
    const uint32_t j_begin = blockIdx.y * (uint32_t)kSlice;
    const uint32_t j_end = min(j_begin + (uint32_t)kSlice, nt);
    float px[kQpl], py[kQpl], pz[kQpl];
    double acc[kQpl];
#pragma unroll
    for (int q = 0; q < kQpl; ++q) {
        const uint32_t i = q0 + q * kThreads;
        const bool live = i < n;
        px[q] = live ? points[3 * (size_t)i] : 0.f;
        py[q] = live ? points[3 * (size_t)i + 1] : 0.f;
        pz[q] = live ? points[3 * (size_t)i + 2] : 0.f;
        // an infinite coordinate counts as NaN: inf alone can cancel to a finite angle
        if (!finite3(px[q], py[q], pz[q])) px[q] = __builtin_nanf("");
        acc[q] = 0.0;
    }
    for (uint32_t j0 = j_begin; j0 < j_end; j0 += kTile) {
        __syncthreads();   // the previous tile has been read
#pragma unroll
        for (int t = tid; t < kTile; t += kThreads) {
            const uint32_t j = j0 + t;
            float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (j < j_end) {
                uint32_t fi[3];
                if (face_indices(faces, j, nv, fi)) {
                    const float *a = verts + 3 * (size_t)fi[0], *b = verts + 3 * (size_t)fi[1],
                                *c = verts + 3 * (size_t)fi[2];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        v[k] = a[k];
                        v[3 + k] = b[k];
                        v[6 + k] = c[k];
                    }
                    // as for the queries: an infinite coordinate counts as NaN
                    if (!(finite3(v[0], v[1], v[2]) && finite3(v[3], v[4], v[5]) && finite3(v[6], v[7], v[8])))
                        v[0] = __builtin_nanf("");
                }
            }
            float *w = s_w + 36 * (t >> 2) + (t & 3);
#pragma unroll
            for (int k = 0; k < 9; ++k) w[4 * k] = v[k];
        }
        __syncthreads();
        const int cnt = ((int)min((uint32_t)kTile, j_end - j0) + 3) >> 2;   // records of four
        for (int g = 0; g < cnt; ++g) {
            f4 r[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) r[k] = s_t[g][k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int q = 0; q < kQpl; ++q)
                    acc[q] += (double)solid_angle(px[q], py[q], pz[q], r[0][k], r[1][k], r[2][k], r[3][k], r[4][k],
                                                  r[5][k], r[6][k], r[7][k], r[8][k]);
            }
        }
    }
    const size_t row = (size_t)blockIdx.y * n;
#pragma unroll
    for (int q = 0; q < kQpl; ++q) {
        const uint32_t i = q0 + q * kThreads;
        if (i < n) out[row + i] = final ? acc[q] / kFourPi : acc[q];
    }
}

// the per-slice sums (slices, n) in ascending slice order from slice 0's, then over 4 pi
__global__ __launch_bounds__(kThreads) void k_winding_combine(const double *__restrict__ part, uint32_t n,
                                                              uint32_t slices, double *__restrict__ w) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n) return;
    double t = part[i];
    for (uint32_t s = 1; s < slices; ++s) t += part[(size_t)s * n + i];
    w[i] = t / kFourPi;
}

// sample s: u_k = draw k of ray s of stream PNR_RNG_VOLUME, width 3, offset 0
__global__ __launch_bounds__(kThreads) void k_box_sample(float lx, float ly, float lz, float ex, float ey, float ez,
                                                         uint64_t seed, uint32_t n, float *__restrict__ points) {
    const uint32_t s = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (s >= n) return;
    const RngSrc src{nullptr, seed, 0, PNR_RNG_VOLUME};
    points[3 * (size_t)s] = __fmaf_rn(rng_uniform(src, s, 3, 0), ex, lx);
    points[3 * (size_t)s + 1] = __fmaf_rn(rng_uniform(src, s, 3, 1), ey, ly);
    points[3 * (size_t)s + 2] = __fmaf_rn(rng_uniform(src, s, 3, 2), ez, lz);
}

struct Plan {
    uint32_t n, nt, slices;
    size_t total;   // the per-slice sums (slices, n) fp64
};

static int plan(int64_t n, int64_t n_faces, Plan &pl) {
    if (n < 1 || n_faces < 1)
        return fail(PNR_ERR_INVALID, "pnr_winding: n and n_faces must be >= 1 (got %lld, %lld)", (long long)n,
                    (long long)n_faces);
    if (n > kMaxCount || n_faces > kMaxCount || n_faces > kMaxSlices * kSlice)
        return fail(PNR_ERR_UNSUPPORTED, "pnr_winding: n or n_faces above 2^31 - 1, or n_faces above %lld (got %lld, %lld)",
                    (long long)(kMaxSlices * kSlice), (long long)n, (long long)n_faces);
    pl.n = (uint32_t)n;
    pl.nt = (uint32_t)n_faces;
    pl.slices = (uint32_t)((n_faces + kSlice - 1) / kSlice);
    // one slice writes w directly; 256 bytes keep "0 = refused" unambiguous
    pl.total = pl.slices > 1 ? align256(sizeof(double) * (size_t)pl.slices * (size_t)n) : 256;
    return PNR_OK;
}

}  // namespace wnk

size_t winding_workspace_bytes(int64_t n, int64_t n_faces) {
    wnk::Plan pl;
    return wnk::plan(n, n_faces, pl) == PNR_OK ? pl.total : 0;
}

int launch_winding(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *points,
                   int64_t n, void *ws, size_t bytes, double *w, hipStream_t st) {
    wnk::Plan pl;
    int rc = wnk::plan(n, n_faces, pl);
    if (rc) return rc;
    if (n_verts < 1) return fail(PNR_ERR_INVALID, "pnr_winding: n_verts must be >= 1 (got %lld)", (long long)n_verts);
    if (n_verts > kMaxCount) return fail(PNR_ERR_UNSUPPORTED, "pnr_winding: n_verts above 2^31 - 1");
    const dim3 grid(blocks(pl.n, wnk::kQ), pl.slices);
    if (pl.slices == 1) {
        hipLaunchKernelGGL(wnk::k_winding, grid, dim3(wnk::kThreads), 0, st, verts, (uint32_t)n_verts, faces, pl.nt,
                           points, pl.n, w, 1);
        return launch_ok("winding") ? PNR_OK : PNR_ERR_HIP;
    }
    if (!ws || bytes < pl.total)
        return fail(PNR_ERR_WORKSPACE, "pnr_winding: workspace %zu bytes, needs %zu", bytes, pl.total);
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(wnk::k_winding, grid, dim3(wnk::kThreads), 0, st, verts, (uint32_t)n_verts, faces, pl.nt, points,
                       pl.n, part, 0);
    if (!launch_ok("winding")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(wnk::k_winding_combine, dim3(blocks(pl.n, wnk::kThreads)), dim3(wnk::kThreads), 0,
                       st, part, pl.n, pl.slices, w);
    return launch_ok("winding_combine") ? PNR_OK : PNR_ERR_HIP;
}

int launch_box_sample(const float lo[3], const float ext[3], int64_t n, uint64_t seed, float *points, hipStream_t st) {
    hipLaunchKernelGGL(wnk::k_box_sample, dim3(blocks((size_t)n, wnk::kThreads)), dim3(wnk::kThreads),
                       0, st, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], seed, (uint32_t)n, points);
    return launch_ok("box_sample") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
