// Mesh reconstruction metrics on the device: area-weighted surface sampling of an indexed mesh,
// all-nearest-neighbour search between two point clouds, and the reduction of the two distance
// fields to the sums behind Chamfer-L1 / L2, accuracy / completeness, F-score and normal
// consistency (Occupancy Networks' eval_pointcloud).  The reference has no counterpart: its
// eval/eval.py stops at the STL.  Semantics: include/pnr_abi.h, "Mesh metrics"; tests/mesh_ref.py
// restates them in numpy.
//
// Sampling: area pass (one thread per triangle, fp64, face indices checked through a device flag),
// a blocked-sequential inclusive scan, one thread per sample (Philox draws, binary search).  The
// scan adds sequentially inside a chunk of kChunk = 256 triangles, sequentially over the 256 chunk
// totals of a group, and sequentially over the group totals: a level's offset of child c + 1 is
// fl(offset of c + total of c), the very sum that ends child c, so the CDF is non-decreasing and a
// zero-area triangle repeats its predecessor's value bit for bit.  It is never picked.  A tree scan
// gives neither property.  No atomics: the outputs are bit-identical from run to run.
//
// Nearest neighbour: brute force, |a - b|^2 from the coordinate differences (the expanded form
// |a|^2 + |b|^2 - 2 a.b cancels for surface samples 1e-3 apart at coordinates near 1, and the
// matrix cores can only compute that form).  A workgroup owns kQ = 1024 queries, four per lane in
// registers, and one slice of kSlice rows of b, staged kTile rows at a time in LDS: every lane
// reads the same address (a broadcast, no bank conflict) and three ds_read_b128 feed sixteen
// distance updates.  b is split over blockIdx.y as well as a over blockIdx.x, or 1e5 queries
// would leave most SIMDs idle; k_nearest_combine folds the per-slice minima in ascending slice
// order under the same strict "<", so equal distances resolve to the lowest index whatever the
// slice layout.
//
// Reduction: one workgroup per direction, each thread a strided run in ascending order, waves by
// a fixed butterfly, the wave sums in wave order; fp64 throughout.  A direction's four sums depend
// on that direction's inputs only.
#include "mesh_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace msk {

constexpr int kThreads = 256;
constexpr int kChunk = PNR_MESH_SCAN_CHUNK, kGroup = kChunk * kChunk;
static_assert(kChunk == kThreads, "one thread per chunk of a group, one chunk per thread");

// workspace header: the bad-index flag and the total area, read back by the host
struct Header {
    int32_t bad;
    int32_t pad;
    double total;
};

#pragma clang fp contract(off)
// area[t] = 0.5 |(b - a) x (c - a)| in fp64 from the fp32 vertices, each operation rounded once;
// a face with an index outside [0, V) raises the flag and counts as area 0 (nothing is read)
__global__ __launch_bounds__(kThreads) void k_ms_area(const float *__restrict__ verts, uint32_t nv,
                                                      const int32_t *__restrict__ faces, uint32_t nt,
                                                      double *__restrict__ cdf, Header *__restrict__ hdr) {
    const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (t >= nt) return;
    uint32_t i[3];
    double area = 0.0;
    if (face_indices(faces, t, nv, i)) {
        const float *a = verts + 3 * (size_t)i[0], *b = verts + 3 * (size_t)i[1], *c = verts + 3 * (size_t)i[2];
        const double ax = a[0], ay = a[1], az = a[2];
        const double ux = (double)b[0] - ax, uy = (double)b[1] - ay, uz = (double)b[2] - az;
        const double vx = (double)c[0] - ax, vy = (double)c[1] - ay, vz = (double)c[2] - az;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    } else {
        hdr->bad = 1;   // every writer stores the same value
    }
    cdf[t] = area;
}

// One workgroup per group of kChunk chunks, in place: cdf[t] becomes the inclusive sum of its
// group's areas up to t (chunk-sequential, then the chunk offsets sequential), gtot[group] the
// group's total.
__global__ __launch_bounds__(kThreads) void k_ms_scan_group(double *__restrict__ cdf, uint32_t nt,
                                                            double *__restrict__ gtot) {
    __shared__ double s_tot[kChunk], s_off[kChunk];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kGroup;
    const size_t c0 = base + (size_t)tid * kChunk;
    double acc = 0.0;
    for (int i = 0; i < kChunk; ++i) {
        const size_t e = c0 + i;
        if (e >= nt) break;
        acc += cdf[e];
        cdf[e] = acc;
    }
    s_tot[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int c = 0; c < kChunk; ++c) {
            s_off[c] = run;
            run += s_tot[c];
        }
        gtot[blockIdx.x] = run;
    }
    __syncthreads();
    for (int i = tid; i < kGroup; i += kThreads) {
        const size_t e = base + i;
        if (e >= nt) break;
        cdf[e] = s_off[i / kChunk] + cdf[e];
    }
}

// one thread: goff[g] = the groups before g, sequentially; the total to the header and the caller
__global__ void k_ms_scan_top(const double *__restrict__ gtot, uint32_t ng, double *__restrict__ goff,
                              Header *__restrict__ hdr, double *__restrict__ total_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double run = 0.0;
    for (uint32_t g = 0; g < ng; ++g) {
        goff[g] = run;
        run += gtot[g];
    }
    hdr->total = run;
    *total_out = run;
}

// sample s: (u0, u1, u2) = draws 0 .. 2 of ray s of stream PNR_RNG_MESH, width 3, offset 0
__global__ __launch_bounds__(kThreads) void k_ms_sample(const float *__restrict__ verts,
                                                        const int32_t *__restrict__ faces, uint32_t nt,
                                                        const double *__restrict__ cdf,
                                                        const double *__restrict__ goff,
                                                        const Header *__restrict__ hdr, uint64_t seed, uint32_t n,
                                                        float *__restrict__ points, float *__restrict__ normals,
                                                        int32_t *__restrict__ tri) {
    const uint32_t s = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (s >= n) return;
    const RngSrc src{nullptr, seed, 0, PNR_RNG_MESH};
    const float u0 = rng_uniform(src, s, 3, 0);
    float u1 = rng_uniform(src, s, 3, 1), u2 = rng_uniform(src, s, 3, 2);
    const double target = (double)u0 * hdr->total;
    // the first t with cdf[t] > target: cdf[nt - 1] = total > target, cdf is non-decreasing
    uint32_t lo = 0, hi = nt - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const double c = goff[mid / (uint32_t)kGroup] + cdf[mid];
        if (c > target) hi = mid;
        else lo = mid + 1;
    }
    // lo's indices passed k_ms_area's check: its area is positive
    const float *a = verts + 3 * (size_t)faces[3 * (size_t)lo], *b = verts + 3 * (size_t)faces[3 * (size_t)lo + 1],
                *c = verts + 3 * (size_t)faces[3 * (size_t)lo + 2];
    if (u1 + u2 > 1.0f) {
        u1 = 1.0f - u1;
        u2 = 1.0f - u2;
    }
    const float av[3] = {a[0], a[1], a[2]}, bv[3] = {b[0], b[1], b[2]}, cv[3] = {c[0], c[1], c[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) points[3 * (size_t)s + k] = (av[k] + u1 * (bv[k] - av[k])) + u2 * (cv[k] - av[k]);
    if (normals) {
        const double ux = (double)bv[0] - av[0], uy = (double)bv[1] - av[1], uz = (double)bv[2] - av[2];
        const double vx = (double)cv[0] - av[0], vy = (double)cv[1] - av[1], vz = (double)cv[2] - av[2];
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        normals[3 * (size_t)s] = (float)(nx / len);
        normals[3 * (size_t)s + 1] = (float)(ny / len);
        normals[3 * (size_t)s + 2] = (float)(nz / len);
    }
    if (tri) tri[s] = (int32_t)lo;
}

struct Plan {
    uint32_t nt, ng;
    size_t off_gtot, off_goff, off_cdf, total;   // Header at offset 0
};

static int plan(int64_t n_faces, Plan &pl) {
    if (n_faces < 1) return fail(PNR_ERR_INVALID, "mesh sample: n_faces must be >= 1 (got %lld)", (long long)n_faces);
    if (n_faces > kMaxCount)
        return fail(PNR_ERR_UNSUPPORTED, "mesh sample: %lld faces do not fit int32 indices", (long long)n_faces);
    pl.nt = (uint32_t)n_faces;
    pl.ng = (pl.nt + (uint32_t)kGroup - 1) / (uint32_t)kGroup;
    pl.off_gtot = 256;
    pl.off_goff = pl.off_gtot + align256(sizeof(double) * (size_t)pl.ng);
    pl.off_cdf = pl.off_goff + align256(sizeof(double) * (size_t)pl.ng);
    pl.total = pl.off_cdf + align256(sizeof(double) * (size_t)pl.nt);
    return PNR_OK;
}

}  // namespace msk

namespace nnk {

constexpr int kThreads = 256, kQpl = 4;
constexpr int kQ = PNR_NEAREST_QUERIES, kTile = PNR_NEAREST_TILE, kSlice = PNR_NEAREST_SLICE;
constexpr int kUnroll = 8;
constexpr int64_t kMaxSlices = 65535;   // gridDim.y
static_assert(kQ == kThreads * kQpl, "four queries per lane");
static_assert(kSlice % kTile == 0 && kTile % kThreads == 0 && kTile % kUnroll == 0 && kUnroll % 4 == 0, "whole tiles");

// d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of the rounded differences; a later row wins only if
// strictly nearer.  Rows of the tile past the slice's end are +inf: never nearer.
__global__ __launch_bounds__(kThreads) void k_nearest(const float *__restrict__ a, uint32_t n,
                                                      const float *__restrict__ b, uint32_t m,
                                                      float *__restrict__ d2_out, int32_t *__restrict__ idx_out) {
    // four rows of b per record, as {x[4], y[4], z[4]}: three ds_read_b128 whose every lane reads
    // the same address feed 16 distance updates, and no padding word is read
    __shared__ f4 s_b[kTile / 4][3];
    float *s_w = reinterpret_cast<float *>(s_b);
    const int tid = threadIdx.x;
    const uint32_t q0 = blockIdx.x * (uint32_t)kQ + tid;
    const uint32_t j_begin = blockIdx.y * (uint32_t)kSlice;
    const uint32_t j_end = min(j_begin + (uint32_t)kSlice, m);
    float ax[kQpl], ay[kQpl], az[kQpl], best[kQpl];
    int32_t bi[kQpl];
#pragma unroll
    for (int q = 0; q < kQpl; ++q) {
        const uint32_t i = q0 + q * kThreads;
        const bool live = i < n;
        ax[q] = live ? a[3 * (size_t)i] : 0.f;
        ay[q] = live ? a[3 * (size_t)i + 1] : 0.f;
        az[q] = live ? a[3 * (size_t)i + 2] : 0.f;
        best[q] = __builtin_inff();
        bi[q] = (int32_t)j_begin;
    }
    for (uint32_t j0 = j_begin; j0 < j_end; j0 += kTile) {
        __syncthreads();   // the previous tile has been read
#pragma unroll
        for (int t = tid; t < kTile; t += kThreads) {
            const uint32_t j = j0 + t;
            const bool live = j < j_end;
            float *w = s_w + 12 * (t >> 2) + (t & 3);
            w[0] = live ? b[3 * (size_t)j] : __builtin_inff();
            w[4] = live ? b[3 * (size_t)j + 1] : __builtin_inff();
            w[8] = live ? b[3 * (size_t)j + 2] : __builtin_inff();
        }
        __syncthreads();
        const int cnt = ((int)min((uint32_t)kTile, j_end - j0) + kUnroll - 1) & ~(kUnroll - 1);
        for (int t0 = 0; t0 < cnt; t0 += kUnroll) {
#pragma unroll
            for (int g = 0; g < kUnroll / 4; ++g) {
                const f4 px = s_b[t0 / 4 + g][0], py = s_b[t0 / 4 + g][1], pz = s_b[t0 / 4 + g][2];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int32_t j = (int32_t)(j0 + t0 + 4 * g + k);
#pragma unroll
                    for (int q = 0; q < kQpl; ++q) {
                        const float dx = __fsub_rn(ax[q], px[k]), dy = __fsub_rn(ay[q], py[k]),
                                    dz = __fsub_rn(az[q], pz[k]);
                        const float d = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
                        const bool nearer = d < best[q];
                        bi[q] = nearer ? j : bi[q];
                        best[q] = nearer ? d : best[q];
                    }
                }
            }
        }
    }
    const size_t row = (size_t)blockIdx.y * n;
#pragma unroll
    for (int q = 0; q < kQpl; ++q) {
        const uint32_t i = q0 + q * kThreads;
        if (i < n) {
            d2_out[row + i] = best[q];
            idx_out[row + i] = bi[q];
        }
    }
}

// the per-slice minima (slices, n) in ascending slice order, strict "<"
__global__ __launch_bounds__(kThreads) void k_nearest_combine(const float *__restrict__ p_d2,
                                                              const int32_t *__restrict__ p_idx, uint32_t n,
                                                              uint32_t slices, float *__restrict__ d2,
                                                              int32_t *__restrict__ idx) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n) return;
    float best = p_d2[i];
    int32_t bi = p_idx[i];
    for (uint32_t s = 1; s < slices; ++s) {
        const float d = p_d2[(size_t)s * n + i];
        if (d < best) {
            best = d;
            bi = p_idx[(size_t)s * n + i];
        }
    }
    d2[i] = best;
    idx[i] = bi;
}

struct Plan {
    uint32_t n, m, slices;
    size_t off_idx, total;   // partial d2 (slices, n) at offset 0, partial idx (slices, n) at off_idx
};

static int plan(int64_t n, int64_t m, Plan &pl) {
    if (n < 1 || m < 1)
        return fail(PNR_ERR_INVALID, "nearest: n and m must be >= 1 (got %lld, %lld)", (long long)n, (long long)m);
    if (n > kMaxCount || m > kMaxSlices * kSlice)
        return fail(PNR_ERR_UNSUPPORTED, "nearest: n above 2^31 - 1 or m above %lld (got %lld, %lld)",
                    (long long)(kMaxSlices * kSlice), (long long)n, (long long)m);
    pl.n = (uint32_t)n;
    pl.m = (uint32_t)m;
    pl.slices = (uint32_t)((m + kSlice - 1) / kSlice);
    // one slice writes the outputs directly; 256 bytes keep "0 = refused" unambiguous
    const size_t part = pl.slices > 1 ? align256(sizeof(float) * (size_t)pl.slices * (size_t)n) : 0;
    pl.off_idx = part;
    pl.total = pl.slices > 1 ? 2 * part : 256;
    return PNR_OK;
}

}  // namespace nnk

namespace mdk {

constexpr int kThreads = 1024, kWaves = kThreads / kWave;

// blockIdx.x = direction: 0 scores d2_ab / idx_ab (n entries, normals_a against normals_b[idx]),
// 1 the reverse.  out[4 dir + {0, 1, 2, 3}] = sum sqrt(d2), sum d2, count sqrt(d2) < tau,
// sum |n . n'|.
__global__ __launch_bounds__(kThreads) void k_md_reduce(const float *__restrict__ d2_ab,
                                                        const int32_t *__restrict__ idx_ab, uint32_t n,
                                                        const float *__restrict__ d2_ba,
                                                        const int32_t *__restrict__ idx_ba, uint32_t m,
                                                        const float *__restrict__ normals_a,
                                                        const float *__restrict__ normals_b, double tau,
                                                        double *__restrict__ out) {
    __shared__ double s_red[4][kWaves];
    const int tid = threadIdx.x, dir = blockIdx.x;
    const float *d2 = dir ? d2_ba : d2_ab;
    const int32_t *idx = dir ? idx_ba : idx_ab;
    const uint32_t cnt = dir ? m : n, other = dir ? n : m;
    const float *own = dir ? normals_b : normals_a, *oth = dir ? normals_a : normals_b;
    const bool with_normals = own && oth;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = tid; i < cnt; i += kThreads) {
        const double q = (double)d2[i], d = sqrt(q);
        acc[0] += d;
        acc[1] += q;
        acc[2] += d < tau ? 1.0 : 0.0;
        const uint32_t j = (uint32_t)idx[i];
        if (with_normals && j < other) {   // an index from elsewhere is skipped, never read through
            const float *p = own + 3 * (size_t)i, *r = oth + 3 * (size_t)j;
            acc[3] += fabs((double)p[0] * (double)r[0] + (double)p[1] * (double)r[1] + (double)p[2] * (double)r[2]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double w = wave_sum(acc[k]);
        if ((tid & (kWave - 1)) == 0) s_red[k][tid / kWave] = w;
    }
    __syncthreads();
    if (tid < 4) {
        double t = s_red[tid][0];
        for (int w = 1; w < kWaves; ++w) t += s_red[tid][w];
        out[4 * dir + tid] = t;
    }
}

}  // namespace mdk

size_t mesh_sample_workspace_bytes(int64_t n_faces) {
    msk::Plan pl;
    return msk::plan(n_faces, pl) == PNR_OK ? pl.total : 0;
}

int launch_mesh_sample(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int64_t n,
                       uint64_t seed, void *ws, size_t bytes, float *points, float *normals, int32_t *tri,
                       double *total_area, hipStream_t st) {
    msk::Plan pl;
    int rc = msk::plan(n_faces, pl);
    if (rc) return rc;
    if (n < 1 || n_verts < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: n and n_verts must be >= 1 (got %lld, %lld)", (long long)n,
                    (long long)n_verts);
    if (n > kMaxCount || n_verts > kMaxCount)
        return fail(PNR_ERR_UNSUPPORTED, "pnr_mesh_sample: n or n_verts above 2^31 - 1");
    if (!ws || bytes < pl.total)
        return fail(PNR_ERR_WORKSPACE, "pnr_mesh_sample: workspace %zu bytes, needs %zu", bytes, pl.total);
    char *w = static_cast<char *>(ws);
    msk::Header *hdr = reinterpret_cast<msk::Header *>(w);
    double *gtot = reinterpret_cast<double *>(w + pl.off_gtot), *goff = reinterpret_cast<double *>(w + pl.off_goff);
    double *cdf = reinterpret_cast<double *>(w + pl.off_cdf);
    if (hipMemsetAsync(hdr, 0, sizeof(msk::Header), st) != hipSuccess)
        return fail(PNR_ERR_HIP, "pnr_mesh_sample: memset failed");
    hipLaunchKernelGGL(msk::k_ms_area, dim3(blocks(pl.nt, msk::kThreads)), dim3(msk::kThreads), 0, st, verts,
                       (uint32_t)n_verts, faces, pl.nt, cdf, hdr);
    if (!launch_ok("ms_area")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(msk::k_ms_scan_group, dim3(pl.ng), dim3(msk::kThreads), 0, st, cdf, pl.nt, gtot);
    if (!launch_ok("ms_scan_group")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(msk::k_ms_scan_top, dim3(1), dim3(64), 0, st, gtot, pl.ng, goff, hdr, total_area);
    if (!launch_ok("ms_scan_top")) return PNR_ERR_HIP;
    // the flag and the total before anything is read through a face index: the one read-back
    msk::Header h;
    rc = read_index_flag(&h, hdr, sizeof(h), st, n_verts, "pnr_mesh_sample", "totals");
    if (rc) return rc;
    if (!(h.total > 0.0) || !(h.total < __builtin_inf()))
        return fail(PNR_ERR_INVALID, "pnr_mesh_sample: the total area is %g, nothing to sample", h.total);
    hipLaunchKernelGGL(msk::k_ms_sample, dim3(blocks((size_t)n, msk::kThreads)), dim3(msk::kThreads), 0, st, verts,
                       faces, pl.nt, cdf, goff, hdr, seed, (uint32_t)n, points, normals, tri);
    return launch_ok("ms_sample") ? PNR_OK : PNR_ERR_HIP;
}

size_t nearest_workspace_bytes(int64_t n, int64_t m) {
    nnk::Plan pl;
    return nnk::plan(n, m, pl) == PNR_OK ? pl.total : 0;
}

int launch_nearest(const float *a, int64_t n, const float *b, int64_t m, void *ws, size_t bytes, float *d2,
                   int32_t *idx, hipStream_t st) {
    nnk::Plan pl;
    int rc = nnk::plan(n, m, pl);
    if (rc) return rc;
    const dim3 grid(blocks(pl.n, nnk::kQ), pl.slices);
    if (pl.slices == 1) {
        hipLaunchKernelGGL(nnk::k_nearest, grid, dim3(nnk::kThreads), 0, st, a, pl.n, b, pl.m, d2, idx);
        return launch_ok("nearest") ? PNR_OK : PNR_ERR_HIP;
    }
    if (!ws || bytes < pl.total)
        return fail(PNR_ERR_WORKSPACE, "pnr_nearest: workspace %zu bytes, needs %zu", bytes, pl.total);
    char *w = static_cast<char *>(ws);
    float *p_d2 = reinterpret_cast<float *>(w);
    int32_t *p_idx = reinterpret_cast<int32_t *>(w + pl.off_idx);
    hipLaunchKernelGGL(nnk::k_nearest, grid, dim3(nnk::kThreads), 0, st, a, pl.n, b, pl.m, p_d2, p_idx);
    if (!launch_ok("nearest")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(nnk::k_nearest_combine, dim3(blocks(pl.n, nnk::kThreads)), dim3(nnk::kThreads),
                       0, st, p_d2, p_idx, pl.n, pl.slices, d2, idx);
    return launch_ok("nearest_combine") ? PNR_OK : PNR_ERR_HIP;
}

int launch_mesh_distance_reduce(const float *d2_ab, const int32_t *idx_ab, int64_t n, const float *d2_ba,
                                const int32_t *idx_ba, int64_t m, const float *normals_a, const float *normals_b,
                                double tau, double *out, hipStream_t st) {
    if (n < 1 || m < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_distance_reduce: n and m must be >= 1 (got %lld, %lld)", (long long)n,
                    (long long)m);
    if (n > kMaxCount || m > kMaxCount)
        return fail(PNR_ERR_UNSUPPORTED, "pnr_mesh_distance_reduce: n or m above 2^31 - 1");
    hipLaunchKernelGGL(mdk::k_md_reduce, dim3(2), dim3(mdk::kThreads), 0, st, d2_ab, idx_ab, (uint32_t)n, d2_ba,
                       idx_ba, (uint32_t)m, normals_a, normals_b, tau, out);
    return launch_ok("md_reduce") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
