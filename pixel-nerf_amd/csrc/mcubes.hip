// Isosurface extraction (marching cubes) on the device: the mesh step of eval/eval.py:105
// (skimage.measure.marching_cubes) and src/util/recon.py:71 (mcubes.marching_cubes) on a grid that
// is already in HBM.  Semantics: include/pnr_abi.h, "Isosurface extraction"; tests/mc_ref.py
// restates them in numpy and the outputs are compared bit for bit.
//
// Output order is part of the contract: vertices by (owner grid point, axis), faces by (cell,
// position in the case table), both in the grid's linear order ((x * ny + y) * nz + z).  A
// workgroup's share of the output is contiguous only if its share of the grid is contiguous in
// that order, so a "brick" is a run of kBrick = 1024 consecutive linear indices: whole z-rows
// (lanes along z, coalesced loads; the +y / +x neighbours of a wave are two more coalesced rows
// that the next row's / plane's workgroups read again out of L2).  No LDS staging: a run has no
// compact halo (its +x neighbours are a whole plane away), and the pass is bound by the edge map
// and output bytes, not by the re-read of the grid ("Isosurface extraction").
//
// Three passes, no atomics, nothing allocated:
//   k_mc_count       per brick, the (vertices, triangles) it will emit, packed in one word
//   k_mc_scan        one workgroup: exclusive scan of the brick counts (int64), the two totals
//   k_mc_emit_verts  recomputes the crossings; vertex at its scanned slot, slot (or -1) into the
//                    edge map, one int32 per (grid point, axis)
//   k_mc_emit_faces  recomputes the case; three edge-map lookups per triangle (owner = this
//                    grid point or a +1 neighbour)
// Inside a brick the slot of a point is a DPP wave scan plus an LDS step over the four waves.
#include <cstring>

#include "pnr_common.h"
#include "pnr_launch.h"

namespace pnr {

#define PNR_MC_TABLE_QUAL static const
#define PNR_MC_TABLE_NAME kMcTable
#define PNR_MC_NTRI_NAME kMcNtri
#include "mc_table.h"
#undef PNR_MC_TABLE_QUAL
#undef PNR_MC_TABLE_NAME
#undef PNR_MC_NTRI_NAME

namespace mck {

#define PNR_MC_TABLE_QUAL static __constant__
#define PNR_MC_TABLE_NAME d_table
#define PNR_MC_NTRI_NAME d_ntri
#include "mc_table.h"
#undef PNR_MC_TABLE_QUAL
#undef PNR_MC_TABLE_NAME
#undef PNR_MC_NTRI_NAME

constexpr int kThreads = 256, kWaves = kThreads / kWave, kIters = 4, kBrick = kThreads * kIters;
constexpr int kMaxDim = 1024;

struct Dims {
    int nx, ny, nz;
    uint32_t n, sy, sx;   // points (<= 2^30), stride of +y (nz) and of +x (ny * nz)
};

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false);
}
// inclusive sum scan over the 64 lanes (the sequence of wave_scan_mul, pnr_common.h); every lane
// of the wave must be active
__device__ __forceinline__ int wave_scan_add_i(int x) {
    x += dpp_i<0x111>(0, x);          // row_shr:1
    x += dpp_i<0x112>(0, x);          // row_shr:2
    x += dpp_i<0x114>(0, x);          // row_shr:4
    x += dpp_i<0x118>(0, x);          // row_shr:8
    x += dpp_i<0x142, 0xa>(0, x);     // row_bcast:15 -> rows 1, 3
    x += dpp_i<0x143, 0xc>(0, x);     // row_bcast:31 -> rows 2, 3
    return x;
}

// One grid point p = (i, j, k): its value, the values of its +x / +y / +z neighbours, which of its
// three owned edges cross the level (bit a = axis a), and, if it is the minimum corner of a cell,
// the cell's case (otherwise -1).  NaN > level is false: NaN is outside.
struct Point {
    int i, j, k;
    float v0, v[3];
    int cross, cas;
};

template <bool WANT_CASE>
__device__ __forceinline__ Point classify(const float *__restrict__ g, const Dims &d, uint32_t p, float level) {
    Point pt;
    const uint32_t r = p / (uint32_t)d.nz;
    pt.k = (int)(p - r * (uint32_t)d.nz);
    pt.i = (int)(r / (uint32_t)d.ny);
    pt.j = (int)(r - (uint32_t)pt.i * (uint32_t)d.ny);
    const bool hx = pt.i + 1 < d.nx, hy = pt.j + 1 < d.ny, hz = pt.k + 1 < d.nz;
    pt.v0 = g[p];
    pt.v[0] = hx ? g[p + d.sx] : pt.v0;
    pt.v[1] = hy ? g[p + d.sy] : pt.v0;
    pt.v[2] = hz ? g[p + 1] : pt.v0;
    const int in0 = pt.v0 > level, inx = pt.v[0] > level, iny = pt.v[1] > level, inz = pt.v[2] > level;
    pt.cross = (int)(hx && inx != in0) | (int)(hy && iny != in0) << 1 | (int)(hz && inz != in0) << 2;
    pt.cas = -1;
    if (WANT_CASE && hx && hy && hz) {
        const int c3 = g[p + d.sx + d.sy] > level, c5 = g[p + d.sx + 1] > level, c6 = g[p + d.sy + 1] > level,
                  c7 = g[p + d.sx + d.sy + 1] > level;
        pt.cas = in0 | inx << 1 | iny << 2 | c3 << 3 | inz << 4 | c5 << 5 | c6 << 6 | c7 << 7;
    }
    return pt;
}

// k_mc_count: counts[brick] = vertices | triangles << 16 (at most 3 and 5 per point: 3072 and 5120
// per brick)
__global__ __launch_bounds__(kThreads) void k_mc_count(const float *__restrict__ g, Dims d, float level,
                                                       uint32_t *__restrict__ counts) {
    __shared__ int s_w[kWaves];
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)kBrick;
    int packed = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const uint32_t p = base + it * kThreads + tid;
        if (p < d.n) {
            const Point pt = classify<true>(g, d, p, level);
            packed += __popc(pt.cross) | (pt.cas >= 0 ? (int)d_ntri[pt.cas] : 0) << 16;
        }
    }
    const int incl = wave_scan_add_i(packed);
    if ((tid & 63) == 63) s_w[tid >> 6] = incl;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = (uint32_t)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
}

// k_mc_scan: offs[brick] = {vertices, triangles} emitted before the brick (int64); the totals go
// to the workspace (pnr_mc_emit reads them) and to the caller's slot.  One workgroup walks the
// bricks in chunks of 256 with a running carry.
__global__ __launch_bounds__(kThreads) void k_mc_scan(const uint32_t *__restrict__ counts, uint32_t nb,
                                                      int64_t *__restrict__ offs, int64_t *__restrict__ totals,
                                                      int64_t *__restrict__ counts_dev) {
    __shared__ int s_v[2][kWaves], s_t[2][kWaves];
    const int tid = threadIdx.x, wave = tid >> 6;
    int64_t carry_v = 0, carry_t = 0;
    int buf = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kThreads, buf ^= 1) {
        const uint32_t b = b0 + tid;
        const uint32_t c = b < nb ? counts[b] : 0u;
        const int v = (int)(c & 0xffffu), t = (int)(c >> 16);
        const int iv = wave_scan_add_i(v), itr = wave_scan_add_i(t);
        if ((tid & 63) == 63) {
            s_v[buf][wave] = iv;
            s_t[buf][wave] = itr;
        }
        __syncthreads();   // one barrier per chunk: the buffers alternate
        int pre_v = 0, pre_t = 0, tot_v = 0, tot_t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            pre_v += w < wave ? s_v[buf][w] : 0;
            pre_t += w < wave ? s_t[buf][w] : 0;
            tot_v += s_v[buf][w];
            tot_t += s_t[buf][w];
        }
        if (b < nb) {
            offs[2 * (size_t)b] = carry_v + pre_v + iv - v;
            offs[2 * (size_t)b + 1] = carry_t + pre_t + itr - t;
        }
        carry_v += tot_v;
        carry_t += tot_t;
    }
    if (tid == 0) {
        totals[0] = carry_v;
        totals[1] = carry_t;
        counts_dev[0] = carry_v;
        counts_dev[1] = carry_t;
    }
}

// exclusive position of this thread's `n` items among the brick's, in (iteration, thread) order =
// linear grid order; `run` carries the items of the earlier iterations.  One barrier: s_w is
// indexed by the iteration.
__device__ __forceinline__ int brick_slot(int n, int it, int tid, int (*s_w)[kWaves], int &run) {
    const int wave = tid >> 6;
    const int incl = wave_scan_add_i(n);
    if ((tid & 63) == 63) s_w[it][wave] = incl;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        pre += w < wave ? s_w[it][w] : 0;
        tot += s_w[it][w];
    }
    const int excl = run + pre + incl - n;
    run += tot;
    return excl;
}

// k_mc_emit_verts: the vertex of every owned crossing edge at its slot, and the slot (or -1) in
// edge_map[3 p + axis].  Position along the edge from the lower-index corner a to the higher b:
// t = (level - a) / (b - a), NaN or below 0 -> 0, above 1 -> 1, coordinate = index + t; each
// operation rounded once (no contraction), so the result does not depend on which cell asks.
// Nothing is stored at or past verts_cap.
__global__ __launch_bounds__(kThreads) void k_mc_emit_verts(const float *__restrict__ g, Dims d, float level,
                                                            const int64_t *__restrict__ offs,
                                                            float *__restrict__ verts, int64_t verts_cap,
                                                            int32_t *__restrict__ edge_map) {
    __shared__ int s_w[kIters][kWaves];
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)kBrick;
    const int64_t first = offs[2 * (size_t)blockIdx.x];
    int run = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const uint32_t p = base + it * kThreads + tid;
        const bool live = p < d.n;
        Point pt;
        pt.cross = 0;
        if (live) pt = classify<false>(g, d, p, level);
        int64_t slot = first + brick_slot(__popc(pt.cross), it, tid, s_w, run);
        if (!live) continue;
        const float at[3] = {(float)pt.i, (float)pt.j, (float)pt.k};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int32_t m = -1;
            if (pt.cross >> a & 1) {
                float t = __fdiv_rn(__fsub_rn(level, pt.v0), __fsub_rn(pt.v[a], pt.v0));
                t = t > 0.f ? t : 0.f;
                t = t < 1.f ? t : 1.f;
                if ((uint64_t)slot < (uint64_t)verts_cap) {   // also false for a negative slot (a foreign workspace)
                    float *o = verts + 3 * slot;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = c == a ? __fadd_rn(at[c], t) : at[c];
                    m = (int32_t)slot;
                }
                ++slot;
            }
            edge_map[3 * (size_t)p + a] = m;
        }
    }
}

// k_mc_emit_faces: the triangles of every cell at their slots; a triangle's three vertices are the
// edge-map entries of its three edges (edge e = 4 axis + j: owner = this point + the (j & 1,
// j >> 1) offset on the two other axes).  Nothing is stored at or past faces_cap.
__global__ __launch_bounds__(kThreads) void k_mc_emit_faces(const float *__restrict__ g, Dims d, float level,
                                                            const int64_t *__restrict__ offs,
                                                            const int32_t *__restrict__ edge_map,
                                                            int32_t *__restrict__ faces, int64_t faces_cap) {
    __shared__ int s_w[kIters][kWaves];
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)kBrick;
    const int64_t first = offs[2 * (size_t)blockIdx.x + 1];
    int run = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const uint32_t p = base + it * kThreads + tid;
        int cas = -1;
        if (p < d.n) cas = classify<true>(g, d, p, level).cas;
        const int nt = cas >= 0 ? (int)d_ntri[cas] : 0;
        const int64_t slot = first + brick_slot(nt, it, tid, s_w, run);
        for (int q = 0; q < nt; ++q) {
            if ((uint64_t)(slot + q) >= (uint64_t)faces_cap) break;   // also a negative slot
            int32_t *o = faces + 3 * (slot + q);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = d_table[cas][3 * q + c];
                const int a = e >> 2, u = e & 1, v = e >> 1 & 1;
                const uint32_t dx = a == 0 ? 0 : u, dy = a == 0 ? u : (a == 1 ? 0 : v), dz = a == 2 ? 0 : v;
                const uint32_t owner = p + dx * d.sx + dy * d.sy + dz;
                o[c] = edge_map[3 * (size_t)owner + a];
            }
        }
    }
}

struct Plan {
    Dims d;
    uint32_t nb;
    size_t off_cnt, off_offs, off_map, total;   // totals (2 x int64) at offset 0
    bool empty;                                 // a dimension of 1: no cells
};

static int plan(int nx, int ny, int nz, Plan &pl) {
    if (nx < 1 || ny < 1 || nz < 1) return fail(PNR_ERR_INVALID, "marching cubes: grid dimensions must be >= 1");
    if (nx > kMaxDim || ny > kMaxDim || nz > kMaxDim)
        return fail(PNR_ERR_UNSUPPORTED, "marching cubes: grid dimensions above %d (got %d x %d x %d)", kMaxDim, nx,
                    ny, nz);
    pl.d = Dims{nx, ny, nz, (uint32_t)nx * (uint32_t)ny * (uint32_t)nz, (uint32_t)nz, (uint32_t)ny * (uint32_t)nz};
    pl.nb = (pl.d.n + kBrick - 1) / kBrick;
    pl.empty = nx < 2 || ny < 2 || nz < 2;
    pl.off_cnt = 256;
    pl.off_offs = pl.off_cnt + align256(sizeof(uint32_t) * (size_t)pl.nb);
    pl.off_map = pl.off_offs + align256(2 * sizeof(int64_t) * (size_t)pl.nb);
    pl.total = pl.off_map + align256(3 * sizeof(int32_t) * (size_t)pl.d.n);
    return PNR_OK;
}

}  // namespace mck

size_t mc_workspace_bytes(int nx, int ny, int nz) {
    mck::Plan pl;
    return mck::plan(nx, ny, nz, pl) == PNR_OK ? pl.total : 0;
}

void mc_case_table(int8_t out[256][16]) { memcpy(out, kMcTable, sizeof(kMcTable)); }

int launch_mc_count(const float *grid, int nx, int ny, int nz, float level, void *ws, size_t bytes,
                    int64_t *counts_dev, hipStream_t st) {
    mck::Plan pl;
    int rc = mck::plan(nx, ny, nz, pl);
    if (rc) return rc;
    if (bytes < pl.total) return fail(PNR_ERR_WORKSPACE, "pnr_mc_count: workspace %zu bytes, needs %zu", bytes, pl.total);
    char *w = static_cast<char *>(ws);
    int64_t *totals = reinterpret_cast<int64_t *>(w);
    if (pl.empty) {
        if (hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(counts_dev, 0, 2 * sizeof(int64_t), st) != hipSuccess)
            return fail(PNR_ERR_HIP, "pnr_mc_count: memset failed");
        return PNR_OK;
    }
    uint32_t *counts = reinterpret_cast<uint32_t *>(w + pl.off_cnt);
    int64_t *offs = reinterpret_cast<int64_t *>(w + pl.off_offs);
    hipLaunchKernelGGL(mck::k_mc_count, dim3(pl.nb), dim3(mck::kThreads), 0, st, grid, pl.d, level, counts);
    if (!launch_ok("mc_count")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(mck::k_mc_scan, dim3(1), dim3(mck::kThreads), 0, st, counts, pl.nb, offs, totals, counts_dev);
    return launch_ok("mc_scan") ? PNR_OK : PNR_ERR_HIP;
}

int launch_mc_emit(const float *grid, int nx, int ny, int nz, float level, void *ws, size_t bytes, float *verts,
                   int64_t verts_cap, int32_t *faces, int64_t faces_cap, hipStream_t st) {
    mck::Plan pl;
    int rc = mck::plan(nx, ny, nz, pl);
    if (rc) return rc;
    if (bytes < pl.total) return fail(PNR_ERR_WORKSPACE, "pnr_mc_emit: workspace %zu bytes, needs %zu", bytes, pl.total);
    char *w = static_cast<char *>(ws);
    if (!pl.empty) {
        const int64_t *offs = reinterpret_cast<const int64_t *>(w + pl.off_offs);
        int32_t *edge_map = reinterpret_cast<int32_t *>(w + pl.off_map);
        hipLaunchKernelGGL(mck::k_mc_emit_verts, dim3(pl.nb), dim3(mck::kThreads), 0, st, grid, pl.d, level, offs,
                           verts, verts_cap, edge_map);
        if (!launch_ok("mc_emit_verts")) return PNR_ERR_HIP;
        hipLaunchKernelGGL(mck::k_mc_emit_faces, dim3(pl.nb), dim3(mck::kThreads), 0, st, grid, pl.d, level, offs,
                           edge_map, faces, faces_cap);
        if (!launch_ok("mc_emit_faces")) return PNR_ERR_HIP;
    }
    // the totals of pnr_mc_count against the capacities: the one read-back of this call
    int64_t tot[2] = {0, 0};
    if (hipMemcpyAsync(tot, w, sizeof(tot), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(PNR_ERR_HIP, "pnr_mc_emit: reading the totals failed: %s", hipGetErrorString(hipGetLastError()));
    if (tot[0] > verts_cap || tot[1] > faces_cap)
        return fail(PNR_ERR_INVALID,
                    "pnr_mc_emit: capacities (%lld vertices, %lld faces) below the counted %lld and %lld; the "
                    "outputs are truncated",
                    (long long)verts_cap, (long long)faces_cap, (long long)tot[0], (long long)tot[1]);
    return PNR_OK;
}

}  // namespace pnr
