// Mesh cleanup on the device: weld equal vertices, label the connected components of an indexed
// mesh, and sum per-component area / signed volume, so that the floaters of a density mesh can be
// dropped before it is scored.  The reference has no counterpart (trimesh's split is the usual host
// route).  Semantics: include/pnr_abi.h, "Mesh cleanup"; tests/meshclean_ref.py restates them.
//
// Weld: an open-addressing table of vertex indices in the workspace (capacity a power of two >= 2 V,
// -1 = empty), keyed by the canonicalised coordinate bits (-0 -> +0).  k_weld_insert claims a slot
// with atomicCAS(-1 -> i); a slot that is taken is compared through the index the CAS RETURNED
// against the read-only coordinates: the same point lowers the slot with atomicMin, another point
// probes on.  A slot never changes its point once claimed and is never emptied, so all copies of a
// point meet in one slot and that slot ends at their lowest index whatever the arrival order.  No
// thread waits for another; a probe sequence ends because half the table stays empty.
// k_weld_lookup, a launch later, reads the settled table.
//
// Components: union-find over the vertex indices with min-hooking.  parent[x] <= x always, a root
// has parent[x] == x, and a root is only ever hooked below itself by atomicCAS(parent[hi], hi, lo):
// the root of a tree is its lowest index.  Inside the hook launch a parent written by another XCD
// is read only through agent-scope atomic loads or taken from the value a failed CAS returned,
// never re-read through a plain load (the private L2s can serve a stale line); every retry starts
// from a strictly lower index, so the loops end after finitely many steps and no thread waits for
// another (lock-free).  Path halving lowers parent[x] to a grandparent with atomicMin, which keeps
// both invariants.  k_cc_flatten, a launch later, follows the settled parents with plain loads and
// writes the labels; it writes nothing it reads.  Integer atomics only: the labels are a function
// of the mesh, not of the schedule.
//
// Sums: one workgroup per component walks the component's faces in the order the caller lists them
// (ascending face index), thread j adding positions j, j + B, j + 2 B, ... from 0, the threads
// folded by a fixed butterfly and the waves in ascending order.  The order is a function of the
// component's own face sequence: bit-identical from run to run and inside any larger mesh.
#include "mesh_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace mck {

constexpr int kThreads = PNR_MESH_CLEAN_BLOCK;
constexpr int kSumThreads = 1024, kSumWaves = kSumThreads / kWave;
constexpr int64_t kMaxVerts = (int64_t)1 << 29;   // the weld table (2 .. 4 V slots) keeps 32-bit slot indices
constexpr int kLaunches = 3;                      // init, hook, flatten

__device__ __forceinline__ uint32_t canon_bits(float x) { return __float_as_uint(x + 0.0f); }   // -0 + 0 = +0

__device__ __forceinline__ uint32_t hash3(uint32_t x, uint32_t y, uint32_t z) {
    uint32_t h = x * 0x9E3779B1u;
    h = (h << 13 | h >> 19) ^ (y * 0x85EBCA77u);
    h = (h << 13 | h >> 19) ^ (z * 0xC2B2AE3Du);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__global__ __launch_bounds__(kThreads) void k_weld_insert(const float *__restrict__ verts, uint32_t nv,
                                                          int32_t *table, uint32_t mask) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= nv) return;
    const float x = verts[3 * (size_t)i], y = verts[3 * (size_t)i + 1], z = verts[3 * (size_t)i + 2];
    if (!(x == x && y == y && z == z)) return;   // a NaN coordinate equals nothing: never in the table
    uint32_t h = hash3(canon_bits(x), canon_bits(y), canon_bits(z)) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const int32_t prev = atomicCAS(&table[h], -1, (int32_t)i);
        if (prev < 0) return;   // claimed
        const float *p = verts + 3 * (size_t)(uint32_t)prev;   // prev < nv: only indices are stored
        if (p[0] == x && p[1] == y && p[2] == z) {
            if ((uint32_t)prev > i) atomicMin(&table[h], (int32_t)i);
            return;
        }
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(kThreads) void k_weld_lookup(const float *__restrict__ verts, uint32_t nv,
                                                          const int32_t *__restrict__ table, uint32_t mask,
                                                          int32_t *__restrict__ remap) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= nv) return;
    const float x = verts[3 * (size_t)i], y = verts[3 * (size_t)i + 1], z = verts[3 * (size_t)i + 2];
    int32_t r = (int32_t)i;
    if (x == x && y == y && z == z) {
        uint32_t h = hash3(canon_bits(x), canon_bits(y), canon_bits(z)) & mask;
        for (uint32_t probe = 0; probe <= mask; ++probe) {
            const int32_t s = table[h];
            if ((uint32_t)s >= nv) break;   // empty: cannot happen after the insert pass
            const float *p = verts + 3 * (size_t)s;
            if (p[0] == x && p[1] == y && p[2] == z) {
                r = s;
                break;
            }
            h = (h + 1) & mask;
        }
    }
    remap[i] = r;
}

// ---- connected components ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_cc_init(int32_t *__restrict__ parent, uint32_t nv) {
    const uint32_t v = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (v < nv) parent[v] = (int32_t)v;
}

__device__ __forceinline__ int32_t load_parent(int32_t *parent, int32_t x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as far as this thread can see (an older value only names a node that was a root
// earlier: the CAS of the hook is what decides); at most x steps, every one to a lower index
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t x) {
    int32_t p = load_parent(parent, x);
    while (p != x) {
        const int32_t g = load_parent(parent, p);
        if (g != p) atomicMin(&parent[x], g);   // path halving: x is no root, g < p is in its tree
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b) {
    int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return;   // hi was a root and now hangs below lo
        // hi had been hooked already: go on from the parent the CAS returned (old < hi)
        ra = find_root(parent, old);
        rb = lo;
    }
}

__global__ __launch_bounds__(kThreads) void k_cc_hook(const int32_t *__restrict__ faces, uint32_t nt, uint32_t nv,
                                                      int32_t *parent, int32_t *bad) {
    const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (t >= nt) return;
    uint32_t i[3];
    if (!face_indices(faces, t, nv, i)) {
        atomicOr(bad, 1);
        return;
    }
    if (i[0] != i[1]) unite(parent, (int32_t)i[0], (int32_t)i[1]);
    if (i[1] != i[2]) unite(parent, (int32_t)i[1], (int32_t)i[2]);
}

// thread i < nv labels vertex i, thread i < nt face i; `parent` is only read here
__global__ __launch_bounds__(kThreads) void k_cc_flatten(const int32_t *__restrict__ parent, uint32_t nv,
                                                         const int32_t *__restrict__ faces, uint32_t nt,
                                                         int32_t *__restrict__ vert_label,
                                                         int32_t *__restrict__ face_label) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i < nv) {
        int32_t x = (int32_t)i, p = parent[x];
        while (p != x) {
            x = p;
            p = parent[x];
        }
        vert_label[i] = x;
    }
    if (i < nt) {
        const uint32_t i0 = (uint32_t)faces[3 * (size_t)i], i1 = (uint32_t)faces[3 * (size_t)i + 1],
                       i2 = (uint32_t)faces[3 * (size_t)i + 2];
        int32_t x = -1;   // a face with a bad index (the call fails): no label, nothing read through it
        if (i0 < nv && i1 < nv && i2 < nv) {
            x = (int32_t)i0;
            int32_t p = parent[x];
            while (p != x) {
                x = p;
                p = parent[x];
            }
        }
        face_label[i] = x;
    }
}

// ---- per-component sums ----------------------------------------------------------------------------
// the header fixes where the face terms round: no contraction
#pragma clang fp contract(off)
__device__ __forceinline__ void face_terms(const float *__restrict__ verts, uint32_t nv,
                                           const int32_t *__restrict__ faces, uint32_t nt, int64_t t, double &area,
                                           double &vol) {
    area = 0.0;
    vol = 0.0;
    if (t < 0 || t >= (int64_t)nt) return;
    uint32_t i[3];
    if (!face_indices(faces, (size_t)t, nv, i)) return;
    const float *pa = verts + 3 * (size_t)i[0], *pb = verts + 3 * (size_t)i[1], *pc = verts + 3 * (size_t)i[2];
    const double ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1],
                 cz = pc[2];
    const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    const double mx = by * cz - bz * cy, my = bz * cx - bx * cz, mz = bx * cy - by * cx;
    vol = (ax * mx + ay * my) + az * mz;
}

__global__ __launch_bounds__(kSumThreads) void k_component_sums(const float *__restrict__ verts, uint32_t nv,
                                                                const int32_t *__restrict__ faces, uint32_t nt,
                                                                const int64_t *__restrict__ order,
                                                                const int64_t *__restrict__ seg_start,
                                                                double *__restrict__ out) {
    __shared__ double s_red[2][kSumWaves];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    int64_t k0 = seg_start[c], k1 = seg_start[c + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > (int64_t)nt ? (int64_t)nt : k1;
    double acc_a = 0.0, acc_v = 0.0;
    for (int64_t k = k0 + tid; k < k1; k += kSumThreads) {
        double a, v;
        face_terms(verts, nv, faces, nt, order[k], a, v);
        acc_a += a;
        acc_v += v;
    }
    const double wa = wave_sum(acc_a), wv = wave_sum(acc_v);
    if ((tid & (kWave - 1)) == 0) {
        s_red[0][tid / kWave] = wa;
        s_red[1][tid / kWave] = wv;
    }
    __syncthreads();
    if (tid < 2) {
        double t = s_red[tid][0];
        for (int w = 1; w < kSumWaves; ++w) t += s_red[tid][w];
        out[2 * (size_t)c + tid] = tid ? t / 6.0 : t;
    }
}

static uint32_t table_capacity(int64_t nv) {
    uint32_t cap = 256;
    while ((int64_t)cap < 2 * nv) cap <<= 1;
    return cap;
}

}  // namespace mck

size_t mesh_weld_workspace_bytes(int64_t n_verts) {
    if (n_verts < 1) {
        fail(PNR_ERR_INVALID, "pnr_mesh_weld: n_verts must be >= 1 (got %lld)", (long long)n_verts);
        return 0;
    }
    if (n_verts > mck::kMaxVerts) {
        fail(PNR_ERR_UNSUPPORTED, "pnr_mesh_weld: n_verts above 2^29 (got %lld)", (long long)n_verts);
        return 0;
    }
    return align256(sizeof(int32_t) * (size_t)mck::table_capacity(n_verts));
}

int launch_mesh_weld(const float *verts, int64_t n_verts, void *ws, size_t bytes, int32_t *remap, hipStream_t st) {
    const size_t need = mesh_weld_workspace_bytes(n_verts);
    if (!need) return n_verts < 1 ? PNR_ERR_INVALID : PNR_ERR_UNSUPPORTED;
    if (!ws || bytes < need)
        return fail(PNR_ERR_WORKSPACE, "pnr_mesh_weld: workspace %zu bytes, needs %zu", bytes, need);
    const uint32_t nv = (uint32_t)n_verts, cap = mck::table_capacity(n_verts);
    int32_t *table = static_cast<int32_t *>(ws);
    if (hipMemsetAsync(table, 0xff, sizeof(int32_t) * (size_t)cap, st) != hipSuccess)   // every slot -1
        return fail(PNR_ERR_HIP, "pnr_mesh_weld: memset failed");
    const dim3 grid(blocks(nv, mck::kThreads));
    hipLaunchKernelGGL(mck::k_weld_insert, grid, dim3(mck::kThreads), 0, st, verts, nv, table, cap - 1);
    if (!launch_ok("weld_insert")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(mck::k_weld_lookup, grid, dim3(mck::kThreads), 0, st, verts, nv, table, cap - 1, remap);
    return launch_ok("weld_lookup") ? PNR_OK : PNR_ERR_HIP;
}

static int components_check(int64_t n_verts, int64_t n_faces) {
    if (n_verts < 1 || n_faces < 0)
        return fail(PNR_ERR_INVALID, "pnr_mesh_components: n_verts must be >= 1 and n_faces >= 0 (got %lld, %lld)",
                    (long long)n_verts, (long long)n_faces);
    if (n_verts > kMaxCount || n_faces > kMaxCount)
        return fail(PNR_ERR_UNSUPPORTED, "pnr_mesh_components: n_verts or n_faces above 2^31 - 1");
    return PNR_OK;
}

size_t mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    if (components_check(n_verts, n_faces)) return 0;
    return 256 + align256(sizeof(int32_t) * (size_t)n_verts);   // the flag, then the parents
}

int launch_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_verts, void *ws, size_t bytes,
                           int32_t *vert_label, int32_t *face_label, int32_t *launches, hipStream_t st) {
    int rc = components_check(n_verts, n_faces);
    if (rc) return rc;
    const size_t need = mesh_components_workspace_bytes(n_verts, n_faces);
    if (!ws || bytes < need)
        return fail(PNR_ERR_WORKSPACE, "pnr_mesh_components: workspace %zu bytes, needs %zu", bytes, need);
    const uint32_t nv = (uint32_t)n_verts, nt = (uint32_t)n_faces;
    int32_t *bad = static_cast<int32_t *>(ws);
    int32_t *parent = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + 256);
    if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess)
        return fail(PNR_ERR_HIP, "pnr_mesh_components: memset failed");
    hipLaunchKernelGGL(mck::k_cc_init, dim3(blocks(nv, mck::kThreads)), dim3(mck::kThreads), 0, st, parent, nv);
    if (!launch_ok("cc_init")) return PNR_ERR_HIP;
    if (nt) {
        hipLaunchKernelGGL(mck::k_cc_hook, dim3(blocks(nt, mck::kThreads)), dim3(mck::kThreads), 0, st, faces, nt, nv,
                           parent, bad);
        if (!launch_ok("cc_hook")) return PNR_ERR_HIP;
    }
    hipLaunchKernelGGL(mck::k_cc_flatten, dim3(blocks(nv > nt ? nv : nt, mck::kThreads)), dim3(mck::kThreads), 0, st,
                       parent, nv, faces, nt, vert_label, face_label);
    if (!launch_ok("cc_flatten")) return PNR_ERR_HIP;
    if (launches) *launches = nt ? mck::kLaunches : mck::kLaunches - 1;
    // the index flag: the one read-back, as pnr_mesh_sample's
    int32_t h_bad = 0;
    return read_index_flag(&h_bad, bad, sizeof(h_bad), st, n_verts, "pnr_mesh_components", "index flag");
}

int launch_mesh_component_sums(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                               const int64_t *order, const int64_t *seg_start, int64_t n_components, double *out,
                               hipStream_t st) {
    if (n_verts < 1 || n_faces < 1 || n_components < 1)
        return fail(PNR_ERR_INVALID, "pnr_mesh_component_sums: n_verts, n_faces and n_components must be >= 1");
    if (n_verts > kMaxCount || n_faces > kMaxCount || n_components > kMaxCount)
        return fail(PNR_ERR_UNSUPPORTED, "pnr_mesh_component_sums: a count above 2^31 - 1");
    hipLaunchKernelGGL(mck::k_component_sums, dim3((uint32_t)n_components), dim3(mck::kSumThreads), 0, st, verts,
                       (uint32_t)n_verts, faces, (uint32_t)n_faces, order, seg_start, out);
    return launch_ok("component_sums") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
