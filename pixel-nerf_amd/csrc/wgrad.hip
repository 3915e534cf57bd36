// Weight gradients of the ResnetFC 512 x 512 layers (training backward).
//
// Replaces the weight-gradient GEMMs autograd runs for every nn.Linear of ResnetFC
// (resnetfc.py:132-184): G_j = dY_j^T X_j (512 x 512), a sum over the P points of the
// outer products of the layer's output gradient dY_j and its input X_j, both P x 512
// fp32 row-major (the dy slots of pnr_mlp_backward and the activation save).
//
// Work decomposition (both kernels):
//   * a workgroup (8 waves, one per CU) owns a 256 x 256 output block of one layer over a
//     chunk of points; wave w owns 128 x 64 of it (n half w & 1, k quarter w >> 1):
//     8 x 4 tiles of 16 x 16, 128 accumulator VGPRs;
//   * points advance in steps of 32 (one MFMA k-step): each thread loads 16 floats of one
//     point row of dY and of X (16 threads per 1 KB row), splits them and stores the parts
//     row-major ([point][column], 544-B rows: 512 B + 32 B pad);  MFMA operands (8
//     consecutive points of one column per lane) come back with ds_read_b64_tr_b16, the
//     hardware transpose read.  Point p of a step is stored at row pi(p) (bits 2 and 3
//     swapped): the 8 rows one 32-lane half of a transpose read touches then sit 8 banks
//     apart under the 136-dword pitch (conflict-free), every 8-lane group of a
//     ds_write_b128 stores 128 consecutive bytes (conflict-free), and a tile's operand is
//     a constant byte offset from the lane's base (immediate offsets, no address VALU);
//   * split-K over point chunks with deterministic per-chunk partials and a fixed-order
//     reduction (k_wgrad_reduce); the 4 blocks of one (layer, chunk) run on one XCD so
//     each dY / X column block's 2x reuse is served from that XCD's L2.
//
// k_wgrad_h (default): f16x3 products on v_mfma_f32_16x16x32_f16 -- every operand scaled by
// a power of two per (chunk, channel) and split into two fp16 parts (22 significand bits),
// hi*hi + hi*lo + lo*hi: half the MFMAs of the split-bf16 kernel.  The two-part images take
// 68 KB, so they are double-buffered: step s + 1's split runs in four pieces between step s's
// MFMAs (the scheduler interleaves the VALU and the LDS stores with them), one barrier per step.
// Scales: a running per-channel exponent E_c (the operand is v 2^-E_c).  A split value that
// reaches 2^15 raises a flag; after the step's barrier the workgroup then re-reads that step,
// takes the channel maxima (LDS atomics), moves E_c of the overflowing channels so that the
// maximum lands in [2^5, 2^6), multiplies the accumulator rows / columns by 2^(E_old - E_new)
// (exact) and splits the step again.  The chunk's first 4 steps set the first scales; a channel
// still all zero then takes its tensor's maximum (on a training step's data, channels turning
// on later were 98 % of the scale moves).  Measured: 0.34 % of a training step's 32-point steps
// retune.  Every value keeps 22 bits down to 2^-8 of its channel's running maximum, and an
// absolute error below 2^-30 of that maximum beneath it; the result is acc 2^(E_row + E_col).
//
// Bound of k_wgrad_h, per output element: an element whose terms all come from values far
// below their channel's running maximum M in the chunk (e.g. X_j nonzero only where dY_i is
// 2^-20 of M_i) keeps only the absolute error ~2^-30 M of those values, not fp32 relative error:
// values below 2^-8 M lose low bits (the second fp16 part goes subnormal), values below ~2^-19 M
// lose the first part's bits too, and below ~2^-30 M they flush to zero.
// (tests/test_gpu_train.py::test_weight_grad_wide_dynamic_range measures both kernels.)
//
// k_wgrad (PNR_WGRAD_BF16X6, ABI 4, per call; the round-2 kernel): split-bf16 products on
// v_mfma_f32_16x16x32_bf16, three exact bf16 parts per operand and the six largest products
// (dropped terms < 2^-24 |x y|), no scaling (bf16 has fp32's exponent range); one image set,
// split and MFMAs separated by two barriers per step.
#include "pnr_common.h"
#include "pnr_launch.h"

namespace pnr {
namespace wg {

constexpr int H = 512;
constexpr int BM = 256;                  // output block edge
constexpr int PS = 32;                   // points per step (MFMA k)
constexpr int NTHR = 512;
constexpr int PITCH = 2 * BM + 32;       // bytes per image row (bank offset 8 per row)
constexpr int IMG_BYTES = PS * PITCH;    // one bf16 part image: 17,408 B
constexpr int LDS_BYTES = 6 * IMG_BYTES; // dY and X, 3 parts each = 104,448 B
constexpr int MAX_JOBS = 16;

struct Args {
    const float *dy[MAX_JOBS];
    const float *x[MAX_JOBS];
    float *partial;          // [job][chunk][512][512]
    int n_jobs, chunks, n_units;
    int64_t n_points, chunk_points;
};

typedef short s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4 lds_s4;

// image row of point p (0..31) of a step: bits 2 and 3 swapped
__device__ __forceinline__ int prow(int p) { return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1); }

// MFMA operand of 16 columns: lane l receives column c0 + (l & 15), points 8 (l >> 4) ..
// + 7.  `base` = image + 2 c0 bytes; lo / hi = the lane's byte offsets of its points
// 8g + q and 8g + 4 + q (q = (l & 15) >> 2) plus 8 ((l & 3)) within the 16 columns.
// V = bf8 or h8: the same 16 bytes either way.
template <typename V>
__device__ __forceinline__ V tr_frag(const char *base, int lo, int hi) {
    const s4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4 *)(base + lo));
    const s4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4 *)(base + hi));
    typedef short s8 __attribute__((ext_vector_type(8)));
    const s8 v = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return __builtin_bit_cast(V, v);
}

// Shared by both kernels.  blockIdx -> (unit u = (job, chunk), block (nb, kb) of its 4); the 4 blocks of a unit share an
// XCD.  Points [p0, p1) are the unit's chunk.
struct Unit {
    int u, job, chunk, nb, kb;
    int64_t p0, p1;
};
// false for the workgroups past the last unit (the whole workgroup: uniform)
__device__ __forceinline__ bool unit_of(const Args &a, Unit &t) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3, b4 = local & 3;
    t.u = 8 * (local >> 2) + xcd;
    if (t.u >= a.n_units) return false;
    t.job = t.u / a.chunks, t.chunk = t.u % a.chunks;
    t.nb = b4 & 1, t.kb = b4 >> 1;
    t.p0 = (int64_t)t.chunk * a.chunk_points;
    t.p1 = t.p0 + a.chunk_points < a.n_points ? t.p0 + a.chunk_points : a.n_points;
    return true;
}

// staging role of a thread: point r of the step, columns 8j .. 8j+7 and 128+8j .. 128+8j+7 (j = t & 15)
// of the block's dY and X; woff = its byte offset in an image (+ 256 for the second 8 columns)
struct Stage {
    int r, jc, woff;
    const float *dsrc, *xsrc;
};
__device__ __forceinline__ Stage stage_of(const Args &a, const Unit &t, int tid) {
    Stage s;
    s.r = tid >> 4, s.jc = tid & 15;
    s.dsrc = a.dy[t.job] + t.nb * BM + 8 * s.jc;
    s.xsrc = a.x[t.job] + t.kb * BM + 8 * s.jc;
    s.woff = PITCH * prow(s.r) + 16 * s.jc;
    return s;
}

// the thread's 16 + 16 floats of point row p: 4 f4 of dY and 4 of X.  Returns ok = the row is a
// point of the chunk; a row past it reads row 0 (an in-bounds address) and is staged as zeros.
__device__ __forceinline__ bool load_row(const Stage &s, int64_t p, int64_t p1, f4 (&d)[4], f4 (&x)[4]) {
    const bool ok = p < p1;
    const int64_t pc = ok ? p : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = 128 * (i >> 1) + 4 * (i & 1);
        d[i] = *reinterpret_cast<const f4 *>(s.dsrc + pc * H + col);
        x[i] = *reinterpret_cast<const f4 *>(s.xsrc + pc * H + col);
    }
    return ok;
}

// a wave's 128 x 64 of the block: 8 x 4 tiles of 16 x 16
typedef f4 BlockAcc[8][4];
__device__ __forceinline__ void acc_zero(BlockAcc &acc) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
}

// a lane's place in its wave's tiles: the wave's corner (n0, k0) of the block, the lane's C rows
// 4 g + e and column li of a tile, and its transpose-read offsets t_lo / t_hi
struct TileLane {
    int n0, k0, g, li, t_lo, t_hi;
};
// the lane's transpose-read byte offset of points 8g + 4 half + q, column pair pp
__device__ __forceinline__ int tr_off(int lane, int half) {
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
    return PITCH * prow(8 * g + 4 * half + q) + 8 * pp;
}
__device__ __forceinline__ TileLane tile_lane(int wave, int lane) {
    return TileLane{128 * (wave & 1), 64 * (wave >> 1), lane >> 4, lane & 15, tr_off(lane, 0), tr_off(lane, 1)};
}

// partial block of unit u: C rows (n) 4 (l >> 4) + e, column (k) l & 15 of each 16 x 16 tile;
// finish(value, i, j, e) is the stored element
template <typename F>
__device__ __forceinline__ void store_block(const Args &a, const Unit &t, const TileLane &tl, const BlockAcc &acc,
                                            F finish) {
    float *out = a.partial + (int64_t)t.u * H * H + (int64_t)(t.nb * BM + tl.n0) * H + t.kb * BM + tl.k0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                out[(int64_t)(16 * i + 4 * tl.g + e) * H + 16 * j + tl.li] = finish(acc[i][j][e], i, j, e);
}

__global__ __launch_bounds__(NTHR, 1) void k_wgrad(Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    Unit U;
    if (!unit_of(a, U)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Stage S = stage_of(a, U, tid);
    f4 sd[4], sx[4];   // the staged row (load_row)
    bool ok = true;    // it is a point of the chunk (else it is staged as zeros)
    // The zeroing of a row past the chunk happens in put(), not after the loads: a select right
    // after them made the compiler wait for them (s_waitcnt vmcnt(0)) before the step's MFMAs,
    // exposing a full L2 / HBM latency per 32-point step on every wave.
    // 16 floats -> 3 parts x 2 chunks of 8 bf16 at (row pi(r), bytes 16 jc and 256 + 16 jc)
    auto put = [&](char *img0, const f4 (&v)[4]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u4 q0, q1, q2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 &w = v[2 * h + (j >> 1)];
                float x0 = (j & 1) ? w.z : w.x, x1 = (j & 1) ? w.w : w.y;
                if (!ok) x0 = x1 = 0.f;
                unsigned e0, e1, e2;
                split_pair(x0, x1, e0, e1, e2);
                q0[j] = e0; q1[j] = e1; q2[j] = e2;
            }
            char *d = img0 + S.woff + 256 * h;
            *reinterpret_cast<u4 *>(d) = q0;
            *reinterpret_cast<u4 *>(d + IMG_BYTES) = q1;
            *reinterpret_cast<u4 *>(d + 2 * IMG_BYTES) = q2;
        }
    };
    char *imd = lds, *imx = lds + 3 * IMG_BYTES;

    BlockAcc acc;
    acc_zero(acc);
    const TileLane T = tile_lane(wave, lane);
    const int t_lo = T.t_lo, t_hi = T.t_hi;
    const char *ad = imd + 2 * T.n0, *ax = imx + 2 * T.k0;
    const int64_t p0 = U.p0, p1 = U.p1;

    ok = load_row(S, p0 + S.r, p1, sd, sx);
#pragma unroll 1
    for (int64_t pb = p0; pb < p1; pb += PS) {
        __syncthreads();   // the previous step's fragment reads are done
        put(imd, sd);
        put(imx, sx);
        __syncthreads();
        if (pb + PS < p1) ok = load_row(S, pb + PS + S.r, p1, sd, sx);   // in flight during this step's MFMAs
        bf8 xb[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) xb[j][pt] = tr_frag<bf8>(ax + pt * IMG_BYTES + 32 * j, t_lo, t_hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bf8 da[3];
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) da[pt] = tr_frag<bf8>(ad + pt * IMG_BYTES + 32 * i, t_lo, t_hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f4 v = acc[i][j];
                v = mfma_bf(da[2], xb[j][0], v);
                v = mfma_bf(da[1], xb[j][1], v);
                v = mfma_bf(da[0], xb[j][2], v);
                v = mfma_bf(da[1], xb[j][0], v);
                v = mfma_bf(da[0], xb[j][1], v);
                v = mfma_bf(da[0], xb[j][0], v);
                acc[i][j] = v;
            }
        }
    }
    store_block(a, U, T, acc, [](float v, int, int, int) { return v; });
}

// ---- f16x3, double-buffered (k_wgrad_h) --------------------------------------------------
constexpr int SET_BYTES = 4 * IMG_BYTES;            // dY hi | dY lo | X hi | X lo: 69,632 B
constexpr int HS_SC = 2 * SET_BYTES;                // sc[512]: 2^-E per channel (dY 0..255, X 256..511)
constexpr int HS_E = HS_SC + 512 * 4;               // E[512] (int)
constexpr int HS_RS = HS_E + 512 * 4;               // rs[512]: 2^(E_old - E_new) of the last retune
constexpr int HS_MAX = HS_RS + 512 * 4;             // chmax[512] (|v| bits, LDS atomic max)
constexpr int HS_FLAG = HS_MAX + 512 * 4;           // flag[2]: step index of an overflow, by parity; tmax[2]
constexpr int LDS_BYTES_H = HS_FLAG + 16;           // 147,472 B
constexpr int E_UNSET = -100;                       // no nonzero value seen: scale 2^100
constexpr float OVF = 32768.f;                      // |v 2^-E| >= 2^15: the channel's scale moves
constexpr int E_HEAD = 5;                           // a moved channel's maximum lands in [2^H, 2^(H+1))
constexpr int INIT_STEPS = 4;                       // steps whose maxima set the chunk's first scales

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

// v0 s0, v1 s1 (8 channels of one point row, scaled) -> two fp16 parts: hi at d, lo at
// d + IMG_BYTES.  Returns the maximum of m and every |split value|.
__device__ __forceinline__ float split_store8(const f4 &v0, const f4 &v1, const f4 &s0, const f4 &s1, char *d,
                                              float m = 0.f) {
    const f4 y0 = v0 * s0, y1 = v1 * s1;
    u4 hi, lo;
    const f2 q[4] = {f2{y0.x, y0.y}, f2{y0.z, y0.w}, f2{y1.x, y1.y}, f2{y1.z, y1.w}};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hi[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(q[e], h2));
        lo[e] = resid_pk(hi[e], q[e].x, q[e].y);
        m = fmaxf(m, fmaxf(fabsf(q[e].x), fabsf(q[e].y)));
    }
    *reinterpret_cast<u4 *>(d) = hi;
    *reinterpret_cast<u4 *>(d + IMG_BYTES) = lo;
    return m;
}

#ifdef PNR_WGH_STATS   // diagnostic: [0] retunes after step 0, [1] steps, [2] workgroups, channel scale moves
                       // after step 0: [3] from unset (no nonzero value yet), [4] by growth (tools/wgrad_stats.py)
__device__ unsigned long long g_wgh_stats[5];
#endif

__global__ __launch_bounds__(NTHR, 1) void k_wgrad_h(Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float *sc = reinterpret_cast<float *>(lds + HS_SC);
    int *Ee = reinterpret_cast<int *>(lds + HS_E);
    float *rs = reinterpret_cast<float *>(lds + HS_RS);
    unsigned *chmax = reinterpret_cast<unsigned *>(lds + HS_MAX);
    int *flag = reinterpret_cast<int *>(lds + HS_FLAG);
    unsigned *tmax = reinterpret_cast<unsigned *>(lds + HS_FLAG + 8);   // dY, X maxima of a retune
    Unit U;
    if (!unit_of(a, U)) return;
    const int64_t p0 = U.p0, p1 = U.p1;
    const int nsteps = p1 > p0 ? (int)((p1 - p0 + PS - 1) / PS) : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Stage S = stage_of(a, U, tid);
    const int r = S.r, jc = S.jc, woff = S.woff;
    // (slow path) v 2^-E -> two fp16 parts of 8 channels x 2 at (row pi(r), bytes 16 jc and
    // 256 + 16 jc) of the image pair at img (hi) / img + IMG_BYTES (lo); a row past the chunk
    // (!ok) is staged as zeros
    auto put = [&](char *img, const float *scb, const f4 (&v)[4], bool ok) {
        const f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float *sh = scb + 128 * h + 8 * jc;
            split_store8(ok ? v[2 * h] : z, ok ? v[2 * h + 1] : z, *reinterpret_cast<const f4 *>(sh),
                         *reinterpret_cast<const f4 *>(sh + 4), img + woff + 256 * h);
        }
    };

    BlockAcc acc;
    acc_zero(acc);
    const TileLane T = tile_lane(wave, lane);
    const int n0 = T.n0, k0 = T.k0, g = T.g, li = T.li, t_lo = T.t_lo, t_hi = T.t_hi;

    // the slow path: re-read step `step`, move the scales of its overflowing channels, rescale the
    // accumulators and split the step again into image set `set`
    auto retune = [&](int step, char *set, int scan) {
        f4 td[4], tx[4];
        bool tok;
        // channel maxima (and each tensor's maximum over its 256 channels) of the staged rows
        auto note = [&]() {
            if (!tok) return;
            float md = 0.f, mx = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 128 * (i >> 1) + 8 * jc + 4 * (i & 1);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    atomicMax(chmax + c + e, __float_as_uint(fabsf(td[i][e])));
                    atomicMax(chmax + 256 + c + e, __float_as_uint(fabsf(tx[i][e])));
                    md = fmaxf(md, fabsf(td[i][e]));
                    mx = fmaxf(mx, fabsf(tx[i][e]));
                }
            }
            atomicMax(tmax, __float_as_uint(md));
            atomicMax(tmax + 1, __float_as_uint(mx));
        };
        // the maxima of steps step + 1 .. step + scan - 1 too (the chunk's first scales)
        for (int q = 1; q < scan; ++q) {
            tok = load_row(S, p0 + (int64_t)(step + q) * PS + r, p1, td, tx);
            note();
        }
        tok = load_row(S, p0 + (int64_t)step * PS + r, p1, td, tx);
        note();
        __syncthreads();
        {   // channel tid
            const int eo = Ee[tid];
            // a channel without a nonzero value so far takes its tensor's maximum: its scale is
            // then set before its first nonzero step (98 % of the scale moves of a training step
            // were such channels turning on, each one a retune)
            const unsigned mb = chmax[tid] == 0u && eo == E_UNSET ? tmax[tid >> 8] : chmax[tid];
            chmax[tid] = 0u;
            const float m = __uint_as_float(mb);
            float ratio = 1.f;
            if (!(m * sc[tid] < OVF)) {
                int en = (int)((mb >> 23) & 255u) - 127 - E_HEAD;   // m in [2^k, 2^(k+1)): k - E_HEAD
                en = en < E_UNSET ? E_UNSET : (en > 127 ? 127 : en);
                if (en > eo) {
#ifdef PNR_WGH_STATS
                    if (step > 0) atomicAdd(&g_wgh_stats[eo == E_UNSET ? 3 : 4], 1ull);
#endif
                    ratio = __builtin_ldexpf(1.f, eo - en);
                    Ee[tid] = en;
                    sc[tid] = __builtin_ldexpf(1.f, -en);
                }
            }
            rs[tid] = ratio;
        }
        __syncthreads();
        if (tid < 2) tmax[tid] = 0u;   // read by every channel before the barrier
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float cs = rs[256 + k0 + 16 * j + li];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f4 rw = *reinterpret_cast<const f4 *>(rs + n0 + 16 * i + 4 * g);
                acc[i][j] *= rw * cs;
            }
        }
        put(set, sc, td, tok);
        put(set + 2 * IMG_BYTES, sc + 256, tx, tok);
        __syncthreads();
    };

    if (tid < 512) {
        sc[tid] = 0x1p100f;
        Ee[tid] = E_UNSET;
        chmax[tid] = 0u;
    }
    if (tid < 2) {
        flag[tid] = -1;
        tmax[tid] = 0u;
    }
    __syncthreads();
    if (nsteps > 0) retune(0, lds, nsteps < INIT_STEPS ? nsteps : INIT_STEPS);
    // Step s + 1's split runs inside step s's MFMA loop, in four pieces (piece k = tensor k >> 1,
    // column half k & 1: 8 values of the thread's row) after row tiles 1, 3, 5, 7, so the
    // scheduler interleaves its VALU and LDS stores with the MFMAs.  Each piece's registers are
    // reloaded with step s + 2's values right after its split: a full step of load latency.
    f4 stg[4][2];
    auto load_piece = [&](int step, int k) {
        const int64_t p = p0 + (int64_t)step * PS + r;
        const int64_t pc = p < p1 ? p : 0;   // rows past the chunk: a valid row, zeroed by okf
        const float *src = ((k >> 1) ? S.xsrc : S.dsrc) + pc * H + 128 * (k & 1);
        stg[k][0] = *reinterpret_cast<const f4 *>(src);
        stg[k][1] = *reinterpret_cast<const f4 *>(src + 4);
    };
    if (nsteps > 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) load_piece(1, k);
#pragma unroll 1
    for (int s = 0; s < nsteps; ++s) {
        char *cur = lds + (s & 1) * SET_BYTES, *nxt = lds + ((s + 1) & 1) * SET_BYTES;
        const float okf = p0 + (int64_t)(s + 1) * PS + r < p1 ? 1.f : 0.f;   // step s + 1's row
        float m = 0.f;   // max |split value| of step s + 1 (a last step's split is never read)
        auto put_piece = [&](int k) {
            const float *scb = sc + 256 * (k >> 1) + 128 * (k & 1) + 8 * jc;
            m = split_store8(stg[k][0], stg[k][1], *reinterpret_cast<const f4 *>(scb) * okf,
                             *reinterpret_cast<const f4 *>(scb + 4) * okf,
                             nxt + 2 * IMG_BYTES * (k >> 1) + woff + 256 * (k & 1), m);
            load_piece(s + 2, k);
        };
        const char *ad = cur + 2 * n0, *ax = cur + 2 * IMG_BYTES + 2 * k0;
        h8 xb[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) xb[j][pt] = tr_frag<h8>(ax + pt * IMG_BYTES + 32 * j, t_lo, t_hi);
        // dY fragments one row tile ahead: tile i + 1's reads are in flight during tile i's MFMAs
        h8 dh = tr_frag<h8>(ad, t_lo, t_hi), dl = tr_frag<h8>(ad + IMG_BYTES, t_lo, t_hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            h8 nh = dh, nl = dl;
            if (i < 7) {
                nh = tr_frag<h8>(ad + 32 * (i + 1), t_lo, t_hi);
                nl = tr_frag<h8>(ad + IMG_BYTES + 32 * (i + 1), t_lo, t_hi);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f4 v = acc[i][j];
                v = mfma_h(dl, xb[j][0], v);
                v = mfma_h(dh, xb[j][1], v);
                v = mfma_h(dh, xb[j][0], v);
                acc[i][j] = v;
            }
            if (i & 1) put_piece(i >> 1);
            dh = nh;
            dl = nl;
        }
        if (!(m < OVF)) flag[(s + 1) & 1] = s + 1;   // NaN-safe: a NaN maximum retunes too
        __syncthreads();   // step s + 1's images are complete; step s's reads are done
        if (s + 1 < nsteps && flag[(s + 1) & 1] == s + 1) {
            retune(s + 1, nxt, 1);
#ifdef PNR_WGH_STATS
            if (tid == 0) atomicAdd(&g_wgh_stats[0], 1ull);
#endif
        }
    }
#ifdef PNR_WGH_STATS
    if (tid == 0) {
        atomicAdd(&g_wgh_stats[1], (unsigned long long)nsteps);
        atomicAdd(&g_wgh_stats[2], 1ull);
    }
#endif
    // partial block G = acc 2^(E_row + E_col)
    store_block(a, U, T, acc, [&](float v, int i, int j, int e) {
        return __builtin_ldexpf(v, Ee[n0 + 16 * i + 4 * g + e] + Ee[256 + k0 + 16 * j + li]);
    });
}

// G_j = sum over chunks (in chunk order) of the partials; one thread per 4 outputs
struct Outs {
    float *g[MAX_JOBS];
};
__global__ void k_wgrad_reduce(Outs o, const float *__restrict__ partial, int n_jobs, int chunks) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n_jobs * (H * H / 4)) return;
    const int job = (int)(t / (H * H / 4));
    const int64_t e = 4 * (t % (H * H / 4));
    const float *src = partial + (int64_t)job * chunks * H * H + e;
    f4 s = *reinterpret_cast<const f4 *>(src);
    for (int c = 1; c < chunks; ++c) s += *reinterpret_cast<const f4 *>(src + (int64_t)c * H * H);
    *reinterpret_cast<f4 *>(o.g[job] + e) = s;
}

// chunk count: about 5 rounds of one workgroup per CU over all jobs (4 blocks per
// (layer, chunk)), >= 8 steps per chunk
inline int wgrad_chunks(int n_jobs, int64_t n_points) {
    const int target = (int)(4.875 * device_cu_count());
    int c = (target + 2 * n_jobs) / (4 * n_jobs);
    const int64_t max_c = (n_points + 8 * PS - 1) / (8 * PS);
    if (c > max_c) c = (int)max_c;
    return c < 1 ? 1 : c;
}

}  // namespace wg

#ifdef PNR_WGH_STATS
extern "C" int pnr_wgrad_stats(unsigned long long *out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(wg::g_wgh_stats), sizeof(wg::g_wgh_stats)) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[5] = {0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(wg::g_wgh_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

size_t wgrad_workspace_bytes(int n_jobs, int64_t n_points) {
    if (n_jobs < 1 || n_jobs > wg::MAX_JOBS || n_points < 1) return 0;
    return sizeof(float) * (size_t)n_jobs * wg::wgrad_chunks(n_jobs, n_points) * wg::H * wg::H;
}

int launch_wgrad(const float *const *dy, const float *const *x, float *const *g, int n_jobs, int64_t n_points,
                 void *ws, size_t ws_bytes, int arith, hipStream_t st) {
    if (arith != PNR_WGRAD_F16X3 && arith != PNR_WGRAD_BF16X6)
        return fail(PNR_ERR_INVALID, "weight grad: arithmetic %d is not PNR_WGRAD_F16X3 / PNR_WGRAD_BF16X6", arith);
    if (n_jobs < 1 || n_jobs > wg::MAX_JOBS) return fail(PNR_ERR_UNSUPPORTED, "weight grad: 1..16 layers");
    if (n_points < 0) return fail(PNR_ERR_INVALID, "weight grad: n_points < 0");
    if (n_points == 0) {
        for (int j = 0; j < n_jobs; ++j)
            if (hipMemsetAsync(g[j], 0, sizeof(float) * wg::H * wg::H, st) != hipSuccess)
                return fail(PNR_ERR_HIP, "weight grad: hipMemsetAsync failed");
        return PNR_OK;
    }
    const size_t need = wgrad_workspace_bytes(n_jobs, n_points);
    if (!ws || ws_bytes < need) return fail(PNR_ERR_WORKSPACE, "weight grad: workspace %zu < %zu", ws_bytes, need);
    wg::Args a = {};
    wg::Outs o = {};
    for (int j = 0; j < n_jobs; ++j) {
        if (!dy[j] || !x[j] || !g[j]) return fail(PNR_ERR_INVALID, "weight grad: NULL matrix (layer %d)", j);
        if (misaligned(15, dy[j], x[j], g[j]))
            return fail(PNR_ERR_INVALID, "weight grad: matrices must be 16-byte aligned");
        a.dy[j] = dy[j];
        a.x[j] = x[j];
        o.g[j] = g[j];
    }
    a.n_jobs = n_jobs;
    a.chunks = wg::wgrad_chunks(n_jobs, n_points);
    a.n_units = n_jobs * a.chunks;
    a.n_points = n_points;
    a.chunk_points = ((n_points + a.chunks - 1) / a.chunks + wg::PS - 1) / wg::PS * wg::PS;
    a.partial = static_cast<float *>(ws);
    // units padded to a multiple of 8 (one per XCD), 4 workgroups each
    const dim3 grid((unsigned)((a.n_units + 7) / 8 * 8 * 4));
    if (arith == PNR_WGRAD_BF16X6)
        hipLaunchKernelGGL(wg::k_wgrad, grid, dim3(wg::NTHR), wg::LDS_BYTES, st, a);
    else
        hipLaunchKernelGGL(wg::k_wgrad_h, grid, dim3(wg::NTHR), wg::LDS_BYTES_H, st, a);
    if (!launch_ok("wgrad")) return PNR_ERR_HIP;
    const int64_t nt = (int64_t)n_jobs * (wg::H * wg::H / 4);
    hipLaunchKernelGGL(wg::k_wgrad_reduce, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, o, a.partial,
                       n_jobs, a.chunks);
    return launch_ok("wgrad_reduce") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
