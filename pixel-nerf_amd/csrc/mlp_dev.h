// Device building blocks that k_point_mlp (mlp.hip) and k_mlp_bwd (mlp_bwd.hip) inline: the three
// GEMM families, the fp16 weight ring, the relu publish, bias helpers, the projected-latent and latent-gather stages,
// the activation-save stores and the tile claim.
#pragma once
#include "pnr_diag.h"
#include <cstddef>
#include <type_traits>

#include "mlp_layout.h"

namespace pnr {
namespace mlpk {

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

typedef f4 Acc[RTW][CT];

// The lane index through an empty asm: per-lane LDS / global addresses derived from it are
// recomputed at each inlined use instead of hoisted out of the tile loop, where the 256
// registers of a wave at 2 waves per SIMD turned them into scratch spills whose reloads
// each cost a memory latency.
__device__ __forceinline__ int opaque_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// relu(acc) of this wave's rows -> save slot [point][512] (points of this tile < n_points)
__device__ __forceinline__ void save_relu(const Acc &acc, float *slot, int64_t tile, int64_t n_points,
                                          int wave, int lane) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        if (p >= n_points) continue;
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            const f4 v = acc[r][c];
            *reinterpret_cast<f4 *>(slot + p * H + 16 * (RTW * wave + r) + 4 * g) = relu4(v);
        }
    }
}

// [acc > 0] of this wave's rows -> mask slot [point][64 bytes].  Byte 8 wave + 2g + w of a
// point holds rows 16 (RTW wave + r) + 4g + e, r = 2w + h, at bit 4h + e: a lane's 16 bits
// are one contiguous 2-byte store per point, and a wave's 64 rows are one 8-byte word pair.
__device__ __forceinline__ void save_mask(const Acc &acc, uint32_t *mslot, int64_t tile, int64_t n_points,
                                          int wave, int lane) {
    static_assert(RTW == 4, "mask bytes assume 4 row tiles per wave");
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
    auto nib = [](const f4 &v) {
        return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
    };
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        const uint32_t bits = nib(acc[0][c]) | (nib(acc[1][c]) << 4) | (nib(acc[2][c]) << 8) | (nib(acc[3][c]) << 12);
        if (p < n_points)
            *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(mslot) + p * 64 + 8 * wave + 2 * g) =
                (uint16_t)bits;
    }
}

// acc[r][c] (+)= W(rows of this wave) * IN^T over nkb k-blocks.
//   wp  : this layer's packed weights, already offset to this wave's first row
//         tile and this lane (stride KB_FLOATS per k-block, 256 per row tile)
//   inb : LDS activation buffer, already offset to this lane's (column, k) slot
// Software pipeline: k-block kb+1's A (8 x f4) and B (4 x f4) are loaded while
// kb's 128 MFMAs issue.
template <int NK>
__device__ __forceinline__ void gemm(Acc &acc, const float *__restrict__ wp, const float *inb) {
    f4 A[RTW], B[CT];
#pragma unroll
    for (int r = 0; r < RTW; ++r) A[r] = *reinterpret_cast<const f4 *>(wp + r * 256);
#pragma unroll
    for (int c = 0; c < CT; ++c) B[c] = *reinterpret_cast<const f4 *>(inb + c * 16 * LDS_LD);
#pragma unroll 2
    for (int kb = 0; kb < NK; ++kb) {
        f4 An[RTW], Bn[CT];
        const int kn = kb + 1 < NK ? kb + 1 : kb;
#pragma unroll
        for (int r = 0; r < RTW; ++r)
            An[r] = *reinterpret_cast<const f4 *>(wp + (int64_t)kn * KB_FLOATS + r * 256);
#pragma unroll
        for (int c = 0; c < CT; ++c)
            Bn[c] = *reinterpret_cast<const f4 *>(inb + c * 16 * LDS_LD + kn * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < RTW; ++r) acc[r][c] = mfma(A[r][j], B[c][j], acc[r][c]);
#pragma unroll
        for (int r = 0; r < RTW; ++r) A[r] = An[r];
#pragma unroll
        for (int c = 0; c < CT; ++c) B[c] = Bn[c];
    }
}

typedef float f8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split3(const f4 &lo, const f4 &hi, bf8 &x0, bf8 &x1, bf8 &x2) {
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    u4 p0, p1, p2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned a, b, c;
        split_pair(x[2 * q], x[2 * q + 1], a, b, c);
        p0[q] = a;
        p1[q] = b;
        p2[q] = c;
    }
    x0 = __builtin_bit_cast(bf8, p0);
    x1 = __builtin_bit_cast(bf8, p1);
    x2 = __builtin_bit_cast(bf8, p2);
}

// workgroup barrier that waits only for LDS traffic: a __syncthreads() would also
// emit s_waitcnt vmcnt(0) and drain the weight prefetch that spans k-steps.  k_point_mlp
// uses it for every barrier: no wave there reads global memory another wave of the
// workgroup wrote (outputs, activation saves and per-wave scratch are written once per
// address), so global loads in flight (projected rows, biases) cross its barriers.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

constexpr int A_DIST = 3;                          // weight prefetch distance (row tiles)
constexpr int A_RING = A_DIST < 4 ? 4 : 8;         // register ring (divides RTW = 8)

// Split-bf16 GEMM: acc[r][c] += sum over the NTERM largest products of the exact
// 3-way splits of W and IN (6 terms: error ~ fp32 unit roundoff; 9 terms: every
// product exact, only fp32 accumulation rounds) on v_mfma_f32_16x16x32_bf16.
//   wp   : packed layer + this wave's first row tile + lane*4 (floats)
//   inbw : LDS activations at (column 16*wave + cl, k 8g): the tile this wave splits
//   stg  : LDS staging ring, 2 x [ct][part][lane][8 bf16] (24 KB)
// Each wave splits ONE column tile of the next k-step into the staging ring (a
// quarter of the split VALU) and all waves read every tile's parts from it; A
// fragments stream from L2 three row tiles ahead into a 4-deep register ring.
template <int NKS, int NTERM>
__device__ __forceinline__ void gemm_split(Acc &acc, const float *__restrict__ wp, const float *inbw,
                                           float *stg, int wave, int lane) {
    bf8 ra[A_RING][3];
    auto loadA = [&](bf8 (&dst)[3], int ks, int r) {
        const float *src = wp + (int64_t)ks * SKS_FLOATS + r * SRT_FLOATS;
#pragma unroll
        for (int q = 0; q < 3; ++q) dst[q] = *reinterpret_cast<const bf8 *>(src + q * 256);
    };
    // wave w splits the k-half w / 4 (4 values per lane) of column tile w % 4
    auto split_own = [&](int ks, int buf) {
        const float *bp = inbw + 32 * ks;
        const f4 v = *reinterpret_cast<const f4 *>(bp);
        unsigned a0, a1, a2, b0, b1, b2;
        split_pair(v.x, v.y, a0, a1, a2);
        split_pair(v.z, v.w, b0, b1, b2);
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        float *d = stg + buf * STG_FLOATS + (wave % CT) * 768 + lane * 4 + 2 * (wave / CT);
        *reinterpret_cast<u2 *>(d) = u2{a0, b0};
        *reinterpret_cast<u2 *>(d + 256) = u2{a1, b1};
        *reinterpret_cast<u2 *>(d + 512) = u2{a2, b2};
    };
    split_own(0, 0);
#pragma unroll
    for (int r = 0; r < A_DIST; ++r) loadA(ra[r], 0, r);
    lds_barrier();
#pragma unroll 1
    for (int ks = 0; ks < NKS; ++ks) {
        const int kn = ks + 1 < NKS ? ks + 1 : ks;   // branch-free tail: redundant re-split
        bf8 b0[CT], b1[CT], b2[CT];
        const float *sp = stg + (ks & 1) * STG_FLOATS + lane * 4;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            b0[c] = *reinterpret_cast<const bf8 *>(sp + c * 768);
            b1[c] = *reinterpret_cast<const bf8 *>(sp + c * 768 + 256);
            b2[c] = *reinterpret_cast<const bf8 *>(sp + c * 768 + 512);
        }
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            // split after the first row tile so its LDS reads don't gate the k-step start
            if (r == 1) split_own(kn, (ks + 1) & 1);
            const int rn = r + A_DIST;
            if (rn < RTW) loadA(ra[rn % A_RING], ks, rn);
            else loadA(ra[rn % A_RING], kn, rn - RTW);
            // keep the prefetch where it is: without the barrier the scheduler sinks
            // the loads next to their use to save registers and serializes the ring
            __builtin_amdgcn_sched_barrier(0);
            const bf8 *a = ra[r % A_RING];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                f4 v = acc[r][c];
                if (NTERM >= 9) {
                    v = mfma_bf(a[2], b2[c], v);
                    v = mfma_bf(a[1], b2[c], v);
                    v = mfma_bf(a[2], b1[c], v);
                }
                v = mfma_bf(a[2], b0[c], v);
                v = mfma_bf(a[1], b1[c], v);
                v = mfma_bf(a[0], b2[c], v);
                v = mfma_bf(a[1], b0[c], v);
                v = mfma_bf(a[0], b1[c], v);
                v = mfma_bf(a[0], b0[c], v);
                acc[r][c] = v;
            }
        }
        lds_barrier();
    }
}

// ---- scaled-fp16 mode (PREC 3) -----------------------------------------------------
// W * 2^eW and every IN column * 2^e_col are split exactly enough into two fp16 parts
// (x = x0 + x1 + O(2^-22 x)); three products x0 y0 + x0 y1 + x1 y0 are exact in the
// f32 accumulate of v_mfma_f32_16x16x32_f16 (dropped x1 y1 < 2^-22 |x y|).  The
// power-of-two scales keep both operands in fp16's normal range (max <= 2^14) and are
// undone exactly on the fp32 accumulators.
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

// 4 values * s -> packed fp16 parts (2 dwords each): v_cvt_pk_f16_f32 (RNE), residuals
__device__ __forceinline__ void split_f16x4(const f4 &v, float s, u2 &p0, u2 &p1) {
    const f2 a = {v.x * s, v.y * s}, b = {v.z * s, v.w * s};
    const unsigned a0 = __builtin_bit_cast(unsigned, __builtin_convertvector(a, h2));
    const unsigned b0 = __builtin_bit_cast(unsigned, __builtin_convertvector(b, h2));
    p0 = u2{a0, b0};
    p1 = u2{resid_pk(a0, a.x, a.y), resid_pk(b0, b.x, b.y)};
}

// Swizzle: the 16-B chunk index of element k (k >> 3) is XORed with (column >> 2) & 3.
// With the 1056-B pitch the B reads stay conflict-free and the producers' 8-B stores
// (16 columns x one chunk) drop from 4-way to 2-way bank conflicts.  k % 4 == 0.
__device__ __forceinline__ int swz(int col, int k) {
    return 8 * ((k >> 3) ^ ((col >> 2) & 3)) + (k & 7);
}

// acc[r][c] += (W 2^eW)(IN 2^e) over NKS k-steps of 32 from the pre-split LDS image:
// no staging, no split, no barrier inside the layer (waves run free).  A fragments
// stream from L2 A_DIST row tiles ahead; the last k-step is peeled so no load is in
// flight when the accumulators are handed back.
//   pb0 / pb1: P0 / P1 at (column cl, k 8g) of column tile 0
// The weight register ring of gemm_f16: row tile t = RTW * ks + r of the layer's stream lives
// in slot t % slots.  hring_prime issues the first DIST row tiles; gemm_f16_primed runs the
// layer on a primed ring.  Priming the next layer's ring before the publish that precedes it
// (k_point_mlp) lets those loads' L2 latency pass under the publish and its LDS-only barriers.
// NP: parts per slot (2: f16x3's w0 / w1; 1: the single-part layers of PREC 1)
template <int DIST, int NP = 2>
struct HRing {
    static constexpr int slots = DIST < RTW ? RTW : 2 * RTW;
    h8 ra[slots][NP];
};

template <int DIST, int NP>
__device__ __forceinline__ void hring_load(HRing<DIST, NP> &R, const float *__restrict__ wp, int slot, int ks, int r) {
    const float *src = wp + (int64_t)ks * sks_h_floats(NP) + r * srt_h_floats(NP);
    R.ra[slot][0] = *reinterpret_cast<const h8 *>(src);
    if constexpr (NP > 1) R.ra[slot][1] = *reinterpret_cast<const h8 *>(src + 256);
}

template <int DIST, int NKS = KS32, int NP = 2>
__device__ __forceinline__ void hring_prime(HRing<DIST, NP> &R, const float *__restrict__ wp) {
#pragma unroll
    for (int t = 0; t < DIST; ++t) hring_load(R, wp, t, (t / RTW) & (NKS - 1), t % RTW);
}

// Fair pipe sharing between the two waves of a SIMD (waves w and w ^ 4): each GEMM iteration a
// wave publishes its running iteration count in LDS and takes issue priority 1 while it is behind
// its SIMD-mate (the count read one iteration earlier), 0 otherwise.  At equal priority the older
// wave wins every MFMA slot, so without this the younger wave finished each layer alone, with a
// one-k-step weight prefetch that a solo wave's MFMA rate does not cover.
struct Fair {
    int *prog;   // LDS: iteration count per wave (8 ints)
    int wave, it, mate;
};
template <int NKS, int DIST = H_DIST, int NP = 2>
__device__ __forceinline__ void gemm_f16_primed(Acc &acc, HRing<DIST, NP> &R, const float *__restrict__ wp,
                                                const _Float16 *pb0, const _Float16 *pb1, Fair *F = nullptr) {
    constexpr int H_RING = HRing<DIST, NP>::slots;   // register ring slots
    static_assert(DIST < H_RING && H_RING % RTW == 0, "ring");
    constexpr int U = H_RING / RTW;   // k-steps per loop iteration (static ring slots)
    static_assert(NKS % U == 0, "k-steps");
    static_assert((NKS & (NKS - 1)) == 0, "rotation mask");
    // one k-step; ph = ks % U (static), tail = this is one of the last U k-steps
    auto kstep = [&](int ks, auto ph_tag, auto tail_tag) {
        constexpr int ph = decltype(ph_tag)::value;
        constexpr bool tail = decltype(tail_tag)::value;
        h8 b0[CT], b1[CT];
        const int kr = ks & (NKS - 1);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            b0[c] = *reinterpret_cast<const h8 *>(pb0 + c * 16 * ROWH + 32 * kr);
            if constexpr (NP > 1) b1[c] = *reinterpret_cast<const h8 *>(pb1 + c * 16 * ROWH + 32 * kr);
        }
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            const int tn = ph * RTW + r + DIST;            // prefetch target, relative to the iteration
            if (!tail || tn < U * RTW)
                hring_load(R, wp, tn % H_RING, (ks - ph + tn / RTW) & (NKS - 1), tn % RTW);
            __builtin_amdgcn_sched_barrier(0);
            const h8 *a = R.ra[(ph * RTW + r) % H_RING];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                f4 v = acc[r][c];
                if constexpr (NP > 1) {
                    v = mfma_h(a[1], b0[c], v);
                    v = mfma_h(a[0], b1[c], v);
                }
                v = mfma_h(a[0], b0[c], v);
                acc[r][c] = v;
            }
        }
    };
    auto iter = [&](int ks0, auto tail_tag) {
        if (F) {
            const int it = ++F->it;
            // the mate's count loaded one iteration ago (its LDS latency passed under the MFMAs)
            if (it > __builtin_amdgcn_readfirstlane(F->mate)) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(1);
            F->prog[F->wave] = it;
            F->mate = F->prog[F->wave ^ 4];
        }
        kstep(ks0, std::integral_constant<int, 0>{}, tail_tag);
        if constexpr (U > 1) kstep(ks0 + 1, std::integral_constant<int, 1>{}, tail_tag);
    };
#pragma unroll 1
    for (int ks = 0; ks + U < NKS; ks += U) iter(ks, std::false_type{});
    iter(NKS - U, std::true_type{});
    if (F) __builtin_amdgcn_s_setprio(0);
}

template <int NKS, int DIST = H_DIST, int NP = 2>
__device__ __forceinline__ void gemm_f16(Acc &acc, const float *__restrict__ wp, const _Float16 *pb0,
                                         const _Float16 *pb1, Fair *F = nullptr) {
    HRing<DIST, NP> R;
    hring_prime<DIST, NKS, NP>(R, wp);
    gemm_f16_primed<NKS, DIST, NP>(acc, R, wp, pb0, pb1, F);
}

// 4 (or 8) fp32 values -> scaled fp16 parts written to P0 / P1 at half offset `off`
__device__ __forceinline__ void put_split4(_Float16 *P0, _Float16 *P1, int off, const f4 &v, float s) {
    u2 p0, p1;
    split_f16x4(v, s, p0, p1);
    *reinterpret_cast<u2 *>(P0 + off) = p0;
    *reinterpret_cast<u2 *>(P1 + off) = p1;
}

// relu(acc) (RELU) or |acc| of this wave's rows -> per-column partial maxima cmax[column][wave slot]
template <bool RELU = true>
__device__ __forceinline__ void relu_colmax(const Acc &acc, float *cmax, int wave, int lane) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        float m = 0.f;   // max(0, ...) = the max of the relu'd values
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            f4 v = acc[r][c];
            if constexpr (!RELU) v = f4{fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)};
            m = max3_nc(max3_nc(m, v.x, v.y), v.z, v.w);
        }
        m = rows_max(m);
        if (g == 0) cmax[(16 * c + cl) * 8 + wave] = m;
    }
}

// after relu_colmax + barrier: relu(acc) (RELU) or acc, * 2^e_col split into P0 / P1 (this
// wave's rows), e_col -> ecol[column] (LDS, wave 0) and -> e_col (this lane's columns 16 c + cl:
// every wave computes the same exponents, so the next GEMM takes them from registers)
// A relu-publish store: lanes g and g ^ 1 (16 apart) hold rows 4g .. 4g + 3 of one column in
// both parts; one v_permlane16_swap per dword leaves the column's 8-row P0 chunk (16 B, k order)
// in the even lane and its P1 chunk in the odd one, stored with ONE ds_write_b128 at the lane's
// plane (Pl: P0 for even g, P1 for odd g).  Eight consecutive lanes then write eight distinct
// bank quads (the B-read swizzle), where two ds_write_b64 per lane were 2-way bank conflicted:
// the same bytes at the same addresses, half the LDS-array cycles.
__device__ __forceinline__ void put_split4_pair(_Float16 *Pl, int off, const f4 &v, float s) {
    u2 p0, p1;
    split_f16x4(v, s, p0, p1);
    const auto w0 = __builtin_amdgcn_permlane16_swap(p0.x, p1.x, false, false);
    const auto w1 = __builtin_amdgcn_permlane16_swap(p0.y, p1.y, false, false);
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<u4 *>(Pl + off) = u4{w0[0], w1[0], w0[1], w1[1]};
}
// The single-part publish (PREC 1): relu(acc) * 2^e_col rounded ONCE to fp16 (v_cvt_pk_f16_f32,
// RNE), no residual, P0 only.  The store keeps the pair store's shape with the row-tile pair
// (r, r + 1) in the place of the part pair: lanes g and g ^ 1 hold rows 4g .. 4g + 3 of one column
// in both row tiles; after one v_permlane16_swap per dword the even lane holds row tile r's 8-row
// chunk (16 B, k order) and the odd lane row tile r + 1's, each stored with ONE ds_write_b128 in
// P0.  Per store instruction a lane row's 16 columns land at the pitch / swizzle addresses of
// f16x3's publish (eight consecutive lanes, eight distinct bank quads), and the image keeps the
// layout the B reads are conflict-free on; 8 stores per lane and layer where f16x3 issues 16.
__device__ __forceinline__ void put_f16x4_pair(_Float16 *q, int off, const f4 &va, const f4 &vb, float s) {
    const f2 a0 = {va.x * s, va.y * s}, a1 = {va.z * s, va.w * s};
    const f2 b0 = {vb.x * s, vb.y * s}, b1 = {vb.z * s, vb.w * s};
    const u2 pa = {__builtin_bit_cast(unsigned, __builtin_convertvector(a0, h2)),
                   __builtin_bit_cast(unsigned, __builtin_convertvector(a1, h2))};
    const u2 pb = {__builtin_bit_cast(unsigned, __builtin_convertvector(b0, h2)),
                   __builtin_bit_cast(unsigned, __builtin_convertvector(b1, h2))};
    const auto w0 = __builtin_amdgcn_permlane16_swap(pa.x, pb.x, false, false);
    const auto w1 = __builtin_amdgcn_permlane16_swap(pa.y, pb.y, false, false);
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<u4 *>(q + off) = u4{w0[0], w1[0], w0[1], w1[1]};
}
template <bool RELU = true, int NP = 2>
__device__ __forceinline__ void relu_store_split(const Acc &acc, _Float16 *P0, _Float16 *P1,
                                                 const float *cmax, int *ecol, int wave, int lane,
                                                 int (&e_col)[CT]) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
    // store bases of row tiles r = 0 and 1 (r + 2: +32 halves, the swizzle only XORs the low two
    // chunk bits; column tile c: +16 ROWH, the swizzle depends on column bits 2-3 only), so the
    // 16 stores take constant ds_write offsets
    _Float16 *Pl = (NP > 1 && (g & 1)) ? P1 : P0;
    const int kb = 16 * RTW * wave + 4 * (g & ~1);
    _Float16 *q0 = Pl + cl * ROWH + swz(cl, kb), *q1 = Pl + cl * ROWH + swz(cl, kb + 16);
    // every column exponent first: a wave's LDS operations complete in order, so a cmax read
    // issued after stores waits for them (s_waitcnt lgkmcnt), which serialized the four column
    // tiles' reads behind the previous tiles' stores
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int col = 16 * c + cl;
        const f4 m0 = *reinterpret_cast<const f4 *>(cmax + col * 8);
        const f4 m1 = *reinterpret_cast<const f4 *>(cmax + col * 8 + 4);
        e_col[c] = scale_exp(max3_nc(max3_nc(m0.x, m0.y, m0.z), max3_nc(m0.w, m1.x, m1.y), max_nc(m1.z, m1.w)));
    }
    if (wave == 0 && g == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) ecol[16 * c + cl] = e_col[c];
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int col = 16 * c + cl;
        const float sc = __builtin_ldexpf(1.f, e_col[c]);
        if constexpr (NP == 1) {
            // even lane rows store row tile 2j's chunk (q0), odd ones row tile 2j + 1's (q1)
            static_assert(RTW % 2 == 0, "row-tile pairs");
#pragma unroll
            for (int j = 0; j < RTW / 2; ++j) {
                const f4 va = RELU ? relu4(acc[2 * j][c]) : acc[2 * j][c];
                const f4 vb = RELU ? relu4(acc[2 * j + 1][c]) : acc[2 * j + 1][c];
                put_f16x4_pair((g & 1) ? q1 : q0, c * 16 * ROWH + j * 32, va, vb, sc);
            }
        } else {
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            const f4 v = acc[r][c];
            const f4 o = RELU ? relu4(v) : v;
            put_split4_pair((r & 1) ? q1 : q0, c * 16 * ROWH + (r >> 1) * 32, o, sc);
        }
        }
    }
}

// this wave's rows of a bias vector (loaded ahead of use: the loads cross LDS-only barriers)
__device__ __forceinline__ void load_bias(f4 (&b)[RTW], const float *__restrict__ bias, int wave, int lane) {
    const int g = opaque_lane(lane) >> 4;
#pragma unroll
    for (int r = 0; r < RTW; ++r) b[r] = *reinterpret_cast<const f4 *>(bias + 16 * (RTW * wave + r) + 4 * g);
}
__device__ __forceinline__ void set_bias(Acc &acc, const f4 (&b)[RTW], bool accumulate) {
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[r][c] = accumulate ? acc[r][c] + b[r] : b[r];
}

// acc = bias (per output row) [+ acc]
__device__ __forceinline__ void add_bias(Acc &acc, const float *__restrict__ bias, int wave, int lane,
                                         bool accumulate) {
    const int g = opaque_lane(lane) >> 4;
#pragma unroll
    for (int r = 0; r < RTW; ++r) {
        const f4 b = *reinterpret_cast<const f4 *>(bias + 16 * (RTW * wave + r) + 4 * g);
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[r][c] = accumulate ? acc[r][c] + b : b;
    }
}

// IN^T[column][row] = relu(acc) for this wave's rows (4 consecutive rows per lane)
__device__ __forceinline__ void store_relu(const Acc &acc, float *inbuf, int wave, int lane) {
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const f4 v = acc[r][c];
            const f4 o = relu4(v);
            *reinterpret_cast<f4 *>(inbuf + (16 * c + cl) * LDS_LD + 16 * (RTW * wave + r) + 4 * g) = o;
        }
}

#ifdef PNR_PHASE_TIMING   // pnr_diag.h; the counters g_phase are mlp.hip's
constexpr int PT_SLOTS = 20;
#endif

struct GemmCtx {
    int64_t wl_off, ws_off;   // f32 / split fragment offsets of this wave + lane
    const float *inb4;        // f32 B: column 16c + cl, k 16kb + 4g
    const float *inbw;        // split: own column tile 16*wave + cl, k 8g
    float *stg;               // split staging ring
    const float *hdr;         // pack header (PREC 3 weight scale exponents)
    const _Float16 *pb0, *pb1;  // PREC 3: P0 / P1 at (column cl, k 8g)
    const int *ecol;          // PREC 3: scale exponent of each IN column
    int ecl[CT];              // PREC 3: this lane's columns' exponents from the wave's last publish
    Fair fair;                // PREC 3 forward: pipe sharing with the SIMD-mate (fair.prog NULL: off)
    int wave, lane;
#ifdef PNR_PHASE_TIMING
    uint64_t pt[PT_SLOTS], pt_last;
#endif
};

// lin_z(z) - bias of the bilinear latent sample z of every column of the tile, staged in
// LDS as fp32 stage[column][LDS_LD]: resnetfc.py:160-163 on grid_sample's blend
// (encoder.py:102-108), evaluated by linearity as the blend of four rows of the projected
// latent P = latent W_z^T (proj.hip), torch's nw, ne, sw, se summation order.  Wave w blends
// the COLS / WAVES columns [8w, 8w + 8); each load instruction reads one contiguous 1 KB half
// of a corner's 2 KB row.  The stage aliases the GEMM input image, so the first loads are
// issued BEFORE the barrier that frees it and land while the wave waits for its SIMD-mate's
// GEMM; blends and LDS writes come after.
// The stage is run-deduplicated.  A wave's 8 columns are consecutive
// samples of one ray, and consecutive samples mostly project into the same latent cell
// (cfg3: 2.1 runs of equal cell per 8 columns, cfg2: 4.9): the 4 corner rows of a run are
// loaded ONCE and blended with each of its columns' weights (the blend arithmetic per column
// is unchanged).  Three register slots (96 VGPRs, the two-batch stage holds 128) rotate over
// the runs: runs 0-2 are issued before the barrier that frees the stage, run k + 3 as soon
// as run k's columns are blended.  The run pattern is wave-uniform (SGPR bit mask), so every
// branch below is a scalar branch.
struct CellRows {
    f4 c[2][4];   // [channel half][corner nw, ne, sw, se]
};
__device__ __forceinline__ void cell_load(CellRows &C, const float *__restrict__ pz, const float *gtab, int cj,
                                          int lane) {
    const f4 to = *reinterpret_cast<const f4 *>(gtab + cj * 8);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint32_t ch = half * 256 + opaque_lane(lane) * 4;
        C.c[half][0] = *reinterpret_cast<const f4 *>(pz + __float_as_uint(to.x) + ch);
        C.c[half][1] = *reinterpret_cast<const f4 *>(pz + __float_as_uint(to.y) + ch);
        C.c[half][2] = *reinterpret_cast<const f4 *>(pz + __float_as_uint(to.z) + ch);
        C.c[half][3] = *reinterpret_cast<const f4 *>(pz + __float_as_uint(to.w) + ch);
    }
}
__device__ __forceinline__ void cell_blend_store(const CellRows &C, const float *gtab, float *stage, int cj,
                                                 int lane) {
    const f4 tw = *reinterpret_cast<const f4 *>(gtab + cj * 8 + 4);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint32_t ch = half * 256 + opaque_lane(lane) * 4;
        const f4 *c = C.c[half];
        f4 zz;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            zz[q] = add_rn(add_rn(add_rn(mul_rn(c[0][q], tw.x), mul_rn(c[1][q], tw.y)), mul_rn(c[2][q], tw.z)),
                           mul_rn(c[3][q], tw.w));
        *reinterpret_cast<f4 *>(stage + cj * LDS_LD + ch) = zz;
    }
}
// bit j set: column c0 + j starts a run (its nw corner offset, which fixes all four corners,
// differs from column c0 + j - 1's); bit 0 always set
__device__ __forceinline__ uint32_t cell_run_starts(const float *gtab, int c0) {
    uint32_t starts = 1u;
    uint32_t prev = __builtin_amdgcn_readfirstlane(__float_as_uint(gtab[c0 * 8]));
#pragma unroll
    for (int j = 1; j < COLS / WAVES; ++j) {
        const uint32_t k = __builtin_amdgcn_readfirstlane(__float_as_uint(gtab[(c0 + j) * 8]));
        if (k != prev) starts |= 1u << j;
        prev = k;
    }
    return starts;
}
// the whole stage of one wave, including the barrier that frees the image it aliases
__device__ __forceinline__ void stage_proj_runs(const float *__restrict__ pz, const float *gtab, float *stage,
                                                int wave, int lane) {
    constexpr int NC = COLS / WAVES;
    const int c0 = NC * wave;
    const uint32_t starts = cell_run_starts(gtab, c0);
    // first run start after column j (NC = none)
    auto next = [&](int j) -> int {
        const uint32_t m = starts & ~((2u << j) - 1u);
        return m ? __builtin_ctz(m) : NC;
    };
    CellRows A, B, C;
    int a = 0, b = next(0), c = b < NC ? next(b) : NC;
    cell_load(A, pz, gtab, c0 + a, lane);
    if (b < NC) cell_load(B, pz, gtab, c0 + b, lane);
    if (c < NC) cell_load(C, pz, gtab, c0 + c, lane);
    lds_barrier();   // the previous GEMM's image reads are done: the stage may overwrite it
    int j = 0;
    for (;;) {
        // A holds the run [a, b), B [b, c), C [c, d)
        const int d = c < NC ? next(c) : NC;
        for (; j < b; ++j) cell_blend_store(A, gtab, stage, c0 + j, lane);
        if (j >= NC) break;
        if (d < NC) cell_load(A, pz, gtab, c0 + d, lane);
        const int e = d < NC ? next(d) : NC;
        for (; j < c; ++j) cell_blend_store(B, gtab, stage, c0 + j, lane);
        if (j >= NC) break;
        if (e < NC) cell_load(B, pz, gtab, c0 + e, lane);
        const int f = e < NC ? next(e) : NC;
        for (; j < d; ++j) cell_blend_store(C, gtab, stage, c0 + j, lane);
        if (j >= NC) break;
        if (f < NC) cell_load(C, pz, gtab, c0 + f, lane);
        a = d;
        b = e;
        c = f;
    }
}
// stage_proj_runs' twin on the latent itself (the lin_z GEMM follows): z = the bilinear sample of
// the latent's four corner rows (torch's nw, ne, sw, se summation order) of every column, written
// as the GEMM's input image -- fp32 image[column][LDS_LD], or (HP) scaled by the column's maximum
// over all 512 channels and split into P0 / P1 with its exponent in ecol.  Wave w walks its
// COLS / WAVES columns; each load instruction reads one contiguous 1 KB half of a corner's 2 KB
// channel row (lane = 4 channels).  zsave (training forward, or NULL): the tile's rows of the
// activation save's z region, of which the first n_valid are points.  Callers barrier before
// (the image is free) and after.
template <bool HP>
__device__ __forceinline__ void stage_latent_gather(const float *__restrict__ latent, const float *gtab, float *image,
                                                    _Float16 *P0, _Float16 *P1, int *ecol, float *zsave,
                                                    int64_t n_valid, int wave, int lane) {
#pragma unroll 4
    for (int j = 0; j < COLS / WAVES; ++j) {
        const int cj = (COLS / WAVES) * wave + j;
        const f4 to = *reinterpret_cast<const f4 *>(gtab + cj * 8);
        const f4 tw = *reinterpret_cast<const f4 *>(gtab + cj * 8 + 4);
        f4 zh[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const uint32_t ch = half * 256 + opaque_lane(lane) * 4;
            const f4 c0 = *reinterpret_cast<const f4 *>(latent + __float_as_uint(to.x) + ch);
            const f4 c1 = *reinterpret_cast<const f4 *>(latent + __float_as_uint(to.y) + ch);
            const f4 c2 = *reinterpret_cast<const f4 *>(latent + __float_as_uint(to.z) + ch);
            const f4 c3 = *reinterpret_cast<const f4 *>(latent + __float_as_uint(to.w) + ch);
            f4 zz;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                zz[q] = add_rn(add_rn(add_rn(mul_rn(c0[q], tw.x), mul_rn(c1[q], tw.y)), mul_rn(c2[q], tw.z)),
                               mul_rn(c3[q], tw.w));
            if constexpr (HP) zh[half] = zz;
            else *reinterpret_cast<f4 *>(image + cj * LDS_LD + ch) = zz;
            if (zsave && cj < n_valid) *reinterpret_cast<f4 *>(zsave + (int64_t)cj * H + ch) = zz;
        }
        if constexpr (HP) {
            // column max over the wave (all 512 channels), scale, split
            float m = 0.f;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
                m = fmaxf(m, fmaxf(fmaxf(fabsf(zh[hf][0]), fabsf(zh[hf][1])), fmaxf(fabsf(zh[hf][2]), fabsf(zh[hf][3]))));
            m = wave_max(m);
            const int e = scale_exp(m);
            const float sc = __builtin_ldexpf(1.f, e);
            put_split4(P0, P1, cj * ROWH + swz(cj, lane * 4), zh[0], sc);
            put_split4(P0, P1, cj * ROWH + swz(cj, 256 + lane * 4), zh[1], sc);
            if (lane == 0) ecol[cj] = e;
        }
    }
}
// x[r][c] += stage rows of this wave (column 16c + cl, rows 16 (RTW wave + r) + 4g ..)
__device__ __forceinline__ void add_stage(Acc &x, const float *stage, int wave, int lane) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const f4 v = *reinterpret_cast<const f4 *>(stage + (16 * c + cl) * LDS_LD + 16 * (RTW * wave + r) + 4 * g);
            f4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = add_rn(x[r][c][q], v[q]);
            x[r][c] = o;
        }
}

// hidx: header slot of the layer's weight scale (0 lin_in, 1 + packed 512-wide index).
// R: a ring primed (hring_prime) on this layer's weights, or nullptr (PREC 3 only).
// OWN (PREC 3, the input image written by the wave's last publish): the column exponents come from
// that publish's registers (g.ecl) instead of LDS, so the accumulator scaling does not wait on a read.
// NP (PREC 3 / 1): the parts of this layer's weights and input image; PREC 1 runs its 512-wide
// layers with 1 and lin_in with 2 (g.ws_off is the offset in the mode's 512-wide layers).
template <int PREC, int NK, int DIST = H_DIST, bool OWN = false, int NP = nparts(PREC)>
__device__ __forceinline__ void layer_gemm(Acc &acc, const float *layer_base, GemmCtx &g, int hidx,
                                           HRing<DIST, NP> *R = nullptr) {
    PT(g, 3);
    PT_COUNT(g, 5);
    if constexpr (PREC == 0) {
        gemm<NK>(acc, layer_base + g.wl_off, g.inb4);
    } else if constexpr (is_h(PREC)) {
        // the accumulators run in the products' scale 2^(eW + e_col): exact for powers of
        // two, so the fp32 rounding sequence is that of the unscaled sum
        const int cl = opaque_lane(g.lane) & 15;
        const int ew = (int)g.hdr[HDR_ESCALE + hidx];
        float sa[CT], ia[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int e = (OWN ? g.ecl[c] : g.ecol[16 * c + cl]) + ew;
            sa[c] = __builtin_ldexpf(1.f, e);
            ia[c] = __builtin_ldexpf(1.f, -e);
        }
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                acc[r][c] *= sa[c];
            }
        Fair *F = g.fair.prog ? &g.fair : nullptr;
        // this wave's first row tile + this lane, in the layer's own part count
        const int wso = NP == nparts(PREC) ? (int)g.ws_off : RTW * g.wave * srt_h_floats(NP) + g.lane * 4;
        if (R) gemm_f16_primed<NK / 2, DIST, NP>(acc, *R, layer_base + opaque_lane(wso), g.pb0, g.pb1, F);
        else gemm_f16<NK / 2, DIST, NP>(acc, layer_base + opaque_lane(wso), g.pb0, g.pb1, F);
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                acc[r][c] *= ia[c];
            }
    } else {
        gemm_split<NK / 2, PREC>(acc, layer_base + g.ws_off, g.inbw, g.stg, g.wave, g.lane);
    }
    PT(g, 2);
}

// One lane's global atomic add of 1 to *p; the old value is returned to every lane.  The lane mask
// is narrowed and restored inside the asm, so the caller is straight-line code with no divergent
// region.  (The tile claim was `if (tid == 0) *s_next = grab();`: ROCm 7.2's register allocator
// placed a spill of the thread id in that branch's join block BEFORE its EXEC restore, so only
// lane 0 stored it and every other lane reloaded stale scratch -- the round-5 illegal-address
// faults.  isa_lint.py now rejects any build with a spill in that position.)  Called by a whole
// wave with every lane active, so lane 0 is the lane that adds.
__device__ __forceinline__ int claim_one(int *p) {
    int old;
    unsigned long long saved;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "s_nop 4\n\t"
        "global_atomic_add %0, %2, %3, off sc0\n\t"
        "s_mov_b64 exec, %1\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_nop 4"
        : "=&v"(old), "=&s"(saved)
        : "v"(p), "v"(1)
        : "memory");
    return __builtin_amdgcn_readfirstlane(old);
}

}  // namespace mlpk
}  // namespace pnr
