// Layouts of the fused MLP (mlp.hip, mlp_bwd.hip, mlp_pack.hip): the tile constants, the weight
// pack, the activation save and the LDS maps of k_point_mlp and k_mlp_bwd.  Host and device; no
// kernels.
#pragma once
#include "pnr_common.h"

namespace pnr {
namespace mlpk {

constexpr int H = 512;             // d_hidden == d_latent (only width implemented)
constexpr int NRT = H / 16;        // 32 row tiles per layer
constexpr int NKB = H / 16;        // 32 k-blocks (16 k each) for K = 512
constexpr int NKB_IN = 4;          // lin_in k-blocks (d_in <= 64, zero padded)
constexpr int WAVES = 8;           // two waves per SIMD
constexpr int NTHR = 64 * WAVES;
constexpr int RTW = NRT / WAVES;   // row tiles per wave (4 at 8 waves)
constexpr int CT = 4;              // column tiles (16 columns each)
constexpr int COLS = 16 * CT;      // 64 points per tile
constexpr int LDS_LD = H + 4;      // floats per column in the LDS activation buffer
constexpr int KB_FLOATS = NRT * 256;          // one k-block of a packed layer (32 KB)
constexpr int LAYER_FLOATS = NKB * KB_FLOATS; // one packed 512x512 layer (1 MB)
constexpr int HDR = 64;            // header floats: pe freqs [0,16), phases [16,32)
// split-bf16 modes (PREC 6 / 9): v_mfma_f32_16x16x32_bf16, k-steps of 32
constexpr int KS32 = H / 32;       // 16 k-steps for K = 512
constexpr int KS32_IN = 2;         // lin_in (d_in <= 64)
constexpr int SRT_FLOATS = 768;    // one (k-step, row tile): 3 parts x 64 lanes x 8 bf16
constexpr int SKS_FLOATS = NRT * SRT_FLOATS;  // one k-step of a packed layer (96 KB)
// scaled-fp16 mode (PREC 3): 2 parts x 64 lanes x 8 f16 per (k-step, row tile)
constexpr int SRT16_FLOATS = 512;
constexpr int SKS16_FLOATS = NRT * SRT16_FLOATS;  // 64 KB
constexpr int HDR_ESCALE = 32;     // header floats [32, 64): per-layer weight scale exponents
                                   // (PREC 3): [32] lin_in, [33 + j] packed 512-wide layer j
// half-precision modes: 3 = f16x3 (two parts), 1 = f16 (one part in the 512-wide layers)
__host__ __device__ constexpr bool is_h(int prec) { return prec == 3 || prec == 1; }
__host__ __device__ constexpr int nparts(int prec) { return prec == 1 ? 1 : 2; }
// floats of one (k-step, row tile) / one k-step of an NP-part fp16 layer: NP x 64 lanes x 8 f16
__host__ __device__ constexpr int srt_h_floats(int np) { return np * 256; }
__host__ __device__ constexpr int sks_h_floats(int np) { return NRT * srt_h_floats(np); }
static_assert(srt_h_floats(2) == SRT16_FLOATS && sks_h_floats(2) == SKS16_FLOATS, "two-part layout");
// 512-wide layers: PREC 1 streams one part; lin_in keeps the two-part layout in both fp16 modes
__host__ __device__ constexpr int sks_floats(int prec) {
    return prec == 3 ? SKS16_FLOATS : prec == 1 ? sks_h_floats(1) : SKS_FLOATS;
}
__host__ __device__ constexpr int sks_in_floats(int prec) { return is_h(prec) ? SKS16_FLOATS : SKS_FLOATS; }
constexpr int STG_FLOATS = CT * 3 * 256;   // one split-bf16 staging buffer: [ct][part][lane][8 bf16]
// LDS image of the GEMM input in PREC 3: each activation column c scaled by 2^e_c and
// split ONCE by its producer into two fp16 parts, P0 / P1 = [column][ROWH halves]
// (4 B per element, the same as fp32).  The row pitch (1056 B = 66 x 16 B) makes the
// B-fragment ds_read_b128 of every lane group hit 16 distinct 16-B bank quads.
constexpr int ROWH = H + 16;                    // halves per column row
constexpr int PART_HALVES = COLS * ROWH;        // one part (67,584 B)
constexpr int H_DIST = 4;          // f16 weight prefetch distance (row tiles), every kernel: 4 measured
                                   // 1.7 % faster than 3 on the forward (5, 6 slower), and the training
                                   // step 1.2 % faster (17.29 -> 17.10 ms) although k_mlp_bwd spills

struct Layout {
    int prec;                      // 0 = f32 MFMA, 6 / 9 = split-bf16 products, 3 = scaled f16 (two parts),
                                   // 1 = scaled f16 (one part)
    int n_linz, n_l512, n_blocks, ncomb, d_in, d_out, pe_n;
    int64_t layer_floats;
    int64_t off_lin_in, off_l512, off_lin_out, off_bias, nbias, off_out32, total;
};

inline Layout make_layout(const pnr_mlp_desc &d) {
    Layout L;
    L.n_blocks = d.n_blocks;
    L.n_linz = d.combine_layer < d.n_blocks ? d.combine_layer : d.n_blocks;
    L.ncomb = L.n_linz;
    L.n_l512 = L.n_linz + 2 * d.n_blocks;
    L.d_in = d.d_in;
    L.d_out = d.d_out;
    L.pe_n = d.pe_n;
    L.prec = d.precision;
    L.layer_floats = L.prec ? (int64_t)KS32 * sks_floats(L.prec) : (int64_t)LAYER_FLOATS;
    L.off_lin_in = HDR;
    L.off_l512 = L.off_lin_in + (L.prec ? (int64_t)KS32_IN * sks_in_floats(L.prec) : (int64_t)NKB_IN * KB_FLOATS);
    L.off_lin_out = L.off_l512 + (int64_t)L.n_l512 * L.layer_floats;
    L.off_bias = L.off_lin_out + (int64_t)NKB * 256;
    L.nbias = (int64_t)(1 + L.n_l512) * H + 16;
    // PREC 3 / 1: lin_out's weights in fp32 as [input channel][4 outputs] (the VALU head, k_point_mlp)
    L.off_out32 = ((L.off_bias + L.nbias + 63) / 64) * 64;
    L.total = L.off_out32 + (is_h(L.prec) ? 4 * H : 0);
    return L;
}

// packed L512 layer index of block `blk`, kind 0 = lin_z, 1 = fc_0, 2 = fc_1
__host__ __device__ inline int layer_index(int blk, int kind, int n_linz) {
    return blk < n_linz ? 3 * blk + kind : 3 * n_linz + 2 * (blk - n_linz) + (kind - 1);
}

// floats of the activation save per point (Args::save): the fp32 regions, then the relu
// sign masks of the 2 nb + 1 relu slots, [slot][point][64 bytes] (save_mask's bit order)
// for the backward's masks
__host__ __device__ constexpr int64_t save_floats_per_point(int n_blocks) {
    return 64 + (int64_t)H * (2 + 2 * n_blocks) + 16 * (2 * n_blocks + 1);
}
__host__ __device__ constexpr int64_t save_mask_offset(int n_blocks, int64_t n_points) {
    return (64 + (int64_t)H * (2 + 2 * n_blocks)) * n_points;
}

// the power-of-two exponent e with m * 2^e <= 2^14 (fp16 max 65504), clamped to [-64, 40]: the
// scale of a packed layer's weights (k_layer_escale) and of an activation column
__device__ __forceinline__ int scale_exp(float m) {
    if (!(m > 0.f) || !(m < 3.0e38f)) return 0;       // zero / inf / nan: unscaled
    int e = 14 - __builtin_amdgcn_frexp_expf(m);      // m < 2^frexp_exp
    return e < -64 ? -64 : (e > 40 ? 40 : e);
}

// ---- LDS maps: offsets in floats from the start of dynamic LDS ------------------------------
// The kernels form their pointers from these and the launchers pass lds_bytes().
// k_point_mlp: first the GEMM input image, which the fp32 stage of the projected latent aliases.
// fp16 modes (PREC 3 / 1): P0 | P1, [column][ROWH halves] each; else the fp32 activations
// [column][LDS_LD], then the split staging ring stg (2 x STG_FLOATS).  Then gtab (per-column gather
// records: 4 corner offsets | 4 weights) and petab (the pack header's PE freqs / phases, 32; s_next,
// the next tile, at + 32).  fp16 modes also: cmax [column][wave] and ecol [column] (a publish's
// partial maxima and exponents) before petab, prog (Fair's count per wave) in its tail, and hpart
// (head partials [wave][column][4]) after it.  The fused march appends [mreg, end): the ray's z and
// head outputs, the epilogue scratch w | cdf | sort, near / far, the fine pack's PE table petab_f.
// The lean instantiation appends ltab after the march region: launch constants that every tile's
// features need, computed once per workgroup (LeanTab).
struct FwdLds {
    int stg, gtab, cmax, ecol, petab, s_next, prog, hpart, mreg, mscr, mnf, petab_f, end, ltab;
};
// ltab slots (floats): the coarse draw's constants (march_dev.h CoarseSteps), then the projection's
// (k_point_mlp: the latent size as floats, the pixel -> grid scales and the half extents)
enum LeanTab { LT_END = 0, LT_LSTEP, LT_STEP, LT_PAD, LT_WLF, LT_HLF, LT_KX, LT_KY, LT_HX, LT_HY, LT_FLOATS = 16 };
constexpr int IMG_H_FLOATS = PART_HALVES;           // P0 + P1 in floats (two halves per float)
constexpr int MARCH_BUF_FLOATS = 640;               // z [128] | raw [128][4]
constexpr FwdLds fwd_lds(bool hp) {
    FwdLds m = {};
    m.stg = COLS * LDS_LD;
    m.gtab = hp ? IMG_H_FLOATS : m.stg + 2 * STG_FLOATS;
    m.cmax = m.gtab + COLS * 8;
    m.ecol = m.cmax + COLS * 8;
    m.petab = hp ? m.ecol + COLS : m.gtab + COLS * 8;
    m.s_next = m.petab + 32;
    m.prog = m.petab + 40;
    m.hpart = m.petab + 64;
    m.mreg = hp ? m.hpart + WAVES * COLS * 4 : m.petab + 36;
    m.mscr = m.mreg + MARCH_BUF_FLOATS;
    m.mnf = m.mscr + 3 * 128;
    m.petab_f = m.mnf + 4;
    m.end = m.petab_f + 32;
    m.ltab = m.end;
    return m;
}
constexpr size_t lds_bytes(const FwdLds &m, bool march) { return sizeof(float) * (size_t)(march ? m.end : m.mreg); }
constexpr size_t lds_bytes_lean(const FwdLds &m) { return sizeof(float) * (size_t)(m.ltab + LT_FLOATS); }
constexpr int MARCH_LDS_FLOATS = fwd_lds(true).end - fwd_lds(true).mreg;

// k_mlp_bwd: P0 | P1 | cmax | ecol | prog as the forward's fp16 map, no gather records
struct BwdLds {
    int cmax, ecol, prog, end;
};
constexpr BwdLds bwd_lds() {
    BwdLds m = {};
    m.cmax = IMG_H_FLOATS;
    m.ecol = m.cmax + COLS * 8;
    m.prog = m.ecol + COLS;
    m.end = m.prog + WAVES;
    return m;
}
constexpr size_t lds_bytes(const BwdLds &m) { return sizeof(float) * (size_t)m.end; }

static_assert(lds_bytes(fwd_lds(true), false) == 147968 && lds_bytes(fwd_lds(false), false) == 158864 &&
              lds_bytes(bwd_lds()) == 137504, "LDS totals");
static_assert(lds_bytes(fwd_lds(true), true) == 147968 + 4 * MARCH_LDS_FLOATS &&
              lds_bytes(fwd_lds(false), true) == 158864 + 4 * MARCH_LDS_FLOATS &&
              fwd_lds(false).end - fwd_lds(false).mreg == MARCH_LDS_FLOATS, "LDS totals with the march region");
static_assert(lds_bytes(fwd_lds(true), true) <= 160 * 1024 && lds_bytes(fwd_lds(false), true) <= 160 * 1024 &&
              lds_bytes(bwd_lds()) <= 160 * 1024, "one workgroup's LDS");
static_assert(lds_bytes_lean(fwd_lds(true)) == lds_bytes(fwd_lds(true), true) + 4 * LT_FLOATS &&
              lds_bytes_lean(fwd_lds(true)) <= 160 * 1024 && fwd_lds(true).ltab % 4 == 0,
              "the lean table fits beside the fp16 map and the march region, 16-byte aligned");
static_assert(sizeof(float) * COLS * LDS_LD <= 2 * sizeof(_Float16) * PART_HALVES,
              "the fp32 stage fits in the split image it aliases");

}  // namespace mlpk
}  // namespace pnr
