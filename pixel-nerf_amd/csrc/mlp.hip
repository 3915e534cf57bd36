// Fused per-point pixelNeRF model and ray march on gfx950 MFMA.
//
// Replaces PixelNeRFNet.forward (models.py:146-266) for the shipped conf:
//   world->camera transform (162-165), positional encoding (code.py:30-42),
//   view directions (184-196), pinhole projection + bilinear border gather of
//   the encoder latent (206-221, encoder.py:80-109), ResnetFC (resnetfc.py:132-184)
//   with the multi-view mean at combine_layer (util.py:461-471), and the
//   sigmoid/relu head (258-265); with the fused march (Args::march) also the coarse
//   draws, the composite and the fine draws of NeRFRenderer.forward (nerf.py:251-303).
//
// Work decomposition:
//   * a workgroup = 8 waves (two per SIMD) = a tile of 64 points ("columns"); persistent
//     workgroups, one per CU, take tiles (or a ray's tiles) from per-XCD counters.
//   * every layer is OUT^T (512 x 64) = W (512 x K) * IN^T (K x 64).  Wave w owns output
//     rows [64w, 64w + 64) for all 64 columns: 4 row tiles x 4 column tiles = 16
//     accumulators; x (the residual stream) and h stay in registers for the whole network.
//   * f16x3 (PREC 3, the default): IN^T lives in LDS already scaled per column and split
//     into two fp16 planes P0 / P1 by its producer (features, latent stage, relu publish);
//     W is pre-packed (k_pack_f16) in A-fragment order with a per-layer scale and streamed
//     from L2 through a register ring H_DIST row tiles ahead of v_mfma_f32_16x16x32_f16.
//     fp32 (PREC 0) and split-bf16 (PREC 6 / 9) keep an fp32 image and their own GEMMs.
//   * f16 (PREC 1, inference on the projected-latent path only): the f16x3 schedule with ONE
//     part in every 512 -> 512 layer: W 2^eW and relu(acc) 2^e_col are each rounded once to fp16
//     (RNE), one v_mfma_f32_16x16x32_f16 product per k-step, fp32 accumulation, the scales undone
//     exactly.  The weight stream of those layers is single-part (half of f16x3's bytes) and the
//     publish writes P0 only.  Left as in f16x3: lin_in (2 k-steps, d_in 42: two-part features
//     and weights, three products), the lin_z contribution (the fp32 projected latent), the
//     multi-view mean and the head (fp32 from the accumulators).
// Diagnostic build knobs: pnr_diag.h.
#include "pnr_diag.h"
#include <atomic>
#include <cstddef>

// the timing builds' counters live in this translation unit alone (pnr_diag.h's stamps add to them)
#ifdef PNR_EPI_TIMING
__device__ unsigned long long g_epi[8];
#endif

#include "march_dev.h"
#include "mlp_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace mlpk {

#ifdef PNR_PHASE_TIMING
__device__ unsigned long long g_phase[PT_SLOTS];
#endif

// ------------------------------------------------------------------------------
struct Args {
    const float *packed;
    Layout L;
    // points: render mode (rays + z) or query mode (xyz + dirs)
    int render_mode;
    const float *rays, *zs;
    int K;
    int64_t rays_per_obj;
    const float *xyz, *dirs;
    int64_t points_per_obj;
    int64_t n_points;
    // scene
    const float *latent, *cams;
    int ns, hl, wl;
    float img_w, img_h;
    float *out;
    float *xsum;       // scratch: gridDim.x x 2 x (COLS * H) floats; of a workgroup's pair of regions the
                       // first is unused, the second holds the multi-view sum
    int64_t n_tiles;
    // training forward (NS == 1): activations for the backward, fp32 row-major [point][width]:
    //   features (64) | z (512) | relu(x) into fc_0 of block b (512 each) |
    //   relu(h) of block b (512 each) | relu(x) into lin_out (512)          (save_floats())
    float *save;
    // projected latent (k_latent_proj, PZ kernels): lin_z block b reads proj + b * proj_stride,
    // (n_obj * n_views, H_l, W_l, 512) like the latent
    const float *proj;
    int64_t proj_stride;
    // dynamic tile scheduling: 8 per-XCD tile counters, 64 B apart (zeroed per launch)
    int *tile_ctr;
    // fused ray march (render mode, K = 64 m.kpt): a workgroup takes a ray's kpt tiles in a
    // row, keeps their z and head outputs in LDS and composites the ray in the epilogue of
    // its last tile (march_epilogue); `out` may then be NULL (raw never reaches HBM)
    int march;
    MarchCfg m;
};

// The march config read where it is used (kernarg s_loads through a pointer the compiler cannot
// see through): hoisted out of the tile loop, its ~30 loop-invariant dwords held SGPRs across
// the GEMMs and spilled them (256 SGPR spills, 40 B/lane of VGPR scratch against 16).
typedef const __attribute__((address_space(4))) MarchCfg *CfgPtr;
// (k_point_mlp's only parameter is Args, so Args::m sits at offsetof(Args, m) in the kernarg
// segment; taking &a instead would copy the whole by-value Args to the stack)
__device__ __forceinline__ CfgPtr march_cfg(const Args &) {
    uint64_t v = (uint64_t)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() +
                            offsetof(Args, m));
    asm volatile("" : "+s"(v));
    return (CfgPtr)v;
}
__device__ __forceinline__ RngSrc ld_rng(const __attribute__((address_space(4))) RngSrc &r) {
    RngSrc o;
    o.p = r.p;
    o.seed = r.seed;
    o.offset = r.offset;
    o.stream = r.stream;
    return o;
}
// Fused ray march, one wave: composite ray b from the z / head outputs its kpt tiles left in
// LDS (buf: z [128] | raw [128][4]; nf: near, far) with the standalone composite's code
// (composite_wave), then, in a coarse pass that feeds a fine pass, draw the ray's fine
// samples (sample_fine_wave) from the weights it just computed (scr: w | cdf | sort).  The
// Philox draws come first: they depend only on the ray, so their latency overlaps the
// composite's.
template <int S>
__device__ __forceinline__ void march_ray(const Args &a, int64_t b, const float *buf, const float *nf, float *scr,
                                          int lane, bool fine_pass) {
    const CfgPtr c = march_cfg(a);
    EPI_DECL
    const int kf = fine_pass ? 0 : c->kf;   // the single-launch fine pass draws nothing
    FineDraws d = {0.f, 0.f, 0.f};
    if (kf > 0) d = fine_draws(lane, b, kf, c->kfd, ld_rng(c->u_fine), ld_rng(c->u_jit), ld_rng(c->n_depth));
    const float near = nf[0], far = nf[1];
    float zk[S], wk[S];
    f4 v[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {   // composite_wave's lane ownership: sample 64 i + lane
        zk[i] = buf[64 * i + lane];
        v[i] = *reinterpret_cast<const f4 *>(buf + 128 + 4 * (64 * i + lane));
    }
    const float depth = fine_pass
        ? composite_wave<S>(lane, b, COLS * S, far, zk, v, c->white_bkgd, c->weights_f, c->rgb_f, c->depth_f, wk)
        : composite_wave<S>(lane, b, COLS * S, far, zk, v, c->white_bkgd, c->weights, c->rgb, c->depth, wk);
    EPI_T(0);
#ifdef PNR_EPI_TIMING
    if (lane == 0) atomicAdd(&g_epi[7], 1ull);
#endif
    if (kf > 0) {
        float *w = scr;
#pragma unroll
        for (int i = 0; i < S; ++i) w[64 * i + lane] = wk[i];
        wave_lds_sync();
        // single launch: the sorted fine depths also go to buf's z region (whose coarse depths
        // composite_wave and the sort's inputs have consumed) for the ray's fine tiles.
        // scr + 128 / scr + 256: this epilogue's fixed form of FineLds (march_dev.h) behind the ray's 128
        // weights, cdf (kc + 1 <= 65 floats) then the sort buffer (n_sort <= 128); no origin here
        sample_fine_wave(lane, b, near, far, COLS * S, w, buf, depth, kf, c->kfd, c->depth_std, RngSrc{}, RngSrc{},
                         RngSrc{}, c->lindisp != 0, c->n_sort, scr + 128, scr + 256, nullptr, c->z_fine, nullptr,
                         nullptr, true, d, c->single ? const_cast<float *>(buf) : nullptr);
    }
}
__device__ __forceinline__ void march_epilogue(const Args &a, int64_t b, const float *buf, const float *nf,
                                               float *scr, int lane, bool fine_pass) {
    if ((fine_pass ? march_cfg(a)->kpt_f : march_cfg(a)->kpt) == 1) march_ray<1>(a, b, buf, nf, scr, lane, fine_pass);
    else march_ray<2>(a, b, buf, nf, scr, lane, fine_pass);
}

// Loads of launch inputs that no kernel of the launch writes (rays, cameras, ray order), through the
// constant address space: with a wave-uniform address they are scalar loads into SGPRs.
typedef const __attribute__((address_space(4))) float *CFloatPtr;
typedef const __attribute__((address_space(4))) int *CIntPtr;
__device__ __forceinline__ CFloatPtr as_const(const float *p) { return (CFloatPtr)(uint64_t)p; }
__device__ __forceinline__ CIntPtr as_const(const int *p) { return (CIntPtr)(uint64_t)p; }

// Multi-view mean (combine_interleaved, util.py:461-471: sum over views, then / ns; ns > 1): view
// v's x joins the running sum in this thread's slots of xs (v = 0 starts it); after the last
// view x = sum / ns.
__device__ __forceinline__ void view_mean(Acc &x, float *xs, int v, int ns) {
    const float nsf = (float)ns;
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            f4 *ptr = reinterpret_cast<f4 *>(xs + (r * CT + c) * 256);
            const f4 sum = v == 0 ? x[r][c] : *ptr + x[r][c];
            if (v < ns - 1) *ptr = sum;
            else x[r][c] = sum / nsf;
        }
}

// PZ: lin_z from the projected latent (gather_proj) instead of the latent gather + GEMM;
// MARCH: the fused ray march (a.m), a separate instantiation so that the plain point model
// keeps its own register allocation;
// LEAN: the render of one source view by a per-pass fused march (modes 1 and 2) without an
// activation save, which is every launch of the headline (launch_point_mlp selects it).  What such
// a launch never takes is compiled out -- the view loop and the multi-view sum, the activation
// save, the single-launch march's fine tiles, the point-query loads -- and what is the same for
// all 512 threads of a tile is scalar: the tile index, the unit's ray (origin, direction, near /
// far) and the object's camera row are SGPRs loaded by scalar loads, not per-lane copies.  The
// per-lane arithmetic is the general kernel's, op for op, so the outputs are bit-identical
// (tests/test_gpu_mlp_lean.py).
template <int PREC, bool PZ, bool MARCH, bool LEAN = false>
__global__ __launch_bounds__(NTHR) void k_point_mlp(Args a) {
    static_assert(!LEAN || (PZ && MARCH && is_h(PREC)), "LEAN is the fused-march render on the projected latent");
    constexpr int KD = H_DIST;   // weight ring distance
    constexpr bool HP = is_h(PREC);      // a scaled-fp16 mode: f16x3 (3) or f16 (1)
    constexpr int NP = nparts(PREC);     // parts of the 512-wide layers' weights and of the publish
    static_assert(PREC != 1 || PZ, "PREC 1 is built for the projected-latent path only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr FwdLds M = fwd_lds(HP);      // the LDS map (mlp_layout.h): every region is inbuf + its offset
    float *inbuf = smem;                   // the start of dynamic LDS; fp32 modes: the image, COLS x LDS_LD
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int cl = lane & 15;
    const Layout &L = a.L;

    // per-lane fragment bases
    const int64_t wl_off = (int64_t)(RTW * wave) * 256 + lane * 4;         // f32 fragments
    const int64_t ws_off = (int64_t)(RTW * wave) * (HP ? srt_h_floats(NP) : SRT_FLOATS) + lane * 4;
    const float *inb = inbuf + cl * LDS_LD + 4 * g;     // B (f32): column 16c + cl, k 16kb + 4g
    GemmCtx gc;
    gc.wl_off = wl_off;
    gc.ws_off = ws_off;
    gc.inb4 = inb;
    gc.inbw = inbuf + (16 * (wave % CT) + cl) * LDS_LD + 8 * g + 4 * (wave / CT);
    gc.stg = inbuf + M.stg;
    // (PREC 1: the 512-wide layers' image is P0 alone; P1 holds lin_in's second feature part.  The
    // image region is sized by the fp32 stage of the projected latent that aliases it, so the map
    // and the launch's LDS size are PREC 3's.)
    _Float16 *P0 = reinterpret_cast<_Float16 *>(smem);
    _Float16 *P1 = P0 + PART_HALVES;
    float *gtab = inbuf + M.gtab;
    float *cmax = inbuf + M.cmax;             // PREC 3: per-column partial maxima (64 x 8)
    int *ecol = reinterpret_cast<int *>(inbuf + M.ecol);
    // PE freqs [0, 16) / phases [16, 32) of the pack header, in LDS: the feature loop indexes
    // them per lane, and vector global loads there put a memory latency in every iteration
    float *petab = inbuf + M.petab;
    // (the one-time LDS fills below are whole-wave writes -- lanes 32 apart store the same value --
    // rather than `if (tid < 32)` branches: no divergent region for a misplaced spill, claim_one)
    if (wave == 0) petab[lane & 31] = a.packed[lane & 31];   // visible after the first barrier of a tile
    gc.hdr = a.packed;
    // B fragment (column 16c + cl, k 32 ks + 8g): swz keeps it linear in ks and c
    gc.pb0 = P0 + cl * ROWH + swz(cl, 8 * g);
    gc.pb1 = P1 + cl * ROWH + swz(cl, 8 * g);
    gc.ecol = ecol;
    gc.fair.prog = nullptr;
    gc.fair.wave = wave;
    gc.fair.it = 0;
    gc.fair.mate = 0;
    if constexpr (HP) {
        gc.fair.prog = reinterpret_cast<int *>(inbuf + M.prog);
        if (wave == 0) gc.fair.prog[lane & (WAVES - 1)] = 0;   // visible after the first barrier
    }
    gc.wave = wave;
    gc.lane = lane;
#ifdef PNR_PHASE_TIMING
    for (int i = 0; i < PT_SLOTS; ++i) gc.pt[i] = 0;
    gc.pt_last = __builtin_amdgcn_s_memtime();
#endif
    // feature role: thread -> (column col, part qt of WAVES); FPT features each
    constexpr int FPT = 64 / WAVES;

    // relu(acc) -> the next GEMM's input image (callers barrier before and after)
    // activation save slots (training forward)
    // Every region has PS = n_points * n_views rows: row v P + p holds (view v, point p) of
    // the per-view stages (features, z, the blocks before the combine layer), row p the
    // per-point stages after it (their other rows are unused).
    const int64_t P = a.n_points, PS = P * a.ns;
    float *sv_f = a.save, *sv_z = a.save ? a.save + PS * 64 : nullptr;
    auto sv_slot = [&](int i) { return sv_z + PS * H * (1 + i); };   // i: block b -> x_in, nb + b -> h, 2nb -> x_f
    uint32_t *sv_mask = a.save ? reinterpret_cast<uint32_t *>(a.save + save_mask_offset(L.n_blocks, PS)) : nullptr;
    // Barrier between a GEMM that reads the input image and the publish that rewrites it.
    // PREC 3's publish writes only its column maxima before its own internal barrier, and
    // the image after it, so there the barrier is redundant and waves that finish their GEMM
    // early start the publish VALU under their SIMD-mate's MFMAs.
    auto pre_publish_sync = [&]() {
        if constexpr (!HP)
            lds_barrier();
    };
    auto publish_relu = [&](const Acc &acc, int64_t tile, int save_idx, int64_t row0) {
        if constexpr (!LEAN) {
            if (a.save) {
                save_relu(acc, sv_slot(save_idx) + row0 * H, tile, P, wave, lane);
                save_mask(acc, sv_mask + PS * 16 * save_idx + row0 * 16, tile, P, wave, lane);
            }
        }
        if constexpr (HP) {
            // (phase-timing slots 17, 13-15, 16: glue split into the ring prime / bias loads
            // before the publish, colmax VALU, its barrier, the split, the closing barrier)
            PT(gc, 17);
            relu_colmax(acc, cmax, wave, lane);
            PT(gc, 13);
            lds_barrier();
            PT(gc, 14);
            relu_store_split<true, NP>(acc, P0, P1, cmax, ecol, wave, lane, gc.ecl);
            PT(gc, 15);
        } else {
            store_relu(acc, inbuf, wave, lane);
        }
    };

    Acc x, h;
    // Dynamic, XCD-aware tile order.  Workgroups are placed round-robin on the 8 XCDs
    // (blockIdx.x % 8); XCD x owns the contiguous tile range [x T / 8, (x + 1) T / 8)
    // (neighbouring tiles are neighbouring rays, which sample neighbouring latent pixels, so
    // each XCD's L2 holds its own band of the projected latent).  Its workgroups take tiles
    // from that range through an atomic counter and, once it is empty, from the other XCDs'
    // ranges: a slower CU or XCD no longer leaves the rest of the chip idle at the end of
    // the launch.  The next tile is fetched before the head, so the atomic's latency hides.
    int *s_next = reinterpret_cast<int *>(inbuf + M.s_next);
    float *hpart = inbuf + M.hpart;   // PREC 3 head: per-wave partials [wave][column][4] (8 KB)
    // fused march (MARCH): the ray's z [128] | head outputs [128][4], the epilogue scratch,
    // near / far.  (Deferring a ray's epilogue into the next tile, under the SIMD-mate's MFMAs,
    // was measured: the double buffers and the call inside the GEMM region cost more in spills
    // than it hid.)
    float *mreg = inbuf + M.mreg;
    float *mscr = inbuf + M.mscr;
    float *mnf = inbuf + M.mnf;
    const int kpt = MARCH ? march_cfg(a)->kpt : 1;   // tiles per ray and pass when marching
    // tiles per scheduling unit (a ray when marching): its kpt tiles, and with the single-launch
    // march (m.single) its kpt_f fine tiles after them
    const bool single = !LEAN && MARCH && march_cfg(a)->single;   // (LEAN: false at compile time)
    const int upt = single ? kpt + march_cfg(a)->kpt_f : kpt;
    // single launch: the fine tiles' PE table from the fine pack's header (the packs
    // of two MLPs may carry different tables); visible after the first barrier
    float *petab_f = inbuf + M.petab_f;
    if (single && wave == 1) petab_f[lane & 31] = march_cfg(a)->packed_f[lane & 31];
    // the projection's launch constants (proj_consts, pnr_common.h)
    auto proj_consts = [&]() -> ProjK { return pnr::proj_consts(a.wl, a.hl, a.img_w, a.img_h); };
    // LEAN: ltab, the launch constants that a tile's features need, computed once (every lane
    // computes the same values; wave 0 stores them, visible after the first barrier).  Computed in
    // the loop they are hoisted out of it as uniform floats in VGPRs that live across every tile,
    // which the allocator spills to scratch and reloads in each tile's feature phase.
    float *ltab = inbuf + M.ltab;
    if constexpr (LEAN) {
        const CoarseSteps cs = coarse_steps(COLS * kpt);
        const ProjK pk = proj_consts();
        if (wave == 0) {
            ltab[LT_END] = cs.end;
            ltab[LT_LSTEP] = cs.lstep;
            ltab[LT_STEP] = cs.step;
            ltab[LT_WLF] = pk.wlf;
            ltab[LT_HLF] = pk.hlf;
            ltab[LT_KX] = pk.kx;
            ltab[LT_KY] = pk.ky;
            ltab[LT_HX] = pk.hx;
            ltab[LT_HY] = pk.hy;
        }
    }
    // the next unit's first tile, claimed by wave 0 (wave-uniform: every value here is scalar)
    auto grab = [&]() -> int {
        const int64_t T = a.n_tiles / upt;
        const int x0 = blockIdx.x & 7;
        for (int k = 0; k < 8; ++k) {
            const int x = (x0 + k) & 7;
            const int64_t lo = x * T / 8, hi = (x + 1) * T / 8;
            if (lo >= hi) continue;
            const int64_t i = lo + claim_one(a.tile_ctr + 16 * x);
            if (i < hi) return (int)(i * upt);
        }
        return (int)a.n_tiles;
    };
    if (wave == 0) *s_next = grab();
    lds_barrier();
    // the tile taken from s_next; LEAN: broadcast, so the tile and what derives from it are scalar
    auto take = [&]() -> int64_t {
        const int t = *s_next;
        if constexpr (LEAN) return __builtin_amdgcn_readfirstlane(t);
        else return t;
    };
    for (int64_t tile = take(); tile < a.n_tiles; tile = take()) {
        // this tile within its unit: pass_f = a fine tile of the single-launch march; sub = the
        // tile within its pass (the ray's kpt_t tiles of K_t = 64 kpt_t samples)
        // (LEAN: upt = kpt is 1 or 2, launch_point_mlp: a shift instead of a 64-bit division)
        const int64_t unit = LEAN ? (upt == 2 ? tile >> 1 : tile) : tile / upt;
        const int s_in = (int)(tile - unit * upt);
        const bool pass_f = single && s_in >= kpt;
        const int sub = pass_f ? s_in - kpt : s_in;
        const int kpt_t = pass_f ? march_cfg(a)->kpt_f : kpt;
        // MARCH: the unit's ray (pnr_render_cfg.ray_order; read at use, an L2-hit scalar load);
        // an entry out of range marches the unit's own index instead of faulting
        auto ray_of = [&]() -> int64_t {
            const int *o = MARCH ? march_cfg(a)->order : nullptr;
            if (!o) return unit;
            if constexpr (LEAN) {
                // a scalar load; the unit count n_tiles / upt as above, in 32 bits (n_tiles < 2^31,
                // launch_point_mlp), so the range check is scalar compares
                const int r = as_const(o)[unit];
                const int n_units = upt == 2 ? (int)a.n_tiles >> 1 : (int)a.n_tiles;
                return r >= 0 && r < n_units ? (int64_t)r : unit;
            } else {
                const int64_t r = o[unit];
                return r >= 0 && r < a.n_tiles / upt ? r : unit;
            }
        };
        // the pass's pack and projected latent (read at use: no per-tile SGPR state)
        auto PK = [&]() -> const float * { return pass_f ? march_cfg(a)->packed_f : a.packed; };
        auto PJ_ = [&]() -> const float * { return pass_f ? march_cfg(a)->proj_f : a.proj; };
        const float *bias = PK() + L.off_bias;
        gc.hdr = PK();
        // the multi-view sum's slots of this thread: the second of the workgroup's pair of 128 KB
        // regions of a.xsum, L2-resident (the first is unused; the address is formed at use: nothing
        // per tile stays live across the GEMMs)
        auto xs_ptr = [&]() {
            return a.xsum + (int64_t)blockIdx.x * (2 * COLS * H) + COLS * H + wave * (RTW * CT * 256) + opaque_lane(lane) * 4;
        };
        auto W512 = [&](int layer) -> const float * { return PK() + L.off_l512 + (int64_t)layer * L.layer_floats; };
        // ---- one 512 -> 512 layer: publish relu(src) as the input image, then dst (+)= W relu(src) + b.
        // fp16 modes prime the layer's weight ring, and every mode loads its bias rows, before the
        // publish.  The pre_publish_sync that frees the image is the caller's.
        auto relu_layer = [&](const Acc &src, Acc &dst, int layer, int save_idx, int64_t row0, bool accumulate)
                              __attribute__((always_inline)) {
            HRing<KD, NP> R;
            if constexpr (HP) hring_prime(R, W512(layer) + opaque_lane((int)gc.ws_off));
            f4 nb[RTW];
            load_bias(nb, bias + (1 + layer) * H, wave, lane);
            publish_relu(src, tile, save_idx, row0);
            lds_barrier();
            PT(gc, 16);
            set_bias(dst, nb, accumulate);
            layer_gemm<PREC, NKB, KD, HP>(dst, W512(layer), gc, 1 + layer, HP ? &R : nullptr);
        };
        // ---- residual block blk (resnetfc.py:69-84) on the packed layers l0 (fc_0) and l0 + 1 (fc_1):
        // h = fc_0(relu(x)); x += fc_1(relu(h)).  row0: the view's first row of the activation save.
        auto res_block = [&](int blk, int l0, int64_t row0) __attribute__((always_inline)) {
            relu_layer(x, h, l0, blk, row0, false);
            pre_publish_sync();
            relu_layer(h, x, l0 + 1, L.n_blocks + blk, row0, true);
        };

        // source views (LEAN: one, so no view loop; else read at use like every launch constant)
        auto NS = [&]() -> int {
            if constexpr (LEAN) return 1;
            else return a.ns;
        };
        for (int v = 0; v < NS(); ++v) {
            // per view: keeps the feature addresses out of scratch across the GEMMs
            const int tid_t = opaque_lane(tid);
            const int col = tid_t / WAVES, qt = tid_t % WAVES;
            const int64_t p_raw = tile * COLS + col;
            const int64_t p = p_raw < a.n_points ? p_raw : a.n_points - 1;
            // the point (re-read per view from L2 rather than held in registers across the
            // per-view blocks' GEMMs)
            float px, py, pz, dx, dy, dz, zz = 0.f;
            int64_t obj;
            // LEAN: the object's camera row and the ray's near / far, fetched with the ray
            float cam_s[16], nf_s[2];
            if constexpr (LEAN) {
                // The unit's ray and the object's camera row by scalar loads: 8 + 16 SGPRs that
                // every lane's arithmetic below reads as scalar operands (the same fp32 operations
                // on the same values as the general path's per-lane copies).
                const int64_t b = ray_of();
                const int kk = sub * COLS + col;
                const int kt = COLS * kpt_t;
                const CFloatPtr rp = as_const(a.rays) + b * 8;
                float ray[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) ray[i] = rp[i];
                // one object per launch is the common case: no 64-bit division then (the divisor
                // through an empty asm: the division's set-up is not hoisted out of the tile loop)
                int64_t rpo = a.rays_per_obj;
                asm volatile("" : "+s"(rpo));
                obj = b < rpo ? 0 : b / rpo;
                const CFloatPtr cp = as_const(a.cams) + obj * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) cam_s[i] = cp[i];
                if (march_cfg(a)->sample_coarse) {
                    const CfgPtr m = march_cfg(a);
                    const CoarseSteps cs = {ltab[LT_END], ltab[LT_LSTEP], ltab[LT_STEP]};
                    zz = coarse_z_at(ld_rng(m->u_coarse), b, kt, kk, ray[6], ray[7], m->lindisp != 0, cs);
                    float *zo = m->z_out;
                    if (zo && qt == 0) zo[b * kt + kk] = zz;
                } else {
                    zz = a.zs[b * kt + kk];
                }
                dx = ray[3]; dy = ray[4]; dz = ray[5];
                px = add_rn(ray[0], mul_rn(zz, dx));
                py = add_rn(ray[1], mul_rn(zz, dy));
                pz = add_rn(ray[2], mul_rn(zz, dz));
                nf_s[0] = ray[6];
                nf_s[1] = ray[7];
            } else if (a.render_mode) {
                // ray b, sample kk of its pass (MARCH: the unit's ray, K = 64 kpt_t)
                const int64_t b = MARCH ? ray_of() : p / a.K;
                const int kk = MARCH ? sub * COLS + col : (int)(p - b * a.K);
                const int kt = MARCH ? COLS * kpt_t : a.K;
                const float *ray = a.rays + b * 8;
                if (MARCH && pass_f) {
                    // single launch: the coarse epilogue left the ray's sorted fine depths in
                    // mreg (its wave joins this barrier after writing them)
                    lds_barrier();
                    zz = mreg[kk];
                } else if (MARCH && march_cfg(a)->sample_coarse) {
                    // the coarse draw in the prologue (nerf.py:98-118), or the given depth
                    const CfgPtr m = march_cfg(a);
                    zz = coarse_z(ld_rng(m->u_coarse), b, kt, kk, ray[6], ray[7], m->lindisp != 0);
                    float *zo = m->z_out;
                    if (zo && qt == 0 && v == 0) zo[b * kt + kk] = zz;
                } else {
                    zz = a.zs[b * kt + kk];
                }
                dx = ray[3]; dy = ray[4]; dz = ray[5];
                // points = o + z * d  (nerf.py:185)
                px = add_rn(ray[0], mul_rn(zz, dx));
                py = add_rn(ray[1], mul_rn(zz, dy));
                pz = add_rn(ray[2], mul_rn(zz, dz));
                obj = b / a.rays_per_obj;
            } else {
                px = a.xyz[p * 3 + 0]; py = a.xyz[p * 3 + 1]; pz = a.xyz[p * 3 + 2];
                if (a.dirs) { dx = a.dirs[p * 3 + 0]; dy = a.dirs[p * 3 + 1]; dz = a.dirs[p * 3 + 2]; }
                else { dx = dy = dz = 0.f; }
                obj = p / a.points_per_obj;
            }
            PT_WAIT();
            PT(gc, 8);
            // ---- per (point, view) geometry (this thread's column) ----------------
            const float *cam_p = a.cams + (obj * NS() + v) * 16;
            auto cam = [&](int i) -> float {
                if constexpr (LEAN) return cam_s[i];
                else return cam_p[i];
            };
            float xr[3], vd[3], xc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float r0 = cam(3 * i), r1 = cam(3 * i + 1), r2 = cam(3 * i + 2);
                xr[i] = add_rn(add_rn(mul_rn(r0, px), mul_rn(r1, py)), mul_rn(r2, pz));
                vd[i] = add_rn(add_rn(mul_rn(r0, dx), mul_rn(r1, dy)), mul_rn(r2, dz));
                xc[i] = add_rn(xr[i], cam(9 + i));
            }
            const float fx = cam(12), fy = cam(13), cx = cam(14), cy = cam(15);
            PT_WAIT();
            PT(gc, 9);
            // features f = FPT qt .. FPT qt + FPT - 1 of [xyz_rot | PE | viewdir_cam | 0]
            lds_barrier();   // previous users of inbuf are done
            PT(gc, 10);
            if (MARCH && qt == 0 && v == 0) {   // for the epilogue
                if (!pass_f) mreg[sub * COLS + col] = zz;
                if (col == 0 && sub == 0) {
                    if constexpr (LEAN) {
                        mnf[0] = nf_s[0];
                        mnf[1] = nf_s[1];
                    } else {
                        const float *rr = a.rays + ray_of() * 8;
                        mnf[0] = rr[6];
                        mnf[1] = rr[7];
                    }
                }
            }
            {
                const int npe = 3 * L.pe_n;
                const float *pet = MARCH && pass_f ? petab_f : petab;   // this pass's PE table
                float fv[FPT];
#pragma unroll
                for (int i = 0; i < FPT; ++i) {
                    const int f = FPT * qt + i;
                    float val = 0.f;
                    if (f < 3) val = xr[f];
                    else if (f < 3 + npe) {
                        const int m = f - 3, q = m / 3, d = m - 3 * q;
                        const float xd = d == 0 ? xr[0] : (d == 1 ? xr[1] : xr[2]);
                        val = sinf(add_rn(pet[16 + q], mul_rn(xd, pet[q])));   // code._phases, _freqs
                    } else if (f < 6 + npe) {
                        const int d = f - 3 - npe;
                        val = d == 0 ? vd[0] : (d == 1 ? vd[1] : vd[2]);
                    }
                    fv[i] = val;
                }
                if constexpr (!LEAN) {
                    if (a.save && p_raw < a.n_points) {
#pragma unroll
                        for (int i = 0; i < FPT / 4; ++i)
                            *reinterpret_cast<f4 *>(sv_f + (v * P + p_raw) * 64 + FPT * qt + 4 * i) =
                                f4{fv[4 * i], fv[4 * i + 1], fv[4 * i + 2], fv[4 * i + 3]};
                    }
                }
                if constexpr (HP) {
                    // column max over its WAVES feature threads (adjacent lanes), scale, split
                    float m = 0.f;
#pragma unroll
                    for (int i = 0; i < FPT; ++i) m = fmaxf(m, fabsf(fv[i]));
#pragma unroll
                    for (int o = 1; o < WAVES; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                    const int e = scale_exp(m);
                    const float sc = __builtin_ldexpf(1.f, e);
#pragma unroll
                    for (int i = 0; i < FPT / 4; ++i)
                        put_split4(P0, P1, col * ROWH + swz(col, FPT * qt + 4 * i),
                                   f4{fv[4 * i], fv[4 * i + 1], fv[4 * i + 2], fv[4 * i + 3]}, sc);
                    if (qt == 0) ecol[col] = e;
                } else {
#pragma unroll
                    for (int i = 0; i < FPT / 4; ++i)
                        *reinterpret_cast<f4 *>(inbuf + col * LDS_LD + FPT * qt + 4 * i) =
                            f4{fv[4 * i], fv[4 * i + 1], fv[4 * i + 2], fv[4 * i + 3]};
                }
            }
            PT(gc, 11);
            // projection (models.py:206-212) -> grid_sample coords (encoder.py:95-108)
            float u = mul_rn(__fdiv_rn(-xc[0], xc[2]), fx);
            float w = mul_rn(__fdiv_rn(-xc[1], xc[2]), fy);
            u = add_rn(u, cx);
            w = add_rn(w, cy);
            // (LEAN: the launch's constants from ltab instead of registers that live across the tile loop)
            const ProjK pk = [&]() {
                if constexpr (LEAN) {
                    const f4 t = *reinterpret_cast<const f4 *>(ltab + LT_WLF);
                    return ProjK{t.x, t.y, t.z, t.w, ltab[LT_HX], ltab[LT_HY]};
                } else {
                    return proj_consts();
                }
            }();
            const float wlf = pk.wlf, hlf = pk.hlf;
            const float gx = sub_rn(mul_rn(u, pk.kx), 1.f);
            const float gy = sub_rn(mul_rn(w, pk.ky), 1.f);
            float ix = mul_rn(add_rn(gx, 1.f), pk.hx);
            float iy = mul_rn(add_rn(gy, 1.f), pk.hy);
            ix = fminf(fmaxf(ix, 0.f), wlf - 1.f);   // border padding; NaN -> 0
            iy = fminf(fmaxf(iy, 0.f), hlf - 1.f);
            const float x0f = floorf(ix), y0f = floorf(iy);
            const float we = sub_rn(ix, x0f), wn = sub_rn(iy, y0f);
            const float ee = sub_rn(1.f, we), ss = sub_rn(1.f, wn);
            float wnw = mul_rn(ss, ee), wne = mul_rn(ss, we), wsw = mul_rn(wn, ee), wse = mul_rn(wn, we);
            const int x0 = (int)x0f, y0 = (int)y0f;
            const int x1 = x0 + 1 < a.wl ? x0 + 1 : x0, y1 = y0 + 1 < a.hl ? y0 + 1 : y0;
            if (x0 + 1 >= a.wl) { wne = 0.f; wse = 0.f; }
            if (y0 + 1 >= a.hl) { wsw = 0.f; wse = 0.f; }
            if (qt == 0) {
                // per-column gather record: 4 corner offsets (floats from a.latent) + weights
                const uint32_t base = (uint32_t)((obj * NS() + v) * (int64_t)a.hl * a.wl * H);
                const uint32_t o00 = base + (uint32_t)(y0 * a.wl + x0) * H, o01 = base + (uint32_t)(y0 * a.wl + x1) * H;
                const uint32_t o10 = base + (uint32_t)(y1 * a.wl + x0) * H, o11 = base + (uint32_t)(y1 * a.wl + x1) * H;
                float *t = gtab + col * 8;
                *reinterpret_cast<f4 *>(t) = f4{__uint_as_float(o00), __uint_as_float(o01),
                                                __uint_as_float(o10), __uint_as_float(o11)};
                *reinterpret_cast<f4 *>(t + 4) = f4{wnw, wne, wsw, wse};
            }
            PT(gc, 12);
            lds_barrier();   // features visible
            PT(gc, 0);
            // ---- lin_in ---------------------------------------------------------------
            add_bias(x, bias, wave, lane, false);
            layer_gemm<PREC, NKB_IN, KD, false, 2>(x, PK() + L.off_lin_in, gc, 0);   // two-part in PREC 1 too
            // ---- blocks before the combine layer: x += lin_z(z); x = block(x) ------
            for (int blk = 0; blk < L.ncomb; ++blk) {
                const int lz = layer_index(blk, 0, L.ncomb);
                if constexpr (PZ) {
                    // the stage aliases the image the previous GEMM read; publish_relu's
                    // internal barrier orders the add_stage reads before the image writes
                    const float *pz = PJ_() + blk * a.proj_stride;
                    stage_proj_runs(pz, gtab, inbuf, wave, lane);
                    PT(gc, 3);
                    lds_barrier();
                    PT(gc, 1);
                    add_bias(x, bias + (1 + lz) * H, wave, lane, true);
                    add_stage(x, inbuf, wave, lane);
                } else {
                lds_barrier();
                PT(gc, 3);
                float *zsave = a.save && blk == 0 ? sv_z + (v * P + tile * COLS) * H : nullptr;
                stage_latent_gather<HP>(a.latent, gtab, inbuf, P0, P1, ecol, zsave, P - tile * COLS, wave, lane);
                lds_barrier();
                PT(gc, 1);
                add_bias(x, bias + (1 + lz) * H, wave, lane, true);
                layer_gemm<PREC, NKB, KD>(x, PK() + L.off_l512 + (int64_t)lz * L.layer_floats, gc, 1 + lz);
                pre_publish_sync();
                }
                res_block(blk, lz + 1, v * P);
            }
            // ---- multi-view mean (combine_interleaved: sum over views, then / NS) --
            if constexpr (!LEAN) {
                if (a.ns > 1) view_mean(x, xs_ptr(), v, a.ns);
            }
        }
        // ---- blocks after the combine layer ------------------------------------------
        for (int blk = L.ncomb; blk < L.n_blocks; ++blk) {
            const int l0 = layer_index(blk, 1, L.ncomb);
            pre_publish_sync();
            res_block(blk, l0, 0);
        }
        // ---- lin_out(relu(x)) + head [sigmoid(rgb), relu(sigma)]: wave w < CT -> columns 16w..
        if (wave == 0) *s_next = s_in + 1 < upt ? (int)tile + 1 : grab();   // read after the closing barrier
        pre_publish_sync();
        if constexpr (HP) {
            // no publish: the head reads relu(x) from the accumulators (below); only the
            // activation save of lin_out's input remains
            if constexpr (!LEAN) {
                if (a.save) {
                    save_relu(x, sv_slot(2 * L.n_blocks), tile, P, wave, lane);
                    save_mask(x, sv_mask + PS * 16 * (2 * L.n_blocks), tile, P, wave, lane);
                }
            }
        } else {
            publish_relu(x, tile, 2 * L.n_blocks, 0);
            lds_barrier();
        }
        PT(gc, 16);
        PT(gc, 3);
        if (HP) {
            // fp32 head straight from the accumulators (resnetfc.py:184 lin_out on relu(x)):
            // lane (g, cl) holds rows 16 (RTW wave + r) + 4 g + i of column 16 c + cl; it sums
            // W_out^T (fp32, [channel][output] at off_out32) times relu(x) over its 16 rows, then
            // over the wave's four lane rows (rows_sum), and lane row g stores column tile g's
            // partial at hpart[wave][column][output]; after the closing barrier waves 0-3 add the
            // 8 waves' partials in wave order.  Replaces the last layer's colmax / split publish
            // and the split-fp16 head GEMM (the k_point_mlp round-4 head change).
            const int ln = opaque_lane(lane), g4 = ln >> 4, c16 = ln & 15;
            const float *w32 = PK() + L.off_out32;
            f4 o[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RTW; ++r) {
                const f4 *wr = reinterpret_cast<const f4 *>(w32 + 4 * (16 * (RTW * wave + r) + 4 * g4));
                const f4 w[4] = {wr[0], wr[1], wr[2], wr[3]};
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const f4 v = relu4(x[r][c]);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[c][j] = fmaf(v[i], w[i][j], o[c][j]);
                }
            }
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[c][j] = rows_sum(o[c][j]);
            const f4 mine = g4 == 0 ? o[0] : g4 == 1 ? o[1] : g4 == 2 ? o[2] : o[3];
            *reinterpret_cast<f4 *>(hpart + (wave * COLS + 16 * g4 + c16) * 4) = mine;
        } else if (!HP && wave < CT) {   // wave-uniform: the first CT waves own one column tile each
            const float *wo = PK() + L.off_lin_out + lane * 4;
            const float *bi = inbuf + (16 * wave + cl) * LDS_LD + 4 * g;
            f4 o0 = *reinterpret_cast<const f4 *>(bias + (1 + L.n_l512) * H + 4 * g);
            f4 o1 = {0.f, 0.f, 0.f, 0.f}, o2 = o1, o3 = o1;
#pragma unroll 4
            for (int kb = 0; kb < NKB; ++kb) {
                const f4 wv = *reinterpret_cast<const f4 *>(wo + kb * 256);
                const f4 bv = *reinterpret_cast<const f4 *>(bi + kb * 16);
                o0 = mfma(wv.x, bv.x, o0);
                o1 = mfma(wv.y, bv.y, o1);
                o2 = mfma(wv.z, bv.z, o2);
                o3 = mfma(wv.w, bv.w, o3);
            }
            const f4 o = (o0 + o1) + (o2 + o3);
            const int64_t po = tile * COLS + 16 * wave + cl;
            if (g == 0 && po < a.n_points) {
                f4 r;
                r.x = __fdiv_rn(1.f, add_rn(1.f, expf(-o.x)));
                r.y = __fdiv_rn(1.f, add_rn(1.f, expf(-o.y)));
                r.z = __fdiv_rn(1.f, add_rn(1.f, expf(-o.z)));
                r.w = max_nc(o.w, 0.f);   // torch.relu: NaN stays NaN
                if (!MARCH || a.out)   // MARCH: the ray's own points (ray_order)
                    *reinterpret_cast<f4 *>(a.out + (MARCH ? ray_of() * (COLS * kpt_t) + sub * COLS + 16 * wave + cl
                                                           : po) * 4) = r;
                if (MARCH) *reinterpret_cast<f4 *>(mreg + 128 + 4 * (sub * COLS + 16 * wave + cl)) = r;
            }
        }
        PT(gc, 4);
        PT_COUNT(gc, 6);
        lds_barrier();   // s_next and the head partials written
        if (HP && wave < CT) {   // [sigmoid(rgb), relu(sigma)] of column tile `wave`
            const int ln = opaque_lane(lane), gg = ln >> 4, cc = ln & 15;
            const int col = 16 * wave + cc;
            f4 o = *reinterpret_cast<const f4 *>(hpart + col * 4);
#pragma unroll
            for (int w = 1; w < WAVES; ++w) o = o + *reinterpret_cast<const f4 *>(hpart + (w * COLS + col) * 4);
            const f4 b = *reinterpret_cast<const f4 *>(bias + (1 + L.n_l512) * H + 4 * gg);
            o = o + b;
            const int64_t po = tile * COLS + col;
            if (gg == 0 && po < a.n_points) {
                f4 r;
                r.x = __fdiv_rn(1.f, add_rn(1.f, expf(-o.x)));
                r.y = __fdiv_rn(1.f, add_rn(1.f, expf(-o.y)));
                r.z = __fdiv_rn(1.f, add_rn(1.f, expf(-o.z)));
                r.w = max_nc(o.w, 0.f);   // torch.relu: NaN stays NaN
                if (!MARCH || a.out)   // MARCH: the ray's own points (ray_order)
                    *reinterpret_cast<f4 *>(a.out + (MARCH ? ray_of() * (COLS * kpt_t) + sub * COLS + col : po) * 4) = r;
                if (MARCH) *reinterpret_cast<f4 *>(mreg + 128 + 4 * (sub * COLS + 16 * wave + cc)) = r;
            }
        }
        // ---- fused march: the ray's last tile composites it (and draws its fine samples) --
        if (MARCH && sub == kpt_t - 1) {   // the ray's last tile of this pass
            lds_barrier();   // the ray's head outputs visible
            if (wave == WAVES - 1) march_epilogue(a, ray_of(), mreg, mnf, mscr, opaque_lane(lane), pass_f);
        }
    }
#ifdef PNR_PHASE_TIMING
    if (threadIdx.x == 64 * PNR_PT_WAVE)   // the recorded wave
        for (int i = 0; i < PT_SLOTS; ++i) atomicAdd(&g_phase[i], (unsigned long long)gc.pt[i]);
#endif
}

}  // namespace mlpk

// ------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------
#ifdef PNR_EPI_TIMING
extern "C" int pnr_debug_epi(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(::g_epi), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    static const unsigned long long zero[8] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(::g_epi), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef PNR_PHASE_TIMING
// diagnostic: copy (and optionally clear) the phase counters; not part of the ABI
extern "C" int pnr_debug_phase(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mlpk::g_phase), sizeof(unsigned long long) * mlpk::PT_SLOTS) != hipSuccess)
        return -1;
    if (reset) {
        static const unsigned long long zero[mlpk::PT_SLOTS] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mlpk::g_phase), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
int64_t mlp_save_floats(const pnr_mlp_desc &d, int64_t n_points) {
    return mlpk::save_floats_per_point(d.n_blocks) * n_points;
}

size_t mlp_xsum_bytes(int ns) {
    (void)ns;  // one pair of 128 KB regions per resident workgroup (the first unused, the second the
               // multi-view sum; the size is observable: pnr_point_query_workspace_bytes), then the
               // 8 per-XCD tile counters (512 B)
    return sizeof(float) * (size_t)device_cu_count() * 2 * mlpk::COLS * mlpk::H + 512;
}

// The lean instantiation (k_point_mlp<.., LEAN>): a process-wide switch, default on, and the
// kernel the last launch of the process took (pnr_mlp_set_lean / pnr_mlp_last_kernel, pnr_abi.h)
static std::atomic<int> g_mlp_lean{1};
static std::atomic<int> g_mlp_last_kernel{PNR_MLP_KERNEL_NONE};
int mlp_set_lean(int on) { return g_mlp_lean.exchange(on != 0); }
int mlp_last_kernel() { return g_mlp_last_kernel.load(std::memory_order_relaxed); }

// Kernel selection.  PREC comes from the descriptor's precision, PZ / MARCH / LEAN from the call;
// exactly the instantiations that exist: PZ x MARCH for every PREC (f16, PREC 1, has no
// latent-gather form: launch_point_mlp refuses it), and LEAN for the two fp16 modes.
template <int PREC, bool PZ, bool MARCH, bool LEAN = false>
static void launch_kernel(unsigned grid, size_t lds, hipStream_t st, const mlpk::Args &a) {
    hipLaunchKernelGGL((mlpk::k_point_mlp<PREC, PZ, MARCH, LEAN>), dim3(grid), dim3(mlpk::NTHR), lds, st, a);
}
template <int PREC>
static void select_kernel(bool pz, bool march, bool lean, unsigned grid, size_t lds, hipStream_t st,
                          const mlpk::Args &a) {
    if constexpr (mlpk::is_h(PREC)) {
        if (lean) return launch_kernel<PREC, true, true, true>(grid, lds, st, a);
    }
    if constexpr (PREC != 1) {
        if (!pz) return march ? launch_kernel<PREC, false, true>(grid, lds, st, a)
                              : launch_kernel<PREC, false, false>(grid, lds, st, a);
    }
    return march ? launch_kernel<PREC, true, true>(grid, lds, st, a)
                 : launch_kernel<PREC, true, false>(grid, lds, st, a);
}

// Launch the fused model over c.n_points points (render mode if c.rays != nullptr).
int launch_point_mlp(const pnr_scene &sc, const pnr_mlp_desc &d, const PointMlpCall &c, hipStream_t st) {
    const MarchCfg *const march = c.march;
    if (c.n_points == 0) return PNR_OK;
    if (d.precision == PNR_PREC_F16 && (!c.proj || c.save))
        return fail(PNR_ERR_UNSUPPORTED, "precision 1 (f16) is inference only on the projected-latent path: it "
                    "needs the latent projection and takes no activation save; use precision 3 (f16x3)");
    if (c.proj && c.save) return fail(PNR_ERR_UNSUPPORTED, "the activation save (training) needs the latent gather path");
    if (march && (!c.rays || c.save || (march->kpt != 1 && march->kpt != 2) || c.K != mlpk::COLS * march->kpt ||
                  c.n_points % c.K != 0 || (march->kf > 0 && (c.K > 64 || march->n_sort > 128 || c.K + march->kf > march->n_sort))))
        return fail(PNR_ERR_INVALID, "point_mlp: fused march needs K = 64 kpt (kpt 1 or 2) and kc + kf <= 128");
    if (march && march->single &&
        (!c.proj || !march->packed_f || !march->proj_f || march->kf <= 0 || march->kpt != 1 ||
         march->kpt_f * mlpk::COLS != c.K + march->kf || (march->kpt_f != 1 && march->kpt_f != 2) ||
         !march->rgb_f || !march->depth_f || c.n_points % (c.K + march->kpt_f * mlpk::COLS) != 0))
        return fail(PNR_ERR_INVALID, "point_mlp: the single-launch march needs kc = 64, kc + kf = 64 kpt_f, both "
                    "packs and projections, fine outputs, and n_points = n_rays (kc + kc + kf)");
    mlpk::Args a = {};
    a.packed = static_cast<const float *>(c.packed);
    a.L = mlpk::make_layout(d);
    a.render_mode = c.rays != nullptr;
    a.rays = c.rays; a.zs = c.z; a.K = c.K; a.rays_per_obj = c.rays_per_obj;
    a.xyz = c.xyz; a.dirs = c.dirs; a.points_per_obj = c.points_per_obj;
    a.n_points = c.n_points;
    a.latent = sc.latent; a.cams = sc.cams;
    a.ns = sc.n_views; a.hl = sc.latent_h; a.wl = sc.latent_w;
    a.img_w = sc.image_w; a.img_h = sc.image_h;
    a.out = c.out;
    a.xsum = c.xsum;
    a.march = march != nullptr;
    if (march) a.m = *march;
    a.n_tiles = (c.n_points + mlpk::COLS - 1) / mlpk::COLS;
    a.save = c.save;
    a.proj = c.proj;
    a.proj_stride = (int64_t)sc.n_obj * sc.n_views * sc.latent_h * sc.latent_w * mlpk::H;
    const int cus = device_cu_count();
    if (a.n_tiles >= (1ll << 31)) return fail(PNR_ERR_UNSUPPORTED, "more than 2^31 point tiles in one launch");
    a.tile_ctr = reinterpret_cast<int *>(c.xsum + (size_t)cus * 2 * mlpk::COLS * mlpk::H);
    if (hipMemsetAsync(a.tile_ctr, 0, 512, st) != hipSuccess) return fail(PNR_ERR_HIP, "point_mlp: hipMemsetAsync failed");
    const unsigned grid = (unsigned)(a.n_tiles < cus ? a.n_tiles : cus);
    // The lean instantiation: a render (rays) of ONE source view on the projected latent by a
    // per-pass fused march (modes 1 and 2, not the single launch), no activation save, f16x3 or
    // f16.  Every other descriptor takes the general instantiations.
    const bool lean = g_mlp_lean.load(std::memory_order_relaxed) && mlpk::is_h(d.precision) && c.proj && march &&
                      !march->single && c.rays && sc.n_views == 1 && !c.save;
    g_mlp_last_kernel.store(lean ? PNR_MLP_KERNEL_LEAN : PNR_MLP_KERNEL_GENERAL, std::memory_order_relaxed);
    const bool pz = c.proj != nullptr, fused = march != nullptr;
    const size_t lds = lean ? mlpk::lds_bytes_lean(mlpk::fwd_lds(true))   // the march map + the lean table
                            : mlpk::lds_bytes(mlpk::fwd_lds(mlpk::is_h(d.precision)), fused);
    switch (d.precision) {
    case PNR_PREC_F16: select_kernel<1>(pz, fused, lean, grid, lds, st, a); break;
    case PNR_PREC_F16X3: select_kernel<3>(pz, fused, lean, grid, lds, st, a); break;
    case PNR_PREC_BF16X6: select_kernel<6>(pz, fused, lean, grid, lds, st, a); break;
    case PNR_PREC_BF16X9: select_kernel<9>(pz, fused, lean, grid, lds, st, a); break;
    default: select_kernel<0>(pz, fused, lean, grid, lds, st, a);
    }
    return launch_ok("point_mlp") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
