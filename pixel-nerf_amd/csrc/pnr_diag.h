// Diagnostic builds of the fused MLP and ray-march kernels: every build knob the kernels still read.
//
// None of these is defined in the shipped build (pixel-nerf_amd/Makefile); a diagnostic library
// is built next to it with scripts/build_variant.sh NAME WORKTREE -D<knob> and loaded through
// PNR_LIB_PATH by the probes under tools/.  The knobs here only add timers or counters: results
// stay valid, and undefined they compile to nothing.
//
//   PNR_PHASE_TIMING   k_point_mlp: shader cycles per phase of the recorded wave (PT / PT_COUNT
//                      stamps, slots below), summed over workgroups; read by pnr_debug_phase
//                      (tools/mlp_probe.py).  PNR_PT_WAVE=w records wave w (default 0).
//   PNR_EPI_TIMING     the fused march epilogue (march_ray / sample_fine_wave): cycles of its
//                      composite, cdf, draws and sort; read by pnr_debug_epi (tools/gpu_epi_probe.sh).
//   PNR_WGH_STATS      k_wgrad_h: scale-move statistics (pnr_wgrad_stats, tools/wgrad_stats.py).
//
// The ablation knobs (the GEMM-only build and the per-piece ablations of the fused MLP and of
// the weight-gradient kernels: each removes a piece of work, results INVALID, used only to bound
// what that piece costs) are not in the product sources: tools/patches/ablations.diff lists them
// and restores them onto a build copy
// (PATCH=tools/patches/ablations.diff scripts/build_variant.sh NAME WORKTREE -D<knob>).
// Rejected schedule variants are patches under tools/patches/ too, each with its same-box A/B
// result in the header.
#pragma once
#include <cstdint>

// The stamps only: mlp.hip defines the counters g_epi / g_phase they add to, and is the one
// translation unit that stamps the epilogue (march_dev.h's stamps are no-ops in every other one).
#ifdef PNR_EPI_TIMING
#define EPI_DECL uint64_t epi_last_ = __builtin_amdgcn_s_memtime();
#define EPI_T(i)                                                                  \
    do {                                                                          \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                         \
        if (lane == 0) atomicAdd(&g_epi[i], (unsigned long long)(t_ - epi_last_)); \
        epi_last_ = t_;                                                           \
    } while (0)
#else
#define EPI_DECL
#define EPI_T(i) ((void)0)
#endif

// k_point_mlp phase slots (wave cycles per tile, summed): 0 features + projection, 1 latent
// gather / projected-row stage, 2 GEMMs, 3 glue (bias, barriers), 4 lin_out head, 5 GEMM calls,
// 6 tiles, 8-12 feature sub-phases, 13 colmax VALU, 14 colmax barrier, 15 split + stores,
// 16 barrier after the stores, 17 ring prime + bias loads before a publish.
#ifdef PNR_PHASE_TIMING
#define PT(gc, i)                                                     \
    do {                                                              \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();             \
        (gc).pt[i] += t_ - (gc).pt_last;                              \
        (gc).pt_last = t_;                                            \
    } while (0)
#define PT_COUNT(gc, i) ((gc).pt[i] += 1)
#define PT_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#ifndef PNR_PT_WAVE
#define PNR_PT_WAVE 0
#endif
#else
#define PT_WAIT() ((void)0)
#define PT(gc, i) ((void)0)
#define PT_COUNT(gc, i) ((void)0)
#endif
