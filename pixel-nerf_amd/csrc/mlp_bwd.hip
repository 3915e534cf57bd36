// Training backward of the fused MLP: k_mlp_bwd (the input-gradient chain on the forward's fp16
// GEMM, mlp_dev.h) and k_bias_reduce, with their launcher.
#include "mlp_dev.h"
#include "pnr_launch.h"

namespace pnr {
namespace mlpk {

// ---- training backward of ResnetFC (resnetfc.py:132-184, n_views == 1), PREC 3 -------------
// Per 64-point tile, the input-gradient chain in reverse block order on the forward's GEMM
// (W^T packed by k_pack_f16_t, the LDS image holding the signed gradient), with the relu
// masks read from the forward's activation save:
//   dx = (d_o W_out) . [x_f > 0]       (masks: the forward's sign bits, save_mask)
//   for b = nb-1 .. 0:  dY(fc_1 b) = dx
//                       dh = (W_1^T dx) . [h_b > 0]              dY(fc_0 b) = dh
//                       dx = dx + (W_0^T dh) . [x_b > 0]
//                       b < n_linz:  dY(lin_z b) = dx,  dzlat += W_z^T dx
//   dY(lin_in) = dx
// With NS > 1 source views (resnetfc.py:151-172, util.combine_interleaved) the blocks from
// combine_layer on run once per point; dL/d(view mean) / NS then enters the chain of the blocks
// before it once per view, on the forward save's view rows v P + p (masks, dY, dzlat).  View 0
// stores that value as its first dY slot (dY(fc_1, ncomb - 1)); views 1.. reload it from there.
// The output gradients dY of every layer go to global memory for the weight gradients
// (dW = dY^T IN over the points) and the bias gradients (column sums).  Slot order, chosen
// so that those are strided batched GEMMs over the save's slots:
//   dy[b] = dY(fc_0 b),  dy[nb] = dY(lin_in),  dy[nb + 1 + b] = dY(fc_1 b);
//   dY(lin_z b) = dy[nb + b] (the same values).
struct BwdArgs {
    const float *hdr;        // forward pack (header: weight scale exponents)
    const float *packed_t;   // k_pack_f16_t output
    const float *w_out;      // lin_out weight (4 x 512, fp32)
    const float *save;       // forward activation save (Args::save)
    const float *d_o;        // (P, 4) gradient of the pre-head output
    float *dy;               // (2 nb + 1) x (NS P) x 512; the slots of the blocks from combine_layer
                             // on use their first P rows
    float *dzlat;            // (NS P, 512) gradient of the sampled latent (n_linz > 0)
    float *bsum;             // NULL, or [workgroup][2 nb + 1][512] column sums of each dy slot
                             // over the workgroup's tiles (its tiles in order: deterministic)
    Layout L;
    int64_t n_points, n_tiles;
    int ns;                  // source views per point (the save's view rows)
};

// sum over the 16 lanes of a DPP row (every lane gets it; lane 0's order is the fixed tree
// ((a + a8) + (a4 + a12)) + ...)
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0x128>(0.f, v);   // row_ror:8
    v += dpp_f<0x124>(0.f, v);   // row_ror:4
    v += dpp_f<0x122>(0.f, v);   // row_ror:2
    v += dpp_f<0x121>(0.f, v);   // row_ror:1
    return v;
}

// this lane's fragment of row tile r of its wave in row `row` of a [row][512] matrix: channels
// 16 (RTW wave + r) + 4 g .. + 3
__device__ __forceinline__ const f4 *frag_at(const float *base, int64_t row, int wave, int r, int g) {
    return reinterpret_cast<const f4 *>(base + row * H + 16 * (RTW * wave + r) + 4 * g);
}
__device__ __forceinline__ f4 *frag_at(float *base, int64_t row, int wave, int r, int g) {
    return const_cast<f4 *>(frag_at(static_cast<const float *>(base), row, wave, r, g));
}

__device__ __forceinline__ void acc_zero(Acc &a) {
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) a[r][c] = f4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void acc_add(Acc &a, const Acc &b) {
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) a[r][c] += b[r][c];
}
__device__ __forceinline__ void acc_div(Acc &a, float d) {
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) a[r][c] = a[r][c] / d;
}

// this wave's rows of acc -> slot [point][512] (points < n_points)
__device__ __forceinline__ void store_rows(const Acc &acc, float *slot, int64_t tile, int64_t n_points,
                                           int wave, int lane, float *bs = nullptr, bool first = false) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        if (p >= n_points) continue;
#pragma unroll
        for (int r = 0; r < RTW; ++r) *frag_at(slot, p, wave, r, g) = acc[r][c];
    }
    if (bs) {   // bias gradient: this tile's column sums of the wave's rows, added to bs
        f4 sr[RTW];
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            f4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (tile * COLS + 16 * c + cl < n_points) t += acc[r][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = row16_sum(t[e]);
            sr[r] = t;
        }
        if (cl == 0) {
#pragma unroll
            for (int r = 0; r < RTW; ++r) {
                f4 *q = frag_at(bs, 0, wave, r, g);
                *q = first ? sr[r] : *q + sr[r];
            }
        }
    }
}
// store_rows' twin: acc <- this wave's rows of slot (a point past n_points reads the last point)
__device__ __forceinline__ void load_rows(Acc &acc, const float *slot, int64_t tile, int64_t n_points, int wave,
                                          int lane) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        const int64_t pc = p < n_points ? p : n_points - 1;
#pragma unroll
        for (int r = 0; r < RTW; ++r) acc[r][c] = *frag_at(slot, pc, wave, r, g);
    }
}
// store_rows, accumulating, on rows row0 + p: slot = first ? acc : slot + acc (points < n_points)
__device__ __forceinline__ void add_rows(const Acc &acc, float *slot, int64_t row0, int64_t tile, int64_t n_points,
                                         int wave, int lane, bool first) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        if (p >= n_points) continue;
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            f4 *q = frag_at(slot, row0 + p, wave, r, g);
            *q = first ? acc[r][c] : *q + acc[r][c];
        }
    }
}
// relu backward masks from the forward's sign bits (save_mask): this lane's two words of
// each of its CT points, loaded before the GEMM whose output they mask
typedef unsigned u2m __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void load_mask(u2m (&mk)[CT], const uint32_t *mslot, int64_t tile, int64_t n_points,
                                          int wave, int lane) {
    const int cl = opaque_lane(lane) & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t p = tile * COLS + 16 * c + cl;
        const int64_t pc = p < n_points ? p : n_points - 1;
        mk[c] = *reinterpret_cast<const u2m *>(mslot + pc * 16 + 2 * wave);
    }
}
// acc *= [activation > 0] (torch's relu backward); 0 past n_points
__device__ __forceinline__ void relu_mask(Acc &acc, const u2m (&mk)[CT], int64_t tile, int64_t n_points,
                                          int lane) {
    lane = opaque_lane(lane);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const bool valid = tile * COLS + 16 * c + cl < n_points;
#pragma unroll
        for (int r = 0; r < RTW; ++r) {
            // byte 2g + (r >> 1) of the wave's 8 bytes, bit 4 (r & 1) + e
            const int byte = 2 * g + (r >> 1);
            const uint32_t nib = valid ? (byte >= 4 ? mk[c].y : mk[c].x) >> (8 * (byte & 3) + 4 * (r & 1)) : 0u;
            const f4 v = acc[r][c];
            acc[r][c] = f4{(nib & 1u) ? v.x : 0.f, (nib & 2u) ? v.y : 0.f, (nib & 4u) ? v.z : 0.f,
                           (nib & 8u) ? v.w : 0.f};
        }
    }
}

__global__ __launch_bounds__(NTHR) void k_mlp_bwd(BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, cl = lane & 15;
    const Layout &L = a.L;
    const int nb = L.n_blocks;
    const int64_t P = a.n_points, PS = P * a.ns;
    // blocks [nc, nb) run per point, [0, nc) per view (all per point when NS == 1)
    const int nc = a.ns > 1 ? L.ncomb : 0;
    constexpr BwdLds M = bwd_lds();   // the LDS map (mlp_layout.h)
    _Float16 *P0 = reinterpret_cast<_Float16 *>(smem);
    _Float16 *P1 = P0 + PART_HALVES;
    float *cmax = smem + M.cmax;
    int *ecol = reinterpret_cast<int *>(smem + M.ecol);
    GemmCtx gc = {};
    gc.ws_off = (int64_t)(RTW * wave) * SRT16_FLOATS + lane * 4;
    gc.hdr = a.hdr;
    gc.pb0 = P0 + cl * ROWH + swz(cl, 8 * g);
    gc.pb1 = P1 + cl * ROWH + swz(cl, 8 * g);
    gc.ecol = ecol;
    gc.fair.prog = reinterpret_cast<int *>(smem + M.prog);
    gc.fair.wave = wave;
    if (threadIdx.x < WAVES) gc.fair.prog[threadIdx.x] = 0;
    gc.wave = wave;
    gc.lane = lane;
    // relu sign masks of the forward: slot b: relu(x_b), nb + b: relu(h_b), 2 nb: x_f; every
    // region has PS rows (view rows v P + p before combine_layer)
    const uint32_t *msk = reinterpret_cast<const uint32_t *>(a.save + save_mask_offset(nb, PS));
    auto mask_slot = [&](int i, int64_t row0) { return msk + PS * 16 * i + row0 * 16; };
    u2m mk[CT];
    auto dy_slot = [&](int i, int64_t row0) { return a.dy + PS * H * i + row0 * H; };
    auto bs_slot = [&](int i) -> float * {
        return a.bsum ? a.bsum + ((int64_t)blockIdx.x * (2 * nb + 1) + i) * H : nullptr;
    };
    auto publish = [&](const Acc &acc) {
        // no barrier first: the column maxima are written before the internal barrier and the
        // image after it, when every wave has left the GEMM that read the previous image
        relu_colmax<false>(acc, cmax, wave, lane);
        __syncthreads();
        relu_store_split<false>(acc, P0, P1, cmax, ecol, wave, lane, gc.ecl);
        __syncthreads();
    };

    Acc x, h;
    // segments of the chain: NS == 1: blocks nb-1 .. 0; else blocks nb-1 .. nc per point, then
    // nc-1 .. 0 once per view on its rows v P + p
    const int n_seg = a.ns == 1 ? 1 : 1 + a.ns;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        {   // dx = (d_o W_out) . [x_f > 0]
            load_mask(mk, mask_slot(2 * nb, 0), tile, P, wave, lane);
            f4 wo[4][RTW];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < RTW; ++r) wo[j][r] = *frag_at(a.w_out, j, wave, r, g);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int64_t p = tile * COLS + 16 * c + cl;
                const f4 d = p < P ? *reinterpret_cast<const f4 *>(a.d_o + p * 4) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < RTW; ++r)
                    x[r][c] = ((d.x * wo[0][r] + d.y * wo[1][r]) + d.z * wo[2][r]) + d.w * wo[3][r];
            }
            relu_mask(x, mk, tile, P, lane);
        }
        for (int sgi = 0; sgi < n_seg; ++sgi) {
            const int v = sgi - 1;   // the view of a per-view segment
            const int b_hi = sgi == 0 ? nb : nc, b_lo = sgi == 0 ? nc : 0;
            const int64_t row0 = v > 0 ? (int64_t)v * P : 0;
            // the first store of the workgroup to the bias partials of these slots
            const bool first = tile == blockIdx.x && v <= 0;
            if (v == 0)   // torch.mean's backward: dL/d(mean) / NS to every view
                acc_div(x, (float)a.ns);
            else if (v > 0 && nc > 0)   // the same, as view 0 stored it (this lane's own rows)
                load_rows(x, dy_slot(nb + nc, 0), tile, P, wave, lane);
            // one step of the chain: h = W_li^T . image, then . [saved activation of mask slot mi > 0]
            // if masked (the mask words are loaded before the GEMM and land during it)
            auto chain_step = [&](int li, bool masked, int mi = 0) {
                acc_zero(h);
                if (masked) load_mask(mk, mask_slot(mi, row0), tile, P, wave, lane);
                layer_gemm<3, NKB, H_DIST, true>(h, a.packed_t + (int64_t)li * L.layer_floats, gc, 1 + li);
                if (masked) relu_mask(h, mk, tile, P, lane);
            };
            bool published = false;
            for (int b = b_hi - 1; b >= b_lo; --b) {
                if (!published) publish(x);
                store_rows(x, dy_slot(nb + 1 + b, row0), tile, P, wave, lane, bs_slot(nb + 1 + b), first);
                const int l1 = layer_index(b, 2, L.n_linz), l0 = layer_index(b, 1, L.n_linz);
                chain_step(l1, true, nb + b);   // fc_1
                store_rows(h, dy_slot(b, row0), tile, P, wave, lane, bs_slot(b), first);
                publish(h);
                chain_step(l0, true, b);   // fc_0
                acc_add(x, h);
                published = false;
                if (b < L.n_linz) {
                    publish(x);
                    published = true;
                    chain_step(layer_index(b, 0, L.n_linz), false);   // lin_z
                    add_rows(h, a.dzlat, row0, tile, P, wave, lane, b == L.n_linz - 1);
                }
            }
            // dY(lin_in) belongs to the segment that ends the chain: with NS > 1 a view's, never the
            // per-point one (combine_layer = 0 gives that one b_lo = 0 too, but its x is the undivided
            // dL/d(mean): it must reach neither dy[nb] nor lin_in's bias partial)
            if (b_lo == 0 && (sgi > 0 || a.ns == 1))
                store_rows(x, dy_slot(nb, row0), tile, P, wave, lane, bs_slot(nb), first);
        }
    }
}

// d_bias[i] = sum over the workgroups of their column-sum partials.  One workgroup per 64
// columns (coalesced 256-B rows), BIAS_SLICES waves each summing a strided slice of the
// workgroup partials, then the slices added in slice order through LDS: a fixed order, so
// the result is deterministic.  The one-thread-per-column loop it replaces was a chain of
// n_wg dependent loads on 22 workgroups (≈0.1 ms per launch, 58 GB/s).
constexpr int BIAS_SLICES = 16;
__global__ void __launch_bounds__(64 * BIAS_SLICES)
k_bias_reduce(const float *__restrict__ part, int n_wg, int n, float *__restrict__ out) {
    __shared__ float acc[BIAS_SLICES][64];
    const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + c;
    float s0 = 0.f, s1 = 0.f;
    if (t < n) {
        int w = sl;
        for (; w + BIAS_SLICES < n_wg; w += 2 * BIAS_SLICES) {
            s0 += part[(int64_t)w * n + t];
            s1 += part[(int64_t)(w + BIAS_SLICES) * n + t];
        }
        if (w < n_wg) s0 += part[(int64_t)w * n + t];
    }
    acc[sl][c] = s0 + s1;
    __syncthreads();
    if (sl == 0 && t < n) {
        float s = acc[0][c];
#pragma unroll
        for (int k = 1; k < BIAS_SLICES; ++k) s += acc[k][c];
        out[t] = s;
    }
}

}  // namespace mlpk

static int64_t mlp_bwd_grid(int64_t n_points) {
    const int64_t tiles = (n_points + mlpk::COLS - 1) / mlpk::COLS;
    const int cus = device_cu_count();
    return tiles < cus ? tiles : cus;
}

size_t mlp_bwd_workspace_bytes(const pnr_mlp_desc &d, int64_t n_points) {
    if (n_points <= 0) return 0;
    return sizeof(float) * (size_t)mlp_bwd_grid(n_points) * (2 * d.n_blocks + 1) * mlpk::H;
}

int launch_mlp_bwd(const pnr_mlp_desc &d, const MlpBwdCall &c, hipStream_t st) {
    int rc = mlp_check_desc(d);
    if (rc) return rc;
    if (d.precision != PNR_PREC_F16X3)
        return fail(PNR_ERR_UNSUPPORTED, "the fused MLP backward implements precision 3 (f16x3); got %d", d.precision);
    mlpk::BwdArgs a = {};
    a.L = mlpk::make_layout(d);
    if (a.L.n_linz > 0 && !c.dzlat) return fail(PNR_ERR_INVALID, "mlp backward: d_zlat is required (n_linz > 0)");
    if (c.n_points == 0) return PNR_OK;
    const size_t need = mlp_bwd_workspace_bytes(d, c.n_points);
    if (c.d_bias && (!c.ws || c.ws_bytes < need))
        return fail(PNR_ERR_WORKSPACE, "mlp backward: workspace %zu < %zu", c.ws_bytes, need);
    a.hdr = static_cast<const float *>(c.packed);
    a.packed_t = static_cast<const float *>(c.packed_t);
    a.w_out = c.w_out;
    a.save = c.save;
    a.d_o = c.d_o;
    a.dy = c.dy;
    a.dzlat = c.dzlat;
    a.bsum = c.d_bias ? static_cast<float *>(c.ws) : nullptr;
    a.n_points = c.n_points;
    a.n_tiles = (c.n_points + mlpk::COLS - 1) / mlpk::COLS;
    a.ns = c.n_views;
    const int64_t grid = mlp_bwd_grid(c.n_points);
    const size_t lds = mlpk::lds_bytes(mlpk::bwd_lds());
    hipLaunchKernelGGL(mlpk::k_mlp_bwd, dim3((unsigned)grid), dim3(mlpk::NTHR), lds, st, a);
    if (!launch_ok("mlp_bwd")) return PNR_ERR_HIP;
    if (c.d_bias) {
        const int n = (2 * d.n_blocks + 1) * mlpk::H;
        hipLaunchKernelGGL(mlpk::k_bias_reduce, dim3((unsigned)((n + 63) / 64)), dim3(64 * mlpk::BIAS_SLICES), 0,
                           st, a.bsum, (int)grid, n, c.d_bias);
        if (!launch_ok("bias_reduce")) return PNR_ERR_HIP;
    }
    return PNR_OK;
}

}  // namespace pnr
