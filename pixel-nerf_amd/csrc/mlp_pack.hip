// Weight packing of the fused MLP: the fragment-order packs that k_point_mlp (mlp.hip) and
// k_mlp_bwd (mlp_bwd.hip) stream, their per-layer scale exponents, and the descriptor checks.
// The pack's layout is mlp_layout.h's.
#include "mlp_layout.h"
#include "pnr_launch.h"

namespace pnr {
namespace mlpk {

struct PackSrc {
    const float *lin_in_w, *lin_in_b, *lin_out_w, *lin_out_b, *pe_f, *pe_p;
    const float *w[24], *b[24];
};

// One thread per packed float.  Fragment element (kb, rt, lane, s) holds
// W[16 rt + (lane & 15)][16 kb + 4 (lane >> 4) + s]: the A operand of k-step
// (kb, s) for row tile rt (v_mfma_f32_16x16x4_f32: lane l holds A[l&15][l>>4]).
__global__ void k_pack(PackSrc s, Layout L, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.total) return;
    float v = 0.0f;
    if (i < HDR) {
        if (i >= HDR_ESCALE && i < HDR_ESCALE + 1 + L.n_l512 && is_h(L.prec)) return;   // k_layer_escale's
        if (i < 16 && i < L.pe_n) v = s.pe_f[i];
        else if (i >= 16 && i < 32 && (i - 16) < L.pe_n) v = s.pe_p[i - 16];
    } else if (i < L.off_lin_out && L.prec) {
        return;   // written by k_pack_split / k_pack_f16
    } else if (i < L.off_l512) {
        const int e = (int)(i - L.off_lin_in);
        const int kb = e / KB_FLOATS, rt = (e / 256) % NRT, lane = (e >> 2) & 63, j = e & 3;
        const int row = 16 * rt + (lane & 15), col = 16 * kb + 4 * (lane >> 4) + j;
        if (col < L.d_in) v = s.lin_in_w[(int64_t)row * L.d_in + col];
    } else if (i < L.off_lin_out) {
        const int64_t r = i - L.off_l512;
        const int layer = (int)(r / LAYER_FLOATS);
        const int e = (int)(r % LAYER_FLOATS);
        const int kb = e / KB_FLOATS, rt = (e / 256) % NRT, lane = (e >> 2) & 63, j = e & 3;
        const int row = 16 * rt + (lane & 15), col = 16 * kb + 4 * (lane >> 4) + j;
        v = s.w[layer][(int64_t)row * H + col];
    } else if (i < L.off_bias) {
        const int e = (int)(i - L.off_lin_out);
        const int kb = e >> 8, lane = (e >> 2) & 63, j = e & 3;
        const int row = lane & 15, col = 16 * kb + 4 * (lane >> 4) + j;
        if (row < L.d_out) v = s.lin_out_w[(int64_t)row * H + col];
    } else if (i >= L.off_out32) {
        const int e = (int)(i - L.off_out32);   // [input channel][output]
        const int ch = e >> 2, j = e & 3;
        if (j < L.d_out) v = s.lin_out_w[(int64_t)j * H + ch];
    } else {
        const int64_t r = i - L.off_bias;
        const int64_t nb = (int64_t)(1 + L.n_l512) * H;
        if (r < H) v = s.lin_in_b[r];
        else if (r < nb) v = s.b[r / H - 1][r % H];
        else if (r - nb < L.d_out) v = s.lin_out_b[r - nb];
    }
    out[i] = v;
}

// Split packer: one thread per (layer, k-step, row tile, lane) -> 8 weights
// W[16 rt + (lane & 15)][32 ks + 8 (lane >> 4) + j], each split exactly into three
// bf16 parts w = w0 + w1 + w2 (RNE), stored part-major: [ks][rt][part][lane][8].
__device__ __forceinline__ unsigned short bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf16_to_f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

__global__ void k_pack_split(PackSrc s, Layout L, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_in = (int64_t)KS32_IN * NRT * 64;
    const int64_t n_l = (int64_t)KS32 * NRT * 64;
    if (t >= n_in + L.n_l512 * n_l) return;
    int layer, ks, rt, lane;
    float *dst;
    if (t < n_in) {
        layer = -1;
        ks = (int)(t / (NRT * 64)); rt = (int)((t / 64) % NRT); lane = (int)(t % 64);
        dst = out + L.off_lin_in + (int64_t)ks * SKS_FLOATS + rt * SRT_FLOATS + lane * 4;
    } else {
        const int64_t r = t - n_in;
        layer = (int)(r / n_l);
        const int64_t e = r % n_l;
        ks = (int)(e / (NRT * 64)); rt = (int)((e / 64) % NRT); lane = (int)(e % 64);
        dst = out + L.off_l512 + layer * L.layer_floats + (int64_t)ks * SKS_FLOATS + rt * SRT_FLOATS + lane * 4;
    }
    const int row = 16 * rt + (lane & 15);
    unsigned short p[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = 32 * ks + 8 * (lane >> 4) + j;
        float w = 0.f;
        if (layer < 0) { if (col < L.d_in) w = s.lin_in_w[(int64_t)row * L.d_in + col]; }
        else w = s.w[layer][(int64_t)row * H + col];
        const unsigned short h0 = bf16_rne(w);
        const float r1 = w - bf16_to_f(h0);
        const unsigned short h1 = bf16_rne(r1);
        const float r2 = r1 - bf16_to_f(h1);
        p[0][j] = h0; p[1][j] = h1; p[2][j] = bf16_rne(r2);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint4 v;
        v.x = p[q][0] | ((unsigned)p[q][1] << 16); v.y = p[q][2] | ((unsigned)p[q][3] << 16);
        v.z = p[q][4] | ((unsigned)p[q][5] << 16); v.w = p[q][6] | ((unsigned)p[q][7] << 16);
        *reinterpret_cast<uint4 *>(dst + q * 256) = v;
    }
}

// Scaled-fp16 mode: per packed layer, the power-of-two exponent eW with
// max|W| * 2^eW <= 2^14 (fp16 max 65504), clamped to [-64, 40].  One block per layer
// (block 0 = lin_in, 1 + j = packed 512-wide layer j, 1 + n_l512 = lin_out), written
// to the pack header slot HDR_ESCALE + block as a float.
// pass 1: max |w| per layer (blockIdx.y = layer block as above), grid-strided over
// blockIdx.x, combined with an integer atomicMax on the float bits (|w| >= 0) in the
// header slot (zeroed by the host first)
__global__ void k_layer_absmax(PackSrc s, Layout L, float *__restrict__ out) {
    const int layer = (int)blockIdx.y - 1;
    const float *w = layer < 0 ? s.lin_in_w : s.w[layer];
    const int64_t n = layer < 0 ? (int64_t)H * L.d_in : (int64_t)H * H;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(w[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned *>(out + HDR_ESCALE + blockIdx.y), __float_as_uint(m));
}
// pass 2: max -> scale exponent (as a float) in place
__global__ void k_layer_escale(int n_slots, float *__restrict__ out) {
    const int i = threadIdx.x;
    if (i < n_slots) out[HDR_ESCALE + i] = (float)scale_exp(out[HDR_ESCALE + i]);
}

// One thread per (layer, k-step, row tile, lane): 8 weights w * 2^eW, each split
// into two fp16 parts w0 = f16(w), w1 = f16(w - w0) (RNE), [ks][rt][part][lane][8].
// (lin_out is not split: the head reads it in fp32 from off_out32.)
// PREC 1: the 512-wide layers hold w0 only, [ks][rt][lane][8] (half the bytes: the stream's L2
// footprint is the point of the mode); lin_in keeps both parts.
__global__ void k_pack_f16(PackSrc s, Layout L, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_in = (int64_t)KS32_IN * NRT * 64;
    const int64_t n_l = (int64_t)KS32 * NRT * 64;
    const int64_t n_all = n_in + L.n_l512 * n_l;
    if (t >= n_all) return;
    int layer, ks, rt, lane;
    float *dst;
    if (t < n_in) {
        layer = -1;
        ks = (int)(t / (NRT * 64)); rt = (int)((t / 64) % NRT); lane = (int)(t % 64);
        dst = out + L.off_lin_in + (int64_t)ks * SKS16_FLOATS + rt * SRT16_FLOATS + lane * 4;
    } else {
        const int64_t r = t - n_in;
        layer = (int)(r / n_l);
        const int64_t e = r % n_l;
        ks = (int)(e / (NRT * 64)); rt = (int)((e / 64) % NRT); lane = (int)(e % 64);
        dst = out + L.off_l512 + layer * L.layer_floats + (int64_t)ks * sks_floats(L.prec) +
              rt * srt_h_floats(nparts(L.prec)) + lane * 4;
    }
    const int np = layer < 0 ? 2 : nparts(L.prec);
    const int ew = (int)out[HDR_ESCALE + 1 + layer];
    const int row = 16 * rt + (lane & 15);
    _Float16 p[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = 32 * ks + 8 * (lane >> 4) + j;
        float w = 0.f;
        if (layer < 0) { if (col < L.d_in) w = s.lin_in_w[(int64_t)row * L.d_in + col]; }
        else w = s.w[layer][(int64_t)row * H + col];
        const float ws = __builtin_ldexpf(w, ew);
        const _Float16 h0 = (_Float16)ws;
        p[0][j] = h0;
        p[1][j] = (_Float16)(ws - (float)h0);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q >= np) break;
        typedef _Float16 h8t __attribute__((ext_vector_type(8)));
        h8t v = {p[q][0], p[q][1], p[q][2], p[q][3], p[q][4], p[q][5], p[q][6], p[q][7]};
        *reinterpret_cast<h8t *>(dst + q * 256) = v;
    }
}

// Backward (training) pack: W^T of every packed 512-wide layer in the k_pack_f16 fragment
// layout, so that IN-gradient = W^T OUT-gradient runs on the forward's GEMM.  One thread
// per (layer, k-step, row tile, lane): A[16 rt + (lane & 15)][32 ks + 8 (lane >> 4) + j] =
// W[32 ks + 8 (lane >> 4) + j][16 rt + (lane & 15)] * 2^eW, eW from the forward pack's
// header (max |W^T| = max |W|).  Output: n_l512 layers of layer_floats, no header.
__global__ void k_pack_f16_t(PackSrc s, Layout L, const float *__restrict__ hdr, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_l = (int64_t)KS32 * NRT * 64;
    if (t >= L.n_l512 * n_l) return;
    const int layer = (int)(t / n_l);
    const int64_t e = t % n_l;
    const int ks = (int)(e / (NRT * 64)), rt = (int)((e / 64) % NRT), lane = (int)(e % 64);
    float *dst = out + layer * L.layer_floats + (int64_t)ks * SKS16_FLOATS + rt * SRT16_FLOATS + lane * 4;
    const int ew = (int)hdr[HDR_ESCALE + 1 + layer];
    const int col = 16 * rt + (lane & 15);
    typedef _Float16 h8t __attribute__((ext_vector_type(8)));
    h8t p0, p1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = 32 * ks + 8 * (lane >> 4) + j;
        const float ws = __builtin_ldexpf(s.w[layer][(int64_t)row * H + col], ew);
        const _Float16 h0 = (_Float16)ws;
        p0[j] = h0;
        p1[j] = (_Float16)(ws - (float)h0);
    }
    *reinterpret_cast<h8t *>(dst) = p0;
    *reinterpret_cast<h8t *>(dst + 256) = p1;
}

}  // namespace mlpk

size_t mlp_packed_bytes(const pnr_mlp_desc &d) {
    return sizeof(float) * (size_t)mlpk::make_layout(d).total;
}

int mlp_check_desc(const pnr_mlp_desc &d) {
    if (d.d_hidden != mlpk::H || d.d_latent != mlpk::H)
        return fail(PNR_ERR_UNSUPPORTED, "fused MLP implements d_hidden = d_latent = 512 (got %d, %d)",
                    d.d_hidden, d.d_latent);
    if (d.d_out != 4) return fail(PNR_ERR_UNSUPPORTED, "d_out must be 4 (got %d)", d.d_out);
    if (d.n_blocks < 1 || d.n_blocks > 8) return fail(PNR_ERR_UNSUPPORTED, "n_blocks in [1, 8] (got %d)", d.n_blocks);
    if (d.combine_layer < 0) return fail(PNR_ERR_INVALID, "combine_layer < 0");
    if (d.pe_n < 0 || d.pe_n > 16) return fail(PNR_ERR_UNSUPPORTED, "pe_n in [0, 16] (got %d)", d.pe_n);
    if (d.d_in != 3 + 3 * d.pe_n + 3)
        return fail(PNR_ERR_UNSUPPORTED, "d_in must be 3 + 3*pe_n + 3 (xyz PE + raw viewdirs); got %d", d.d_in);
    if (d.d_in > 16 * mlpk::NKB_IN) return fail(PNR_ERR_UNSUPPORTED, "d_in <= 64");
    if (d.precision != PNR_PREC_F32 && d.precision != PNR_PREC_F16 && d.precision != PNR_PREC_F16X3 &&
        d.precision != PNR_PREC_BF16X6 && d.precision != PNR_PREC_BF16X9)
        return fail(PNR_ERR_UNSUPPORTED, "precision must be 0 (f32), 1 (f16, one product), 3 (f16x3) or 6 / 9 "
                    "(split bf16); got %d", d.precision);
    return PNR_OK;
}

static int pack_src(const pnr_mlp_weights &w, const mlpk::Layout &L, mlpk::PackSrc &s) {
    const pnr_mlp_desc &d = w.desc;
    s = {};
    s.lin_in_w = w.lin_in_w; s.lin_in_b = w.lin_in_b;
    s.lin_out_w = w.lin_out_w; s.lin_out_b = w.lin_out_b;
    s.pe_f = w.pe_freqs; s.pe_p = w.pe_phases;
    if (!s.lin_in_w || !s.lin_in_b || !s.lin_out_w || !s.lin_out_b || (d.pe_n && (!s.pe_f || !s.pe_p)))
        return fail(PNR_ERR_INVALID, "null weight pointer");
    for (int blk = 0; blk < d.n_blocks; ++blk) {
        for (int kind = 0; kind < 3; ++kind) {
            if (kind == 0 && blk >= L.n_linz) continue;
            const int li = mlpk::layer_index(blk, kind, L.n_linz);
            const float *wp = kind == 0 ? w.lin_z_w[blk] : kind == 1 ? w.fc0_w[blk] : w.fc1_w[blk];
            const float *bp = kind == 0 ? w.lin_z_b[blk] : kind == 1 ? w.fc0_b[blk] : w.fc1_b[blk];
            if (!wp || !bp) return fail(PNR_ERR_INVALID, "null weight pointer (block %d kind %d)", blk, kind);
            s.w[li] = wp;
            s.b[li] = bp;
        }
    }
    return PNR_OK;
}

int mlp_pack(const pnr_mlp_weights &w, void *packed, size_t bytes, hipStream_t st) {
    const pnr_mlp_desc &d = w.desc;
    int rc = mlp_check_desc(d);
    if (rc) return rc;
    mlpk::Layout L = mlpk::make_layout(d);
    if (bytes < sizeof(float) * (size_t)L.total) return fail(PNR_ERR_WORKSPACE, "packed buffer too small");
    mlpk::PackSrc s;
    if ((rc = pack_src(w, L, s))) return rc;
    const int64_t blocks = (L.total + 255) / 256;
    hipLaunchKernelGGL(mlpk::k_pack, dim3((unsigned)blocks), dim3(256), 0, st, s, L,
                       static_cast<float *>(packed));
    if (!launch_ok("mlp_pack")) return PNR_ERR_HIP;
    const int64_t n = (int64_t)(mlpk::KS32_IN + L.n_l512 * mlpk::KS32) * mlpk::NRT * 64;
    if (mlpk::is_h(L.prec)) {
        float *hdr = static_cast<float *>(packed);
        if (hipMemsetAsync(hdr + mlpk::HDR_ESCALE, 0, sizeof(float) * (1 + L.n_l512), st) != hipSuccess)
            return fail(PNR_ERR_HIP, "mlp_pack: hipMemsetAsync failed");
        hipLaunchKernelGGL(mlpk::k_layer_absmax, dim3(32, (unsigned)(1 + L.n_l512)), dim3(256), 0, st, s, L, hdr);
        if (!launch_ok("mlp_layer_absmax")) return PNR_ERR_HIP;
        hipLaunchKernelGGL(mlpk::k_layer_escale, dim3(1), dim3(64), 0, st, 1 + L.n_l512, hdr);
        if (!launch_ok("mlp_layer_escale")) return PNR_ERR_HIP;
        hipLaunchKernelGGL(mlpk::k_pack_f16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           s, L, static_cast<float *>(packed));
        if (!launch_ok("mlp_pack_f16")) return PNR_ERR_HIP;
    } else if (L.prec) {
        hipLaunchKernelGGL(mlpk::k_pack_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           s, L, static_cast<float *>(packed));
        if (!launch_ok("mlp_pack_split")) return PNR_ERR_HIP;
    }
    return PNR_OK;
}

// ---- training backward (PREC 3) ----------------------------------------------------------
size_t mlp_packed_t_bytes(const pnr_mlp_desc &d) {
    if (mlp_check_desc(d) || d.precision != PNR_PREC_F16X3) return 0;
    const mlpk::Layout L = mlpk::make_layout(d);
    return sizeof(float) * (size_t)(L.n_l512 * L.layer_floats);
}

int mlp_pack_t(const pnr_mlp_weights &w, const void *packed, void *packed_t, size_t bytes, hipStream_t st) {
    const pnr_mlp_desc &d = w.desc;
    int rc = mlp_check_desc(d);
    if (rc) return rc;
    if (d.precision != PNR_PREC_F16X3)
        return fail(PNR_ERR_UNSUPPORTED, "the fused MLP backward implements precision 3 (f16x3); got %d", d.precision);
    const mlpk::Layout L = mlpk::make_layout(d);
    if (bytes < mlp_packed_t_bytes(d)) return fail(PNR_ERR_WORKSPACE, "transposed pack buffer too small");
    mlpk::PackSrc s;
    if ((rc = pack_src(w, L, s))) return rc;
    const int64_t n = (int64_t)L.n_l512 * mlpk::KS32 * mlpk::NRT * 64;
    hipLaunchKernelGGL(mlpk::k_pack_f16_t, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, L,
                       static_cast<const float *>(packed), static_cast<float *>(packed_t));
    return launch_ok("mlp_pack_t") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
