// Per-image MSE and mean SSIM of two image stacks on the device: the scoring step of
// eval/calc_metrics.py:188-191 and eval/eval_approx.py (skimage compare_ssim(multichannel=True) /
// compare_psnr) on images that are already in HBM.  Semantics: include/pnr_abi.h, "Image metrics";
// pnr/evaluate.py ssim / psnr_np restate them in numpy and are the yardstick of the tests.
//
// Everything after the fp32 loads is fp64: vx = cov_norm (uxx - ux^2) cancels against
// C2 = 9e-4, and fp32 window moments would leave ~1e-4 relative error in flat regions.
//
// Two launches, no atomics, nothing allocated:
//   k_metrics_tile    one workgroup per (image, channel, kTile x kTile tile of the SSIM map): the
//                     tile plus its 6-pixel halo of x and y in LDS, the five 7-tap window sums
//                     separably (rows, then columns), one (SSIM sum, squared-error sum) partial
//                     per workgroup.  Every pixel's squared error is owned by exactly one tile.
//   k_metrics_finish  one wave per image: the partials of each channel in ascending index order
//                     (each lane a contiguous run, the lanes then added in lane order)
// A partial depends only on its own image's data and the sums run in a fixed order, so a row of
// `out` is bit-identical from run to run and whether the image is scored alone or in a batch.
#include <cstdio>
#include <cstdlib>

#include "pnr_common.h"
#include "pnr_launch.h"

namespace pnr {
namespace imk {

constexpr int kTile = PNR_IMAGE_METRICS_TILE, kWin = 7, kHalo = kWin - 1, kStage = kTile + kHalo;
constexpr int kThreads = kTile * kTile, kWaves = kThreads / kWave;
constexpr int kMaxDim = 8192;
constexpr int64_t kMaxBlocks = (1ll << 24) - 1;   // grid size x block size below 2^32
static_assert(kThreads % kWave == 0 && kThreads <= 1024, "one thread per SSIM value of the tile");

struct Shape {
    int64_t n;
    int h, w, c;
    int ty, tx;   // tiles of the (h - 6) x (w - 6) SSIM map
};

// all five moments and the SSIM expression rounded once per operation, in the order
// evaluate.ssim writes them
#pragma clang fp contract(off)
__device__ __forceinline__ double ssim_value(const double s[5], double c1, double c2) {
    constexpr double inv_n = 1.0 / (kWin * kWin), cov_norm = (double)(kWin * kWin) / (kWin * kWin - 1);
    const double ux = s[0] * inv_n, uy = s[1] * inv_n, uxx = s[2] * inv_n, uyy = s[3] * inv_n, uxy = s[4] * inv_n;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
}

__global__ __launch_bounds__(kThreads) void k_metrics_tile(const float *__restrict__ x, const float *__restrict__ y,
                                                           Shape sh, double c1, double c2,
                                                           double *__restrict__ partial) {
    __shared__ float s_x[kStage][kStage + 1], s_y[kStage][kStage + 1];
    __shared__ double s_row[5][kStage][kTile + 1];
    __shared__ double s_red[2][kWaves];
    const int tid = threadIdx.x;
    // blockIdx.x = ((image * c + channel) * ty + tile row) * tx + tile column
    uint32_t b = blockIdx.x;
    const int tc = (int)(b % (uint32_t)sh.tx);
    b /= (uint32_t)sh.tx;
    const int tr = (int)(b % (uint32_t)sh.ty);
    b /= (uint32_t)sh.ty;
    const int ch = (int)(b % (uint32_t)sh.c);
    const int64_t img = (int64_t)(b / (uint32_t)sh.c);
    const int r0 = tr * kTile, c0 = tc * kTile;
    // the image rows / columns whose squared error this tile owns: its own SSIM rows shifted to
    // the window centre, widened to the image border on the first and last tile
    const int own_r0 = tr == 0 ? 0 : r0 + kHalo / 2, own_r1 = tr == sh.ty - 1 ? sh.h : r0 + kTile + kHalo / 2;
    const int own_c0 = tc == 0 ? 0 : c0 + kHalo / 2, own_c1 = tc == sh.tx - 1 ? sh.w : c0 + kTile + kHalo / 2;
    const int64_t base = img * sh.h * sh.w * sh.c + ch;

    double se = 0.0;
    for (int i = tid; i < kStage * kStage; i += kThreads) {
        const int sr = i / kStage, sc = i - sr * kStage;
        const int r = r0 + sr, c = c0 + sc;
        float a = 0.f, bb = 0.f;
        if (r < sh.h && c < sh.w) {
            const int64_t o = base + ((int64_t)r * sh.w + c) * sh.c;
            a = x[o];
            bb = y[o];
            if (r >= own_r0 && r < own_r1 && c >= own_c0 && c < own_c1) {
                const double d = (double)a - (double)bb;
                se += d * d;
            }
        }
        s_x[sr][sc] = a;
        s_y[sr][sc] = bb;
    }
    __syncthreads();
    // rows: the 7-tap sums of x, y, x^2, y^2, xy for every staged row and every tile column
    for (int i = tid; i < kStage * kTile; i += kThreads) {
        const int sr = i / kTile, oc = i - sr * kTile;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const double a = (double)s_x[sr][oc + k], bb = (double)s_y[sr][oc + k];
            m[0] += a;
            m[1] += bb;
            m[2] += a * a;
            m[3] += bb * bb;
            m[4] += a * bb;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) s_row[q][sr][oc] = m[q];
    }
    __syncthreads();
    // columns: one SSIM value per thread
    const int orow = tid / kTile, oc = tid - orow * kTile;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kWin; ++k)
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += s_row[q][orow + k][oc];
    const bool live = r0 + orow < sh.h - kHalo && c0 + oc < sh.w - kHalo;
    double ss = live ? ssim_value(m, c1, c2) : 0.0;   // a dead slot saw zero padding only

    ss = wave_sum(ss);
    se = wave_sum(se);
    if ((tid & (kWave - 1)) == 0) {
        s_red[0][tid / kWave] = ss;
        s_red[1][tid / kWave] = se;
    }
    __syncthreads();
    if (tid == 0) {
        double a = s_red[0][0], bb = s_red[1][0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) {
            a += s_red[0][wv];
            bb += s_red[1][wv];
        }
        partial[2 * (size_t)blockIdx.x] = a;
        partial[2 * (size_t)blockIdx.x + 1] = bb;
    }
}

// sum over the 64 lanes in lane order, the same in every lane
__device__ __forceinline__ double lanes_in_order(double v) {
    double t = 0.0;
    for (int l = 0; l < kWave; ++l) t += __shfl(v, l, kWave);
    return t;
}

// out[image] = {mse, ssim}: per channel the tile partials in ascending order, then the channels
__global__ __launch_bounds__(256) void k_metrics_finish(const double *__restrict__ partial, Shape sh,
                                                        double *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t img = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x / kWave);
    if (img >= sh.n) return;   // the whole wave
    const int tiles = sh.ty * sh.tx, run = (tiles + kWave - 1) / kWave;
    const int t0 = min(lane * run, tiles), t1 = min(t0 + run, tiles);
    double ssim = 0.0, se = 0.0;
    for (int ch = 0; ch < sh.c; ++ch) {
        const double *p = partial + 2 * ((size_t)img * sh.c + ch) * (size_t)tiles;
        double a = 0.0, bb = 0.0;
        for (int t = t0; t < t1; ++t) {
            a += p[2 * (size_t)t];
            bb += p[2 * (size_t)t + 1];
        }
        a = lanes_in_order(a);
        bb = lanes_in_order(bb);
        ssim += a / ((double)(sh.h - kHalo) * (double)(sh.w - kHalo));
        se += bb;
    }
    if (lane == 0) {
        out[2 * (size_t)img] = se / ((double)sh.h * (double)sh.w * (double)sh.c);
        out[2 * (size_t)img + 1] = ssim / (double)sh.c;
    }
}

static int plan(int64_t n, int h, int w, int c, Shape &sh, size_t &bytes) {
    if (n < 1) return fail(PNR_ERR_INVALID, "image metrics: n must be >= 1 (got %lld)", (long long)n);
    if (c < 1 || c > 4) return fail(PNR_ERR_INVALID, "image metrics: c must be 1 .. 4 (got %d)", c);
    if (h < kWin || w < kWin)
        return fail(PNR_ERR_INVALID, "image metrics: images of %d x %d are smaller than the %d x %d window", h, w,
                    kWin, kWin);
    if (h > kMaxDim || w > kMaxDim)
        return fail(PNR_ERR_UNSUPPORTED, "image metrics: image height / width above %d (got %d x %d)", kMaxDim, h, w);
    sh = Shape{n, h, w, c, (h - kHalo + kTile - 1) / kTile, (w - kHalo + kTile - 1) / kTile};
    const int64_t per_image = (int64_t)c * sh.ty * sh.tx;
    if (n > kMaxBlocks / per_image)
        return fail(PNR_ERR_UNSUPPORTED, "image metrics: %lld images of %d x %d x %d need more than %lld workgroups",
                    (long long)n, h, w, c, (long long)kMaxBlocks);
    bytes = align256((size_t)(n * per_image) * 2 * sizeof(double));
    return PNR_OK;
}

// k1, k2 and data_range cross the ABI as floats but enter C1 and C2 in fp64, where
// (double)0.03f is 2e-8 away from 0.03: each is read as the shortest decimal that rounds to the
// float, the value its caller wrote
static double as_written(float v) {
    char buf[32];
    for (int prec = 1; prec <= 9; ++prec) {
        snprintf(buf, sizeof(buf), "%.*g", prec, (double)v);
        if (strtof(buf, nullptr) == v) return strtod(buf, nullptr);
    }
    return (double)v;
}

}  // namespace imk

size_t image_metrics_workspace_bytes(int64_t n, int h, int w, int c) {
    imk::Shape sh;
    size_t bytes = 0;
    return imk::plan(n, h, w, c, sh, bytes) == PNR_OK ? bytes : 0;
}

int launch_image_metrics(const float *x, const float *y, int64_t n, int h, int w, int c, float data_range, float k1,
                         float k2, void *ws, size_t ws_bytes, double *out, hipStream_t st) {
    imk::Shape sh;
    size_t bytes = 0;
    int rc = imk::plan(n, h, w, c, sh, bytes);
    if (rc) return rc;
    if (!ws || ws_bytes < bytes)
        return fail(PNR_ERR_WORKSPACE, "pnr_image_metrics: workspace %zu bytes, needs %zu", ws_bytes, bytes);
    const double r = imk::as_written(data_range), c1 = imk::as_written(k1) * r, c2 = imk::as_written(k2) * r;
    double *partial = static_cast<double *>(ws);
    const unsigned blocks = (unsigned)(n * c * sh.ty * sh.tx);
    hipLaunchKernelGGL(imk::k_metrics_tile, dim3(blocks), dim3(imk::kThreads), 0, st, x, y, sh, c1 * c1, c2 * c2,
                       partial);
    if (!launch_ok("metrics_tile")) return PNR_ERR_HIP;
    hipLaunchKernelGGL(imk::k_metrics_finish, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, partial, sh, out);
    return launch_ok("metrics_finish") ? PNR_OK : PNR_ERR_HIP;
}

}  // namespace pnr
