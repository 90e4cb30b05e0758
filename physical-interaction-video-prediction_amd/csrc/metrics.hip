// Per-sample evaluation of predicted frames on the device: mean squared error and SSIM (Wang et al. 2004, the Gaussian-window form of tf.image.ssim /
// scikit-image with gaussian_weights=True, use_sample_covariance=False) of N images [N][C][H][W] in ONE launch.
//   A block owns whole images (n = blockIdx.x, += gridDim.x).  Per channel it walks the valid window positions in tiles of MT_TH x MT_TW: the x and y
//   tiles with their win-1 halo go to LDS, a horizontal pass leaves the five row moments (x, y, xx, yy, xy) in LDS as DOUBLES, a vertical pass finishes
//   the window moments, forms the SSIM map value and adds it to the thread's sum.  The next tile's pixels are loaded into registers, all loads in
//   flight at once, before the current tile is computed: one block per CU (N = 256) has nothing else to hide the memory latency behind.
//   Numerics: the variance E[x^2] - mu^2 cancels wherever the image is flat and only C2 = 9e-4 stands under it, so the five moments and the differences
//   are accumulated in fp64 (fp32 moments miss 1e-6 per image by two orders on a bright flat frame); numerator and denominator are rounded to fp32 once
//   and divided there.  The squared error is a pass of its own over the image, in fp64.
//   Order: every sum is a per-thread sum in a fixed order followed by a fixed LDS tree, no atomics: the result of image n depends on that image's data
//   and (C, H, W, win, sigma, data_range) alone -- not on N, the grid, the image's index or the other output being asked for.
#include <math.h>

#include "pivp_kernels.h"

namespace pivp {

constexpr int MT_NT = 512;                        // eight waves, two per SIMD: one wave's LDS and global latency is the other's issue time
constexpr int MT_TW = 32;                         // window positions per tile row: one half-wave per tile row, lanes on consecutive LDS words
constexpr int MT_TH = 28;                         // ... and tile rows: 61.7 KB of static LDS at win = 11; 64 x 64 frames (54 rows of positions) take 28 + 26
constexpr int MT_VB = 2;                          // the vertical pass gives each thread MT_VB rows of one column
constexpr int MT_MAXWIN = 11;

__device__ __forceinline__ double block_sum_f64(double v, double* red) {      // fixed tree over the block's 512 threads; red[] is reusable after the call
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = MT_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double t = red[0];
    return t;
}

template <int WIN>
__global__ __launch_bounds__(MT_NT) void frame_metrics_kernel(const float* pred, const float* truth, int N, int C, int H, int W, float sigma,
                                                              float data_range, float* __restrict__ mse, float* __restrict__ ssim) {
    constexpr int IH = MT_TH + WIN - 1, IW = MT_TW + WIN - 1, IP = IW + 1;      // staged rows / columns, row pitch in floats
    constexpr int SU = (IH * IW + MT_NT - 1) / MT_NT;                           // staged elements per thread
    __shared__ float sx[IH * IP], sy[IH * IP];
    __shared__ double hm[5][IH][MT_TW];
    double* red = &hm[0][0][0];                   // the reductions run outside the tile loop, behind barriers
    static_assert(sizeof(double) * MT_NT <= sizeof(hm), "red[] lives in hm");
    const int tid = threadIdx.x;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const int HW = H * W, CHW = C * HW;
    const int tiles_x = (OW + MT_TW - 1) / MT_TW, tiles_c = tiles_x * ((OH + MT_TH - 1) / MT_TH), ntiles = C * tiles_c;

    // the separable window, normalised to sum 1 in double; sigma <= 0: uniform
    double w[WIN];
    {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            const double d = (double)i - 0.5 * (double)(WIN - 1);
            w[i] = sigma > 0.f ? exp(-(d * d) / (2.0 * (double)sigma * (double)sigma)) : 1.0;
            tot += w[i];
        }
#pragma unroll
        for (int i = 0; i < WIN; ++i) w[i] /= tot;
    }
    const double L = (double)data_range;
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    const bool vec = (CHW & 3) == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth)) & 15) == 0;      // every image then starts on 16 bytes

    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const float* __restrict__ px = pred + (size_t)n * CHW;
        const float* __restrict__ py = truth + (size_t)n * CHW;
        if (mse) {
            // groups of four consecutive pixels, group g to thread g % 512: the order of a thread's sum is the same for the vector and the scalar form
            double acc = 0.0;
            for (int i0 = tid * 4; i0 < CHW; i0 += 4 * MT_NT) {
                float a[4], b[4];
                if (vec) {
                    const f32x4 qa = *reinterpret_cast<const f32x4*>(px + i0), qb = *reinterpret_cast<const f32x4*>(py + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = qa[e]; b[e] = qb[e]; }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = i0 + e < CHW ? px[i0 + e] : 0.f; b[e] = i0 + e < CHW ? py[i0 + e] : 0.f; }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = (double)a[e] - (double)b[e];
                    acc += d * d;
                }
            }
            const double t = block_sum_f64(acc, red);
            if (tid == 0) mse[n] = (float)(t / (double)CHW);
        }
        if (!ssim) continue;
        // tile `it` of the image = (channel, tile row, tile column); its staged elements wait in registers while the tile before it is computed
        float rx[SU], ry[SU];
        auto fetch = [&](int it) {
            const int c = it / tiles_c, rem = it - c * tiles_c, tyi = rem / tiles_x;
            const int ty0 = tyi * MT_TH, tx0 = (rem - tyi * tiles_x) * MT_TW;
            const float* __restrict__ cx = px + (size_t)c * HW;
            const float* __restrict__ cy = py + (size_t)c * HW;
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = tid + u * MT_NT, r = i / IW, q = i - r * IW;
                const int gy = ty0 + r, gx = tx0 + q;
                const bool in = i < IH * IW && gy < H && gx < W;      // outside the image: zero, and only positions that are masked below see it
                rx[u] = in ? cx[gy * W + gx] : 0.f;
                ry[u] = in ? cy[gy * W + gx] : 0.f;
            }
        };
        fetch(0);
        double acc = 0.0;
        for (int it = 0; it < ntiles; ++it) {
            const int rem = it % tiles_c, tyi = rem / tiles_x;
            const int ty0 = tyi * MT_TH, tx0 = (rem - tyi * tiles_x) * MT_TW;
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = tid + u * MT_NT, r = i / IW, q = i - r * IW;
                if (i < IH * IW) { sx[r * IP + q] = rx[u]; sy[r * IP + q] = ry[u]; }
            }
            __syncthreads();
            if (it + 1 < ntiles) fetch(it + 1);
            // horizontal pass: row moments of every staged row that lies in the image
            const int rows = H - ty0 < IH ? H - ty0 : IH;
            for (int i = tid; i < rows * MT_TW; i += MT_NT) {
                const int r = i / MT_TW, q = i - r * MT_TW;
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {
                    const double x = (double)sx[r * IP + q + k], y = (double)sy[r * IP + q + k];
                    const double wx = w[k] * x, wy = w[k] * y;
                    m0 += wx; m1 += wy; m2 += wx * x; m3 += wy * y; m4 += wx * y;
                }
                hm[0][r][q] = m0; hm[1][r][q] = m1; hm[2][r][q] = m2; hm[3][r][q] = m3; hm[4][r][q] = m4;
            }
            __syncthreads();
            // vertical pass: MT_VB rows of one column per thread, each row moment read once for both.  A row past `rows` is stale: it only
            // reaches positions past the last valid one, which are dropped
            const int q = tid % MT_TW, r0 = (tid / MT_TW) * MT_VB;
            if (r0 < MT_TH && ty0 + r0 < OH && tx0 + q < OW) {
                double m[MT_VB][5];
#pragma unroll
                for (int j = 0; j < MT_VB; ++j)
#pragma unroll
                    for (int e = 0; e < 5; ++e) m[j][e] = 0.0;
#pragma unroll
                for (int k = 0; k < WIN + MT_VB - 1; ++k) {
                    double v[5];
#pragma unroll
                    for (int e = 0; e < 5; ++e) v[e] = hm[e][r0 + k][q];
#pragma unroll
                    for (int j = 0; j < MT_VB; ++j)
                        if (k - j >= 0 && k - j < WIN) {
#pragma unroll
                            for (int e = 0; e < 5; ++e) m[j][e] += w[k - j] * v[e];
                        }
                }
#pragma unroll
                for (int j = 0; j < MT_VB; ++j) {
                    if (ty0 + r0 + j < OH) {
                        const double mx = m[j][0], my = m[j][1];
                        const double vx = m[j][2] - mx * mx, vy = m[j][3] - my * my, vxy = m[j][4] - mx * my;
                        const float num = (float)((2.0 * mx * my + C1) * (2.0 * vxy + C2));
                        const float den = (float)((mx * mx + my * my + C1) * (vx + vy + C2));
                        acc += (double)(num / den);
                    }
                }
            }
            // the next tile's LDS stores touch sx / sy only (the horizontal pass that read them lies behind the barrier above), and a barrier
            // separates them from the next horizontal pass's writes to hm
        }
        const double t = block_sum_f64(acc, red);
        if (tid == 0) ssim[n] = (float)(t / ((double)C * (double)OH * (double)OW));
    }
}

int frame_metrics(const float* pred, const float* truth, int N, int C, int H, int W, int win, float sigma, float data_range, float* mse,
                  float* ssim, hipStream_t s) {
    PIVP_CHECK_ARG(pred && truth && (mse || ssim));
    PIVP_CHECK_ARG(N >= 1 && C >= 1 && win >= 3 && win <= MT_MAXWIN && (win & 1) == 1 && H >= win && W >= win);
    PIVP_CHECK_ARG(data_range > 0.f && data_range <= 3.4028234e38f && sigma == sigma && fabsf(sigma) <= 3.4028234e38f);
    PIVP_CHECK_ARG((long long)C * H * W < (1ll << 31));
    const int grid = N < 2 * pivp_cu_count() ? N : 2 * pivp_cu_count();      // at most two blocks share a CU (61.7 KB of LDS each at win = 11)
#define PIVP_FM_LAUNCH(WIN_)                                                                                                                  \
    case WIN_:                                                                                                                                \
        hipLaunchKernelGGL(frame_metrics_kernel<WIN_>, dim3(grid), dim3(MT_NT), 0, s, pred, truth, N, C, H, W, sigma, data_range, mse, ssim); \
        break
    switch (win) {
        PIVP_FM_LAUNCH(3);
        PIVP_FM_LAUNCH(5);
        PIVP_FM_LAUNCH(7);
        PIVP_FM_LAUNCH(9);
        PIVP_FM_LAUNCH(11);
    }
#undef PIVP_FM_LAUNCH
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
