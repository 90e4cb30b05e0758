// Image terms of the training objective on the device (include/pivp_loss.h): extra MSE, L1, the gradient-difference loss and DSSIM = 1 - SSIM of N
// predicted images [N][C][H][W] against their ground truth, and the gradient of the weighted total with respect to the prediction.
//   A block owns whole images (n = blockIdx.x, += gridDim.x) in both kernels, as frame_metrics_kernel (csrc/metrics.hip) does: every per-image sum is a
//   per-thread fp64 sum in a fixed order followed by a fixed LDS tree, no atomics, so image n's numbers depend on that image alone.
//   pointwise_loss_kernel (mse, l1, gdl): one pass, groups of four consecutive pixels per thread.  A pixel GATHERS the up to four edge terms that touch
//     it (its own up / left edge, and the down / right neighbour's edge with the opposite sign) -- no scatter.  A thread adds only the up and left edges of
//     its pixels to the value, so every edge is counted once.  fp64 from the first difference on: the sign branches are those of a float64 restatement.
//   dssim_kernel<WIN>: per channel, tiles of DS_T x DS_T OUTPUT pixels q.  d S_p / d y_q = w_{q-p} (alpha_p + beta_p y_q + gamma_p x_q) over the valid window
//     positions p that see q, so the gradient is three maps (alpha, beta, gamma) over the positions, passed through the transposed separable window.  A
//     tile needs the maps on a win-1 halo above / left of it, and those need pixels on a further win-1 halo around: pixels (T + 2R)^2 -> row moments ->
//     maps (T + R)^2 -> row sums of the maps -> T^2 gradients, R = win - 1.  The position with a tile pixel's own index belongs to the tile (valid
//     positions are a subset of the pixels): its S is added to the value there and nowhere else.
//     Numerics: the three per-pixel terms cancel wherever prediction and truth are close (a trained model), so moments, maps and both transposed passes
//     are fp64 and the gradient is rounded to fp32 once (fp32 maps or an fp32 filter miss 1e-6 of the image's largest element by one to two orders on
//     flat frames).  The geometry differs from frame_metrics_kernel's (halo on both sides, maps kept), so the moment pass is restated here, with the same
//     window and constants; S is the fp64 quotient.
//   image_loss_finish_kernel: the means over n in ascending order, the weighted total, zeros for terms that were not computed.
#include <math.h>

#include "../../include/pivp_loss.h"
#include "pivp_kernels.h"

namespace pivp {

constexpr int IL_NT = 256;                        // pointwise kernel
constexpr int DS_NT = 512;                        // DSSIM kernel: eight waves
constexpr int DS_T = 16;                          // output pixels per tile side: 64.3 KB of static LDS at win = 11
constexpr int DS_MAXWIN = 11;

template <int NT>
__device__ __forceinline__ double il_block_sum(double v, double* red) {      // fixed tree over the block; red[] is reusable after the call
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double t = red[0];
    return t;
}

__device__ __forceinline__ double il_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

struct PointwiseArgs {
    const float* pred; const float* truth;
    int N, C, H, W;
    int on_mse, on_l1, on_gdl;
    double k_mse, k_l1, k_v, k_h;                 // gradient factors: 2 w_mse / (N CHW), w_l1 / (N CHW), w_gdl / (N C (H-1) W), w_gdl / (N C H (W-1))
    float* values; double* wsv;                   // [4][N] each
    float* grad; int grad_add;                    // grad_add: the DSSIM part is there already
};

__global__ __launch_bounds__(IL_NT) void pointwise_loss_kernel(PointwiseArgs a) {
    __shared__ double red[IL_NT];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, HW = H * W, CHW = a.C * HW;
    // 16-byte accesses: every image and every row then starts on 16 bytes, and a group of four never straddles a row
    const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.pred) | reinterpret_cast<uintptr_t>(a.truth) | reinterpret_cast<uintptr_t>(a.grad)) & 15) == 0;
    for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
        const float* __restrict__ py = a.pred + (size_t)n * CHW;
        const float* __restrict__ px = a.truth + (size_t)n * CHW;
        float* __restrict__ pg = a.grad ? a.grad + (size_t)n * CHW : nullptr;
        double s_mse = 0.0, s_l1 = 0.0, s_v = 0.0, s_h = 0.0;
        // group g = four consecutive pixels, to thread g % IL_NT: the order of a thread's sums is the same for the vector and the element-wise form
        for (int i0 = tid * 4; i0 < CHW; i0 += 4 * IL_NT) {
            float yc[4], xc[4], yu[4], xu[4], yd[4], xd[4], yl[4], xl[4], yr[4], xr[4];
            bool up[4], dn[4], lf[4], rt[4], in[4];
            if (vec) {
                const int pl = i0 % HW, i = pl / W, j = pl - i * W;
                const f32x4 qy = *reinterpret_cast<const f32x4*>(py + i0), qx = *reinterpret_cast<const f32x4*>(px + i0);
                f32x4 uy = {0.f, 0.f, 0.f, 0.f}, ux = uy, dy = uy, dx = uy;
                float ly = 0.f, lx = 0.f, ry = 0.f, rx = 0.f;
                if (a.on_gdl) {
                    if (i > 0) { uy = *reinterpret_cast<const f32x4*>(py + i0 - W); ux = *reinterpret_cast<const f32x4*>(px + i0 - W); }
                    if (i < H - 1) { dy = *reinterpret_cast<const f32x4*>(py + i0 + W); dx = *reinterpret_cast<const f32x4*>(px + i0 + W); }
                    if (j > 0) { ly = py[i0 - 1]; lx = px[i0 - 1]; }
                    if (j + 4 < W) { ry = py[i0 + 4]; rx = px[i0 + 4]; }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    in[e] = true;
                    yc[e] = qy[e]; xc[e] = qx[e]; yu[e] = uy[e]; xu[e] = ux[e]; yd[e] = dy[e]; xd[e] = dx[e];
                    up[e] = i > 0; dn[e] = i < H - 1; lf[e] = j + e > 0; rt[e] = j + e < W - 1;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    yl[e] = e > 0 ? qy[e > 0 ? e - 1 : 0] : ly; xl[e] = e > 0 ? qx[e > 0 ? e - 1 : 0] : lx;
                    yr[e] = e < 3 ? qy[e < 3 ? e + 1 : 3] : ry; xr[e] = e < 3 ? qx[e < 3 ? e + 1 : 3] : rx;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int idx = i0 + e;
                    in[e] = idx < CHW;
                    const int pl = in[e] ? idx % HW : 0, i = pl / W, j = pl - i * W;
                    up[e] = in[e] && a.on_gdl && i > 0; dn[e] = in[e] && a.on_gdl && i < H - 1;
                    lf[e] = in[e] && a.on_gdl && j > 0; rt[e] = in[e] && a.on_gdl && j < W - 1;
                    yc[e] = in[e] ? py[idx] : 0.f; xc[e] = in[e] ? px[idx] : 0.f;
                    yu[e] = up[e] ? py[idx - W] : 0.f; xu[e] = up[e] ? px[idx - W] : 0.f;
                    yd[e] = dn[e] ? py[idx + W] : 0.f; xd[e] = dn[e] ? px[idx + W] : 0.f;
                    yl[e] = lf[e] ? py[idx - 1] : 0.f; xl[e] = lf[e] ? px[idx - 1] : 0.f;
                    yr[e] = rt[e] ? py[idx + 1] : 0.f; xr[e] = rt[e] ? px[idx + 1] : 0.f;
                }
            }
            float gout[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double y = (double)yc[e], x = (double)xc[e];
                const double d = y - x;
                double g = 0.0;
                if (in[e]) {
                    if (a.on_mse) { s_mse += d * d; g += a.k_mse * d; }
                    if (a.on_l1) { s_l1 += fabs(d); g += a.k_l1 * il_sign(d); }
                    if (a.on_gdl) {
                        if (up[e]) {       // the pixel's own vertical edge: counted in the value here
                            const double dv = y - (double)yu[e], t = fabs(dv) - fabs(x - (double)xu[e]);
                            s_v += fabs(t); g += a.k_v * (il_sign(t) * il_sign(dv));
                        }
                        if (dn[e]) {       // the edge of the pixel below: this pixel is its subtrahend
                            const double dv = (double)yd[e] - y, t = fabs(dv) - fabs((double)xd[e] - x);
                            g -= a.k_v * (il_sign(t) * il_sign(dv));
                        }
                        if (lf[e]) {
                            const double dh = y - (double)yl[e], t = fabs(dh) - fabs(x - (double)xl[e]);
                            s_h += fabs(t); g += a.k_h * (il_sign(t) * il_sign(dh));
                        }
                        if (rt[e]) {
                            const double dh = (double)yr[e] - y, t = fabs(dh) - fabs((double)xr[e] - x);
                            g -= a.k_h * (il_sign(t) * il_sign(dh));
                        }
                    }
                }
                gout[e] = (float)g;
                if (pg && a.grad_add && in[e]) gout[e] = (float)((double)pg[i0 + e] + g);
            }
            if (pg) {
                if (vec) *reinterpret_cast<f32x4*>(pg + i0) = f32x4{gout[0], gout[1], gout[2], gout[3]};
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (in[e]) pg[i0 + e] = gout[e];
                }
            }
        }
        const double t_mse = a.on_mse ? il_block_sum<IL_NT>(s_mse, red) : 0.0;
        const double t_l1 = a.on_l1 ? il_block_sum<IL_NT>(s_l1, red) : 0.0;
        const double t_v = a.on_gdl ? il_block_sum<IL_NT>(s_v, red) : 0.0;
        const double t_h = a.on_gdl ? il_block_sum<IL_NT>(s_h, red) : 0.0;
        if (tid == 0) {
            const double v0 = t_mse / (double)CHW, v1 = t_l1 / (double)CHW;
            const double v2 = a.on_gdl ? t_v / ((double)a.C * (double)(H - 1) * (double)W) + t_h / ((double)a.C * (double)H * (double)(W - 1)) : 0.0;
            a.wsv[0 * (size_t)a.N + n] = v0; a.wsv[1 * (size_t)a.N + n] = v1; a.wsv[2 * (size_t)a.N + n] = v2;
            a.values[0 * (size_t)a.N + n] = (float)v0; a.values[1 * (size_t)a.N + n] = (float)v1; a.values[2 * (size_t)a.N + n] = (float)v2;
        }
    }
}

template <int WIN>
__global__ __launch_bounds__(DS_NT) void dssim_kernel(const float* pred, const float* truth, int N, int C, int H, int W, float sigma, float data_range,
                                                      double gscale, float* __restrict__ values, double* __restrict__ wsv, float* __restrict__ grad) {
    constexpr int R = WIN - 1;
    constexpr int PS = DS_T + 2 * R, PP = PS + 1;         // staged pixel rows / columns, row pitch in floats
    constexpr int MS = DS_T + R;                          // map rows / columns
    __shared__ float sx[PS * PP], sy[PS * PP];
    __shared__ double hm[5][PS][MS];                      // row moments; later the row sums of the three maps, and the reductions' scratch
    __shared__ double am[3][MS][MS];                      // alpha, beta, gamma
    double (*h2)[MS][DS_T] = reinterpret_cast<double (*)[MS][DS_T]>(&hm[0][0][0]);
    double* red = &hm[0][0][0];
    static_assert(sizeof(double) * DS_NT <= sizeof(hm) && sizeof(double) * 3 * MS * DS_T <= sizeof(hm), "red[] and h2[] live in hm");
    static_assert(sizeof(float) * 2 * PS * PP + sizeof(double) * (5 * PS * MS + 3 * MS * MS) <= 65536, "static LDS");
    const int tid = threadIdx.x;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const int HW = H * W, CHW = C * HW;
    const int tiles_x = (W + DS_T - 1) / DS_T, tiles_y = (H + DS_T - 1) / DS_T, tiles_c = tiles_x * tiles_y, ntiles = C * tiles_c;

    // the separable window, normalised to sum 1 in double; sigma <= 0: uniform (frame_metrics_kernel's)
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

    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const float* __restrict__ py = pred + (size_t)n * CHW;
        const float* __restrict__ px = truth + (size_t)n * CHW;
        float* __restrict__ pg = grad ? grad + (size_t)n * CHW : nullptr;
        double acc = 0.0;
        for (int it = 0; it < ntiles; ++it) {
            const int c = it / tiles_c, rem = it - c * tiles_c, tyi = rem / tiles_x;
            const int q0y = tyi * DS_T, q0x = (rem - tyi * tiles_x) * DS_T;      // the tile's first output pixel
            const int o0y = q0y - R, o0x = q0x - R;                                // ... first map position = first staged pixel
            const float* __restrict__ cy = py + (size_t)c * HW;
            const float* __restrict__ cx = px + (size_t)c * HW;
            __syncthreads();      // the tile before has read sx / sy / h2
            for (int i = tid; i < PS * PS; i += DS_NT) {
                const int r = i / PS, q = i - r * PS;
                const int gy = o0y + r, gx = o0x + q;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                sx[r * PP + q] = in ? cx[gy * W + gx] : 0.f;
                sy[r * PP + q] = in ? cy[gy * W + gx] : 0.f;
            }
            __syncthreads();
            // horizontal pass: the five row moments of every staged row in the image, at every valid position column.  Without a gradient only the
            // tile's own positions (map rows / columns >= R) are needed
            for (int i = tid; i < PS * MS; i += DS_NT) {
                const int r = i / MS, j = i - r * MS;
                const int gy = o0y + r, gpx = o0x + j;
                if (gy < 0 || gy >= H || gpx < 0 || gpx >= OW || (!pg && (j < R || r < R))) continue;
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {
                    const double x = (double)sx[r * PP + j + k], y = (double)sy[r * PP + j + k];
                    const double wx = w[k] * x, wy = w[k] * y;
                    m0 += wx; m1 += wy; m2 += wx * x; m3 += wy * y; m4 += wx * y;
                }
                hm[0][r][j] = m0; hm[1][r][j] = m1; hm[2][r][j] = m2; hm[3][r][j] = m3; hm[4][r][j] = m4;
            }
            __syncthreads();
            // vertical pass: the window moments, S and the three maps.  A position outside the valid range carries zeros; its row moments were never
            // written and are not read
            for (int i = tid; i < MS * MS; i += DS_NT) {
                const int a = i / MS, j = i - a * MS;
                const int gpy = o0y + a, gpx = o0x + j;
                const bool valid = gpy >= 0 && gpy < OH && gpx >= 0 && gpx < OW;
                const bool own = a >= R && j >= R;
                double al = 0.0, be = 0.0, ga = 0.0;
                if (valid && (pg || own)) {
                    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
#pragma unroll
                        for (int e = 0; e < 5; ++e) m[e] += w[k] * hm[e][a + k][j];
                    }
                    const double mx = m[0], my = m[1];
                    const double vx = m[2] - mx * mx, vy = m[3] - my * my, vxy = m[4] - mx * my;
                    const double A1 = 2.0 * mx * my + C1, A2 = 2.0 * vxy + C2, B1 = mx * mx + my * my + C1, B2 = vx + vy + C2;
                    const double iB = 1.0 / (B1 * B2);
                    const double S = (A1 * A2) * iB;
                    if (own) acc += S;
                    // d S / d m_y at fixed raw second moments, 2 d S / d m_yy, d S / d m_xy
                    al = 2.0 * mx * (A2 - A1) * iB - 2.0 * my * S * (1.0 / B1 - 1.0 / B2);
                    be = -2.0 * S / B2;
                    ga = 2.0 * A1 * iB;
                }
                am[0][a][j] = al; am[1][a][j] = be; am[2][a][j] = ga;
            }
            __syncthreads();
            if (pg) {
                // transposed window, rows: position column q - l sees pixel column q with weight w[l]
                for (int i = tid; i < MS * DS_T; i += DS_NT) {
                    const int a = i / DS_T, b = i - a * DS_T;
                    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
                    for (int l = 0; l < WIN; ++l) {
                        t0 += w[l] * am[0][a][b + R - l]; t1 += w[l] * am[1][a][b + R - l]; t2 += w[l] * am[2][a][b + R - l];
                    }
                    h2[0][a][b] = t0; h2[1][a][b] = t1; h2[2][a][b] = t2;
                }
                __syncthreads();
                // ... columns, the per-pixel combination and the one rounding
                for (int i = tid; i < DS_T * DS_T; i += DS_NT) {
                    const int a = i / DS_T, b = i - a * DS_T;
                    const int gy = q0y + a, gx = q0x + b;
                    if (gy >= H || gx >= W) continue;
                    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        t0 += w[k] * h2[0][a + R - k][b]; t1 += w[k] * h2[1][a + R - k][b]; t2 += w[k] * h2[2][a + R - k][b];
                    }
                    const double y = (double)sy[(a + R) * PP + b + R], x = (double)sx[(a + R) * PP + b + R];
                    pg[(size_t)c * HW + gy * W + gx] = (float)(gscale * (t0 + y * t1 + x * t2));
                }
            }
        }
        const double t = il_block_sum<DS_NT>(acc, red);
        if (tid == 0) {
            const double v = 1.0 - t / ((double)C * (double)OH * (double)OW);
            wsv[3 * (size_t)N + n] = v;
            values[3 * (size_t)N + n] = (float)v;
        }
    }
}

// one block: rows of terms that were not computed are zeroed, thread k adds term k's per-image doubles in ascending n
__global__ __launch_bounds__(IL_NT) void image_loss_finish_kernel(const double* __restrict__ wsv, int N, double w0, double w1, double w2, double w3,
                                                                  int on0, int on1, int on2, int on3, float* __restrict__ values,
                                                                  float* __restrict__ terms) {
    __shared__ double mean[4];
    const int on[4] = {on0, on1, on2, on3};
    for (int k = 0; k < 4; ++k)
        if (!on[k]) for (int n = threadIdx.x; n < N; n += IL_NT) values[(size_t)k * N + n] = 0.f;
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        double s = 0.0;
        if (on[k]) for (int n = 0; n < N; ++n) s += wsv[(size_t)k * N + n];
        mean[k] = s / (double)N;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double wk[4] = {w0, w1, w2, w3};
        double tot = 0.0;
        for (int k = 0; k < 4; ++k) {
            terms[k] = (float)mean[k];
            if (on[k]) tot += wk[k] * mean[k];
        }
        terms[4] = (float)tot;
    }
}

__global__ __launch_bounds__(256) void frame_seed_add_kernel(float* __restrict__ go, const float* __restrict__ seed, long n, int vec) {
    const long stride = (long)gridDim.x * blockDim.x;
    if (vec) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += stride) {
            f32x4 a = reinterpret_cast<f32x4*>(go)[i];
            const f32x4 b = reinterpret_cast<const f32x4*>(seed)[i];
            a += b;
            reinterpret_cast<f32x4*>(go)[i] = a;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) go[i] += seed[i];
    }
}

// go[i] += seed[i]: the caller's d loss / d gen_images joins the sweep's own seed (pivp_plan_set_frame_grad)
int frame_seed_add(float* go, const float* seed, long n, hipStream_t s) {
    PIVP_CHECK_ARG(go && seed && n >= 1);
    const int vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(go) | reinterpret_cast<uintptr_t>(seed)) & 15) == 0;
    const long work = vec ? n / 4 : n;
    long blocks = (work + 255) / 256;
    const long cap = 8l * pivp_cu_count();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(frame_seed_add_kernel, dim3((unsigned)blocks), dim3(256), 0, s, go, seed, n, vec);
    return PIVP_LAUNCH_STATUS();
}

static bool il_finite(float v) { return v == v && fabsf(v) <= 3.4028234e38f; }

static bool image_loss_sizes_ok(int N, int C, int H, int W) { return N >= 1 && C >= 1 && H >= 1 && W >= 1; }

}  // namespace pivp

using namespace pivp;

extern "C" long long pivp_image_loss_ws_bytes(int N, int C, int H, int W, const pivp_image_loss_t* spec) {
    if (!spec || !image_loss_sizes_ok(N, C, H, W)) return PIVP_ERR_BADARG;
    return 4ll * N * (long long)sizeof(double);
}

extern "C" int pivp_image_loss(const float* pred, const float* truth, int N, int C, int H, int W, const pivp_image_loss_t* spec, float* values,
                               float* terms, float* grad, void* ws, void* stream) {
    PIVP_CHECK_ARG(pred && truth && spec && values && terms && ws);
    PIVP_CHECK_ARG(image_loss_sizes_ok(N, C, H, W) && (long long)C * H * W < (1ll << 31));
    PIVP_CHECK_ARG(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth) | reinterpret_cast<uintptr_t>(values) |
                     reinterpret_cast<uintptr_t>(terms) | reinterpret_cast<uintptr_t>(grad)) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
    const pivp_image_loss_t sp = *spec;
    PIVP_CHECK_ARG(il_finite(sp.w_mse) && il_finite(sp.w_l1) && il_finite(sp.w_gdl) && il_finite(sp.w_dssim) && il_finite(sp.sigma));
    PIVP_CHECK_ARG(sp.data_range > 0.f && il_finite(sp.data_range));
    PIVP_CHECK_ARG(sp.win >= 3 && sp.win <= DS_MAXWIN && (sp.win & 1) == 1);
    const bool on_mse = sp.w_mse != 0.f, on_l1 = sp.w_l1 != 0.f, on_gdl = sp.w_gdl != 0.f, on_ds = sp.w_dssim != 0.f;
    PIVP_CHECK_ARG(!on_ds || (H >= sp.win && W >= sp.win));
    PIVP_CHECK_ARG(!on_gdl || (H >= 2 && W >= 2));
    hipStream_t s = (hipStream_t)stream;
    double* wsv = static_cast<double*>(ws);
    const double dN = (double)N, chw = (double)C * (double)H * (double)W;
    if (on_ds) {
        const int OH = H - sp.win + 1, OW = W - sp.win + 1;
        const double gscale = -(double)sp.w_dssim / (dN * ((double)C * (double)OH * (double)OW));
        const int grid = N < 2 * pivp_cu_count() ? N : 2 * pivp_cu_count();      // at most two blocks share a CU (64 KB of LDS each at win = 11)
#define PIVP_DS_LAUNCH(WIN_)                                                                                                                        \
    case WIN_:                                                                                                                                      \
        hipLaunchKernelGGL(dssim_kernel<WIN_>, dim3(grid), dim3(DS_NT), 0, s, pred, truth, N, C, H, W, sp.sigma, sp.data_range, gscale, values, wsv, \
                           grad);                                                                                                                   \
        break
        switch (sp.win) {
            PIVP_DS_LAUNCH(3);
            PIVP_DS_LAUNCH(5);
            PIVP_DS_LAUNCH(7);
            PIVP_DS_LAUNCH(9);
            PIVP_DS_LAUNCH(11);
        }
#undef PIVP_DS_LAUNCH
        if (hipGetLastError() != hipSuccess) return PIVP_ERR_LAUNCH;
    }
    if (on_mse || on_l1 || on_gdl || (!on_ds && grad)) {      // (no weight at all: the pass still writes the zero gradient)
        PointwiseArgs a;
        a.pred = pred; a.truth = truth; a.N = N; a.C = C; a.H = H; a.W = W;
        a.on_mse = on_mse; a.on_l1 = on_l1; a.on_gdl = on_gdl;
        a.k_mse = 2.0 * (double)sp.w_mse / (dN * chw);
        a.k_l1 = (double)sp.w_l1 / (dN * chw);
        a.k_v = on_gdl ? (double)sp.w_gdl / (dN * ((double)C * (double)(H - 1) * (double)W)) : 0.0;
        a.k_h = on_gdl ? (double)sp.w_gdl / (dN * ((double)C * (double)H * (double)(W - 1))) : 0.0;
        a.values = values; a.wsv = wsv; a.grad = grad; a.grad_add = on_ds ? 1 : 0;
        const int cap = 8 * pivp_cu_count();
        hipLaunchKernelGGL(pointwise_loss_kernel, dim3(N < cap ? N : cap), dim3(IL_NT), 0, s, a);
        if (hipGetLastError() != hipSuccess) return PIVP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3(1), dim3(IL_NT), 0, s, wsv, N, (double)sp.w_mse, (double)sp.w_l1, (double)sp.w_gdl,
                       (double)sp.w_dssim, (int)on_mse, (int)on_l1, (int)on_gdl, (int)on_ds, values, terms);
    return PIVP_LAUNCH_STATUS();
}
