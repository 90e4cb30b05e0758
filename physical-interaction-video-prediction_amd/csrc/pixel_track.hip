// pixel_track: one timestep of designated-pixel tracking (Finn & Levine 2017, visual MPC).  The step's compositing (TM:720-728) is a linear
// map "previous frame -> next frame"; applied to P probability planes instead of the RGB frame, with the synthesised layer sigmoid(enc7)
// set to zero, it gives where the mass of a designated pixel goes:
//   CDNA: out = m0*D + sum_{k<NM-1} m_{k+2} * (D (*) kern_k)      (zip truncation: the last kernel pairs with no mask)
//   STP : out = m0*D + (sum_{q>=2} m_q) * warp_theta(D)           (all warps share one theta)
//   DNA : out = m0*D + m1 * sum_taps kn_tap * shift_tap(D)        (slice quirk of TM:400; nothing synthesised, nothing zeroed)
// `masks` are the SOFTMAXED masks [B][NM+1][HW] the head wrote (masks_out of composite / frame_head), read once per pixel and reused for all
// P planes.  Same band / halo staging and the same arithmetic order as composite_kernel (csrc/heads.hip), so that
// composite(prev = D, layer0 = 0) and this kernel agree to rounding.  fp32 FMAs in a fixed order, no atomics: bit-reproducible.
#include "pivp_kernels.h"

namespace pivp {

#ifndef PIVP_CP_TR
#define PIVP_CP_TR 4
#endif
constexpr int PT_TR = PIVP_CP_TR;       // image rows per block, as composite_kernel
constexpr int PT_KL = 11 * 28;          // LDS floats of the CDNA kernel table (28-float rows: 7 ds_read_b128 per kernel)
constexpr int PT_MAXP = 8;

template <int MODE>
__global__ __launch_bounds__(256) void pixel_track_kernel(const float* __restrict__ pin, const float* __restrict__ masks,
                                                          const float* __restrict__ aux, float* __restrict__ pout,
                                                          int P, int H, int W, int NM, int stp_zero) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int NP = NM + 1;
    const int HW = H * W;
    const int b = blockIdx.y;
    const int y0 = blockIdx.x * PT_TR;
    const int rows = min(PT_TR, H - y0);
    const int p0 = y0 * W, np = rows * W;
    const int PW = W + 4;
    const int tid = threadIdx.x;
    float* kl = sm;                                  // [11][28], CDNA only
    float* tile = sm + (MODE == 0 ? PT_KL : 0);      // [P][PT_TR+4][PW], CDNA / DNA
    const float* pb = pin + (size_t)b * P * HW;
    const float* mb = masks + (size_t)b * NP * HW;

    // a pixel's masks (and, DNA, its 25 raw taps): requested one pixel ahead of their use
    float mk[12];
    float kn[MODE == 2 ? 25 : 1];
    auto load_px = [&](int pp) {
        const bool ok = pp < np;
        const int p = p0 + pp;
#pragma unroll
        for (int m = 0; m < 12; ++m) mk[m] = (m < NP && ok) ? mb[(size_t)m * HW + p] : 0.f;
        if (MODE == 2) {
#pragma unroll
            for (int i = 0; i < 25; ++i) kn[i] = ok ? aux[((size_t)b * 25 + i) * HW + p] : 0.f;
        }
    };

    // ---- staging: every global load of the block is issued before the first LDS store (one L2 round trip per block) ----
    load_px(tid);
    if (MODE != 1) {
        constexpr int PR = (PT_TR + 4 + 2) / 3;      // tile rows per thread when 256 / PW >= 3 (W <= 81), else looped below
        float tp[PT_MAXP][PR];
        const int x = tid % PW, r0 = tid / PW, rstep = 256 / PW;   // PW <= 256 (checked by the launcher)
        const bool prow = tid < rstep * PW;
#pragma unroll
        for (int c = 0; c < PT_MAXP; ++c)
#pragma unroll
            for (int u = 0; u < PR; ++u) {
                const int r = r0 + u * rstep, iy = y0 + r - 2, ix = x - 2;
                tp[c][u] = (c < P && prow && r < PT_TR + 4 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                               ? pb[(size_t)c * HW + iy * W + ix] : 0.f;
            }
        float tk[2] = {0.f, 0.f};
        if (MODE == 0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i2 = tid + 256 * u, k = i2 / 28, e = i2 - k * 28;
                tk[u] = (i2 < PT_KL && k < NM && e < 25) ? aux[((size_t)b * NM + k) * 25 + e] : 0.f;
            }
        }
        if (prow) {
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c)
#pragma unroll
                for (int u = 0; u < PR; ++u) {
                    const int r = r0 + u * rstep;
                    if (c < P && r < PT_TR + 4) tile[(c * (PT_TR + 4) + r) * PW + x] = tp[c][u];
                }
            for (int r = r0 + PR * rstep; r < PT_TR + 4; r += rstep) {   // wide frames: remaining rows
                const int iy = y0 + r - 2, ix = x - 2;
                const bool in = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                for (int c = 0; c < P; ++c)
                    tile[(c * (PT_TR + 4) + r) * PW + x] = in ? pb[(size_t)c * HW + iy * W + ix] : 0.f;
            }
        }
        if (MODE == 0) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (tid + 256 * u < PT_KL) kl[tid + 256 * u] = tk[u];
        }
        __syncthreads();
    }

    for (int pp = tid; pp < np; pp += 256) {
        const int p = p0 + pp;
        const int y = p / W, x = p - y * W;
        const int ry = y - y0;
        float* ob = pout + (size_t)b * P * HW + p;
        if (MODE == 0) {
            float keff[25];
#pragma unroll
            for (int i = 0; i < 25; ++i) keff[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                if (k < NM - 1) {
                    const float mq = mk[k + 2];
                    float kv[28];
#pragma unroll
                    for (int q = 0; q < 7; ++q) {
                        const f32x4 t4 = *reinterpret_cast<const f32x4*>(kl + k * 28 + q * 4);
                        kv[q * 4] = t4[0]; kv[q * 4 + 1] = t4[1]; kv[q * 4 + 2] = t4[2]; kv[q * 4 + 3] = t4[3];
                    }
#pragma unroll
                    for (int i = 0; i < 25; ++i) keff[i] = fmaf(mq, kv[i], keff[i]);
                }
            }
            const float m0 = mk[0];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pt = tile + (c * (PT_TR + 4) + ry) * PW + x;
                    float t = 0.f;
#pragma unroll
                    for (int i = 0; i < 5; ++i)
#pragma unroll
                        for (int j = 0; j < 5; ++j) t = fmaf(keff[i * 5 + j], pt[i * PW + j], t);
                    ob[(size_t)c * HW] = m0 * pt[2 * PW + 2] + t;
                }
            }
        } else if (MODE == 1) {
            const float* th = aux + (size_t)b * 6;
            // coordinates in fp64, exactly as composite_kernel<1>
            const double xs = -1.0 + 2.0 * (double)x / (double)(W - 1);
            const double ys = -1.0 + 2.0 * (double)y / (double)(H - 1);
            double gu = (double)th[0] * xs + (double)th[1] * ys + (double)th[2];
            double gv = (double)th[3] * xs + (double)th[4] * ys + (double)th[5];
            if (!stp_zero) { gu = fmin(fmax(gu, -1.0), 1.0); gv = fmin(fmax(gv, -1.0), 1.0); }
            const double u = (gu + 1.0) * (double)(W - 1) * 0.5;
            const double v = (gv + 1.0) * (double)(H - 1) * 0.5;
            double u0 = floor(u), v0 = floor(v);
            if (!stp_zero) { u0 = fmin(fmax(u0, 0.0), (double)(W - 2)); v0 = fmin(fmax(v0, 0.0), (double)(H - 2)); }
            const float wu1 = (float)(u - u0), wv1 = (float)(v - v0);
            const int iu = (int)u0, iv = (int)v0;
            float msum = 0.f;
#pragma unroll
            for (int q = 2; q < 12; ++q) msum += mk[q];   // mk[q >= NP] is 0
            const float m0 = mk[0];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pc = pb + (size_t)c * HW;
                    float t = 0.f;
#pragma unroll
                    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
                        for (int du = 0; du < 2; ++du) {
                            const int uu = iu + du, vv = iv + dv;
                            const float wgt = (dv ? wv1 : 1.f - wv1) * (du ? wu1 : 1.f - wu1);
                            if ((unsigned)uu < (unsigned)W && (unsigned)vv < (unsigned)H)
                                t = fmaf(wgt, pc[vv * W + uu], t);
                        }
                    ob[(size_t)c * HW] = m0 * pc[p] + msum * t;
                }
            }
        } else {
            float kw[25];
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 25; ++i) {
                kw[i] = fmaxf(kn[i] - 1e-12f, 0.f) + 1e-12f;
                sum += kw[i];
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int i = 0; i < 25; ++i) kw[i] = kw[i] * inv;
            const float m0 = mk[0], m1 = mk[1];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pt = tile + (c * (PT_TR + 4) + ry) * PW + x;
                    float t = 0.f;
#pragma unroll
                    for (int xk = 0; xk < 5; ++xk)
#pragma unroll
                        for (int yk = 0; yk < 5; ++yk) {
                            const bool ok = (y + xk < H) && (x + yk < W);   // TM:400 slice quirk
                            t = fmaf(kw[xk * 5 + yk], ok ? pt[xk * PW + yk] : 0.f, t);
                        }
                    ob[(size_t)c * HW] = m0 * pt[2 * PW + 2] + m1 * t;
                }
            }
        }
    }
}

// the geometry pivp_composite accepts (csrc/heads.hip: its LDS footprint and tile width)
static bool composite_geometry_ok(int H, int W, int num_masks, int mode) {
    if (H <= 1 || W <= 1 || num_masks < 1 || num_masks > 11 || mode < 0 || mode > 2) return false;
    if (mode == 2 && num_masks != 1) return false;   // TM:389-390
    const int NP = num_masks + 1;
    const int np = PT_TR * W;
    const size_t lds = sizeof(float) * ((size_t)NP * (np + 2 * (NP - 1)) + 2 * NP * (np / NP + 2) + 3 * (PT_TR + 4) * (W + 4) + PT_KL);
    return lds <= 160 * 1024 && W + 4 <= 256;
}

int pixel_track(const float* planes_in, const float* masks, const float* aux, float* planes_out, int B, int P, int H, int W,
                int num_masks, int mode, int stp_zero_border, hipStream_t s) {
    PIVP_CHECK_ARG(planes_in && masks && aux && planes_out && planes_in != planes_out && B > 0 && P >= 1 && P <= PT_MAXP);
    PIVP_CHECK_ARG(composite_geometry_ok(H, W, num_masks, mode));
    const int lds = mode == 1 ? 0 : (int)(sizeof(float) * ((size_t)P * (PT_TR + 4) * (W + 4) + (mode == 0 ? PT_KL : 0)));
    constexpr int kCap = (int)(sizeof(float) * ((size_t)PT_MAXP * (PT_TR + 4) * 256 + PT_KL));   // the most any accepted geometry asks for
    static PerDeviceOnce once[3];
    const dim3 grid((H + PT_TR - 1) / PT_TR, B);
#define PIVP_LAUNCH_PT(M)                                                                                                          \
    do {                                                                                                                           \
        if (pivp_ensure_dyn_lds(once[M], reinterpret_cast<const void*>(&pixel_track_kernel<M>), kCap) != PIVP_OK) return PIVP_ERR_LAUNCH; \
        hipLaunchKernelGGL((pixel_track_kernel<M>), grid, dim3(256), lds, s, planes_in, masks, aux, planes_out, P, H, W, num_masks, \
                           stp_zero_border);                                                                                       \
    } while (0)
    if (mode == 0) PIVP_LAUNCH_PT(0);
    else if (mode == 1) PIVP_LAUNCH_PT(1);
    else PIVP_LAUNCH_PT(2);
#undef PIVP_LAUNCH_PT
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
