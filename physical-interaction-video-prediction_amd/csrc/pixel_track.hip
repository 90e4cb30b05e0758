// pixel_track: one timestep of designated-pixel tracking (Finn & Levine 2017, visual MPC).  The step's compositing (TM:720-728) is a linear
// map "previous frame -> next frame"; applied to P probability planes instead of the RGB frame, with the synthesised layer sigmoid(enc7)
// set to zero, it gives where the mass of a designated pixel goes:
//   CDNA: out = m0*D + sum_{k<NM-1} m_{k+2} * (D (*) kern_k)      (zip truncation: the last kernel pairs with no mask)
//   STP : out = m0*D + (sum_{q>=2} m_q) * warp_theta(D)           (all warps share one theta)
//   DNA : out = m0*D + m1 * sum_taps kn_tap * shift_tap(D)        (slice quirk of TM:400; nothing synthesised, nothing zeroed)
// `masks` are the SOFTMAXED masks [B][NM+1][HW] the head wrote (masks_out of composite / frame_head), read once per pixel and reused for all
// P planes.  The band / halo staging and the transforms are composite_kernel's (csrc/heads.hip), from csrc/frame_transform.h, so
// composite(prev = D, layer0 = 0) and this kernel agree bit for bit.  fp32 FMAs in a fixed order, no atomics: bit-reproducible.
#include "pivp_kernels.h"
#include "frame_transform.h"

namespace pivp {

constexpr int PT_TR = BAND_TR;          // image rows per block, as composite_kernel
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
    float* tile = sm + (MODE == 0 ? CDNA_KL : 0);    // [P][PT_TR+4][PW], CDNA / DNA
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
        float tp[PT_MAXP][BAND_PR];
        band_tile_request<PT_MAXP>(tp, pb, P, true, tid, y0, H, W);
        float tk[2] = {0.f, 0.f};
        if (MODE == 0) cdna_table_request(tk, aux, b, NM, tid);
        band_tile_file<PT_MAXP>(tp, tile, pb, P, true, tid, y0, H, W);
        if (MODE == 0) cdna_table_file(tk, kl, tid);
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
            for (int k = 0; k < 10; ++k)
                if (cdna_kernel_paired(k, NM)) cdna_blend_add(mk[k + 2], kl + k * 28, keff);
            const float m0 = mk[0];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pt = tile + (c * (PT_TR + 4) + ry) * PW + x;
                    const float t = taps5x5(keff, pt, 0, PW);
                    ob[(size_t)c * HW] = m0 * pt[2 * PW + 2] + t;
                }
            }
        } else if (MODE == 1) {
            const StpSample sp = stp_sample(aux + (size_t)b * 6, x, y, H, W, stp_zero);
            const float msum = stp_mask_sum(mk);
            const float m0 = mk[0];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pc = pb + (size_t)c * HW;
                    const float t = stp_gather(pb, (size_t)c * HW, sp, H, W);
                    ob[(size_t)c * HW] = m0 * pc[p] + msum * t;
                }
            }
        } else {
            float kw[25];
            dna_weights([&](int i) { return kn[i]; }, kw);
            const float m0 = mk[0], m1 = mk[1];
            load_px(pp + 256);
#pragma unroll
            for (int c = 0; c < PT_MAXP; ++c) {
                if (c < P) {
                    const float* pt = tile + (c * (PT_TR + 4) + ry) * PW + x;
                    const float t = dna_apply(kw, pt, 0, PW, y, x, H, W);
                    ob[(size_t)c * HW] = m0 * pt[2 * PW + 2] + m1 * t;
                }
            }
        }
    }
}

int pixel_track(const float* planes_in, const float* masks, const float* aux, float* planes_out, int B, int P, int H, int W,
                int num_masks, int mode, int stp_zero_border, hipStream_t s) {
    PIVP_CHECK_ARG(planes_in && masks && aux && planes_out && planes_in != planes_out && B > 0 && P >= 1 && P <= PT_MAXP);
    PIVP_CHECK_ARG(composite_serves(H, W, num_masks, mode));      // the geometry pivp_composite accepts: its LDS footprint and tile width
    const int lds = mode == 1 ? 0 : (int)(sizeof(float) * ((size_t)P * (PT_TR + 4) * (W + 4) + (mode == 0 ? CDNA_KL : 0)));
    constexpr int kCap = (int)(sizeof(float) * ((size_t)PT_MAXP * (PT_TR + 4) * 256 + CDNA_KL));   // the most any accepted geometry asks for
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
