// Output heads of one timestep: 1x1 channel mixes on enc6 (mask logits + enc7), the CDNA kernel
// generator, the STP parameter regressor, and the fused flat-softmax + transform + compositing
// kernel that produces the next frame.  "TM" = src/models/train_model.py of the reference.
#include "pivp_kernels.h"
#include "frame_transform.h"
#include "skinny_linear.h"

namespace pivp {

// ------------------------------------------------------------------------------------------
// heads_1x1: masks = relu(Deconv1x1(enc6)) (TM:718-719) and enc7 = Deconv1x1(enc6) with the
// variant's activation (CDNA TM:315-317, STP TM:454-455, DNA TM:387-388) in ONE pass over enc6.
// e6 NHWC [B][HW][64]; wm [64][NP], we [64][NE] (the reference's deconv (Cin,Cout,1,1) layout);
// outputs planar [B][planes][HW] because the mask softmax is defined on the NCHW-flat order.
// Each WAVE owns 64 consecutive pixels: it loads its 64 x 64 tile with coalesced 16-B loads (1 KB per instruction), applies
// the optional LayerNorm, passes the tile through its private LDS region to turn "lane = 4 channels of a pixel" into "lane =
// pixel", and computes all outputs for its pixels; an output's 64 weights are 16 wave-uniform ds_read_b128.  No block
// barrier after the weight table is in place (the first version had the four waves share each sub-tile, two barriers and one
// load round trip per sub-tile: 1.5 TB/s).
// Optional fused input stage: with ln_part != null, e6 is the RAW enc6 output and
// relu(LayerNorm(e6)) (norm_enc6, TM:601; statistics from the enc6 kernel's (count, mean, M2)
// partials, gamma/beta NHWC-flat) is applied while the tile is staged, so the normalised map is
// neither written nor re-read (it IS written to y_out when that is non-null: training keeps it).
// ------------------------------------------------------------------------------------------
constexpr int HD_MAXOUT = 36;
constexpr int HD_XP = 68;  // 272-B rows: conflict-free per-lane ds_read_b128

__global__ __launch_bounds__(256) void heads_1x1_kernel(const float* __restrict__ e6, const float* __restrict__ wm,
                                                        const float* __restrict__ bm, const float* __restrict__ we,
                                                        const float* __restrict__ be, float* __restrict__ mask_logits,
                                                        float* __restrict__ enc7, float* __restrict__ layer0,
                                                        int total_px, int HW, int NP, int NE, int mode,
                                                        const float* __restrict__ ln_part, int ln_nparts,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        float* __restrict__ y_out, float* __restrict__ stat_out) {
    __shared__ __attribute__((aligned(16))) float xt[4][64 * HD_XP];     // one tile per wave
    __shared__ __attribute__((aligned(16))) float wl[HD_MAXOUT * 64];   // [output][k]
    __shared__ float bl[HD_MAXOUT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NO = NP + NE;
    for (int i = tid; i < 64 * NO; i += 256) {
        const int k = i / NO, o = i - k * NO;
        wl[o * 64 + k] = o < NP ? wm[k * NP + o] : we[k * NE + (o - NP)];
    }
    if (tid < NO) bl[tid] = tid < NP ? bm[tid] : be[tid - NP];
    const int px0 = (blockIdx.x * 4 + wave) * 64;     // this wave's pixels
    // the tile's loads go out before the barrier that publishes the weight table
    f32x4 rx[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int f = lane + 64 * j, p = f >> 4, cv = (f & 15) * 4;
        rx[j] = *reinterpret_cast<const f32x4*>(e6 + (size_t)min(px0 + p, total_px - 1) * 64 + cv);   // clamped: rows past the end are never stored
    }
    if (ln_part && px0 < total_px) {   // a wave's 64 pixels never straddle samples (HW % 64 == 0, checked by the launcher)
        const int bs = px0 / HW;
        float mean, rstd;
        ln_merge_partials(ln_part, bs, ln_nparts, eps, mean, rstd);
        if (lane == 0 && stat_out && px0 == bs * HW) { stat_out[bs * 2] = mean; stat_out[bs * 2 + 1] = rstd; }
#pragma unroll
        for (int j4 = 0; j4 < 16; j4 += 4) {          // gamma / beta in batches of four rows: 8 more loads in flight
            f32x4 g[4], bb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = lane + 64 * (j4 + u), p = f >> 4, cv = (f & 15) * 4;
                const size_t gi = (size_t)(min(px0 + p, total_px - 1) - bs * HW) * 64 + cv;
                g[u] = *reinterpret_cast<const f32x4*>(gamma + gi);
                bb[u] = *reinterpret_cast<const f32x4*>(beta + gi);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = lane + 64 * (j4 + u), p = f >> 4, cv = (f & 15) * 4;
                f32x4 v = rx[j4 + u];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf((v[e] - mean) * rstd * g[u][e] + bb[u][e], 0.f);
                if (y_out && px0 + p < total_px) *reinterpret_cast<f32x4*>(y_out + (size_t)(px0 + p) * 64 + cv) = v;
                rx[j4 + u] = v;
            }
        }
    }
    float* mt = xt[wave];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int f = lane + 64 * j, p = f >> 4, cv = (f & 15) * 4;
        *reinterpret_cast<f32x4*>(mt + p * HD_XP + cv) = rx[j];
    }
    __syncthreads();                                  // weight table ready (and, within the wave, its tile)
    if (px0 >= total_px) return;
    float xr[64];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(mt + lane * HD_XP + q * 4);
        xr[q * 4] = v[0]; xr[q * 4 + 1] = v[1]; xr[q * 4 + 2] = v[2]; xr[q * 4 + 3] = v[3];
    }
    const int px = px0 + lane;
    const int b = px / HW, p = px - b * HW;
    for (int o = 0; o < NO; ++o) {
        float acc = bl[o];
        const float* wo = wl + o * 64;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(wo + q * 4);
            acc = fmaf(xr[q * 4], w4[0], acc); acc = fmaf(xr[q * 4 + 1], w4[1], acc);
            acc = fmaf(xr[q * 4 + 2], w4[2], acc); acc = fmaf(xr[q * 4 + 3], w4[3], acc);
        }
        if (px < total_px) {
            if (o < NP) {
                mask_logits[((size_t)b * NP + o) * HW + p] = fmaxf(acc, 0.f);
            } else {
                const int oe = o - NP;
                if (mode != 1) acc = fmaxf(acc, 0.f);
                enc7[((size_t)b * NE + oe) * HW + p] = acc;
                if (mode != 2) layer0[((size_t)b * NE + oe) * HW + p] = sigmoidf_(acc);
            }
        }
    }
}

int heads_1x1(const float* e6, const float* wm, const float* bm, const float* we, const float* be,
              float* mask_logits, float* enc7, float* layer0, int B, int HW, int nmask_planes, int nenc7,
              int enc7_mode, hipStream_t s, const float* ln_part, int ln_nparts, const float* gamma, const float* beta,
              float eps, float* y_out, float* stat_out) {
    PIVP_CHECK_ARG(e6 && wm && bm && we && be && mask_logits && enc7 && B > 0 && HW > 0);
    PIVP_CHECK_ARG(nmask_planes >= 1 && nenc7 >= 1 && nmask_planes + nenc7 <= HD_MAXOUT);
    PIVP_CHECK_ARG(enc7_mode >= 0 && enc7_mode <= 2 && (enc7_mode == 2 || layer0));
    PIVP_CHECK_ARG(!ln_part || (ln_nparts > 0 && gamma && beta && HW % 64 == 0));
    const int total = B * HW;
    hipLaunchKernelGGL(heads_1x1_kernel, dim3((total + 255) / 256), dim3(256), 0, s, e6, wm, bm, we, be,
                       mask_logits, enc7, layer0, total, HW, nmask_planes, nenc7, enc7_mode,
                       ln_part, ln_nparts, gamma, beta, eps, y_out, stat_out);
    return PIVP_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------
// Skinny Linear on flatten(hidden5): out[b][o] = sum_k x[b][k] * wt[k][o].
// K is split in slices of 64 and the batch in groups of 8; each block writes its partial sums and the
// finisher adds them in a fixed order (bitwise reproducible).
// wt is K-major with 256 padded columns; x is the NHWC-flat hidden5 (the checkpoint permutes
// cdna_kerns/W's in-feature axis from c*64+y*8+x to (y*8+x)*128+c at load time).
// ------------------------------------------------------------------------------------------
int cdna_kernel_partials_slices(int K) { return (K + LIN_KS - 1) / LIN_KS; }

template <typename ACC>
__global__ __launch_bounds__(256) void skinny_linear_partials_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                                     float* __restrict__ partials, int B, int K) {
    skinny_linear_partials_body<ACC>(x, wt, partials, B, K, blockIdx.x, blockIdx.y, gridDim.x);
}

// CDNA finisher (TM:326-329): cdna_finish_block of skinny_linear.h, one block per sample
__global__ __launch_bounds__(256) void cdna_kernels_finish_kernel(const float* __restrict__ partials, const float* __restrict__ bias,
                                                                  float* __restrict__ kerns, int B, int KS, int nout, float* __restrict__ vpre) {
    __shared__ float v[256];
    cdna_finish_block(partials, bias, kerns, B, KS, nout, vpre, blockIdx.x, v);
}

// the mask counts cdna_kernels() takes: its finisher is one block of 256 threads, a thread per kernel tap (asked by plan_serves_forward / _backward, plan.h)
bool cdna_kernels_serves(int num_masks) { return num_masks >= 1 && num_masks * 25 <= 256; }

int cdna_kernels(const float* hidden5, const float* wt, const float* bias, float* partials, float* kerns,
                 int B, int K, int num_masks, hipStream_t s, float* vpre) {
    PIVP_CHECK_ARG(hidden5 && wt && bias && partials && kerns && B > 0 && K > 0 && cdna_kernels_serves(num_masks));
    const int KS = cdna_kernel_partials_slices(K);
    hipLaunchKernelGGL(skinny_linear_partials_kernel<float>, dim3(KS, (B + LIN_BG - 1) / LIN_BG), dim3(256), 0, s, hidden5, wt, partials, B, K);
    hipLaunchKernelGGL(cdna_kernels_finish_kernel, dim3(B), dim3(256), 0, s, partials, bias, kerns, B, KS, num_masks * 25, vpre);
    return PIVP_LAUNCH_STATUS();
}

// the K-slice partial sums alone (the finisher then runs inside frame_head_kernel, csrc/frame_head.hip); dbl: accumulate in fp64 (STP)
int motion_partials(const float* hidden5, const float* wt, float* partials, int B, int K, int dbl, hipStream_t s) {
    PIVP_CHECK_ARG(hidden5 && wt && partials && B > 0 && K > 0);
    const int KS = cdna_kernel_partials_slices(K);
    if (dbl) hipLaunchKernelGGL(skinny_linear_partials_kernel<double>, dim3(KS, (B + LIN_BG - 1) / LIN_BG), dim3(256), 0, s, hidden5, wt, partials, B, K);
    else hipLaunchKernelGGL(skinny_linear_partials_kernel<float>, dim3(KS, (B + LIN_BG - 1) / LIN_BG), dim3(256), 0, s, hidden5, wt, partials, B, K);
    return PIVP_LAUNCH_STATUS();
}

// STP finisher (TM:458-468): stp_finish_block of skinny_linear.h
__global__ __launch_bounds__(128) void stp_params_finish_kernel(const float* __restrict__ partials, const float* __restrict__ b1,
                                                                const float* __restrict__ w2, const float* __restrict__ b2,
                                                                float* __restrict__ theta, int B, int KS, float* __restrict__ s1_out) {
    __shared__ float s1[100];
    stp_finish_block(partials, b1, w2, b2, theta, B, KS, s1_out, blockIdx.x, s1);
}

int stp_params(const float* hidden5, const float* wt1, const float* b1, const float* w2, const float* b2,
               float* partials, float* theta, int B, int K, hipStream_t s, float* s1_out) {
    PIVP_CHECK_ARG(hidden5 && wt1 && b1 && w2 && b2 && partials && theta && B > 0 && K > 0);
    const int KS = cdna_kernel_partials_slices(K);
    hipLaunchKernelGGL(skinny_linear_partials_kernel<double>, dim3(KS, (B + LIN_BG - 1) / LIN_BG), dim3(256), 0, s, hidden5, wt1, partials, B, K);
    hipLaunchKernelGGL(stp_params_finish_kernel, dim3(B), dim3(128), 0, s, partials, b1, w2, b2, theta, B, KS, s1_out);
    return PIVP_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------
// composite: flat softmax of the mask logits + motion transform of the previous frame + mask
// weighted sum -> next frame, one pass, nothing intermediate written to HBM.
//   masks (TM:720-722): the reference reshapes the NCHW mask tensor to (-1, NP) and softmaxes
//     axis 1, i.e. over NP CONSECUTIVE elements of the per-sample planar buffer (NP = num_masks+1);
//     groups cut across pixels/rows/planes.  Reproduced exactly: group of flat index f is f / NP.
//   CDNA (TM:341-349, TM:725-727): out = m0*prev + m1*sigmoid(enc7) + sum_{k<NM-1} m_{k+2} * (prev (*) kern_k);
//     the last generated kernel never pairs with a mask (zip truncation) and is skipped.
//     Evaluated as one 5x5 correlation with the per-pixel blended kernel sum_k m_{k+2} kern_k.
//   STP (TM:465-471): all NM-1 warps are the same affine warp -> (sum_{q>=2} m_q) * warp(prev).
//   DNA (TM:392-415): per-pixel 25-tap kernel from enc7, with the reference's slice quirk
//     (shifted copies are cut at H-xk / W-yk).
// One block = one sample x CP_TR (4) image rows; the frame tile with its 2-pixel halo, the logit windows
// (tile +- NP-1 flat elements per plane) and the sample's kernels are staged in LDS.
// ------------------------------------------------------------------------------------------
// The arithmetic of each piece is frame_transform.h's; this kernel stages the operands and composes them.
constexpr int CP_TR = BAND_TR;

#ifdef PIVP_CP_STAMPS
__device__ long long pivp_cp_stamps[8];
#define CP_STAMP(i) do { if (blockIdx.x == 1 && blockIdx.y == 3 && threadIdx.x == 0) pivp_cp_stamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define CP_STAMP(i)
#endif
template <int MODE>
__global__ __launch_bounds__(256) void composite_kernel(const float* __restrict__ prev, const float* __restrict__ logits,
                                                        const float* __restrict__ layer0, const float* __restrict__ aux,
                                                        float* __restrict__ out, float* __restrict__ masks_out,
                                                        int H, int W, int NM, int stp_zero) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int NP = NM + 1;
    const int HW = H * W;
    const int b = blockIdx.y;
    const int y0 = blockIdx.x * CP_TR;
    const int rows = min(CP_TR, H - y0);
    const int p0 = y0 * W, np = rows * W;
    const int win = np + 2 * (NP - 1);
    const int G = np / NP + 2;
    float* kl = sm;                         // [11][28] (CDNA: 25 taps per kernel + 3 pad); 16-B aligned rows
    float* lg = sm + CDNA_KL;                 // [NP][win]
    float* gmx = lg + NP * win;             // [NP][G]
    float* ginv = gmx + NP * G;             // [NP][G]
    float* prevt = ginv + NP * G;           // [3][CP_TR+4][W+4]
    const int PW = W + 4;
    const int tid = threadIdx.x;
    const float* lgb = logits + (size_t)b * NP * HW;
    const FlatSoftmax sx(NP);
    CP_STAMP(0);

    // ---- staging: EVERY global load of the block is issued before the first LDS store, so the block pays one L2 / MALL
    // round trip (~2k cycles) instead of one per element (first version) or per batch --------------------------------
    {
        float tl[12][3];
#pragma unroll
        for (int m = 0; m < 12; ++m)
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                const int jx = tid + 256 * jj;
                const int F = m * HW + p0 - (NP - 1) + jx;
                tl[m][jj] = (m < NP && jx < win && F >= 0 && F < NP * HW) ? lgb[F] : 0.f;
            }
        float tp[3][BAND_PR];
        const float* pb = prev + (size_t)b * 3 * HW;
        band_tile_request<3>(tp, pb, 3, MODE != 1, tid, y0, H, W);
        float tk[2] = {0.f, 0.f};
        if (MODE == 0) cdna_table_request(tk, aux, b, NM, tid);
#pragma unroll
        for (int m = 0; m < 12; ++m)
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                const int jx = tid + 256 * jj;
                if (m < NP && jx < win) lg[m * win + jx] = tl[m][jj];
            }
        band_tile_file<3>(tp, prevt, pb, 3, MODE != 1, tid, y0, H, W);
        if (MODE == 0) cdna_table_file(tk, kl, tid);
        for (int m = 0; m < NP; ++m)                              // windows longer than 3 x 256 elements (4 W + 2 (NP - 1) > 768: W >= 187 at 12 planes, 192 at 2)
            for (int jx = tid + 768; jx < win; jx += 256) {
                const int F = m * HW + p0 - (NP - 1) + jx;
                lg[m * win + jx] = (F >= 0 && F < NP * HW) ? lgb[F] : 0.f;
            }
    }
    __syncthreads();
    CP_STAMP(1);
    sx.groups<ExpFast>(lg, win, G, HW, p0, np, gmx, ginv, tid, 256);
    __syncthreads();

    CP_STAMP(2);
    for (int pp = tid; pp < np; pp += 256) {
        const int p = p0 + pp;
        const int y = p / W, x = p - y * W;
        const int ry = y - y0;
        float l0v[3] = {0.f, 0.f, 0.f};   // issued first: their latency hides under the mask / kernel arithmetic
        if (MODE != 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) l0v[c] = layer0[((size_t)b * 3 + c) * HW + p];
        }
        float mk[12];
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            if (m < NP) {
                mk[m] = sx.at<ExpFast>(lg + m * win, gmx + m * G, ginv + m * G, HW, p0, m, pp);
                if (masks_out) masks_out[((size_t)b * NP + m) * HW + p] = mk[m];
            } else {
                mk[m] = 0.f;
            }
        }
        float o3[3];
        if (MODE == 0) {
            float keff[25];
#pragma unroll
            for (int i = 0; i < 25; ++i) keff[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k)
                if (cdna_kernel_paired(k, NM)) cdna_blend_add(mk[k + 2], kl + k * 28, keff);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int at = (c * (CP_TR + 4) + ry) * PW + x;
                const float* pt = prevt + at;   // (the centre tap through the pointer: with prevt[at + ..] composite_kernel<2> takes 143 registers for 120)
                const float t = taps5x5(keff, prevt, at, PW);
                const float pc = pt[2 * PW + 2];
                o3[c] = mk[0] * pc + mk[1] * l0v[c] + t;
            }
        } else if (MODE == 1) {
            const StpSample sp = stp_sample(aux + (size_t)b * 6, x, y, H, W, stp_zero);
            const float msum = stp_mask_sum(mk);
            const float* pb = prev + (size_t)b * 3 * HW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = stp_gather(pb, (size_t)c * HW, sp, H, W);
                o3[c] = mk[0] * pb[(size_t)c * HW + p] + mk[1] * l0v[c] + msum * t;
            }
        } else {
            float kw[25];
            dna_weights([&](int i) { return aux[((size_t)b * 25 + i) * HW + p]; }, kw);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int at = (c * (CP_TR + 4) + ry) * PW + x;
                const float* pt = prevt + at;   // (the centre tap through the pointer: with prevt[at + ..] composite_kernel<2> takes 143 registers for 120)
                const float t = dna_apply(kw, prevt, at, PW, y, x, H, W);
                o3[c] = mk[0] * pt[2 * PW + 2] + mk[1] * t;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * HW + p] = o3[c];
        CP_STAMP(3 + (pp >= 256));
    }
    CP_STAMP(5);
}
#ifdef PIVP_CP_STAMPS
}
extern "C" int pivp_debug_cp_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(pivp::pivp_cp_stamps), 8 * sizeof(long long)) == hipSuccess ? 0 : -2;
}
namespace pivp {
#endif

// the frames and mask counts composite() takes (what pivp_plan_create asks before it accepts a configuration: plan_serves_forward, plan.h)
bool composite_serves(int H, int W, int num_masks, int mode) {
    if (H <= 1 || W <= 1 || num_masks < 1 || num_masks > 11 || mode < 0 || mode > 2) return false;
    if (mode == 2 && num_masks != 1) return false;   // TM:389-390
    return composite_lds_bytes(W, num_masks) <= 160 * 1024 && W + 4 <= 256;      // (a thread per column of a padded row)
}

int composite(const float* prev, const float* mask_logits, const float* layer0, const float* aux,
              float* out, float* masks_out, int B, int H, int W, int num_masks, int mode, int stp_zero_border,
              hipStream_t s) {
    PIVP_CHECK_ARG(prev && mask_logits && aux && out && B > 0 && composite_serves(H, W, num_masks, mode) && (mode == 2 || layer0));
    const size_t lds = composite_lds_bytes(W, num_masks);
    dim3 grid((H + CP_TR - 1) / CP_TR, B);
#define PIVP_LAUNCH_CP(M)                                                                                   \
    do {                                                                                                    \
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&composite_kernel<M>),                        \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)        \
            return PIVP_ERR_LAUNCH;                                                                         \
        hipLaunchKernelGGL((composite_kernel<M>), grid, dim3(256), lds, s, prev, mask_logits, layer0, aux,  \
                           out, masks_out, H, W, num_masks, stp_zero_border);                               \
    } while (0)
    if (mode == 0) PIVP_LAUNCH_CP(0);
    else if (mode == 1) PIVP_LAUNCH_CP(1);
    else PIVP_LAUNCH_CP(2);
#undef PIVP_LAUNCH_CP
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
