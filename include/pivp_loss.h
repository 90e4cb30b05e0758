/* Training objectives beyond the reference's L2: entry points of libpivp_hip.so that score predicted frames with L1 / gradient-difference / DSSIM
 * terms and hand their gradient to the backward sweep, beside the model's C ABI of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*,
 * PIVP_ERR_BADARG with nothing launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).  Bound by
 * `_lib.LOSS_SIGNATURES`; the ABI version of pivp_hip.h covers this header too. */
#ifndef PIVP_LOSS_H
#define PIVP_LOSS_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weights of the four image terms and the SSIM window: win odd in 3 .. 11, Gaussian sigma (<= 0: the uniform window), data_range L > 0. */
typedef struct { float w_mse, w_l1, w_gdl, w_dssim; int win; float sigma, data_range; } pivp_image_loss_t;

/* Bytes of the workspace the image loss needs for N images: the four per-image terms as doubles.  PIVP_ERR_BADARG (-1) for N, C, H or W < 1 or a
 * null spec. */
long long pivp_image_loss_ws_bytes(int N, int C, int H, int W, const pivp_image_loss_t* spec);

/* The weighted L1 / gradient-difference / DSSIM (and extra-MSE) terms of N predicted images against their ground truth, pred and truth
 * [N][C][H][W] fp32, and the gradient of the weighted total with respect to pred.  Per image, y = pred and x = truth:
 *     mse_n   = mean (y - x)^2                              l1_n = mean |y - x|
 *     gdl_n   = sum | |y[i,j] - y[i-1,j]| - |x[i,j] - x[i-1,j]| | / (C (H-1) W)  +  sum | |y[i,j] - y[i,j-1]| - |x[i,j] - x[i,j-1]| | / (C H (W-1))
 *               (Mathieu et al. 2016 with alpha = 1)
 *     dssim_n = 1 - ssim_n, ssim_n by the definition of the per-sample metrics op of pivp_hip.h: separable window, valid positions, biased moments,
 *               mean over positions and channels.
 *   values [4][N]: the four terms per image (mse, l1, gdl, dssim).   terms [5]: terms[k] = the mean of term k over n, k < 4 (fp64 sums of the
 *   unrounded per-image terms in ascending n, rounded once); terms[4] = sum_k w_k * terms[k].   A term whose weight is 0 is not computed: its
 *   values and its mean are written as 0.
 *   grad [N][C][H][W] or null: d terms[4] / d pred; written, not accumulated, every element (all-zero weights give zeros).  sign(0) = 0 in every
 *   absolute value, torch's rule.
 *   ws: the workspace of the size query above, 8-byte aligned; scratch, overwritten by every call.
 * Arithmetic is fp64 from the first difference to the single rounding of each output; with w_dssim != 0 and another weight != 0 the gradient is the
 * fp32 DSSIM part plus the rest, rounded a second time.  No atomics: every sum is a per-thread sum in a fixed order and a fixed tree, so values and
 * gradient of image n depend on that image's data, on (C, H, W, win, sigma, data_range) and on the quotients w_k / N alone -- not on the grid, the
 * image's index or what else the call was asked for (grad or no grad, other weights).
 * Up to three launches.  PIVP_ERR_BADARG: a null pred / truth / spec / values / terms / ws, pred / truth / values / terms / grad off 4 bytes or ws
 * off 8, N, C, H or W < 1, C*H*W >= 2^31, win even or outside 3 .. 11, H or W < win with w_dssim != 0, H or W < 2 with w_gdl != 0, a non-finite
 * weight or sigma, data_range not positive and finite. */
int pivp_image_loss(const float* pred, const float* truth, int N, int C, int H, int W, const pivp_image_loss_t* spec, float* values, float* terms,
                    float* grad, void* ws, void* stream);

/* An additional d loss / d gen_images for the plan's backward sweep.  seed [(T - ctx)][B][3][H][W] fp32 is aligned with gen_images[ctx-1 .. T-2]
 * (the predictions the plan's own loss scores); every later sweep of the plan seeds go = fscale * (gen - x) + seed until the pointer is replaced.
 * Null (the default) restores the plan's own seed: the sweep's launches and bits are then what they are without this entry point, in deterministic
 * mode too.  The pointer is read on the sweep's stream only, by one extra launch behind the seed's; the memory must stay valid until that sweep has
 * run.  PIVP_ERR_BADARG: a null plan or a seed off 4 bytes. */
int pivp_plan_set_frame_grad(pivp_plan_t* plan, const float* seed);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_LOSS_H */
