/* Planning on a goal image: the entry point of libpivp_hip.so that scores predicted frames against a goal image and hands back the gradient with
 * respect to the frames, beside the model's C ABI of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*, PIVP_ERR_BADARG with nothing
 * launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).  `planning.cem_plan`, `score_actions` and
 * `refine_actions` share it.  Bound by `_lib.GOAL_COST_SIGNATURES`; the ABI version of pivp_hip.h covers this header too. */
#ifndef PIVP_GOAL_COST_H
#define PIVP_GOAL_COST_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weighted squared / absolute error of S x K predicted frames to a goal image, per frame and folded over the steps, and its gradient.
 *   frames [S][K][3][H][W] fp32: what pivp_rollout_predict writes, from the first predicted frame on.
 *   goal [G][3][H][W], G == 1 (one goal for all candidates, g(k) = 0) or G == K (one per sample, g(k) = k).
 *   pixel_w [H][W] or null: non-negative weights, the region of interest; null = all ones.
 *   inv_norm: 1 / (3 * sum(pixel_w)), formed by the caller in double (null pixel_w: 1 / (3 H W)).
 *   step_w [S].   grad: null or [S][K][3][H][W].
 * With d = frames[s][k][c][i] - goal[g(k)][c][i]:
 *     per_step[s][k]   = inv_norm * sum_c sum_i pixel_w[i] * (w_mse * d*d + w_l1 * |d|), rounded to fp32 once; a value that is not finite then (NaN
 *                        or inf, a diverged rollout) is replaced by bad_cost
 *     cost[k]          = (accumulate ? cost[k] : 0) + scale * sum_s step_w[s] * per_step[s][k], s ascending over the stored per_step values; the sum
 *                        is formed in double and added once
 *     grad[s][k][c][i] = scale * step_w[s] * inv_norm * pixel_w[i] * (2 * w_mse * d + w_l1 * sign(d)), sign(0) = 0: d cost[k] / d frames.  Written, not
 *                        accumulated, every element; all zeros for a frame whose per_step was replaced by bad_cost.
 * w_mse = 1, w_l1 = 0, step_w = 1 / S and null pixel_w: the mean squared error over steps and pixels (`refine_actions`' goal-image cost).
 * Arithmetic is fp64 from the first difference to the single rounding of each output.  No atomics and no workspace: one block per frame adds
 * per-thread sums in a fixed order and a fixed tree, so per_step[s][k] and frame (s, k)'s gradient depend on that frame, its goal, the weights and
 * the scalars alone -- not on K, G, the grid, the pointers' alignment or whether grad was asked for.  Two launches.
 * PIVP_ERR_BADARG: a null frames / goal / step_w / cost / per_step, a pointer off 4 bytes, S or K < 1, S * K >= 2^31, H or W < 2, W > 252 or
 * H > 32768 (pivp_plan_cost's frames), G neither 1 nor K, a non-finite w_mse / w_l1 / bad_cost / scale / inv_norm, inv_norm <= 0. */
int pivp_goal_image_cost(const float* frames, const float* goal, int G, const float* pixel_w, float inv_norm, const float* step_w, float w_mse,
                         float w_l1, float bad_cost, float scale, int accumulate, float* cost, float* per_step, float* grad, int S, int K, int H,
                         int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_GOAL_COST_H */
