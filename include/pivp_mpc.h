/* Closed-loop planning (visual MPC: plan, execute the first action, observe, plan again): the two entry points of libpivp_hip.so that let one
 * planning call hand its result to the next, beside the model's C ABI of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*,
 * PIVP_ERR_BADARG with nothing launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).  `planning.cem_plan`'s
 * options and `planning.MPC` use them.  Bound by `_lib.MPC_SIGNATURES`; the ABI version of pivp_hip.h covers this header too. */
#ifndef PIVP_MPC_H
#define PIVP_MPC_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PIVP_CEM_MAX_COLORED_STEPS 64

/* The cross-entropy update of pivp_hip.h, pivp_cem_update, with three options of iCEM (Pinneri et al. 2020): elites kept in the population, the mean as a candidate, and
 * temporally correlated noise.  Every argument up to `iteration` means what it means there; n = steps - t0 is the number of optimised rows.
 * With keep = 0, add_mean = 0 and beta = 0 every output has the bits pivp_cem_update gives.
 *
 * cost given: ranks, refit of mean / std, best_actions / best_cost and elite_idx exactly as pivp_cem_update.  Then
 *   keep (0 <= keep <= elites): for j < keep, rows t0 .. of slot j become rows t0 .. of the rank-j candidate (elite_idx[j]) as they were when
 *       the call began, bit for bit -- the update is in place and an elite may itself lie in a slot below keep; every copy reads before any writes.
 *       These slots are not resampled.  kept_in is ignored.
 * cost NULL (mean, std, best_*, elite_idx left alone, as pivp_cem_update):
 *   kept_in = 1: slots 0 .. keep-1 already hold sequences to evaluate as they lie (a warm start) and are left untouched; kept_in = 0: they are
 *       sampled like every other slot.
 * add_mean = 1: slot `keep` is not sampled; its rows become actions[t][keep][d] = min(max(mean[t-t0][d], low[d]), high[d]), with the mean this call
 *       leaves behind (the refitted one when cost is given).  keep + add_mean <= K.
 * Every other slot k is sampled: actions[t][k][d] = min(max(mean[t-t0][d] + std[t-t0][d] * y[t-t0][k][d], low[d]), high[d]), where z[i][k][d],
 * i = t - t0, is the standard normal pivp_cem_update draws for (k, t, d, iteration, seed) -- same Philox counters, key and Box-Muller pairing; a
 * slot that is not sampled just leaves its numbers unused -- and
 *   beta = 0: y = z.
 *   beta > 0 (n <= PIVP_CEM_MAX_COLORED_STEPS): per (k, d) the sequence over the n rows is y = Q z, y[i] = sum_c Q[i][c] z[c], c ascending, with
 *       the n x n matrix Q of power-law ("colored") noise.  s_j = max(j, 1)^(-beta/2).  Column 0 is the constant s_0.  For 0 < j < n/2 column
 *       2j-1 is sqrt(2) s_j cos(2 pi j i / n) and column 2j is -sqrt(2) s_j sin(2 pi j i / n).  For even n the last column (n-1) is
 *       s_{n/2} cos(pi i).  Every entry is divided by sigma = sqrt(s_0^2 + 2 sum_{0<j<n/2} s_j^2 + [n even] s_{n/2}^2), j ascending.  Each row of Q
 *       has unit norm, so every y[i] is again a standard normal and mean + std * y means what it does with white noise; neighbouring steps are
 *       positively correlated, the more the larger beta.  Q is formed in fp64 -- the angle reduced exactly, (j * i) mod n, before sincospi -- and
 *       y[i] is summed in fp64 and rounded to fp32 once.  beta = 0 is the identity by definition (Q at beta = 0 is an orthogonal matrix, not I).
 * 0 <= keep <= elites, kept_in and add_mean 0 or 1, keep + add_mean <= K, beta finite and >= 0, n <= 64 when beta > 0, and pivp_cem_update's own
 * conditions; anything else: PIVP_ERR_BADARG, nothing launched.  One workgroup, one launch, no workspace, no atomics, fixed order: the same bits
 * on every launch. */
int pivp_cem_update_ex(const float* cost, float* actions, float* mean, float* std, float* best_actions, float* best_cost, const float* low,
                       const float* high, int* elite_idx, int K, int steps, int t0, int elites, float alpha, float min_std,
                       unsigned long long seed, int iteration, int keep, int kept_in, int add_mean, float beta, void* stream);

/* The receding-horizon step between two planning calls: everything a planning call leaves behind moves up by `shift` rows, because the first
 * `shift` actions have been executed.  n = steps - t0 optimised rows, 1 <= shift < n; every copy is exact.  With i the row index, 0 <= i < n:
 *   mean [n][5]:          mean[i] = mean[i + shift] for i < n - shift, tail_mean[d] behind.
 *   std [n][5]:           std[i] = std[i + shift] for i < n - shift, tail_std[d] behind; then every element becomes max(std, std_floor[d]).
 *   actions [steps][K][5] or NULL: slots 0 .. keep-1 of rows t0 .. move up likewise; the tail rows are min(max(tail_mean[d], low[d]), high[d]).
 *                         Rows below t0 and slots from keep on are not touched.  NULL needs keep = 0.
 *   best_actions [n][5] or NULL: moves up likewise, with the same tail as actions.
 *   best_cost [1] or NULL: becomes +inf -- the old value scored another problem.
 * tail_mean, tail_std, std_floor [5] (std_floor >= 0 is the caller's business: the op takes the maximum as it finds it); low, high [5], read only
 * where actions or best_actions is given.  The buffers must not overlap each other.  1 <= K <= 1024, 0 <= keep <= K, 0 <= t0, n <= 65536;
 * anything else or a null mean / std / tail_mean / tail_std / std_floor (or low / high where they are read): PIVP_ERR_BADARG, nothing launched.
 * One workgroup, one launch: elements are read into registers, a barrier, then written, a block of rows at a time in ascending order, so no
 * element is overwritten before it has been read. */
int pivp_cem_shift(float* mean, float* std, float* actions, float* best_actions, float* best_cost, const float* low, const float* high,
                   const float* tail_mean, const float* tail_std, const float* std_floor, int K, int steps, int t0, int keep, int shift,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_MPC_H */
