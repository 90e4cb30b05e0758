/* Input gradients: entry points of libpivp_hip.so that make the backward sweep deliver d loss / d actions and d loss / d state0 and let it leave the
 * parameter gradients and its own loss out, beside the model's C ABI of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*,
 * PIVP_ERR_BADARG with nothing launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).  Bound by
 * `_lib.INPUT_GRAD_SIGNATURES`; the ABI version of pivp_hip.h covers this header too. */
#ifndef PIVP_INPUT_GRAD_H
#define PIVP_INPUT_GRAD_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pivp_plan_set_sweep_mode flags */
#define PIVP_SWEEP_PARAMS 1        /* bit 0: the sweep forms the parameter gradients */
#define PIVP_SWEEP_BUILTIN_LOSS 2  /* bit 1: the sweep seeds itself with the plan's own loss (frame and state MSE) */

/* Where every later pivp_rollout_backward of the plan leaves the gradient of the loss with respect to the actions it was given, dactions
 * [T-1][B][5] fp32 (row t: d loss / d actions[t], the action consumed by step t), and with respect to the initial state states[0], dstate0 [B][5]
 * fp32.  Both are OVERWRITTEN by the sweep, every element by exactly one thread with a plain store (dstate0: by one device-to-device copy behind the
 * sweep's last timestep); neither is read.  Either may be null alone; both null (the default) restores the sweep's own launches and bits.  With
 * dactions set the sweep issues one extra launch per timestep (pivp_action_grad on the step's tensors), with dstate0 one extra copy per sweep; the
 * parameter gradients are bit-identical with and without them.  Same rollout, same bytes: dactions has the same bits in default and deterministic
 * plans alike wherever the data gradients in front of it have (deterministic plans: always).  The memory must stay valid until the sweep has run.
 * PIVP_ERR_BADARG: a null plan, a pointer off 4 bytes. */
int pivp_plan_set_input_grad(pivp_plan_t* plan, float* dactions, float* dstate0);

/* What the plan's later sweeps compute: an OR of PIVP_SWEEP_*; the default 3 is the full sweep.
 *   PIVP_SWEEP_PARAMS cleared: every launch whose only products are parameter gradients is skipped -- the ConvLSTM and stride-2 conv weight-gradient
 *     launches with their side-stream traffic, the bias / column-sum launches, enc0's weight gradient, the norms' parameter reductions.  Kernels that
 *     fuse a parameter gradient with a data gradient run unchanged.  The registered gradient buffers (pivp_plan_set_grad) are still REQUIRED, and
 *     their contents are UNSPECIFIED after such a sweep: clear them before the next full one accumulates.  The gradient-group callback is not
 *     invoked, nothing runs on the plan's side stream and the sweep's final join waits for nothing.  The data gradients, and with them the input
 *     gradients above, are the full sweep's (bit-identical in a deterministic plan).
 *   PIVP_SWEEP_BUILTIN_LOSS cleared: d loss / d gen_images and d loss / d gen_states start from zero fills instead of the plan's own loss terms, so the
 *     sweep differentiates the caller's seed (pivp_plan_set_frame_grad) alone; pivp_rollout_backward returns PIVP_ERR_STATE when no seed is set.
 * PIVP_ERR_BADARG: a null plan, flags outside 0 .. 3. */
int pivp_plan_set_sweep_mode(pivp_plan_t* plan, int flags);
int pivp_plan_get_sweep_mode(const pivp_plan_t* plan);

/* The action half of enc3's smeared-input gradient for B samples (the launch the sweep issues per timestep):
 *     colsum[o]  = sum_p (e3[b][p][o] > 0 ? de3[b][p][o] : 0),  p < HW8, o < 64
 *     dact[b][j] = (use_state ? sum_o w3[64 + j][o] colsum[o] : 0) + sum_o wcs[o * 10 + j] dsnew[b][o],  j < 5
 *   e3 [B][HW8][64]: enc3's output;  de3: its gradient, rows of ldd3 floats (first 64 used);  w3 [74][64] (use_state) enc3's weight, unread and may
 *   be null otherwise;  wcs [5][10] the state predictor's weight;  dsnew [B][5] the gradient of the step's predicted state;  dact [B][5], written.
 * fp64 from the first add, one rounding per output, fixed order, no atomics, no workspace: same bytes, same bits.  One launch, B blocks.
 * PIVP_ERR_BADARG: a null e3 / de3 / wcs / dsnew / dact (w3 with use_state), e3 / de3 off 16 bytes, another pointer off 4, ldd3 < 64 or not a
 * multiple of 4, B or HW8 < 1. */
int pivp_action_grad(const float* e3, const float* de3, int ldd3, const float* w3, const float* wcs, const float* dsnew, float* dact, int B, int HW8,
                     int use_state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_INPUT_GRAD_H */
