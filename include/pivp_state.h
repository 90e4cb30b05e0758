/* Recurrent state across rollouts: entry points of libpivp_hip.so that let a rollout START from a given ConvLSTM state and LEAVE the state behind its
 * last step, and that copy, broadcast and select such states -- what the reference's stateful `Model` does between two `__call__`s without
 * `reset_state()` (TM:230-232, 254-257, 604-618) --, beside the model's C ABI of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*,
 * PIVP_ERR_BADARG with nothing launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).  Bound by
 * `_lib.STATE_SIGNATURES`; the ABI version of pivp_hip.h covers this header too.
 *
 * Layout of the recurrent state of a batch B, fp32, contiguous, c before h for each cell:
 *     for cell i = 0..6 (lstm1 .. lstm7):  c_i [B][H_i][W_i][C_i],  h_i [B][H_i][W_i][C_i]
 * with (H_i, W_i) = (H, W) / {2, 2, 4, 4, 8, 4, 2} and C_i = {32, 32, 64, 64, 128, 64, 32}: fourteen segments, exactly the values the plan's own
 * step buffers hold, in every precision mode (the cell state and output are fp32 in all of them).
 *
 * NOT served by this header alone: the backward sweep through a rollout that started from a given state (truncated back-propagation through time
 * across the call boundary).  The sweep's first timestep has forms of its own for "no recurrent input" -- in the batched weight gradients, in the
 * deterministic slot form and in the data-gradient-only kernel.  pivp_rollout_backward refuses such a rollout (PIVP_ERR_STATE) unless the sweep has been
 * enabled for it through include/pivp_state_grad.h, which also gives the gradient with respect to the initial state and takes one on the final state. */
#ifndef PIVP_STATE_H
#define PIVP_STATE_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PIVP_STATE_SEGMENTS 14

/* Floats per sample of the fourteen segments, in layout order (c_0, h_0, c_1, ...), and their sum (311,296 at 64 x 64; the state of a batch B is
 * B * floats_per_sample floats and segment g starts at B * (sum of the segments in front of it)).  Pure host arithmetic on cfg->height / width: no
 * GPU, no plan.  Either output may be null.  PIVP_ERR_BADARG: a null cfg, a frame size pivp_plan_create would refuse (below 16 or off 8). */
int pivp_state_layout(const pivp_config_t* cfg, long long seg_floats_per_sample[PIVP_STATE_SEGMENTS], long long* floats_per_sample);

/* Where the plan's next rollouts (pivp_rollout_forward, pivp_rollout_predict) take their initial recurrent state from and leave their final one, until
 * registered again.  All null with observed = 0 (the default) restores the plan's own behaviour, launches and bits.
 *   state_in != NULL: the first timestep reads cell i's (c, h) from it (batch = the plan's) instead of starting from zeros; it then runs the ordinary
 *     gate convolution over [x | h], not the first-step form without the h half of K.  Read only, by the first step's kernels.
 *   state_out != NULL: behind the last timestep ONE launch (csrc/state.hip) writes the last step's fourteen tensors to it, every element once.
 *   state_in == state_out is allowed: the read happens at step 0 and the write behind the last step, in stream order.  Otherwise they must not overlap.
 *   observed > 0 (pivp_rollout_predict only; pivp_rollout_forward keeps the configuration's warm start, TM:663): the number of leading steps fed from
 *     context_images, in place of cfg.context_frames, 1 <= observed <= T-1; context_images then holds `observed` frames and track_frame must be
 *     <= observed - 1 (pivp_rollout_predict returns PIVP_ERR_BADARG otherwise).  This is how a prediction is continued: observed = 1, the one
 *     frame being the last predicted one.
 * The memory must stay valid until the rollouts that use it have run.  After a rollout that started from state_in != NULL, pivp_rollout_backward
 * returns PIVP_ERR_STATE unless enabled (see the head of this file); an enabled sweep reads state_in again, so it must then stay unmodified until that sweep.
 * PIVP_ERR_BADARG: a null plan, a pointer off 16 bytes, observed < 0 or > T-1. */
int pivp_plan_set_rollout_state(pivp_plan_t* plan, const float* state_in, float* state_out, int observed);
/* Reads the registration back; any output may be null.  PIVP_ERR_BADARG: a null plan. */
int pivp_plan_get_rollout_state(const pivp_plan_t* plan, const float** state_in, float** state_out, int* observed);

/* dst (batch B_dst) from src (batch B_src), both in the layout above for cfg's frame size: sample b of dst = sample index[b] of src, segment by
 * segment; index: B_dst int32 on the device, every entry in [0, B_src) (TRUSTED: the caller validates it); index == NULL requires B_src == B_dst and is
 * the identity.  Serves broadcast (B_src = 1, index all zero), selection and permutation.  ONE launch, plain 16-byte loads and stores (4-byte ones when
 * src or dst is off 16 bytes), 64-bit offsets, every dst element written once, bit-exact.  src and dst must not overlap.
 * PIVP_ERR_BADARG: a null cfg / src / dst, a frame size as above, B_src or B_dst < 1, index == NULL with B_src != B_dst, a pointer off 4 bytes. */
int pivp_state_copy(const pivp_config_t* cfg, const float* src, int B_src, float* dst, int B_dst, const int* index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_STATE_H */
