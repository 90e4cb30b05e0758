/* Gradients through the recurrent state: entry points of libpivp_hip.so that let pivp_rollout_backward serve a rollout which STARTED from a registered
 * state (pivp_plan_set_rollout_state, include/pivp_state.h), leave d loss / d (that initial state) behind the sweep, and seed the sweep with
 * d (a later loss) / d (the rollout's final state) -- truncated back-propagation through time across calls, and, chained over consecutive windows,
 * the exact one in the memory of a single window.  What a Chainer user of the reference's stateful `Model` gets from calling it twice without
 * reset_state() and back-propagating (TM:230-232, 254-257).  Conventions as in pivp_state.h: int status PIVP_OK / PIVP_ERR_*, PIVP_ERR_BADARG with
 * nothing launched, caller-owned 16-byte-aligned device memory, stream-ordered, no synchronisation, no allocation.  Bound by
 * `_lib.STATE_GRAD_SIGNATURES`; the ABI version of pivp_hip.h covers this header too.
 *
 * Both gradient buffers use the fourteen-segment layout of pivp_state.h at the plan's batch (c_i then h_i for cell i = 0..6, each
 * [B][H_i][W_i][C_i]), fp32 in every precision mode.
 *
 * Everything is opt-in: with enable = 0 and both pointers null (the default) the sweep refuses a rollout that started from a state
 * (PIVP_ERR_STATE), launches nothing new and gives the bits it always gave. */
#ifndef PIVP_STATE_GRAD_H
#define PIVP_STATE_GRAD_H

#include "pivp_state.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the plan's next sweeps (pivp_rollout_backward) do about the recurrent state, until registered again.
 *   enable = 1: a rollout that started from state_in is served.  The state is a CONSTANT of that sweep (truncated BPTT): its first timestep, which the
 *     sweep visits last, reads cell i's c_{-1} and h_{-1} from the state_in the FORWARD rollout read -- the plan remembers that pointer in
 *     pivp_rollout_forward --, for the gate backward and as the h operand of that step's weight gradients.  That memory must therefore stay valid and
 *     UNMODIFIED until the sweep has run.  A forward registered with state_in == state_out has overwritten its own start state: the sweep returns
 *     PIVP_ERR_STATE and launches nothing.  After a rollout from zeros the sweep is the one it always was, bit for bit.
 *   d_state_in != NULL (needs enable = 1 and a rollout that started from a state; otherwise the sweep returns PIVP_ERR_STATE): behind the sweep's t = 0 ONE
 *     launch (csrc/state_grad.hip) writes d loss / d state_in to it, every element once: d c_{-1} of cell i is what the gate backward leaves behind, d h_{-1}
 *     the h columns of that step's input gradient, which then computes them (it skips them otherwise).
 *   d_state_out != NULL: a seed, d (a later loss) / d (the final state of this rollout), read by the sweep's first visited timestep t = T-2: the c
 *     segments start every cell's d c (ONE launch copies them into the plan's buffers), the h segments join the cell's d h in place.  Allowed after
 *     any training rollout, from a state or from zeros, with enable 0 or 1; the seed alone is "something to differentiate" for a sweep without the
 *     built-in loss (pivp_plan_set_sweep_mode) and without a frame seed.  Read only; must stay valid until the sweep has run.
 *   All null and 0 restores the plan's own behaviour.
 * Sweeps without parameter gradients and pivp_plan_set_input_grad work unchanged on such rollouts.
 * PIVP_ERR_BADARG: a null plan, enable other than 0 / 1, a pointer off 16 bytes, d_state_in without enable, the two buffers overlapping each other, or
 * d_state_in overlapping the state_in the plan's last rollout read (the sweep checks that again: PIVP_ERR_STATE).  A refused call changes nothing. */
int pivp_plan_set_state_grad(pivp_plan_t* plan, int enable, const float* d_state_out, float* d_state_in);
/* Reads the registration back; any output may be null.  PIVP_ERR_BADARG: a null plan. */
int pivp_plan_get_state_grad(const pivp_plan_t* plan, int* enable, const float** d_state_out, float** d_state_in);

/* The two kernels alone (tests, other callers of the per-op ABI), for cfg's frame size and batch.
 * gather: d_state_in <- the seven cells' d c (dc[i]: [B][H_i][W_i][C_i], contiguous) and the h columns of their input gradients (din[i]:
 *   [B][H_i][W_i][cx_i + C_i], the columns cx_i .. cx_i + C_i - 1; cx = {32, 32, 32, 64, 64, 128, 96}).  ONE launch, 16-byte loads and stores for
 *   every segment whose source and destination are on 16 bytes (4-byte ones for the others), 64-bit offsets, every destination element written once, no atomics, bit-exact.
 * scatter: dc[i] <- the c segment of cell i of d_state_out, the same kernel the other way; the h segments are not touched.
 * PIVP_ERR_BADARG: a null cfg / pointer / table entry, a frame size pivp_plan_create would refuse, batch < 1, a pointer off 4 bytes. */
int pivp_state_grad_gather(const pivp_config_t* cfg, const float* const dc[7], const float* const din[7], float* d_state_in, void* stream);
int pivp_state_grad_scatter(const pivp_config_t* cfg, const float* d_state_out, float* const dc[7], void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_STATE_GRAD_H */
