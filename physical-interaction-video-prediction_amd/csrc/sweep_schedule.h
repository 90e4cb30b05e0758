// Which timesteps of the backward sweep share a weight-gradient launch.  Integer arithmetic only and nothing from HIP: a host compiler builds it alone
// (tests/test_sweep_schedule_host.py).
#pragma once

namespace pivp {

struct BatchSlot { int batch, slot; bool flush; };      // the step's batch (its parity is the ring), its slot in that ring, and whether it closes the batch

// Step t of a sweep over t = T-2 .. 0 with G timesteps per launch: batches of G counted from the top of the sweep; t = 0 (no h input) on its own.
// With deep batches (G > 2: the bf16 mode's 8) the LAST TWO batched timesteps (t = 2, 1) form a batch of their own: one batch of everything
// is launched at t = 1, when two timesteps of main-stream work are left for 1.4 ms of weight gradients to hide behind -- the sweep then ended with
// the main stream waiting ~0.2 ms per step for the side stream (profiles/r05/NOTES.md).
inline BatchSlot batch_slot(int T, int t, int G) {
    const int k = T - 2 - t, n = T - 2;
    const int tail = (G > 2 && n > 2) ? 2 : 0, body = n - tail, nb_body = (body + G - 1) / G;
    if (t == 0) return {nb_body + (tail ? 1 : 0), 0, true};
    if (k < body) return {k / G, k % G, k % G == G - 1 || k == body - 1};
    return {nb_body, k - body, k == n - 1};
}

// One timestep's place in the rings.  wg_*: where its gate gradients go in the ConvLSTMs' dG rings, wg_flush: it closes its batch.
// eg_*: the same for the dY rings of the five stride-2 3x3 layers (Grads::cat6); eq_next: the ring slot step t + 1 used.
struct StepSlots {
    int wg_ring, wg_slot; bool wg_flush;
    int eg_ring, eg_slot; bool eg_flush;
    int eq_next;
};

}  // namespace pivp
