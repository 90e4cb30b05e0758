"""References for gradient refinement from a belief (tests/test_gpu_belief_refine.py): d cost / d actions of ONE `refine_actions(belief=)` iteration by
float64 autograd through the torch restatement of the model (oracle/torch_restatement.py), called on two windows without reset_state() and with the
recurrent state detached between them, as tests/state_grad_reference.py does -- window 1 observes one frame (that is the belief), window 2 rolls
`HORIZON` steps from the newest frame and feeds itself; the cost is the goal-image cost of include/pivp_goal_cost.h on window 2's frames.  CPU torch only.

`python tests/belief_refine_reference.py` is the batch-seed scan (below)."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the scan at the bottom)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import restatement as R  # noqa: E402
from oracle.torch_restatement import TorchModel  # noqa: E402
from input_grad_reference import rel_errors  # noqa: E402
from state_grad_reference import _detach_state  # noqa: E402

GATE = 2e-3      # the project's model-level input-gradient gate (tests/test_gpu_state_grad.py::test_input_gradients_after_a_carried_start), rel_errors
H = W = 16
B, HORIZON = 2, 3
GOAL = dict(mse=1.0, l1=0.25, step_weights=(0.5, 1.0, 1.5), weight=2.0)      # a `planning.GoalImageCost` with every term in play

# name -> (model kwargs of TorchModel / pivp_amd.Model, init_params kwargs, num_masks, batch kind, batch seed).  The batch seeds are the first of 0, 1,
# 2, ... at which plain float32 autograd of the restatement is itself inside GATE against float64 with a margin of ten (2e-4), so that no ReLU unit
# within fp32 rounding of zero decides the comparison -- the rule of tests/input_grad_reference.py, on this cost.  STP takes moving frames, as
# tests/state_grad_reference.py's STP case does: its sampler's gradient is an image difference, ill-conditioned on white noise.  The scan is this file
# run as a script; what it printed (float32 against float64, relative L2 / largest element; max |reference|):
#   cdna  seed 0  rel L2 8.92e-07 max 9.91e-07; max |ref| 2.0e-02   inside
#   stp   seed 0  rel L2 8.90e-06 max 5.92e-06; max |ref| 2.0e-01   inside
#   dna   seed 0  rel L2 1.05e-06 max 9.48e-07; max |ref| 8.0e-03   inside
CASES = {
    'cdna': (dict(), dict(num_masks=3), 3, 'synthetic', 0),
    'stp': (dict(is_cdna=False, is_stp=True), dict(model_type='STP', num_masks=3), 3, 'moving', 0),
    'dna': (dict(is_cdna=False, is_dna=True), dict(model_type='DNA', num_masks=1), 1, 'synthetic', 0),
}


def case_inputs(name, seed=None):
    """-> dict: model kwargs `mkw`, `nm`, params `P`, `observed` = (frame (1, B, 3, H, W), action (1, B, 5), state (B, 5)) -- what makes the belief --,
    `frame` (1, B, 3, H, W) the newest frame, `state` (B, 5) its robot state, `actions` (HORIZON, B, 5) the sequence to refine, `goal` (3, H, W)."""
    mkw, pkw, nm, kind, bseed = CASES[name]
    P = R.init_params_widened(seed=1, scale=1.0, height=H, width=W, **pkw)
    make = R.moving_batch if kind == 'moving' else R.synthetic_batch
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in make(B, HORIZON + 3, H, W, seed=bseed if seed is None else seed))
    return dict(mkw=dict(mkw, num_frame_before_prediction=1), nm=nm, P=P, observed=(imgs[:1], acts[:1], stas[0]), frame=imgs[1:2], state=stas[1],
                actions=acts[1:1 + HORIZON], goal=np.ascontiguousarray(imgs[HORIZON + 2, 0]))


def goal_cost(gen, goal, dtype):
    """torch: the `GOAL` cost of gen (S, B, 3, H, W) per sample -> (B,), as include/pivp_goal_cost.h states it (all pixel weights 1)."""
    d = gen - torch.tensor(goal, dtype=dtype)
    per_step = (GOAL['mse'] * d * d + GOAL['l1'] * d.abs()).sum(dim=(2, 3, 4)) / (3.0 * gen.shape[3] * gen.shape[4])
    return GOAL['weight'] * (torch.tensor(GOAL['step_weights'], dtype=dtype)[:, None] * per_step).sum(dim=0)


def run(name, dtype=torch.float64, seed=None):
    """-> dict(cost (B,), action_grad (HORIZON, B, 5) = d sum(cost) / d actions), float64 arrays"""
    c = case_inputs(name, seed)
    tm = TorchModel(c['nm'], params=c['P'], dtype=dtype, **c['mkw'])
    frame0, action0, state0 = c['observed']
    pad = lambda a: np.concatenate((a, np.zeros_like(a[:1])))      # (a window of T frames runs T - 1 steps: the last row is never read)
    tm([pad(frame0), pad(action0), pad(state0[None])], 0)
    _detach_state(tm)      # the belief is a constant of the sweep
    a = torch.tensor(c['actions'], dtype=dtype, requires_grad=True)
    images = torch.cat((torch.tensor(c['frame'], dtype=dtype), torch.zeros((HORIZON, B, 3, H, W), dtype=dtype)))
    actions = torch.cat((a, torch.zeros((1, B, 5), dtype=dtype)))
    states = torch.cat((torch.tensor(c['state'], dtype=dtype)[None], torch.zeros((HORIZON, B, 5), dtype=dtype)))
    tm([images, actions, states], 0)
    cost = goal_cost(torch.stack(tm.gen_images), c['goal'], dtype)
    cost.sum().backward()
    return dict(cost=cost.detach().double().numpy(), action_grad=a.grad.double().numpy())


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64, computed once per case and shared; leave it unchanged"""
    return run(name, torch.float64)


if __name__ == '__main__':      # the seed scan: float32 against float64 autograd on the CPU, per case and batch seed
    for name in sys.argv[1:] or list(CASES):
        for seed in range(9):
            r64, r32 = run(name, torch.float64, seed), run(name, torch.float32, seed)
            e = rel_errors(r32['action_grad'], r64['action_grad'])
            ok = max(e) < GATE / 10 and np.abs(r64['action_grad']).max() > 0
            print('%-5s seed %d  rel L2 %.2e max %.2e; max |ref| %.1e   %s' % (name, seed, e[0], e[1], np.abs(r64['action_grad']).max(),
                                                                             'inside' if ok else 'OUTSIDE'), flush=True)
            if ok:
                break
