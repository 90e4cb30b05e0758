"""References for the gradients through a carried recurrent state (include/pivp_state_grad.h), shared by tests/test_gpu_state_grad.py and
tests/test_state_grad_host.py: the float64 torch restatement of the model (oracle/torch_restatement.py) called on two consecutive windows WITHOUT
reset_state().  With the graph left intact, loss1 + loss2 gives the full-BPTT gradients; with tm.c[n] / tm.h[n] replaced between the calls by
detached leaves that require grad it gives the truncated gradients of window 2 and d loss2 / d (the state window 2 started from).  NumPy / CPU torch only.

`python tests/state_grad_reference.py [case ...]` is the batch-seed scan (below)."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the scan at the bottom)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import restatement as R  # noqa: E402
from oracle.torch_restatement import TorchModel, LSTM_NAMES  # noqa: E402
from input_grad_reference import rel_errors  # noqa: E402,F401  (the state gradients' gate is measured with it)

PARAM_GATE = {'CDNA': 2e-3, 'STP': 5e-3, 'DNA': 5e-3}      # tests/test_gpu_train.py's tolerances of _check_grads, per model type
STATE_GATE = 2e-3                                          # per segment, input_grad_reference.rel_errors
CELL_LEVELS = (2, 2, 4, 4, 8, 4, 2)
CELL_CHANNELS = (32, 32, 64, 64, 128, 64, 32)

# name -> (model kwargs of TorchModel / pivp_amd.Model, init_params kwargs, num_masks, frames per window, batch kind, batch seed).  B = 2, 64 x 64, two
# consecutive windows cut out of one batch of 2 T frames.  The batch seeds are the first of 0, 1, 2, ... at which plain float32 autograd of the
# restatement is itself inside the tests' gates against float64 -- _check_grads at PARAM_GATE on the truncated parameter gradients of window 2 and on
# the full ones, rel_errors under STATE_GATE on every segment of d loss2 / d state -- so that no ReLU unit within fp32 rounding of zero decides the
# comparison; the chunked case also needs the truncated and the full reference to differ by ten gates on the ConvLSTM weights.  The scan is this
# file run as a script; what it printed (float32 against float64: worst of 99th percentile / relative L2 over the parameter tensors, truncated and
# full; worst state segment; distance of the truncated to the full reference on the ConvLSTM weights):
#   cdna_T3     seed 0  1.7e-06 / 1.5e-06; 1.8e-06; 0.96   inside
#   cdna_T5     seed 0  1.0e-06 / 1.1e-06; 1.5e-06; 0.95   inside
#   stp_T4      seed 0  2.2e-03 / 1.3e-03; 2.1e-03; 0.99   OUTSIDE (a state segment above 2e-3)      (moving frames: the STP sampler's gradient is an
#               seed 1  1.1e-03 / 1.2e-03; 6.7e-04; 0.98   inside                                      image difference, ill-conditioned on white noise)
#   dna_T4      seed 0  2.1e-03 / 8.7e-04; 4.6e-03; 0.98   OUTSIDE (a state segment above 2e-3)
#               seed 1  1.7e-06 / 1.3e-04; 2.3e-06; 0.98   inside
#   ctx3_T5     seed 0  1.3e-06 / 2.6e-04; 1.4e-06; 0.94   inside
#   nostate_T3  seed 0  2.0e-06 / 1.7e-06; 2.9e-06; 0.97   inside
# The smallest max |reference| over the fourteen state segments is 1.7e-06 .. 8.4e-06: no segment's reference is zero.
CASES = {
    'cdna_T3': (dict(), dict(), 10, 3, 'synthetic', 0),
    'cdna_T5': (dict(), dict(), 10, 5, 'synthetic', 0),
    'stp_T4': (dict(is_cdna=False, is_stp=True), dict(model_type='STP'), 10, 4, 'moving', 1),
    'dna_T4': (dict(is_cdna=False, is_dna=True), dict(model_type='DNA', num_masks=1), 1, 4, 'synthetic', 1),
    'ctx3_T5': (dict(num_frame_before_prediction=3), dict(), 10, 5, 'synthetic', 0),
    'nostate_T3': (dict(use_state=False), dict(use_state=False), 10, 3, 'synthetic', 0),
    'cdna_128_T3': (dict(), dict(height=128, width=128), 10, 3, 'synthetic', 0),      # (the 128 x 128 case takes test_bptt_gradients_128x128's inputs: seed 0)
}
SEEDS_OUTSIDE = {'stp_T4': (0,), 'dna_T4': (0,)}
CHUNKED_CASE = 'cdna_T3'
# The precision-mode tests compare two modes of the library on 'cdna_T3', where a gradient bound of 1e-4 (tests/test_gpu_bf16.py's for bf16x6, which carries no
# clause for it) holds only while the two modes' forward passes agree on every ReLU unit: one unit on different sides of zero moves the whole gradient
# by ~1e-3 (profiles/r06/NOTES.md 3).  Batch seed per mode: the first of 0, 1, 2, ... at which they agree where the bound needs it.  bf16x6 against
# fp32 at seed 0: one unit differs (tests/test_gpu_state_grad.py::test_bf16x6_batch_seed_outside asserts both).
PRECISION_SEEDS = {'bf16': 0, 'fp16x3': 0, 'bf16x6': 1}
PRECISION_SEEDS_OUTSIDE = {'bf16x6': (0,)}
SEED_CASES = ('cdna_T3',)      # final_state_grad alone: the cost is sum(w * final state)


def model_type(name):
    mkw = CASES[name][0]
    return 'STP' if mkw.get('is_stp') else 'DNA' if mkw.get('is_dna') else 'CDNA'


def case_inputs(name, seed=None):
    """-> (model kwargs, num_masks, params, [window 1, window 2]) with window = [images, actions, states] (T, 2, ...) float32"""
    mkw, pkw, nm, T, kind, bseed = CASES[name]
    P = R.init_params_widened(seed=1, scale=1.0, **pkw)
    hw = (pkw.get('height', 64), pkw.get('width', 64))
    make = R.moving_batch if kind == 'moving' else R.synthetic_batch
    imgs, acts, stas = make(2, 2 * T, hw[0], hw[1], seed=bseed if seed is None else seed)
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in (imgs, acts, stas))
    return mkw, nm, P, [[imgs[:T], acts[:T], stas[:T]], [imgs[T:], acts[T:], stas[T:]]]


def state_numel(B, H, W):
    return sum(2 * B * (H // lv) * (W // lv) * C for lv, C in zip(CELL_LEVELS, CELL_CHANNELS))


def pack_state(pairs):
    """[(c_i, h_i)] NCHW tensors of the seven cells -> the flat layout of include/pivp_state.h (c_i then h_i, each [B][H_i][W_i][C_i]) as float64"""
    return np.concatenate([t.detach().permute(0, 2, 3, 1).reshape(-1).double().numpy() for pair in pairs for t in pair])


def unpack_state(flat, B, H, W, dtype):
    """the flat layout -> [(c_i, h_i)] NCHW torch tensors"""
    out, at = [], 0
    for lv, C in zip(CELL_LEVELS, CELL_CHANNELS):
        pair = []
        for _ in range(2):
            n = B * (H // lv) * (W // lv) * C
            pair.append(torch.tensor(np.asarray(flat[at:at + n]).reshape(B, H // lv, W // lv, C), dtype=dtype).permute(0, 3, 1, 2).contiguous())
            at += n
        out.append(tuple(pair))
    return out


def segments(flat, B, H, W):
    """the fourteen segments of a flat state, in layout order"""
    out, at = [], 0
    for lv, C in zip(CELL_LEVELS, CELL_CHANNELS):
        for _ in range(2):
            n = B * (H // lv) * (W // lv) * C
            out.append(flat[at:at + n])
            at += n
    return out


def seed_weights(B, H, W):
    """the fixed random w of the final_state_grad tests, flat layout, float32"""
    return np.random.RandomState(11).standard_normal(state_numel(B, H, W)).astype(np.float32)


def _grads(tm):
    return {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.double().numpy()) for k, v in tm.p.items()}


def _detach_state(tm):
    leaves = []
    for n in LSTM_NAMES:
        tm.c[n] = tm.c[n].detach().clone().requires_grad_(True)
        tm.h[n] = tm.h[n].detach().clone().requires_grad_(True)
        leaves.append((tm.c[n], tm.h[n]))
    return leaves


def run(name, variant, dtype=torch.float64, seed=None):
    """variant 'truncated': window 2 swept with the state it started from detached -> dict(loss1, loss2, grads, state_grad, action_grad, state0_grad);
    'full': loss1 + loss2 with the graph intact -> dict(loss1, loss2, grads);
    'seed_carried' / 'seed_zeros': the cost is sum(seed_weights * final state of window 2), window 2 started from window 1's (detached) state / from
    zeros -> dict(grads, state_grad (carried only))."""
    mkw, nm, P, wins = case_inputs(name, seed)
    tm = TorchModel(nm, params=P, dtype=dtype, requires_grad=True, **mkw)
    out = {}
    leaves = None
    if variant != 'seed_zeros':
        out['loss1'] = tm(wins[0], 0)
        if variant != 'full':
            leaves = _detach_state(tm)
    a = torch.tensor(wins[1][1], dtype=dtype, requires_grad=True)
    s = torch.tensor(wins[1][2], dtype=dtype, requires_grad=True)
    out['loss2'] = tm([torch.tensor(wins[1][0], dtype=dtype), a, s], 0)
    B, _, H, W = wins[1][0].shape[1:]
    if variant == 'full':
        cost = out['loss1'] + out['loss2']
    elif variant == 'truncated':
        cost = out['loss2']
    else:
        w = unpack_state(seed_weights(B, H, W), B, H, W, dtype)
        cost = sum((wc * tm.c[n]).sum() + (wh * tm.h[n]).sum() for (wc, wh), n in zip(w, LSTM_NAMES))
    cost.backward()
    out['grads'] = _grads(tm)
    if leaves is not None:
        out['state_grad'] = pack_state([tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in pair) for pair in leaves])
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    out['action_grad'], out['state0_grad'] = zero(a), zero(s)
    out['loss1'] = float(out['loss1'].detach()) if 'loss1' in out else 0.0
    out['loss2'] = float(out['loss2'].detach())
    return out


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """float64, computed once per (case, variant) and shared; leave it unchanged"""
    return run(name, variant, torch.float64)


def lstm_weight_distance(ga, gb):
    """the largest relative L2 distance of two gradient sets over the seven ConvLSTM weights"""
    return max(np.linalg.norm(ga[n + '/conv/W'] - gb[n + '/conv/W']) / (np.linalg.norm(gb[n + '/conv/W']) + 1e-300) for n in LSTM_NAMES)


if __name__ == '__main__':      # the seed scan: float32 against float64 autograd on the CPU, per case and batch seed
    from test_gpu_train import _check_grads
    names = sys.argv[1:] or [n for n in CASES if '128' not in n]
    for name in names:
        tol = PARAM_GATE[model_type(name)]
        B, H, W = 2, CASES[name][1].get('height', 64), CASES[name][1].get('width', 64)
        for seed in range(9):
            notes, ok = [], True
            for variant in ('truncated', 'full'):
                r64, r32 = run(name, variant, torch.float64, seed), run(name, variant, torch.float32, seed)
                try:
                    worst = _check_grads(r32['grads'], r64['grads'], tol)[0]
                    notes.append('%s params %.2e' % (variant, worst))
                except AssertionError as e:
                    ok = False
                    notes.append('%s params OUTSIDE (%s)' % (variant, str(e)[:60]))
                if variant == 'truncated':
                    errs = [max(rel_errors(a, b)) for a, b in zip(segments(r32['state_grad'], B, H, W), segments(r64['state_grad'], B, H, W))]
                    nz = min(float(np.abs(sg).max()) for sg in segments(r64['state_grad'], B, H, W))
                    ok = ok and max(errs) < STATE_GATE and nz > 0
                    notes.append('state worst segment %.2e (smallest max |ref| %.1e)' % (max(errs), nz))
                    trunc = r64['grads']
                else:
                    dist = lstm_weight_distance(trunc, r64['grads'])
                    notes.append('truncated vs full on the ConvLSTM weights %.2e (%s ten gates)' % (dist, 'over' if dist >= 10 * tol else 'UNDER'))
            print('%-11s seed %d  %s   %s' % (name, seed, '; '.join(notes), 'inside' if ok else 'OUTSIDE'), flush=True)
            if ok:
                break
