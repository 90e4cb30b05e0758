"""References for the input gradients (include/pivp_input_grad.h), shared by tests/test_gpu_input_grad.py and tests/test_input_grad_host.py:
a float64 NumPy restatement of pivp_action_grad, and d loss / d actions, d loss / d states through the float64 torch restatement of the model
(oracle/torch_restatement.py) for the model-level cases.  NumPy / CPU torch only."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the scan at the bottom)
from oracle import restatement as R  # noqa: E402
from oracle.torch_restatement import TorchModel  # noqa: E402


# ---- pivp_action_grad ----------------------------------------------------------------------------------------------------------------------
def action_grad(e3, de3, w3, wcs, dsnew, use_state):
    """e3 [B][HW8][64], de3 [B][HW8][ldd3] (first 64 columns count), w3 [74][64], wcs [5][10], dsnew [B][5] -> dact [B][5] in float64:
    colsum[o] = sum_p (e3 > 0 ? de3 : 0); dact[j] = (use_state ? w3[64+j] . colsum : 0) + sum_o wcs[o][j] dsnew[o]."""
    e3, de3, wcs, dsnew = (np.asarray(a, dtype=np.float64) for a in (e3, de3, wcs, dsnew))
    colsum = np.where(e3 > 0, de3[:, :, :64], 0.0).sum(axis=1)                       # [B][64]
    out = dsnew @ wcs[:, :5]                                                         # [B][5]: sum_o dsnew[b][o] wcs[o][j]
    if use_state:
        out = out + colsum @ np.asarray(w3, dtype=np.float64)[64:69].T               # sum_o colsum[b][o] w3[64+j][o]
    return out


def action_grad_inputs(B, HW8, ldd3, seed, mixed=False):
    """e3 with exact zeros and negatives mixed in; de3 N(0, 1), or (mixed) magnitudes around 1e4 and 1e-3 side by side, where an fp32 running sum
    loses the small terms; columns >= 64 of de3 hold junk the op must not read into the result."""
    rs = np.random.RandomState(seed)
    e3 = rs.standard_normal((B, HW8, 64)).astype(np.float32)
    e3[rs.random_sample(e3.shape) < 0.25] = 0.0
    de3 = rs.standard_normal((B, HW8, ldd3)).astype(np.float32)
    if mixed:
        big = rs.random_sample(de3.shape) < 0.5
        de3 = (de3 * np.where(big, 1e4, 1e-3)).astype(np.float32)
    de3[:, :, 64:] = 1e30
    w3 = (rs.standard_normal((74, 64)) / 8.0).astype(np.float32)
    wcs = (rs.standard_normal((5, 10)) / 3.0).astype(np.float32)
    dsnew = rs.standard_normal((B, 5)).astype(np.float32)
    return dict(e3=e3, de3=de3, w3=w3, wcs=wcs, dsnew=dsnew)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
# name -> (model kwargs of TorchModel / pivp_amd.Model, init_params kwargs, num_masks, T, batch seed).  B = 2 everywhere.  The batch seeds are the first
# of 0, 1, 2, ... at which plain float32 autograd of the restatement is itself inside the tests' 2e-3 gate against float64 (so that no ReLU unit within
# fp32 rounding of zero decides the comparison); the scan is `python tests/input_grad_reference.py`.  Float32 against float64 there: CDNA / DNA 1e-7 ..
# 4e-5.  STP on white-noise frames is ill-conditioned (the sampler's gradient is an image difference): seeds 0, 3, 4, 8 are OUTSIDE in plain float32
# (3e-3 .. 2.6e-2), seeds 1, 2, 5, 6, 7 inside (6e-4 .. 1.6e-3); the case takes seed 6, the one with the smallest float32 error (7e-4).
MODEL_CASES = {
    'cdna_T3': (dict(), dict(), 10, 3, 0),
    'cdna_T5': (dict(), dict(), 10, 5, 0),
    'stp_T4': (dict(is_cdna=False, is_stp=True), dict(model_type='STP'), 10, 4, 6),
    'dna_T4': (dict(is_cdna=False, is_dna=True), dict(model_type='DNA', num_masks=1), 1, 4, 0),
    'nostate_T3': (dict(use_state=False), dict(use_state=False), 10, 3, 0),
    'ctx3_T5': (dict(num_frame_before_prediction=3), dict(), 10, 5, 0),
}
L1_CASE = 'cdna_T3'      # the seed-hook test: the cost is a torch L1 of gen_images[ctx-1:] to l1_target(), alone


def case_inputs(name, seed=None):
    mkw, pkw, nm, T, bseed = MODEL_CASES[name]
    P = R.init_params_widened(seed=1, scale=1.0, **pkw)
    imgs, acts, stas = R.synthetic_batch(2, T, seed=bseed if seed is None else seed)
    return mkw, nm, P, imgs, acts, stas


def l1_target(H=64, W=64):
    return np.random.RandomState(7).random_sample((3, H, W)).astype(np.float32)


def l1_cost(gen, target):
    """torch: mean |gen - target| over everything; gen (T-ctx, B, 3, H, W)."""
    return (gen - target).abs().mean()


def input_grads(name, dtype=torch.float64, l1=False, seed=None):
    """-> (d loss / d actions (T, B, 5), d loss / d states (T, B, 5)) as float64 arrays, by autograd through the restatement run in `dtype`.
    l1: the loss is l1_cost of the predicted frames alone instead of the model's own."""
    mkw, nm, P, imgs, acts, stas = case_inputs(name, seed)
    tm = TorchModel(nm, params=P, dtype=dtype, **mkw)
    a = torch.tensor(acts, dtype=dtype, requires_grad=True)
    s = torch.tensor(stas, dtype=dtype, requires_grad=True)
    loss = tm([torch.tensor(imgs, dtype=dtype), a, s], 0)
    if l1:
        loss = l1_cost(torch.stack(tm.gen_images[tm.ctx - 1:]), torch.tensor(l1_target(), dtype=dtype))
    loss.backward()
    zero = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.double().numpy()
    return zero(a), zero(s)


def rel_errors(got, ref):
    """(relative L2 error, largest element error relative to max |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300), np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300)


if __name__ == '__main__':      # the seed scan: float32 against float64 autograd on the CPU, per case and batch seed
    import sys
    names = sys.argv[1:] or list(MODEL_CASES) + ['l1']
    for name in names:
        l1 = name == 'l1'
        case = L1_CASE if l1 else name
        T = MODEL_CASES[case][3]
        for seed in range(9):
            a64, s64 = input_grads(case, torch.float64, l1, seed)
            a32, s32 = input_grads(case, torch.float32, l1, seed)
            ea, es = rel_errors(a32[:T - 1], a64[:T - 1]), rel_errors(s32[0], s64[0])
            ok = max(ea + es) < 2e-3
            print('%-11s seed %d  actions rel L2 %.2e max %.2e   state0 rel L2 %.2e max %.2e   %s' % (name, seed, ea[0], ea[1], es[0], es[1], 'inside' if ok else 'OUTSIDE'),
                  flush=True)
            if ok and case != 'stp_T4':      # (STP: every seed is listed)
                break
