"""The backward sweep as a whole, held to fp32 accuracy: HIP BPTT against float64 autograd of the torch restatement DIFFERENTIATED ON THE BRANCH THE DEVICE
TOOK.  The model-level tests elsewhere (test_gpu_train.py, test_gpu_train_shapes.py, ...) gate at 2e-3 .. 5e-3 because one ReLU unit within rounding of zero
is masked differently in fp32 and in float64 (train_reference._check_grads).  Here the oracle's ReLUs at enc0 .. enc7 are forced to the masks read from the
device's own activations, so a flip there cannot enter the comparison, and the gate is M = 10 times what the same oracle run in float32 loses against float64
on that branch (train_reference._check_grads_tight: every tensor, relative L2 and largest element, no percentile, no outliers): about 2e-5 where the wide
gate has 2e-3.  The mask logits, the CDNA / DNA kernel shift and STP's hidden layer have no exact tap and keep the oracle's own ReLU; the parameter seeds
below are those at which the float32 and the float64 oracle, unforced, agree on every unit of every site (tests/test_train_tight_host.py recomputes the
condition for the small cases; `python tests/test_gpu_train_tight.py` prints it for all of them).

Per-tensor factors above M = 10 (each needs a one-line reason; none may exceed 50):
  (none: no tensor of any case came within a fifth of the gate)

Observed on the MI355X: the worst ratio of a tensor's error to e32 per case, the larger of two runs, where the gate is 10 (OBSERVED below holds the same
figures as data; two sweeps of one case differ by a few tenths, the weight gradients' fp32 atomics).  e32 itself: relative L2 0.9e-6 .. 2.5e-6, 1.8e-5 for
STP 16 x 16.
  cdna_16x16 1.28 (enc1/b)                cdna_24x32 0.85 (current_state/W)          cdna_24x40_nm7_b3 0.91 (hidden3/norm/gamma)
  cdna_16x16_nm4 1.17 (current_state/W)   cdna_16x16_nm1 1.51 (lstm4/conv/b)         cdna_16x16_ctx1 1.60 (lstm1/conv/b)
  cdna_16x16_ctx3_t5 1.10 (current_state/W)   stp_16x16 0.67 (enc2/b)                stp_40x24_nm2_b3 0.89 (lstm2/conv/b)
  dna_16x16 1.36 (current_state/W)        dna_32x96 1.18 (hidden7/norm/gamma)        cdna_16x16_schedsamp 1.18 (hidden1/norm/gamma)
  cdna_64x64 1.55 (current_state/W)       cdna_64x64_deterministic 1.89 (current_state/W)
  cdna_64x64_bf16x6 1.01 (current_state/b)      cdna_64x64_fp16x3 0.99 (hidden1/norm/gamma)
  cdna_16x16_t5_wgrad_batch0 0.78 (current_state/W)   cdna_16x16_t5_wgrad_batch3 0.84 (current_state/W)
  input gradients: cdna_16x16 1.44 (lstm1/conv/b), stp_16x16 1.02 (d actions)        carried state, cdna_16x16: 1.51 (d actions)
Tapped units the device had on the other side of zero from the float64 oracle: one, in stp_40x24_nm2_b3 (of 622080); the forced mask took it out.
Parameter seeds changed because of a flip: cdna_24x32 went from 3 to 4 before its first gated device run, for the float32 ORACLE's flip on one kind of host
(the comment above CASES); none was changed for a flip on the device or at an untapped site.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the seed scan at the bottom)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import restatement as R  # noqa: E402
import train_reference as TR  # noqa: E402
import state_grad_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

HEAD_KW = {'CDNA': dict(is_cdna=True), 'STP': dict(is_cdna=False, is_stp=True), 'DNA': dict(is_cdna=False, is_dna=True)}
UNFORCED_E32_L2 = {'CDNA': 1e-5, 'DNA': 1e-5, 'STP': 5e-5}      # the seed condition: unforced float32 against float64, worst tensor, beside equal zero patterns

# name -> (head, H, W, num_masks, B, T, parameter seed, oracle / Model kwargs, Model-only kwargs).  The parameter seed is the first of 1, 2, 3, ... that meets the
# seed condition on the CPU (seeds passed over: 24 x 32 seeds 1, 2, 3; DNA 16 x 16 seed 1; scheduled sampling seeds 1, 2 -- one or two units flip in float32).
# CPU torch in float32 rounds differently from one processor to the next: 24 x 32 at seed 3 is clean on one host and has one enc6 unit (-1.3e-6 in float64,
# +2.6e-7 in float32) on the other side on another, so the condition is checked on both kinds of host the suite runs on.  The GPU tests do not lean on it
# alone: a float32 oracle that flips at an untapped site would WIDEN the gate, so they also hold the forced e32 L2 itself to UNFORCED_E32_L2.
# Batches: R.synthetic_batch, R.smooth_batch for STP, batch seed 0.
CASES = {
    'cdna_16x16': ('CDNA', 16, 16, 10, 2, 4, 1, {}, {}),      # ctx 2, T 4: the last step is fed its own prediction, gradients flow through a frame
    'cdna_24x32': ('CDNA', 24, 32, 10, 2, 4, 4, {}, {}),
    'cdna_24x40_nm7_b3': ('CDNA', 24, 40, 7, 3, 4, 1, {}, {}),
    'cdna_16x16_nm4': ('CDNA', 16, 16, 4, 2, 4, 1, {}, {}),
    'cdna_16x16_nm1': ('CDNA', 16, 16, 1, 2, 4, 1, {}, {}),
    'cdna_16x16_ctx1': ('CDNA', 16, 16, 10, 2, 4, 1, dict(num_frame_before_prediction=1), {}),
    'cdna_16x16_ctx3_t5': ('CDNA', 16, 16, 10, 2, 5, 1, dict(num_frame_before_prediction=3), {}),
    'stp_16x16': ('STP', 16, 16, 10, 2, 4, 1, {}, {}),
    'stp_40x24_nm2_b3': ('STP', 40, 24, 2, 3, 3, 1, {}, {}),
    'dna_16x16': ('DNA', 16, 16, 1, 2, 4, 2, {}, {}),
    'dna_32x96': ('DNA', 32, 96, 1, 2, 4, 1, {}, {}),
    'cdna_16x16_schedsamp': ('CDNA', 16, 16, 10, 4, 5, 3, dict(scheduled_sampling_k=2.0), {}),
    # 64 x 64: maps of 32, 16 and 8 rows, where the two fp32-grade split modes run their packed kernels; same M, same rules
    'cdna_64x64': ('CDNA', 64, 64, 10, 2, 3, 1, {}, {}),
    'cdna_64x64_deterministic': ('CDNA', 64, 64, 10, 2, 3, 1, {}, dict(deterministic=True)),
    'cdna_64x64_bf16x6': ('CDNA', 64, 64, 10, 2, 3, 1, {}, dict(precision='bf16x6')),
    'cdna_64x64_fp16x3': ('CDNA', 64, 64, 10, 2, 3, 1, {}, dict(precision='fp16x3')),
    # the dG rings and the batches of the ConvLSTM weight gradients: 4 steps in batches [3, 2, 1] [0] and one launch per step
    'cdna_16x16_t5_wgrad_batch0': ('CDNA', 16, 16, 10, 2, 5, 1, {}, dict(plan_options={'wgrad_batch': 0})),
    'cdna_16x16_t5_wgrad_batch3': ('CDNA', 16, 16, 10, 2, 5, 1, {}, dict(plan_options={'wgrad_batch': 3})),
}
INPUT_GRAD_CASES = ('cdna_16x16', 'stp_16x16')
CARRIED_CASE = 'cdna_16x16'      # two windows of 3 frames (2 steps each) cut out of one batch of 6, window 2 swept from the state window 1 left
SCHEDSAMP_ITER, SCHEDSAMP_RNG = 1.0, 5      # as test_gpu_train.py::test_bptt_gradients_scheduled_sampling_detaches_frames

FACTORS = {}      # case -> {tensor: factor <= 50}: the table in the docstring, as data

# Worst ratio to e32 per case as measured on the MI355X, for the record (the tests print the current one)
OBSERVED = {'cdna_16x16': 1.28, 'cdna_24x32': 0.85, 'cdna_24x40_nm7_b3': 0.91, 'cdna_16x16_nm4': 1.17, 'cdna_16x16_nm1': 1.51, 'cdna_16x16_ctx1': 1.60,
            'cdna_16x16_ctx3_t5': 1.10, 'stp_16x16': 0.67, 'stp_40x24_nm2_b3': 0.89, 'dna_16x16': 1.36, 'dna_32x96': 1.18, 'cdna_16x16_schedsamp': 1.18,
            'cdna_64x64': 1.55, 'cdna_64x64_deterministic': 1.89, 'cdna_64x64_bf16x6': 1.01, 'cdna_64x64_fp16x3': 0.99,
            'cdna_16x16_t5_wgrad_batch0': 0.78, 'cdna_16x16_t5_wgrad_batch3': 0.84,
            'input gradients cdna_16x16': 1.44, 'input gradients stp_16x16': 1.02, 'carried state cdna_16x16': 1.51}


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def case_inputs(name, T=None):
    head, H, W, nm, B, T0, seed, okw, _ = CASES[name]
    P = R.init_params_widened(seed=seed, scale=1.0, num_masks=nm, model_type=head, height=H, width=W)
    batch = (R.smooth_batch if head == 'STP' else R.synthetic_batch)(B, T or T0, H, W)
    return P, batch


def oracle_kwargs(name):
    """the keyword arguments of train_reference._oracle_pass for a case"""
    head, _, _, nm, _, _, _, okw, _ = CASES[name]
    kw = dict(num_masks=nm, **HEAD_KW[head])
    okw = dict(okw)
    if 'scheduled_sampling_k' in okw:
        kw.update(k=okw.pop('scheduled_sampling_k'), it=SCHEDSAMP_ITER, seed=SCHEDSAMP_RNG)
    kw.update(okw)
    return kw


def seed_condition(name):
    """-> (units on different sides of zero in the unforced float32 and float64 oracle, all sites; unforced e32 L2; its bound)"""
    P, batch = case_inputs(name)
    kw = oracle_kwargs(name)
    tm64, _, g64, _ = TR._oracle_pass(P, batch, dtype=torch.float64, record=True, **kw)
    tm32, _, g32, _ = TR._oracle_pass(P, batch, dtype=torch.float32, record=True, **kw)
    assert set(tm64.pre) == set(tm32.pre)
    flips = sum(int(((tm64.pre[key] > 0) != (tm32.pre[key] > 0)).sum()) for key in tm64.pre)
    return flips, TR._e32(g64, g32)[0], UNFORCED_E32_L2[CASES[name][0]]


def _model(pivp, name, **extra):
    head, _, _, nm, _, _, _, okw, mkw = CASES[name]
    m = pivp.Model(nm, prefix='t', keep_activations=True, **dict(HEAD_KW[head], **dict(okw, **dict(mkw, **extra))))
    m.load_state_dict_reference(case_inputs(name)[0])
    return m


def _forward(pivp, m, name, batch):
    if 'scheduled_sampling_k' in CASES[name][7]:
        np.random.seed(SCHEDSAMP_RNG)
    with pivp.using_config('train', True):
        return float(m(list(batch), SCHEDSAMP_ITER if 'scheduled_sampling_k' in CASES[name][7] else 0))


def _check_taps(m, masks, pre, steps, step0=0):
    """The taps the masks were read from are the oracle's post-ReLU activations on the forced branch -- enc7 included, which is only assumed to be tapped
    behind its ReLU: within 1e-3 (a pre-ReLU tensor would be off by the size of its negative entries, 0.1 .. 1)."""
    for site in TR._tapped_sites(m.model_type):
        for st in range(steps):
            want = np.where(masks[(site, step0 + st)], pre[(site, step0 + st)].numpy(), 0.0)
            err = np.abs(m.tap(site, st).cpu().numpy() - want).max()
            assert err < 1e-3, 'tap %s of step %d differs from the oracle on the same branch by %.2e' % (site, st, err)


def _report_and_check(name, what, got, ref64, ref32, tm64):
    near = TR._near_zero_untapped(tm64.pre)
    try:
        e32_l2 = TR._e32(ref64, ref32)[0]
        assert e32_l2 <= UNFORCED_E32_L2[CASES[name][0]], 'the yardstick is off: the float32 oracle is %.2e from float64 on the forced branch' % e32_l2
        worst = TR._check_grads_tight(got, ref64, ref32, FACTORS.get(name))
    except AssertionError:
        print('%s %s: outside the tight gate; oracle units at untapped sites with |pre-activation| < 1e-5: %d (a flip there moves everything in its footprint by '
              '~1e-3; a fault does not need one)' % (name, what, near))
        raise
    print('%s %s: worst ratio to e32 %.2f (%s); untapped units within 1e-5 of zero: %d' % (name, what, worst[0], worst[1], near))
    return worst


def _run_case(pivp, name, input_grad=False):
    head, H, W, nm, B, T, seed, okw, mkw = CASES[name]
    P, batch = case_inputs(name)
    kw = oracle_kwargs(name)
    m = _model(pivp, name)
    loss = _forward(pivp, m, name, batch)                                                  # 1. the HIP forward
    masks, ndiff = TR._device_relu_masks(m, T - 1, TR._oracle_preactivations(P, batch, **kw))      # 2. the branch it took
    print('%s: %d of %d tapped ReLU units on the other side of zero in the float64 oracle' % (name, ndiff, sum(v.size for v in masks.values())))
    tm64, loss64, g64, in64 = TR._oracle_pass(P, batch, masks=masks, dtype=torch.float64, record=True, wrt_inputs=input_grad, **kw)      # 3. the oracle on it
    _, _, g32, in32 = TR._oracle_pass(P, batch, masks=masks, dtype=torch.float32, wrt_inputs=input_grad, **kw)
    _check_taps(m, masks, tm64.pre, T - 1)
    m.cleargrads()
    with pivp.using_config('train', True):
        m.backward(input_grad=input_grad)                                                  # 4. the HIP backward
    got = m.grads_reference()
    if input_grad:      # d loss / d actions[:T-1] and d loss / d states[0] join the case's tensors (actions[T-1] and states[1:] as inputs get none)
        got['d actions'], got['d state0'] = m.action_grad.cpu().numpy(), m.state_grad.cpu().numpy()
        for g, (da, ds) in ((g64, in64), (g32, in32)):
            g['d actions'], g['d state0'] = da[:T - 1], ds[0]
    worst = _report_and_check(name, 'parameters' + (' and inputs' if input_grad else ''), got, g64, g32, tm64)      # 5.
    print('%s: loss hip %.9f oracle %.9f' % (name, loss, loss64))
    assert abs(loss - loss64) < 1e-6                                                       # 6.
    return m, got, g64, worst


@pytest.mark.parametrize('name', list(CASES))
def test_sweep_gradients_within_ten_float32_errors(pivp, name):
    m, got, g64, _ = _run_case(pivp, name)
    head, nm = CASES[name][0], CASES[name][3]
    if head == 'CDNA' and nm > 1:      # the last CDNA kernel never reaches the output (TM:726)
        assert not np.any(got['model/cdna_kerns/W'][25 * (nm - 1):]) and not np.any(got['model/cdna_kerns/b'][25 * (nm - 1):])
    for key, want in CASES[name][8].get('plan_options', {}).items():
        assert want == 0 or m.effective_plan_options()[key] == want      # (0 asks for the precision mode's own batch)
    if 'precision' in CASES[name][8]:
        assert m._active.lib.pivp_plan_get_precision(m._active.h) == {'bf16x6': 3, 'fp16x3': 4}[CASES[name][8]['precision']]


@pytest.mark.parametrize('name', INPUT_GRAD_CASES)
def test_input_gradients_within_ten_float32_errors(pivp, name):
    _, got, g64, _ = _run_case(pivp, name, input_grad=True)
    assert np.any(g64['d actions']) and np.any(g64['d state0'])


def test_carried_state_gradients_within_ten_float32_errors(pivp):
    """Truncated BPTT over a carried ConvLSTM state: window 2's parameter gradients, d loss2 / d (the state it started from) in its fourteen segments, and its
    input gradients.  The oracle's step counter runs on over the two calls, so window 2's masks are those of steps 2 and 3."""
    name = CARRIED_CASE
    head, H, W, nm, B, _, _, _, _ = CASES[name]
    P, (imgs, acts, stas) = case_inputs(name, T=6)
    wins = [[imgs[:3], acts[:3], stas[:3]], [imgs[3:], acts[3:], stas[3:]]]
    kw = oracle_kwargs(name)
    tm = TR._oracle_pass(P, wins[0], record=True, backward=False, **kw)[0]
    TR._oracle_pass(P, wins[1], backward=False, tm=tm)
    pre64 = {key: v.numpy() for key, v in tm.pre.items()}
    m = _model(pivp, name, carry_state=True, state_backward=True)
    m.reset_state()
    masks, ndiff, losses = {}, 0, []
    for w, win in enumerate(wins):
        losses.append(_forward(pivp, m, name, win))
        mk, n = TR._device_relu_masks(m, 2, pre64, step0=2 * w)
        masks.update(mk); ndiff += n
    print('%s carried: %d tapped ReLU units on the other side of zero in the float64 oracle' % (name, ndiff))
    m.cleargrads()
    with pivp.using_config('train', True):
        m.backward(initial_state_grad=True, input_grad=True)
    got = m.grads_reference()
    got['d actions'], got['d state0'] = m.action_grad.cpu().numpy(), m.state_grad.cpu().numpy()
    for g, seg in enumerate(SR.segments(m.initial_state_grad.data.cpu().numpy(), B, H, W)):
        got['d state %s%d' % ('h' if g % 2 else 'c', g // 2 + 1)] = seg
    refs = {}
    for dtype in (torch.float64, torch.float32):
        tm, loss1, _, _ = TR._oracle_pass(P, wins[0], masks=masks, dtype=dtype, record=True, **kw)
        leaves = SR._detach_state(tm)
        _, loss2, g, (da, ds) = TR._oracle_pass(P, wins[1], dtype=dtype, wrt_inputs=True, tm=tm)
        g['d actions'], g['d state0'] = da[:2], ds[0]
        flat = SR.pack_state([tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in pair) for pair in leaves])
        for i, seg in enumerate(SR.segments(flat, B, H, W)):
            g['d state %s%d' % ('h' if i % 2 else 'c', i // 2 + 1)] = seg
        refs[dtype] = (tm, loss1, loss2, g)
    tm64, loss1, loss2, g64 = refs[torch.float64]
    assert all(np.any(g64[k]) for k in g64 if k.startswith('d ')), 'a state or input gradient of the reference is zero: the comparison would mean nothing'
    _report_and_check(name, 'carried state', got, g64, refs[torch.float32][3], tm64)
    assert abs(losses[0] - loss1) < 1e-6 and abs(losses[1] - loss2) < 1e-6


if __name__ == '__main__':      # the seed condition of every committed case, on the CPU
    for name in sys.argv[1:] or list(CASES):
        flips, e, lim = seed_condition(name)
        print('%-28s seed %d  units on different sides of zero %d  unforced e32 L2 %.2e (<= %.0e)  %s' % (name, CASES[name][6], flips, e, lim,
                                                                                                           'ok' if flips == 0 and e <= lim else 'OUTSIDE'), flush=True)
