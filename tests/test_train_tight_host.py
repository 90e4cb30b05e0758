"""Host tests of the tight gradient gate (tests/test_gpu_train_tight.py): the oracle's forced ReLU masks change nothing when they are its own, the committed
parameter seeds meet the seed condition, and the gate rejects faults the wide one (train_reference._check_grads at 2e-3) lets through.  CPU torch only."""
import numpy as np
import pytest
import torch

from oracle.torch_restatement import TorchModel
import train_reference as TR
from test_gpu_train_tight import CASES, case_inputs, oracle_kwargs, seed_condition


@pytest.mark.parametrize('name', ['cdna_16x16', 'stp_16x16', 'dna_16x16'])
def test_forcing_the_oracles_own_masks_changes_no_bit(name):
    P, batch = case_inputs(name)
    kw = oracle_kwargs(name)
    tm, loss, grads, inputs = TR._oracle_pass(P, batch, record=True, wrt_inputs=True, **kw)
    masks = {key: v.numpy() > 0 for key, v in tm.pre.items()}
    T = CASES[name][5]
    sites = {site for site, _ in masks}
    assert sites == set(TR._tapped_sites(CASES[name][0])) | {'masks'} | {dict(CDNA='kern', STP='s1', DNA='kn')[CASES[name][0]]}
    assert all((site, st) in masks for site in sites for st in range(T - 1)) and len(masks) == len(sites) * (T - 1)
    tmf, lossf, gradsf, inputsf = TR._oracle_pass(P, batch, masks=masks, record=True, wrt_inputs=True, **kw)
    assert lossf == loss
    for k in grads:
        assert np.array_equal(gradsf[k], grads[k]), k
    assert np.array_equal(inputsf[0], inputs[0]) and np.array_equal(inputsf[1], inputs[1])
    assert all(torch.equal(tmf.pre[key], tm.pre[key]) for key in tm.pre)
    # ... and a mask that is not the oracle's own is obeyed: one more open unit of enc3 at step 1 moves loss and gradients
    key = ('enc3', 1)
    flat = np.flatnonzero(~masks[key].ravel())
    assert flat.size
    forced = dict(masks)
    forced[key] = masks[key].copy()
    forced[key].ravel()[flat[np.argmin(tm.pre[key].numpy().ravel()[flat])]] = True      # the most negative unit
    loss2, grads2 = TR._autograd_masked(P, batch, forced, torch.float64, **kw)
    assert loss2 != loss and not np.array_equal(grads2['enc3/W'], grads['enc3/W'])
    # sites absent from the dict keep their own ReLU
    part = {k: v for k, v in masks.items() if k[0] in ('enc0', 'enc5')}
    loss3, grads3 = TR._autograd_masked(P, batch, part, torch.float64, **kw)
    assert loss3 == loss and all(np.array_equal(grads3[k], grads[k]) for k in grads)


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if (c[1], c[2]) in ((16, 16), (24, 32))])
def test_committed_seeds_meet_the_seed_condition(name):
    flips, e32_l2, bound = seed_condition(name)
    print('%s: units on different sides of zero %d, unforced e32 L2 %.2e (bound %.0e)' % (name, flips, e32_l2, bound))
    assert flips == 0 and e32_l2 <= bound


class _PerStepEnc5(TorchModel):
    """enc5/W of timestep t is W + delta[t] with delta = 0: d loss / d delta[t] is that timestep's contribution to the gradient of enc5/W"""

    def _deconv(self, n, x):
        if n != 'enc5':
            return TorchModel._deconv(self, n, x)
        import torch.nn.functional as F
        return F.conv_transpose2d(x, self.p[n + '/W'] + self.delta[self.step], self.p[n + '/b'], stride=2, padding=1, output_padding=1)


def test_tight_gate_rejects_faults_the_wide_gate_accepts():
    """The float64 gradients of CDNA 16 x 16 with three faults of the kinds a sweep's glue produces, and the float32 oracle's own gradients as the `got` of a
    correct implementation.  The uniform 0.5 % scale of current_state/W has a relative L2 error of 5e-3 by construction, which is above the wide gate's 2e-3:
    _check_grads sees that one, and the claim "the wide gate accepts it" is made for the same fault at 0.1 % instead; the tight gate must reject both."""
    name = 'cdna_16x16'
    P, batch = case_inputs(name)
    kw = oracle_kwargs(name)
    _, g64 = TR._autograd_masked(P, batch, None, torch.float64, **kw)
    _, g32 = TR._autograd_masked(P, batch, None, torch.float32, **kw)
    T1 = CASES[name][5] - 1
    tm = _PerStepEnc5(kw['num_masks'], params=P, requires_grad=True)
    tm.delta = [torch.zeros(tuple(P['enc5/W'].shape), dtype=torch.float64, requires_grad=True) for _ in range(T1)]
    tm(list(batch), 0).backward()
    steps = [d.grad.numpy() for d in tm.delta]
    assert np.allclose(sum(steps), g64['enc5/W'], rtol=0, atol=1e-12 * np.abs(g64['enc5/W']).max()) and all(np.any(s) for s in steps)

    def faulty(key, value):
        g = dict(g64)
        g[key] = value
        return g
    stripe = g64['lstm5/conv/W'].copy()
    stripe.reshape(stripe.shape[0], -1)[:, 64:96] *= 1.0 + 1e-3                                     # one 32-column stripe of the [512][192 * 25] matrix
    faults = {'a 32-column stripe of lstm5/conv/W scaled by 1 + 1e-3': (faulty('lstm5/conv/W', stripe), True),
              'current_state/W scaled by 1.005': (faulty('current_state/W', g64['current_state/W'] * 1.005), False),
              'current_state/W scaled by 1.001': (faulty('current_state/W', g64['current_state/W'] * 1.001), True),
              'one timestep of enc5/W scaled by 0.999': (faulty('enc5/W', g64['enc5/W'] - 1e-3 * steps[1]), True)}
    TR._check_grads(g32, g64, 2e-3)
    worst = TR._check_grads_tight(g32, g64, g32)
    assert worst[0] <= 1.0 + 1e-12      # the float32 oracle is its own yardstick
    for what, (g, wide_accepts) in faults.items():
        if wide_accepts:
            TR._check_grads(g, g64, 2e-3)
        else:
            with pytest.raises(AssertionError, match='current_state/W'):
                TR._check_grads(g, g64, 2e-3)
        with pytest.raises(AssertionError, match='outside the tight gate'):
            TR._check_grads_tight(g, g64, g32)
        print('rejected by the tight gate:', what)
    # a tensor whose float64 gradient is identically zero must be exactly zero
    zero = dict(g64, **{'enc0/b': np.zeros_like(g64['enc0/b'])})
    got = dict(zero, **{'enc0/b': zero['enc0/b'] + 1e-30})
    with pytest.raises(AssertionError, match='identically zero'):
        TR._check_grads_tight(got, zero, dict(g32, **{'enc0/b': zero['enc0/b']}))
    # a per-tensor factor is capped at 50
    with pytest.raises(AssertionError):
        TR._check_grads_tight(g32, g64, g32, factors={'enc5/W': 51.0})
