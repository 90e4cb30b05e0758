"""GPU tests of the guarded Adam step (include/pivp_optim.h): pivp_grad_stats against the float64 restatement (tests/optim_reference.py), its range,
its non-finite detector and its reproducibility; pivp_adam_step_guarded against pivp_adam_step (bit for bit at rate 1), against Chainer's rule on
the clipped gradient, and its skip; the argument checks; and the same through `Adam` on the model."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_reference as OR  # noqa: E402

pytestmark = pytest.mark.gpu

# every norm and the rate against float64: the kernel's sums are fp64 (1e-16 a term), its only fp32 rounding is the output's, 2^-24 = 6e-8: 16 x that
RTOL = 1e-6


def _ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import optim_ops
    return optim_ops


def _forty_ends(n):
    """40 segments of unequal size over n = 64 * G elements: two one-granule segments in front, 37 random cuts, ends on multiples of 64."""
    G = n // 64
    cuts = np.random.RandomState(40).choice(np.arange(3, G), 37, replace=False)
    return [64 * int(c) for c in sorted([1, 2] + cuts.tolist())] + [n]


SHAPES = {
    'one': (1, [1], [0]),
    'odd': (197, [64, 128, 197], [0, 2, 5]),
    'million': (1000003, [64, 4160, 500032, 1000003], [0, 1, 1, 4]),
    # groups 0 .. 5 with group 3 empty
    'forty': (2 ** 23 + 64, _forty_ends(2 ** 23 + 64), [0] * 6 + [1] * 9 + [2] * 5 + [4] * 12 + [5] * 8),
}


@functools.lru_cache(maxsize=None)
def _gradient(name):
    """randn * 10 ** uniform(-3, 3) per segment, write-protected and shared by the tests."""
    n, ends, groups = SHAPES[name]
    assert len(ends) == len(groups) and ends[-1] == n and all(e % 64 == 0 for e in ends[:-1]) and sorted(set(ends)) == ends
    rs = np.random.RandomState(len(ends))
    g = rs.randn(n).astype(np.float32)
    for a, b in OR.segments(ends):
        g[a:b] *= np.float32(10.0 ** rs.uniform(-3, 3))
    g.flags.writeable = False
    return g


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device='cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _worst(got, ref):
    """Largest |got - ref| / ref over all norms and the rate (0 against 0 counts as 0)."""
    pairs = [(got['norm'], ref['norm']), (got['rate'], ref['rate'])] + list(zip(got['group_norms'], ref['group_norms'])) + \
        list(zip(got['seg_norms'], ref['seg_norms']))
    worst = 0.0
    for a, b in pairs:
        a, b = float(a), float(b)
        worst = max(worst, 0.0 if a == b else abs(a - b) / abs(b) if b != 0 else np.inf)
    return worst


@pytest.mark.parametrize('gscale', [1.0, 0.125])
@pytest.mark.parametrize('name', list(SHAPES))
def test_norms_and_rate_match_float64(name, gscale):
    O = _ops()
    n, ends, groups = SHAPES[name]
    g = _gradient(name)
    free = OR.grad_stats(g, ends, groups, gscale=gscale)                 # no clipping: rate 1 exactly
    thr = 0.37 * free['norm']
    ref = OR.grad_stats(g, ends, groups, gscale=gscale, threshold=thr)
    gd = _dev(g)
    got0 = O.grad_stats(gd, ends, groups, gscale=gscale)
    got = O.grad_stats(gd, ends, groups, gscale=gscale, threshold=thr)
    w0, w = _worst(got0, free), _worst(got, ref)
    print('%s gscale %g: worst relative error %.3e (no threshold) %.3e (threshold)  norm %.6e rate %.8f' % (name, gscale, w0, w, got['norm'], got['rate']))
    assert got0['rate'] == np.float32(1) and got0['nonfinite'] == 0 and got['nonfinite'] == 0
    assert abs(float(ref['rate']) - 0.37) < 1e-6
    assert w0 <= RTOL and w <= RTOL, 'worst relative error of a norm / the rate: %.3e without, %.3e with a threshold (gate %.0e)' % (w0, w, RTOL)
    assert len(got['group_norms']) == 6 and len(got['seg_norms']) == len(ends)
    for k in set(range(6)) - set(groups):
        assert got['group_norms'][k] == 0                                 # a group without segments
    assert np.array_equal(_bits(got['seg_norms']), _bits(got0['seg_norms']))      # the threshold enters the rate only


@pytest.mark.parametrize('value', [1e30, 1e-30])
def test_magnitudes_whose_squares_leave_float32(value):
    """1e30: the squares overflow fp32, the fp64 sums do not; the flag stays down.  1e-30: the squares underflow fp32 to zero, the norm is not zero."""
    O = _ops()
    n, ends, groups = SHAPES['million']
    g = np.full(n, value, np.float32)
    ref = OR.grad_stats(g, ends, groups)
    got = O.grad_stats(_dev(g), ends, groups)
    w = _worst(got, ref)
    assert got['nonfinite'] == 0 and np.isfinite(got['norm']) and got['norm'] > 0 and got['rate'] == np.float32(1)
    assert abs(float(got['norm']) - float(np.float32(value)) * np.sqrt(n)) <= RTOL * float(got['norm'])
    assert w <= RTOL, 'worst relative error at %g: %.3e' % (value, w)


@pytest.mark.parametrize('name,index,value', [('odd', 0, np.nan), ('odd', 196, np.nan), ('million', 250001, np.inf), ('million', 250001, -np.inf)])
def test_one_non_finite_element_raises_the_flag_in_its_segment_and_group_only(name, index, value):
    O = _ops()
    n, ends, groups = SHAPES[name]
    clean = O.grad_stats(_dev(_gradient(name)), ends, groups, threshold=1.0)
    g = _gradient(name).copy()
    g[index] = value
    got = O.grad_stats(_dev(g), ends, groups, threshold=1.0)
    seg = [i for i, (a, b) in enumerate(OR.segments(ends)) if a <= index < b][0]
    assert clean['nonfinite'] == 0 and got['nonfinite'] == 1 and not np.isfinite(got['norm'])
    assert np.flatnonzero(~np.isfinite(got['seg_norms'])).tolist() == [seg]
    assert np.flatnonzero(~np.isfinite(got['group_norms'])).tolist() == [groups[seg]]
    others = [i for i in range(len(ends)) if i != seg]
    assert np.array_equal(_bits(got['seg_norms'][others]), _bits(clean['seg_norms'][others]))
    other_groups = [k for k in range(6) if k != groups[seg]]
    assert np.array_equal(_bits(got['group_norms'][other_groups]), _bits(clean['group_norms'][other_groups]))
    ref = OR.grad_stats(g, ends, groups, threshold=1.0)
    assert ref['nonfinite'] == 1 and float(got['rate']) == float(ref['rate'])      # NaN norm: rate 1; infinite norm: Chainer's rule gives 0


def test_same_bytes_give_the_same_bits():
    O = _ops()
    n, ends, groups = SHAPES['forty']
    gd = _dev(_gradient('forty'))
    a = O.grad_stats(gd, ends, groups, gscale=0.125, threshold=3.0)['raw']
    b = O.grad_stats(gd, ends, groups, gscale=0.125, threshold=3.0)['raw']      # (another workspace, another statistics buffer)
    c = O.grad_stats(gd.clone(), ends, groups, gscale=0.125, threshold=3.0)['raw']
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def _start(n, seed):
    rs = np.random.RandomState(seed)
    p = rs.uniform(-1, 1, n).astype(np.float32)
    grads = [(rs.randn(n) * 10.0 ** rs.uniform(-4, 1, n)).astype(np.float32) for _ in range(3)]
    return p, grads


@pytest.mark.parametrize('gscale', [1.0, 1.0 / 3.0])
def test_guarded_adam_at_rate_one_is_adam_bit_for_bit(gscale):
    """No clipping, finite gradients, three steps on n = 1,000,003: p, m and v equal three pivp_adam_step calls from the same start."""
    O = _ops()
    n, ends, groups = SHAPES['million']
    p0, grads = _start(n, 5)
    pa, ma, va = _dev(p0), torch.zeros(n, device='cuda:0'), torch.zeros(n, device='cuda:0')
    pb, mb, vb = _dev(p0), torch.zeros(n, device='cuda:0'), torch.zeros(n, device='cuda:0')
    lib = O._lib.load()
    ws = torch.empty(lib.pivp_grad_stats_ws_bytes(n, len(ends)) // 8, dtype=torch.float64, device='cuda:0')
    stats = torch.zeros(3 + 6 + len(ends), device='cuda:0')
    se, sg = O.tables(ends, groups)
    for t, g in enumerate(grads):
        gd = _dev(g)
        O.adam_plain(pa, gd, ma, va, t + 1, gscale=gscale)
        O._lib.check(lib.pivp_grad_stats(gd.data_ptr(), n, se.data_ptr(), sg.data_ptr(), len(ends), 6, gscale, 0.0, ws.data_ptr(), stats.data_ptr(),
                                         O.stream()), 'pivp_grad_stats')
        assert O.adam_guarded_rc(pb, gd, mb, vb, stats, t + 1, gscale=gscale) == 0       # skip_nonfinite = 0: no counter needed
        assert float(stats[1]) == 1.0 and float(stats[2]) == 0.0
    for a, b in ((pa, pb), (ma, mb), (va, vb)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(pa, _dev(p0))


def test_clipped_step_matches_chainers_rule_on_the_clipped_gradient():
    """Threshold = 0.1 x the measured norm of the first gradient, two steps.  |p| <= 1 and alpha = 1e-3: float32 parameters carry ~1e-7 of rounding
    over two steps, the step itself ~1e-9 (the argument of test_adam_update_matches_chainer_rule): 1e-6 absolute."""
    O = _ops()
    n, ends, groups = SHAPES['million']
    p0, grads = _start(n, 6)
    grads = grads[:2]
    gds = [_dev(g) for g in grads]
    measured = float(O.grad_stats(gds[0], ends, groups)['norm'])
    thr = 0.1 * measured
    p, m, v = _dev(p0), torch.zeros(n, device='cuda:0'), torch.zeros(n, device='cuda:0')
    rates = []
    for t, gd in enumerate(gds):
        rc, raw = O.grad_stats_rc(gd, ends, groups, threshold=thr)
        assert rc == 0
        ref = OR.grad_stats(grads[t], ends, groups, threshold=thr)
        assert float(ref['rate']) < 0.2 and abs(float(raw[1]) - float(ref['rate'])) <= RTOL * float(ref['rate'])
        rates.append(ref['rate'])
        assert O.adam_guarded_rc(p, gd, m, v, _dev(raw), t + 1) == 0
    pr, mr, vr = OR.guarded_adam_steps(p0, grads, rates)
    err = np.abs(p.cpu().numpy().astype(np.float64) - pr).max()
    print('clipped: rates %s  max |p - float64 rule| %.3e' % ([float(r) for r in rates], err))
    assert err < 1e-6, 'update differs from the rule applied to the clipped gradient by %.2e' % err
    # and the clip is really in there: the unclipped rule lands elsewhere in m
    assert np.abs(m.cpu().numpy() - mr).max() <= 1e-6 * np.abs(mr).max() and np.abs(mr).max() < 0.5 * np.abs(OR.guarded_adam_steps(p0, grads, [1, 1])[1]).max()


def test_skip_nonfinite_keeps_every_bit_and_counts():
    O = _ops()
    n, ends, groups = SHAPES['odd']
    rs = np.random.RandomState(9)
    p0, m0, v0 = rs.uniform(-1, 1, n).astype(np.float32), rs.randn(n).astype(np.float32) * 0.1, rs.rand(n).astype(np.float32)
    g = _gradient('odd').copy()
    g[100] = np.nan
    p, m, v = _dev(p0), _dev(m0), _dev(v0)
    skipped = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    rc, raw = O.grad_stats_rc(_dev(g), ends, groups, threshold=1.0)
    assert rc == 0 and raw[2] == 1
    assert O.adam_guarded_rc(p, _dev(g), m, v, _dev(raw), 1, skip_nonfinite=1, skipped=skipped) == 0
    for t, a in ((p, p0), (m, m0), (v, v0)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
    assert int(skipped.item()) == 1
    # a clean step afterwards is applied -- the plain step's bits -- and the counter stays
    clean = _dev(_gradient('odd'))
    rc, raw = O.grad_stats_rc(clean, ends, groups)
    assert rc == 0 and raw[2] == 0 and raw[1] == 1
    assert O.adam_guarded_rc(p, clean, m, v, _dev(raw), 2, skip_nonfinite=1, skipped=skipped) == 0
    pp, mp, vp = _dev(p0), _dev(m0), _dev(v0)
    O.adam_plain(pp, clean, mp, vp, 2)
    assert torch.equal(p.view(torch.int32), pp.view(torch.int32)) and torch.equal(m.view(torch.int32), mp.view(torch.int32))
    assert torch.equal(v.view(torch.int32), vp.view(torch.int32)) and not np.array_equal(p.cpu().numpy(), p0)
    assert int(skipped.item()) == 1
    # skip_nonfinite = 0 is Chainer's behaviour: the NaN reaches the parameter it belongs to (and only that one: the norm is NaN, the rate 1)
    p, m, v = _dev(p0), _dev(m0), _dev(v0)
    rc, raw = O.grad_stats_rc(_dev(g), ends, groups, threshold=1.0)
    assert raw[1] == 1 and O.adam_guarded_rc(p, _dev(g), m, v, _dev(raw), 1, skip_nonfinite=0, skipped=skipped) == 0
    bad = np.isnan(p.cpu().numpy())
    assert bad[100] and bad.sum() == 1 and np.isnan(m.cpu().numpy()[100]) and np.isnan(v.cpu().numpy()[100]) and int(skipped.item()) == 1


def test_bad_arguments_return_badarg_and_touch_nothing():
    O = _ops()
    n, ends, groups = SHAPES['odd']
    gd = _dev(_gradient('odd'))
    cases = [dict(null=[k]) for k in ('g', 'seg_end', 'seg_group', 'ws', 'stats')]                  # null pointers
    cases += [dict(n=0), dict(n=-1)]                                                                  # n < 1
    cases += [dict(nseg=0), dict(nseg=-3), dict(nseg=O._lib.OPTIM_MAX_SEGMENTS + 1)]                  # nseg < 1 or above the cap
    cases += [dict(ngroups=0), dict(ngroups=7), dict(ngroups=-1)]                                     # ngroups outside 1 .. PIVP_GRAD_GROUPS
    for kw in cases:
        rc, raw = O.grad_stats_rc(gd, ends, groups, **kw)
        assert rc == -1 and len(raw) >= 3 + len(ends) and (raw == O.FILL).all(), kw
    for gscale in (np.inf, np.nan):
        rc, raw = O.grad_stats_rc(gd, ends, groups, gscale=gscale)
        assert rc == -1 and (raw == O.FILL).all()
    rc, raw = O.grad_stats_rc(torch.zeros(n + 1, device='cuda:0')[1:], ends, groups)                  # g off 16 bytes
    assert rc == -1 and (raw == O.FILL).all()
    rc, raw = O.grad_stats_rc(gd, ends, groups, ngroups=1, gscale=1.0)                               # ... and the smallest good ngroups is served
    assert rc == 0 and raw[0] > 0
    # the guarded step
    rs = np.random.RandomState(2)
    p0, m0, v0 = rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)
    p, m, v = _dev(p0), _dev(m0), _dev(v0)
    skipped = torch.full((1,), 5, dtype=torch.int32, device='cuda:0')
    for nonfinite in (0.0, 1.0):
        stats = O.stats_buffer(0.5, nonfinite)
        for kw in [dict(null=[k]) for k in ('p', 'g', 'm', 'v', 'stats')] + [dict(n=0), dict(n=-7), dict(skip_nonfinite=2), dict(skip_nonfinite=-1)]:
            assert O.adam_guarded_rc(p, gd, m, v, stats, 1, skipped=skipped, **kw) == -1, kw
        assert O.adam_guarded_rc(p, gd, m, v, stats, 1, skip_nonfinite=1, skipped=None) == -1          # nowhere to count
    for t, a in ((p, p0), (m, m0), (v, v0)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
    assert int(skipped.item()) == 5


# ---- through the model: B = 2, T = 4, CDNA ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


@pytest.fixture(scope='module')
def start():
    return R.init_params_widened(seed=1), list(R.synthetic_batch(2, 4))


def _model(pivp, P):
    m = pivp.Model(10, prefix='g', keep_activations=True, deterministic=True)
    m.load_state_dict_reference(P)
    return m


@pytest.fixture(scope='module')
def tracked(pivp, start):
    """One update of Adam(track_grad_norm=True) from the common start: (model, optimizer); the tests that read it leave it unchanged."""
    P, x = start
    m = _model(pivp, P)
    opt = pivp.Adam(alpha=0.001, track_grad_norm=True).setup(m)
    opt.update(m, x, 0)
    m.reset_state()
    torch.cuda.synchronize()
    return m, opt


def _norm64(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    return float(np.sqrt(np.sum(a * a)))


def test_model_norms_are_those_of_the_checkpoint_layout_gradients(tracked):
    """The flat buffer's norms against the float64 norms of grads_reference(): padding and the internal layouts add nothing."""
    m, opt = tracked
    gref = m.grads_reference()
    total = np.sqrt(sum(_norm64(g) ** 2 for g in gref.values()))
    for t in (opt.grad_norm, opt.clip_rate, opt.grad_nonfinite):
        assert t.is_cuda and t.dim() == 0 and t.dtype == torch.float32
    worst = abs(float(opt.grad_norm) - total) / total
    norms = opt.param_norms()
    assert list(norms) == list(gref) and total > 0
    for k, g in gref.items():
        assert norms[k].is_cuda and norms[k].dim() == 0
        want = _norm64(g)
        worst = max(worst, abs(float(norms[k]) - want) / want if want else float(norms[k]))
    assert opt.group_norms.is_cuda and tuple(opt.group_norms.shape) == (6,)
    flat = m._flat_grads.cpu().numpy()
    ranges = m.grad_group_ranges()
    assert len(ranges) == 6
    for k, (a, b) in enumerate(ranges):
        want = _norm64(flat[a:b])
        worst = max(worst, abs(float(opt.group_norms[k]) - want) / want)
    print('model: grad norm %.6e, worst relative error of a norm %.3e' % (float(opt.grad_norm), worst))
    assert worst <= RTOL, 'worst relative error of a norm through the model: %.3e' % worst
    assert float(opt.clip_rate) == 1.0 and float(opt.grad_nonfinite) == 0.0 and opt.skipped_steps == 0 and opt.t == 1


def test_tracking_leaves_the_update_bit_identical(pivp, start):
    P, x = start
    out = []
    for kw in (dict(), dict(track_grad_norm=True)):
        m = _model(pivp, P)
        opt = pivp.Adam(alpha=0.001, **kw).setup(m)
        for itr in range(2):
            opt.update(m, x, itr)
            m.reset_state()
        torch.cuda.synchronize()
        out.append((m._flat_params.clone(), opt._m.clone(), opt._v.clone()))
        assert (opt.grad_norm is not None) == bool(kw)
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_clipping_hook_halves_the_first_step(pivp, start, tracked):
    P, x = start
    norm1 = float(tracked[1].grad_norm)
    m = _model(pivp, P)
    opt = pivp.Adam(alpha=0.001).setup(m)
    opt.add_hook(pivp.GradientClipping(0.5 * norm1))
    opt.update(m, x, 0)
    assert abs(float(opt.clip_rate) - 0.5) <= RTOL and float(opt.grad_norm) == norm1 and float(opt.grad_nonfinite) == 0.0
    # the clipped update is another update than the plain one
    assert not torch.equal(opt._m, tracked[1]._m) and torch.allclose(opt._m, 0.5 * tracked[1]._m, rtol=1e-5, atol=0)


def test_inf_in_the_flat_gradient_is_skipped(pivp, start):
    P, x = start
    m = _model(pivp, P)
    opt = pivp.Adam(alpha=0.001, skip_nonfinite=True).setup(m)
    m(x, 0)
    m.cleargrads()
    m.backward()
    m._flat_grads[123457] = float('inf')
    before = m._flat_params.clone()
    opt.step()
    assert torch.equal(m._flat_params.view(torch.int32), before.view(torch.int32))
    assert not opt._m.any() and not opt._v.any()
    assert opt.skipped_steps == 1 and opt.t == 1 and float(opt.grad_nonfinite) == 1.0 and not np.isfinite(float(opt.grad_norm))
    bad = [k for k, t in opt.param_norms().items() if not np.isfinite(float(t))]
    assert len(bad) == 1
    o, n = m._offsets[bad[0]]
    assert o <= 123457 < o + (n + 63) // 64 * 64                          # the readout names the tensor that blew up


def test_guarded_update_never_synchronises(pivp, start):
    P, x = start
    m = _model(pivp, P)
    opt = pivp.Adam(alpha=0.001, skip_nonfinite=True, track_grad_norm=True).setup(m)
    opt.add_hook(pivp.GradientClipping(1.0))
    xd = [torch.tensor(np.asarray(a, dtype=np.float32), device='cuda:0') for a in x]
    opt.update(m, xd, 0)                       # plans, tables and buffers are made once, in front of the loop
    m.reset_state()
    probe = torch.ones(1, device='cuda:0')
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        opt.update(m, xd, 1)
        norm, rate, flag, groups, per = opt.grad_norm, opt.clip_rate, opt.grad_nonfinite, opt.group_norms, opt.param_norms()
        m.reset_state()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert detects, 'torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made'
    assert opt.skipped_steps == 0 and opt.t == 2 and float(norm) > 0 and 0 < float(rate) <= 1 and float(flag) == 0 and len(per) == len(P)
