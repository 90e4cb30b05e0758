"""GPU tests of on-device CEM planning: pivp_plan_cost and pivp_cem_update against the float64 restatement tests/plan_reference.py, and
`planning.cem_plan` end to end on the trained fixtures.

Bounds.  pivp_plan_cost: 1e-5 relative -- a tree sum of <= 16384 non-negative fp32 terms errs by about (log2 n + 2) 2^-24 = 1e-6, the ratio of two
such sums by twice that; the gate leaves about 5x.  pivp_cem_update: mean / std / best_* 1e-6 relative (fp64 sums rounded once); a sample lies
within 1e-5 std + 1e-7 of the reference: the uniforms are exact, the trig argument is exact or rounded by at most 4e-7, |r| <= 5.8, so z is within
2.3e-6; the gate is four times that."""
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as PR  # noqa: E402
import track_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _model(pivp_amd, model_type, nm, P, **kw):
    m = pivp_amd.Model(nm, is_cdna=model_type == 'CDNA', is_stp=model_type == 'STP', is_dna=model_type == 'DNA', prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _rel(got, want):
    """Largest element-wise relative error (an absolute floor of 1e-12 keeps an exact zero comparable)."""
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (np.abs(want) + 1e-12)).max())


def _f32(a):
    return np.asarray(a, dtype=np.float32)


# ---- pivp_plan_cost ---------------------------------------------------------------------------------------------------------------------------------
def _planes(rs, S, K, P, H, W):
    t = (rs.rand(S, K, P, H, W) * rs.rand(S, K, P, H, W) ** 4).astype(np.float32)         # random non-negative planes, most of the mass in few pixels
    t[0, 0, 0] = 0.0; t[0, 0, 0, H // 3, W // 2] = 1.0                                  # a one-hot
    t[1, 1, P - 1] = 0.0                                                                # an all-zero plane
    t[2, 2, 0] = rs.rand(H, W); t[2, 2, 0, H - 1, W - 1] = np.nan                       # a NaN plane
    return t


@pytest.mark.parametrize('H,W', [(64, 64), (128, 128), (30, 72)])
@pytest.mark.parametrize('P', [1, 4, 8])
def test_plan_cost_matches_the_float64_reference(P, H, W):
    torch, pivp_amd = _gpu()
    import plan_ops
    from pivp_amd import planning
    rs = np.random.RandomState(100 * P + H)
    S, K = 3, 5
    track = _planes(rs, S, K, P, H, W)
    goals = np.stack([rs.rand(P) * (H - 1), rs.rand(P) * (W - 1)], axis=1).astype(np.float32)
    step_w, plane_w = (rs.rand(S) + 0.5).astype(np.float32), (rs.rand(P) + 0.5).astype(np.float32)
    miss = float(np.float32(np.sqrt((H - 1) ** 2 + (W - 1) ** 2)))
    cost, mass, edist = plan_ops.plan_cost(track, goals, step_w, plane_w, miss)
    rcost, rmass, redist = PR.plan_cost(track, goals, step_w, plane_w, miss)
    miss_at = np.zeros((S, K, P), bool); miss_at[1, 1, P - 1] = True; miss_at[2, 2, 0] = True
    assert np.array_equal(~(np.isfinite(rmass) & (rmass > 0)), miss_at)
    ok = ~miss_at
    em, ee, ec = np.abs(mass[ok] / rmass[ok] - 1).max(), np.abs(edist / redist - 1).max(), np.abs(cost / rcost - 1).max()
    print('P=%d %dx%d  mass %.2e  edist %.2e  cost %.2e (relative)' % (P, H, W, em, ee, ec))
    assert em < 1e-5 and ee < 1e-5 and ec < 1e-5
    assert mass[1, 1, P - 1] == 0.0 and np.isnan(mass[2, 2, 0])
    assert edist[1, 1, P - 1] == np.float32(miss) and edist[2, 2, 0] == np.float32(miss)      # exactly miss_cost
    assert np.isfinite(cost).all() and np.isfinite(edist).all()                               # NaN never reaches the cost
    assert mass[0, 0, 0] == 1.0 and abs(edist[0, 0, 0] / np.hypot(H // 3 - goals[0, 0], W // 2 - goals[0, 1]) - 1) < 1e-6   # a one-hot: its own distance
    again = plan_ops.plan_cost(track, goals, step_w, plane_w, miss)
    for a, b in zip((cost, mass, edist), again):
        assert a.tobytes() == b.tobytes()                                                     # two launches, equal bits
    # torch's expected_distance on the normalised planes (positive mass only)
    d = torch.from_numpy(track).to('cuda:0')
    m = d.sum(dim=(3, 4))
    te = planning.expected_distance(d / m[..., None, None], torch.from_numpy(goals).to('cuda:0')).cpu().numpy()
    assert np.abs(te[ok] / redist[ok] - 1).max() < 1e-5 and np.abs(edist[ok] / te[ok] - 1).max() < 1e-5


def test_plan_cost_bad_arguments_launch_nothing():
    torch, pivp_amd = _gpu()
    import plan_ops
    rs = np.random.RandomState(0)
    track = rs.rand(2, 3, 2, 16, 16).astype(np.float32)
    args = (track, rs.rand(2, 2) * 15, np.ones(2), np.ones(2), 21.0)
    assert plan_ops.plan_cost_rc(*args)[0] == 0
    for null in ('track', 'goals', 'step_w', 'plane_w', 'cost', 'mass', 'edist'):
        assert plan_ops.plan_cost_rc(*args, null=null)[0] == -1
    for ov in (dict(P=0), dict(P=9), dict(S=0), dict(K=0), dict(K=-1), dict(H=1), dict(W=1), dict(W=253), dict(H=0)):
        assert plan_ops.plan_cost_rc(*args, **ov)[0] == -1, ov
    for miss in (np.nan, np.inf, -np.inf):
        assert plan_ops.plan_cost_rc(*args[:4], miss)[0] == -1


# ---- pivp_cem_update --------------------------------------------------------------------------------------------------------------------------------
def _cem_state(rs, K, Hh, t0=1):
    steps = t0 + Hh
    actions = (rs.randn(steps, K, 5) * 0.7).astype(np.float32)
    mean, std = (rs.randn(Hh, 5) * 0.5).astype(np.float32), (0.3 + rs.rand(Hh, 5)).astype(np.float32)
    cost = rs.permutation(K).astype(np.float32) * 0.37 + 1.0                              # distinct by construction
    best_actions = rs.randn(Hh, 5).astype(np.float32)
    return actions, mean, std, cost, best_actions


def _check_samples(got, ref, std, low, high):
    gate = 1e-5 * np.asarray(std, np.float64)[:, None] + 1e-7
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= gate).all(), float((err / gate).max())
    assert (got >= _f32(low)).all() and (got <= _f32(high)).all()                         # the clamp, exactly
    return float((err / gate).max())


@pytest.mark.parametrize('Hh', [1, 9])
@pytest.mark.parametrize('M', [1, 8])
@pytest.mark.parametrize('K', [16, 200, 1024])
def test_cem_update_matches_the_reference(K, M, Hh):
    torch, pivp_amd = _gpu()
    import plan_ops
    rs = np.random.RandomState(K + 10 * M + Hh)
    t0 = 1
    actions, mean, std, cost, best_actions = _cem_state(rs, K, Hh, t0)
    low, high = np.array([-1.5, -2, -1, -3, -1.2], np.float32), np.array([1.5, 2, 1, 3, 1.2], np.float32)
    kw = dict(t0=t0, elites=M, alpha=0.25, min_std=0.05, seed=0x123456789abcdef, iteration=3)
    for best_cost in (np.inf, 0.5):                                                     # the record is taken / kept
        got = plan_ops.cem_update(cost, actions, mean, std, best_actions, best_cost, low, high, **kw)
        ref = PR.cem_update(cost, actions, mean, std, best_actions, best_cost, low, high, **kw)
        assert got['elites'].tolist() == ref['elites'].tolist()                          # equal, in order
        for name in ('mean', 'std', 'best_actions'):
            assert _rel(got[name], ref[name]) < 1e-6, name
        assert abs(got['best_cost'] - ref['best_cost']) <= 1e-6 * abs(ref['best_cost'])
        assert (got['best_cost'] == 0.5) == (best_cost == 0.5) and (got['std'] >= np.float32(0.05)).all()
        worst = _check_samples(got['actions'][t0:], ref['actions'][t0:], ref['std'], low, high)
        assert np.array_equal(got['actions'][:t0], actions[:t0])                         # rows t < t0 untouched
        clamped = float(((got['actions'][t0:] == low) | (got['actions'][t0:] == high)).mean())
        print('K=%d M=%d Hh=%d  worst sample error / gate %.3f, clamped %.2f' % (K, M, Hh, worst, clamped))
    # the same seed: the same bits; another iteration or seed: other samples
    again = plan_ops.cem_update(cost, actions, mean, std, best_actions, 0.5, low, high, **kw)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got)
    for change in (dict(iteration=4), dict(seed=kw['seed'] + 1), dict(seed=kw['seed'] + 2 ** 32)):
        other = plan_ops.cem_update(cost, actions, mean, std, best_actions, 0.5, low, high, **dict(kw, **change))
        assert not np.array_equal(other['actions'][t0:], got['actions'][t0:]) and np.array_equal(other['mean'], got['mean'])
    # sample-only mode: mean, std, best_* and the elite buffer are left alone
    only = plan_ops.cem_update(None, actions, mean, std, best_actions, 0.5, low, high, **kw)
    assert np.array_equal(only['mean'], mean) and np.array_equal(only['std'], std) and np.array_equal(only['best_actions'], best_actions)
    assert only['best_cost'] == 0.5 and (only['elites'] == -1).all() and np.array_equal(only['actions'][:t0], actions[:t0])
    ref = PR.cem_update(None, actions, mean, std, best_actions, 0.5, low, high, **kw)
    _check_samples(only['actions'][t0:], ref['actions'][t0:], std, low, high)


def test_cem_update_ties_nan_costs_and_bad_arguments():
    torch, pivp_amd = _gpu()
    import plan_ops
    rs = np.random.RandomState(3)
    K, Hh, t0 = 12, 3, 2
    actions, mean, std, _, best_actions = _cem_state(rs, K, Hh, t0)
    cost = np.array([3, 1, np.nan, 1, np.inf, 0.5, 3, np.nan, 0.5, 7, 1, -np.inf], np.float32)
    kw = dict(t0=t0, elites=9, alpha=0.0, min_std=1e-3, seed=5, iteration=0)
    got = plan_ops.cem_update(cost, actions, mean, std, best_actions, np.inf, -np.inf, np.inf, **kw)
    ref = PR.cem_update(cost, actions, mean, std, best_actions, np.inf, -np.inf, np.inf, **kw)
    assert got['elites'].tolist() == ref['elites'].tolist() == [11, 5, 8, 1, 3, 10, 0, 6, 9]
    assert got['best_cost'] == -np.inf and _rel(got['mean'], ref['mean']) < 1e-6 and _rel(got['std'], ref['std']) < 1e-6
    _check_samples(got['actions'][t0:], ref['actions'][t0:], ref['std'], -np.inf, np.inf)
    # all NaN: every cost is +inf, the elites are the first indices and no record is taken
    got = plan_ops.cem_update(np.full(K, np.nan, np.float32), actions, mean, std, best_actions, np.inf, -np.inf, np.inf, **dict(kw, elites=3))
    assert got['elites'].tolist() == [0, 1, 2] and got['best_cost'] == np.inf and np.array_equal(got['best_actions'], best_actions)
    assert np.isfinite(got['actions']).all() and np.isfinite(got['mean']).all()
    good = (cost, actions, mean, std, best_actions, np.inf, -1.0, 1.0)
    for null in ('actions', 'mean', 'std', 'best_actions', 'best_cost', 'low', 'high'):
        assert plan_ops.cem_update_rc(*good, null=null, **kw)[0] == -1
    assert plan_ops.cem_update_rc(*good, null='elites', **kw)[0] == 0                      # the elite buffer is optional
    for ch in (dict(elites=0), dict(elites=K + 1), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=np.nan), dict(min_std=-1.0), dict(t0=-1),
               dict(t0=t0 + Hh), dict(iteration=-1), dict(K=0), dict(K=1025), dict(steps=0)):
        assert plan_ops.cem_update_rc(*good, **dict(kw, **ch))[0] == -1, ch


# ---- cem_plan end to end ----------------------------------------------------------------------------------------------------------------------------
SEED = 3          # CDNA: the reference's elite gaps are 1.8e-2, 3.4e-3, 2.7e-3 with this seed (seed 0: 7.6e-5 in the first iteration)
SETUP = dict(designated_rc=[[32, 32]], goal_rc=[[40, 24]], horizon=4, iterations=3, samples=16, elites=4, init_std=0.5, seed=SEED)


def _scene(model_type):
    P, nm = TR.load_trained(model_type)
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    return P, nm, imgs[:2], stas[0], acts[:1, 0]


def _check_trace(torch, pivp_amd, model_type, nm, P, ctx_imgs, state, past, res, setup, precision='fp32'):
    """Every traced iteration against a fresh rollout and the float64 reference; the whole run against the reference loop's bookkeeping."""
    import plan_ops
    from pivp_amd import planning
    K, M, Hh, its, seed = setup['samples'], setup['elites'], setup['horizon'], setup['iterations'], setup['seed']
    nP = len(setup['designated_rc'])
    t0 = len(past)
    goals = np.asarray(setup['goal_rc'], np.float64)
    miss = float(np.float32(np.sqrt(2 * 63.0 ** 2)))
    st = dict(actions=np.zeros((t0 + Hh, K, 5)), mean=np.zeros((Hh, 5)), std=np.full((Hh, 5), setup.get('init_std', 1.0)),
              best_actions=np.zeros((Hh, 5)), best_cost=np.inf)
    st['actions'][:t0] = np.asarray(past, np.float64)[:, None]
    fresh = _model(pivp_amd, model_type, nm, P, precision=precision)
    planes = planning.one_hot_planes(np.tile(np.asarray(setup['designated_rc'])[None], (K, 1, 1)), 64, 64)
    prev_cost = None
    for it in range(its + 1):
        st = PR.cem_update(prev_cost, st['actions'], st['mean'], st['std'], st['best_actions'], st['best_cost'], -np.inf, np.inf, t0, M, 0.0, 1e-3,
                           seed, it)
        if it > 0:
            rec = res.trace[it - 1]
            assert rec['elites'].cpu().numpy().tolist() == st['elites'].tolist(), it       # the elite set, in order
            assert abs(float(res.best_cost_per_iteration[it - 1]) - st['best_cost']) <= 1e-6 * st['best_cost']
        if it == its:
            break
        rec = res.trace[it]
        cand = rec['actions'].cpu().numpy()
        assert (cand[:t0] == _f32(past)[:, None]).all()                                    # the past, for every candidate
        _check_samples(cand[t0:], st['actions'][t0:], st['std'], -np.inf, np.inf)          # this iteration's candidates (it = 0: the first samples)
        # a fresh rollout of the traced candidates: the same planes, hence the same moments, bit for bit
        fresh.imagine(np.repeat(ctx_imgs, K, axis=1), cand, np.repeat(state, K, axis=0), designated=planes)
        track = fresh.pixel_distrib.cpu().numpy()
        assert track.shape == (Hh, K, nP, 64, 64)
        cost2, mass2, edist2 = plan_ops.plan_cost(track, goals, np.ones(Hh), np.ones(nP), miss)
        assert mass2.tobytes() == rec['mass'].cpu().numpy().tobytes() and cost2.tobytes() == rec['cost'].cpu().numpy().tobytes()
        rcost, rmass, _ = PR.plan_cost(track, goals, np.ones(Hh), np.ones(nP), miss)
        traced = rec['cost'].cpu().numpy()
        assert np.abs(traced / rcost - 1).max() < 1e-5
        srt = np.sort(rcost)
        gap = (srt[M] - srt[M - 1]) / srt[M - 1]
        print('%s it %d: cost %.3f .. %.3f, elite gap %.2e, mass %.3g .. %.3g' % (model_type, it, srt[0], srt[-1], gap, rmass.min(), rmass.max()))
        assert gap > 1e-3                                                                   # the elite-set comparison means something
        st['actions'][t0:] = cand[t0:]                # carry the DEVICE's candidates: the refit is checked on what was rolled out
        prev_cost = traced
    for name in ('mean', 'std'):
        assert _rel(getattr(res, name).cpu().numpy(), st[name]) < 1e-6, name
    assert _rel(res.actions.cpu().numpy(), st['best_actions']) < 1e-6 and abs(float(res.cost) - st['best_cost']) <= 1e-6 * st['best_cost']


def test_cem_plan_end_to_end_on_the_trained_cdna_fixture():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past = _scene('CDNA')
    assert np.abs(past).max() > 0
    m = _model(pivp_amd, 'CDNA', nm, P)
    res = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, **SETUP)
    assert res.actions.shape == (4, 5) and res.mean.shape == (4, 5) and res.std.shape == (4, 5) and res.best_cost_per_iteration.shape == (3,)
    assert all(t.is_cuda for t in (res.actions, res.cost, res.mean, res.std, res.best_cost_per_iteration)) and len(res.trace) == 3
    per = res.best_cost_per_iteration.cpu().numpy()
    assert np.isfinite(per).all() and (np.diff(per) <= 0).all() and float(res.cost) == per.min() == per[-1]
    assert float(res.cost) == min(float(r['cost'].min()) for r in res.trace)
    _check_trace(torch, pivp_amd, 'CDNA', nm, P, ctx_imgs, state, past, res, SETUP)
    # one seed, equal bits (a second model, and the first one again); another seed, other candidates
    res2 = planning.cem_plan(_model(pivp_amd, 'CDNA', nm, P), ctx_imgs, state, past_actions=past, trace=True, **SETUP)
    res3 = planning.cem_plan(m, ctx_imgs, state, past_actions=past, **SETUP)
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
        assert torch.equal(getattr(res, name), getattr(res2, name)) and torch.equal(getattr(res, name), getattr(res3, name)), name
    assert res3.trace is None and all(torch.equal(a[k], b[k]) for a, b in zip(res.trace, res2.trace) for k in a)
    other = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, **dict(SETUP, seed=SEED + 1))
    assert not torch.equal(other.trace[0]['actions'], res.trace[0]['actions'])
    # chunked: the same candidates (the sampler does not see the chunking) at batch 8; costs within the batch-dependence bound of
    # test_score_actions_is_one_imagine_at_batch_k
    ch = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, chunk=8, **dict(SETUP, iterations=1))
    assert torch.equal(ch.trace[0]['actions'], res.trace[0]['actions'])
    c0, c1 = res.trace[0]['cost'].cpu().numpy(), ch.trace[0]['cost'].cpu().numpy()
    print('chunk 8 against 16: largest cost difference %.2e' % np.abs(c0 - c1).max())
    assert np.abs(c0 - c1).max() < 1e-4
    # another past: row 0 of every candidate is it, and it reaches the rollout
    past2 = np.array([[0.3, -0.2, 0.1, 0.4, -0.5]], np.float32)
    o = planning.cem_plan(m, ctx_imgs, state, past_actions=past2, trace=True, **dict(SETUP, iterations=1))
    a0 = o.trace[0]['actions'].cpu().numpy()
    assert (a0[0] == past2[0]).all() and np.array_equal(a0[1:], res.trace[0]['actions'].cpu().numpy()[1:])
    assert not torch.equal(o.trace[0]['cost'], res.trace[0]['cost'])
    # several planes, weights and bounds
    multi = dict(SETUP, designated_rc=[[32, 32], [20, 40], [30, 30]], goal_rc=[[40, 24], [20, 44], [28.5, 30]], iterations=2)
    r = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, plane_weights=[1.0, 0.5, 2.0], step_weights=[0, 0, 0, 1.0],
                          action_low=-0.4, action_high=[0.4, 0.4, 0.4, 0.4, 0.2], **multi)
    a1 = r.trace[1]['actions'].cpu().numpy()[1:]
    assert a1.min() >= np.float32(-0.4) and a1[..., :4].max() <= np.float32(0.4) and a1[..., 4].max() <= np.float32(0.2)
    e = r.trace[1]['edist'].cpu().numpy().astype(np.float64)
    want = (e[3] * np.array([1.0, 0.5, 2.0])).sum(axis=1)
    assert r.trace[1]['edist'].shape == (4, 16, 3) and np.abs(r.trace[1]['cost'].cpu().numpy() / want - 1).max() < 1e-6


def test_cem_plan_on_the_dna_head():
    """The same run on the trained DNA fixture (seed 2: the reference's elite gaps are 6.8e-3, 2.0e-2, 8.6e-2).  The trained STP fixture cannot carry
    the elite-set comparison: its tracked pixel stays in place whatever the actions are, so every candidate costs the same (22.627 = two steps at the
    designated pixel's own distance from the goal) and the gap between the 4th and 5th cost is zero for every seed."""
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    model_type = 'DNA'
    P, nm, ctx_imgs, state, past = _scene(model_type)
    setup = dict(SETUP, seed=2)
    m = _model(pivp_amd, model_type, nm, P)
    res = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, **setup)
    per = res.best_cost_per_iteration.cpu().numpy()
    assert np.isfinite(per).all() and (np.diff(per) <= 0).all() and float(res.cost) == per[-1]
    _check_trace(torch, pivp_amd, model_type, nm, P, ctx_imgs, state, past, res, setup)


def test_cem_plan_bf16_is_finite_and_reproducible():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past = _scene('CDNA')
    runs = [planning.cem_plan(_model(pivp_amd, 'CDNA', nm, P, precision='bf16'), ctx_imgs, state, past_actions=past, trace=True, **SETUP)
            for _ in range(2)]
    a, b = runs
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
        assert torch.isfinite(getattr(a, name)).all() and torch.equal(getattr(a, name), getattr(b, name)), name
    assert all(torch.equal(x[k], y[k]) and torch.isfinite(x[k].float()).all() for x, y in zip(a.trace, b.trace) for k in x)
    assert (np.diff(a.best_cost_per_iteration.cpu().numpy()) <= 0).all()


def test_the_loop_never_synchronises_with_the_host():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past = _scene('CDNA')
    m = _model(pivp_amd, 'CDNA', nm, P)
    kw = dict(SETUP, samples=32, elites=8, chunk=16)
    warm = planning.cem_plan(m, ctx_imgs, state, past_actions=past, **kw)                # plans, workspaces and allocator blocks exist from here on
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda:0')
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            a = planning._check_cem_args(m, ctx_imgs, state, past_actions=past, **kw)
            torch.cuda.set_sync_debug_mode('default')
            b = planning._cem_upload(m, a, ctx_imgs, state)                              # the uploads, once, in front of the loop
            torch.cuda.set_sync_debug_mode('error')
            res = planning._cem_iterate(m, a, b, trace=False)                            # every iteration, the final update included
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not detects:
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made')
    assert torch.equal(res.actions, warm.actions) and torch.equal(res.best_cost_per_iteration, warm.best_cost_per_iteration)


def test_score_actions_still_returns_what_it_did():
    """`planning.score_actions` is untouched by the planner: the by-hand check of tests/test_gpu_imagine.py, and NaN-free agreement with
    pivp_plan_cost on the same planes."""
    torch, pivp_amd = _gpu()
    import plan_ops
    from pivp_amd import planning
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    K, steps = 8, 5
    rs = np.random.RandomState(2)
    cand = (acts[:steps, 0][None] + rs.randn(K, steps, 5) * 0.5).astype(np.float32)
    cand[0] = acts[:steps, 0]
    m = _model(pivp_amd, 'CDNA', nm, P)
    cost = planning.score_actions(m, imgs[:2], stas[0], cand, (32, 32), (40, 24))
    assert cost.shape == (K,) and torch.isfinite(cost).all() and float(cost.min()) > 0
    frames = torch.stack(m.gen_images)
    m2 = _model(pivp_amd, 'CDNA', nm, P)
    m2.imagine(np.repeat(imgs[:2], K, axis=1), np.ascontiguousarray(cand.transpose(1, 0, 2)), np.repeat(stas[0], K, axis=0),
               designated=planning.one_hot_planes(np.tile(np.array([[[32, 32]]]), (K, 1, 1)), 64, 64), normalize=True)
    assert torch.equal(torch.stack(m2.gen_images), frames)
    d = m2.pixel_distrib[:, :, 0]
    rows = torch.arange(64, dtype=torch.float32, device=d.device).view(64, 1)
    cols = torch.arange(64, dtype=torch.float32, device=d.device).view(1, 64)
    dist = torch.sqrt((rows - 40.0) ** 2 + (cols - 24.0) ** 2)
    assert torch.equal((d * dist).sum(dim=(-2, -1)).sum(dim=0), cost)
    m2.imagine(np.repeat(imgs[:2], K, axis=1), np.ascontiguousarray(cand.transpose(1, 0, 2)), np.repeat(stas[0], K, axis=0),
               designated=planning.one_hot_planes(np.tile(np.array([[[32, 32]]]), (K, 1, 1)), 64, 64))
    assert m2.pixel_mass.shape == (4, K, 1)
    hip, _, _ = plan_ops.plan_cost(m2.pixel_distrib.cpu().numpy(), [[40, 24]], np.ones(4), np.ones(1), 89.0)
    assert np.abs(hip / cost.cpu().numpy() - 1).max() < 1e-5
