"""GPU tests of closed-loop planning: pivp_cem_update_ex and pivp_cem_shift against the float64 restatement tests/mpc_reference.py, `cem_plan`'s
closed-loop options and `planning.MPC` on the trained CDNA fixture.

Bounds.  mean / std / best_*: 1e-6 relative, as tests/test_gpu_planning.py (fp64 sums rounded once).  Kept slots, the mean slot and the shift are
copies: exact.  A white sample lies within 1e-5 std + 1e-7 of the reference (that file: a device normal is within 2.3e-6 of the exact one, the gate
four times that).  A colored sample is mean + std * y with y[i] = sum_c Q[i][c] z[c]: the normals' errors add up to at most 2.3e-6 * |Q[i]|_1, and a
row of unit 2-norm has a 1-norm of at most sqrt(n); the sum itself runs in fp64 (its own rounding, n * 2^-53 * |y|, is nothing) and is rounded to
fp32 once, 2^-24 |y| <= 2^-24 * 5.8 sqrt(n) = 3.5e-7 sqrt(n).  Together 2.65e-6 sqrt(n); the gate is four times that, as for white noise:
1.06e-5 sqrt(n) std + 1e-7."""
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_reference as MR  # noqa: E402
import plan_reference as PR  # noqa: E402
import track_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _model(pivp_amd, nm, P, **kw):
    m = pivp_amd.Model(nm, is_cdna=True, prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (np.abs(want) + 1e-12)).max())


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _cem_state(rs, K, n, t0):
    actions = (rs.randn(t0 + n, K, 5) * 0.7).astype(np.float32)
    mean, std = (rs.randn(n, 5) * 0.5).astype(np.float32), (0.3 + rs.rand(n, 5)).astype(np.float32)
    cost = rs.permutation(K).astype(np.float32) * 0.37 + 1.0
    return actions, mean, std, cost, rs.randn(n, 5).astype(np.float32)


# ---- pivp_cem_update_ex ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t0', [0, 1])
@pytest.mark.parametrize('K', [1, 7, 32, 300, 1024])
def test_update_ex_with_the_options_off_is_cem_update_bit_for_bit(K, t0):
    torch, pivp_amd = _gpu()
    import mpc_ops
    import plan_ops
    rs = np.random.RandomState(10 * K + t0)
    n, M = 4, min(K, 5)
    actions, mean, std, cost, best = _cem_state(rs, K, n, t0)
    hard = cost.copy()                                                              # NaNs and ties
    hard[::3] = 2.0
    hard[1::5] = np.nan
    low, high = np.array([-1.5, -2, -1, -3, -1.2], np.float32), np.array([1.5, 2, 1, 3, 1.2], np.float32)
    kw = dict(t0=t0, elites=M, alpha=0.25, min_std=0.05, seed=0x123456789abcdef, iteration=3)
    for c in (None, cost, hard):
        for best_cost in (np.inf, 0.5):
            a = plan_ops.cem_update(c, actions, mean, std, best, best_cost, low, high, **kw)
            b = mpc_ops.cem_update_ex(c, actions, mean, std, best, best_cost, low, high, **kw)
            for name in ('actions', 'mean', 'std', 'best_actions', 'elites'):
                assert a[name].tobytes() == b[name].tobytes(), name
            assert a['best_cost'] == b['best_cost']


def _sample_gate(std, n, beta):
    return ((1.06e-5 * np.sqrt(n)) if beta > 0 else 1e-5) * np.asarray(std, np.float64)[:, None] + 1e-7


def _check_update(got, ref, actions, low, high, t0, n, K, keep, add_mean, beta, fixed):
    """One update against the restatement: -> the worst sample error over its gate.  fixed: the number of leading slots that are copies."""
    for name in ('mean', 'std', 'best_actions'):
        assert _rel(got[name], ref[name]) < 1e-6, name
    assert np.array_equal(got['actions'][:t0], actions[:t0])                         # rows t < t0 untouched
    assert np.array_equal(got['actions'][t0:, :fixed], _f32(ref['actions'][t0:, :fixed]))      # the kept slots: bit for bit
    sampled = np.ones(K, bool)
    sampled[:fixed] = False
    if add_mean:
        sampled[keep] = False
        assert np.array_equal(got['actions'][t0:, keep], np.clip(got['mean'], _f32(low), _f32(high)))      # clamp(mean), of the mean just written
    err = np.abs(got['actions'][t0:, sampled].astype(np.float64) - ref['actions'][t0:, sampled])
    gate = _sample_gate(ref['std'], n, beta)
    assert (err <= gate).all(), float((err / gate).max())
    drawn = got['actions'][t0:, fixed:]                                              # the clamp, exactly (a kept slot holds what it was given)
    assert (drawn >= _f32(low)).all() and (drawn <= _f32(high)).all()
    return float((err / gate).max()) if sampled.any() else 0.0


@pytest.mark.parametrize('n', [1, 2, 3, 8, 9, 64])
def test_update_ex_matches_the_restatement(n):
    torch, pivp_amd = _gpu()
    import mpc_ops
    rs = np.random.RandomState(n)
    K, M, t0 = 7, 3, 1
    actions, mean, std, cost, best = _cem_state(rs, K, n, t0)
    low, high = np.array([-1.5, -2, -1, -3, -1.2], np.float32), np.array([1.5, 2, 1, 3, 1.2], np.float32)
    kw = dict(t0=t0, elites=M, alpha=0.25, min_std=0.05, seed=0xfedcba987654321, iteration=2)
    worst = 0.0
    for beta in (0.0, 0.5, 1.0, 2.0):
        for keep in (0, 2, 3):
            for add_mean in (0, 1):
                opt = dict(keep=keep, add_mean=add_mean, beta=beta)
                got = mpc_ops.cem_update_ex(cost, actions, mean, std, best, np.inf, low, high, **kw, **opt)
                ref = MR.cem_update_ex(cost, actions, mean, std, best, np.inf, low, high, **kw, **opt)
                assert got['elites'].tolist() == ref['elites'].tolist()
                for j in range(keep):                                                    # the elites themselves, as they were
                    assert np.array_equal(got['actions'][t0:, j], actions[t0:, ref['elites'][j]])
                worst = max(worst, _check_update(got, ref, actions, low, high, t0, n, K, keep, add_mean, beta, keep))
                for kept_in in (0, 1):                                                   # sample-only: a warm start's slots stay, a cold one's are drawn
                    got = mpc_ops.cem_update_ex(None, actions, mean, std, best, 0.5, low, high, kept_in=kept_in, **kw, **opt)
                    ref = MR.cem_update_ex(None, actions, mean, std, best, 0.5, low, high, kept_in=kept_in, **kw, **opt)
                    assert np.array_equal(got['mean'], mean) and np.array_equal(got['std'], std) and got['best_cost'] == 0.5 and (got['elites'] == -1).all()
                    worst = max(worst, _check_update(got, ref, actions, low, high, t0, n, K, keep, add_mean, beta, keep if kept_in else 0))
        again = mpc_ops.cem_update_ex(cost, actions, mean, std, best, np.inf, low, high, keep=2, add_mean=1, beta=beta, **kw)
        twice = mpc_ops.cem_update_ex(cost, actions, mean, std, best, np.inf, low, high, keep=2, add_mean=1, beta=beta, **kw)
        assert all(np.asarray(again[k]).tobytes() == np.asarray(twice[k]).tobytes() for k in again)      # the same bits on every launch
    print('n = %d: worst sample error / gate %.3f' % (n, worst))


@pytest.mark.parametrize('K,n', [(7, 3), (300, 9), (1024, 2)])
def test_kept_elites_that_permute_their_own_slots(K, n):
    """The in-place hazard: the elites are slots 1, 2, 0 (keep = 3) or 1, 0 (keep = 2), so every copy's source is another copy's destination."""
    torch, pivp_amd = _gpu()
    import mpc_ops
    rs = np.random.RandomState(K)
    t0 = 1
    actions, mean, std, _, best = _cem_state(rs, K, n, t0)
    kw = dict(t0=t0, elites=min(K, 4), alpha=0.0, min_std=1e-3, seed=9, iteration=1)
    for keep, order in ((3, [1, 2, 0]), (2, [1, 0])):
        cost = np.arange(K, dtype=np.float32) + 10.0
        cost[order] = np.arange(len(order), dtype=np.float32)
        got = mpc_ops.cem_update_ex(cost, actions, mean, std, best, np.inf, -np.inf, np.inf, keep=keep, **kw)
        assert got['elites'][:keep].tolist() == order
        for j, e in enumerate(order):
            assert np.array_equal(got['actions'][t0:, j], actions[t0:, e]), (keep, j)
        assert np.array_equal(got['best_actions'], actions[t0:, order[0]])


def test_colored_noise_statistics_on_the_device():
    """K = 1024, 8 iterations, n = 9, beta = 1: per-row variance and lag-1 correlation within 5 standard errors of 1 and of (Q Q^T)[t, t+1] (the
    restatement passes the same check with the same seeds: tests/test_mpc_host.py)."""
    torch, pivp_amd = _gpu()
    import mpc_ops
    ref, _ = MR.colored_noise_statistics(MR.colored_draws(MR.cem_update_ex), 1.0)
    assert ref < 5.0
    worst, r = MR.colored_noise_statistics(MR.colored_draws(mpc_ops.cem_update_ex), 1.0)
    print('device: worst deviation %.2f standard errors (restatement %.2f); lag-1 correlation %.4f' % (worst, ref, r[0]))
    assert worst < 5.0


# ---- pivp_cem_shift -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keep', [0, 3])
@pytest.mark.parametrize('n', [2, 9])
def test_shift_is_exact(n, keep):
    torch, pivp_amd = _gpu()
    import mpc_ops
    rs = np.random.RandomState(n + keep)
    K, t0 = 7, 1
    actions, mean, std, _, best = _cem_state(rs, K, n, t0)
    low, high = np.array([-0.5, -2, -1, -3, -1.2], np.float32), np.array([1.5, 2, 1, 3, 0.2], np.float32)
    tail_mean, tail_std, floor = _f32([0.9, -0.1, 0.2, 0.0, 0.7]), _f32([1.0, 0.9, 0.8, 0.7, 0.6]), _f32([0.5, 0.0, 0.8, 2.0, 0.1])
    for shift in sorted({1, n - 1}):
        got = mpc_ops.cem_shift(mean, std, actions, best, low, high, tail_mean, tail_std, floor, t0, keep, shift)
        ref = MR.cem_shift(mean, std, actions, best, low, high, tail_mean, tail_std, floor, t0, keep, shift)
        for name in ('mean', 'std', 'actions', 'best_actions'):
            assert np.array_equal(got[name], _f32(ref[name])), (name, shift)
        assert got['best_cost'] == np.inf
        # without the optional buffers
        bare = mpc_ops.cem_shift(mean, std, None, None, low, high, tail_mean, tail_std, floor, 0, 0, shift)
        assert np.array_equal(bare['mean'], got['mean']) and np.array_equal(bare['std'], got['std'])
    for ch in (dict(shift=0), dict(shift=n), dict(keep=K + 1), dict(K=0)):
        assert mpc_ops.cem_shift_rc(mean, std, actions, best, low, high, tail_mean, tail_std, floor, t0, **dict(dict(keep=keep, shift=1), **ch))[0] == -1


# ---- cem_plan with the options --------------------------------------------------------------------------------------------------------------
SETUP = dict(designated_rc=[[32, 32]], goal_rc=[[40, 24]], horizon=3, iterations=2, samples=8, elites=3, init_std=0.5, seed=3)
_SCENE = []


def _scene():
    if not _SCENE:
        P, nm = TR.load_trained('CDNA')
        imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in R.moving_batch(1, 6, 64, 64, seed=123))
        _SCENE.append((P, nm, imgs[:2], stas[0], acts[:1, 0]))
    return _SCENE[0]


def _check_trace(torch, pivp_amd, res, opts, warm=None):
    """Every traced iteration against a fresh rollout and the restated loop (tests/test_gpu_planning.py's check, with the options)."""
    import plan_ops
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past = _scene()
    K, M, n, its, seed = SETUP['samples'], SETUP['elites'], SETUP['horizon'], SETUP['iterations'], SETUP['seed']
    t0, keep = len(past), opts.get('keep', 0)
    miss = float(np.float32(np.sqrt(2 * 63.0 ** 2)))
    st = dict(actions=np.zeros((t0 + n, K, 5)), mean=np.zeros((n, 5)), std=np.full((n, 5), SETUP['init_std']), best_actions=np.zeros((n, 5)), best_cost=np.inf)
    st['actions'][:t0] = np.asarray(past, np.float64)[:, None]
    kept_in = 0
    if warm is not None:
        st['mean'], st['std'] = warm.mean.cpu().numpy().astype(np.float64), warm.std.cpu().numpy().astype(np.float64)
        if warm.kept is not None:
            st['actions'][t0:, :keep] = warm.kept.cpu().numpy()
            kept_in = 1
    fresh = _model(pivp_amd, nm, P)
    planes = planning.one_hot_planes(np.tile(np.asarray(SETUP['designated_rc'])[None], (K, 1, 1)), 64, 64)
    prev_cost = None
    for it in range(its + 1):
        before = st['actions'].copy()
        st = MR.cem_update_ex(prev_cost, st['actions'], st['mean'], st['std'], st['best_actions'], st['best_cost'], -np.inf, np.inf, t0, M, 0.0, 1e-3,
                              seed, it, kept_in=kept_in, **opts)
        if it > 0:
            assert res.trace[it - 1]['elites'].cpu().numpy().tolist() == st['elites'].tolist(), it
            assert abs(float(res.best_cost_per_iteration[it - 1]) - st['best_cost']) <= 1e-6 * st['best_cost']
        if it == its:
            break
        cand = res.trace[it]['actions'].cpu().numpy()
        assert (cand[:t0] == _f32(past)[:, None]).all()
        fixed = keep if (it > 0 or kept_in) else 0
        assert np.array_equal(cand[t0:, :fixed], _f32(st['actions'][t0:, :fixed]))      # kept: the previous iteration's elites (or the warm start's), exactly
        sampled = np.ones(K, bool)
        sampled[:fixed] = False
        if opts.get('add_mean'):
            sampled[keep] = False
            assert _rel(cand[t0:, keep], st['actions'][t0:, keep]) < 1e-6
        err = np.abs(cand[t0:, sampled].astype(np.float64) - st['actions'][t0:, sampled])
        assert (err <= _sample_gate(st['std'], n, opts.get('beta', 0.0))).all()
        fresh.imagine(np.repeat(ctx_imgs, K, axis=1), cand, np.repeat(state, K, axis=0), designated=planes)
        cost2, mass2, _ = plan_ops.plan_cost(fresh.pixel_distrib.cpu().numpy(), SETUP['goal_rc'], np.ones(n), np.ones(1), miss)
        assert cost2.tobytes() == res.trace[it]['cost'].cpu().numpy().tobytes()          # the cost of a fresh rollout of the traced candidates
        st['actions'][t0:] = cand[t0:]                # carry the DEVICE's candidates: the refit is checked on what was rolled out
        prev_cost = cost2
    for name in ('mean', 'std'):
        assert _rel(getattr(res, name).cpu().numpy(), st[name]) < 1e-6, name
    assert _rel(res.actions.cpu().numpy(), st['best_actions']) < 1e-6 and abs(float(res.cost) - st['best_cost']) <= 1e-6 * st['best_cost']
    if keep:
        assert np.array_equal(res.kept.cpu().numpy(), _f32(st['actions'][t0:, :keep]))   # the final update's best sequences
    return st


def test_cem_plan_with_the_options_against_the_restated_loop():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past = _scene()
    m = _model(pivp_amd, nm, P)
    plain = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, **SETUP)
    spelled = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, keep_elites=0, add_mean=False, noise_beta=0.0, warm=None,
                                designated_planes=None, **SETUP)
    one_hot = planning.one_hot_planes([SETUP['designated_rc']], 64, 64)[0]
    planes = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, designated_planes=one_hot, **dict(SETUP, designated_rc=None))
    on_dev = planning.cem_plan(m, ctx_imgs, state, past_actions=past, designated_planes=one_hot.to('cuda:0'), **dict(SETUP, designated_rc=None))
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
        assert torch.equal(getattr(plain, name), getattr(spelled, name)) and torch.equal(getattr(plain, name), getattr(planes, name)), name
        assert torch.equal(getattr(plain, name), getattr(on_dev, name)), name
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for a, b, c in zip(plain.trace, spelled.trace, planes.trace) for k in a)
    assert plain.kept is None
    kept = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, keep_elites=2, **SETUP)
    assert kept.kept.shape == (3, 2, 5) and kept.kept.is_cuda
    _check_trace(torch, pivp_amd, kept, dict(keep=2))
    again = planning.cem_plan(_model(pivp_amd, nm, P), ctx_imgs, state, past_actions=past, trace=True, keep_elites=2, **SETUP)
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration', 'kept'):
        assert torch.equal(getattr(kept, name), getattr(again, name)), name                 # the same seed, the same bits
    assert all(torch.equal(a[k], b[k]) for a, b in zip(kept.trace, again.trace) for k in a)
    assert torch.equal(kept.trace[0]['actions'], plain.trace[0]['actions'])                  # the first population is the plain one: nothing kept yet
    # a kept elite is scored again, in another slot of the batch: the cost it had, within the batch-dependence bound of tests/test_gpu_planning.py
    c0, c1 = kept.trace[0]['cost'].cpu().numpy(), kept.trace[1]['cost'].cpu().numpy()
    assert np.abs(c1[:2] - np.sort(c0)[:2]).max() < 1e-4
    everything = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, keep_elites=2, add_mean=True, noise_beta=1.0, **SETUP)
    _check_trace(torch, pivp_amd, everything, dict(keep=2, add_mean=1, beta=1.0))
    assert not torch.equal(everything.trace[0]['actions'], kept.trace[0]['actions'])
    # a warm start: the shifted plan enters the next call
    w = kept.warm_start(shift=1, tail_mean=0.0, tail_std=0.5, std_floor=0.25)
    ref = MR.cem_shift(kept.mean.cpu().numpy(), kept.std.cpu().numpy(), kept.kept.cpu().numpy(), None, -np.inf, np.inf, 0.0, 0.5, 0.25, 0, 2, 1)
    assert np.array_equal(w.mean.cpu().numpy(), _f32(ref['mean'])) and np.array_equal(w.std.cpu().numpy(), _f32(ref['std']))
    assert np.array_equal(w.kept.cpu().numpy(), _f32(ref['actions'])) and float(w.std.min()) >= 0.25
    warm = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, keep_elites=2, warm=w, **SETUP)
    _check_trace(torch, pivp_amd, warm, dict(keep=2), warm=w)
    assert torch.equal(warm.trace[0]['actions'][1:, :2], w.kept)                             # evaluated as they lie
    no_kept = planning.cem_plan(m, ctx_imgs, state, past_actions=past, trace=True, warm=planning.PlanWarmStart(w.mean, w.std), **SETUP)
    _check_trace(torch, pivp_amd, no_kept, dict(), warm=planning.PlanWarmStart(w.mean, w.std))


# ---- the controller -------------------------------------------------------------------------------------------------------------------------
MPC_SETUP = dict(horizon=3, goal_rc=[[40, 24]], iterations=2, samples=8, elites=3, init_std=0.5, keep_elites=2, warm_iterations=1)


def _no_sync(torch, fn):
    """fn() under torch's sync debug mode -> (whether the mode detects a synchronisation on this build, fn's result)."""
    probe = torch.ones(1, device='cuda:0')
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        out = fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return detects, out


def _run_controller(torch, pivp_amd, seed, steps=3, check=False, quiet_from=None):
    """`steps` control steps of `planning.MPC` in an environment that is a second model with the same weights.  check: every step against the manual
    composition on a third model.  quiet_from: from this step on act() and observe() run under the sync debug mode.  -> (actions, final planes, detects)."""
    from pivp_amd import planning
    P, nm, ctx_imgs, state0, past = _scene()
    dev = 'cuda:0'
    env, m = _model(pivp_amd, nm, P, carry_state=True), _model(pivp_amd, nm, P, carry_state=True)
    ctl = planning.MPC(m, seed=seed, **MPC_SETUP)
    ctl.reset(ctx_imgs, state0, past, designated_rc=[[32, 32]])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    env.imagine(ctx_imgs[:1], past[:, None], state0, observed=1)                        # the world has seen what the robot has
    frame, state = to(ctx_imgs[1:2]), env.gen_states[-1].clone()
    if check:
        man = _model(pivp_amd, nm, P, carry_state=True)
        man.imagine(ctx_imgs[:1], past[:, None], state0, observed=1)
        planes, warm = planning.one_hot_planes([[[32, 32]]], 64, 64, dev), None
        assert torch.equal(man.gen_states[-1], state) and torch.equal(ctl.planes, planes[0])
    actions, detects = [], None
    for step in range(steps):
        quiet = quiet_from is not None and step >= quiet_from
        if quiet:
            detects, action = _no_sync(torch, ctl.act)
        else:
            action = ctl.act()
        assert action.shape == (5,) and action.is_cuda and ctl.step == step
        actions.append(action.clone())
        if check:
            res = planning.cem_plan(man, frame, state, None, MPC_SETUP['goal_rc'], 3, iterations=2 if step == 0 else 1, samples=8, elites=3, init_std=0.5,
                                    keep_elites=2, seed=seed + step, belief=man.recurrent_state(), warm=warm, designated_planes=planes[0])
            for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration', 'kept'):
                assert torch.equal(getattr(res, name), getattr(ctl.last_plan, name)), (step, name)
            assert torch.equal(res.actions[0], action)
        env.imagine(frame, action.view(1, 1, 5), state, observed=1)                     # the world moves
        new_frame, new_state = env.gen_images[-1].clone().view(1, 1, 3, 64, 64), env.gen_states[-1].clone()
        if quiet:
            _no_sync(torch, lambda: ctl.observe(new_frame, new_state))
        else:
            ctl.observe(new_frame, new_state)
        if check:
            man.imagine(frame, action.view(1, 1, 5), state, designated=planes, observed=1)
            assert torch.equal(man.recurrent_state().data, m.recurrent_state().data)        # the belief
            moved, mass = man.pixel_distrib[0], man.pixel_mass[0]
            planes = moved / torch.where(mass > 0, mass, torch.ones_like(mass))[..., None, None]
            assert torch.equal(ctl.planes, planes[0]) and abs(float(ctl.planes.sum()) - 1.0) < 1e-5      # the advected planes are imagine's, renormalised
            warm = res.warm_start(shift=1, tail_mean=0.0, tail_std=0.5, std_floor=0.5)
            assert all(torch.equal(getattr(warm, k), getattr(ctl._warm, k)) for k in ('mean', 'std', 'kept'))
        frame, state = new_frame, new_state
    return torch.stack(actions), ctl.planes.clone(), detects


def test_mpc_steps_are_the_manual_composition_bit_for_bit():
    torch, pivp_amd = _gpu()
    a, planes, _ = _run_controller(torch, pivp_amd, seed=5, check=True)
    b, planes_b, _ = _run_controller(torch, pivp_amd, seed=5)
    c, _, _ = _run_controller(torch, pivp_amd, seed=6)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(planes, planes_b)      # twice: the same bits
    assert not torch.equal(a[0], c[0]) and not torch.equal(a, c)                                 # another seed: other actions
    assert float(planes[0, 32, 32]) < 1.0                                                        # the designated pixel has become a distribution


def test_mpc_act_and_observe_never_synchronise_with_the_host():
    torch, pivp_amd = _gpu()
    a, _, detects = _run_controller(torch, pivp_amd, seed=5, quiet_from=1)                       # step 0 makes the plans, workspaces and allocator blocks
    if not detects:
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made')
    b, _, _ = _run_controller(torch, pivp_amd, seed=5)
    assert torch.equal(a, b)
