"""CPU-side tests of closed-loop planning: the C-ABI surface of include/pivp_mpc.h against `_lib.MPC_SIGNATURES` and the built library, the ops'
refusals (nothing is launched, so they return on a machine without a device), every new ValueError of `planning.cem_plan`, `PlanWarmStart`,
`warm_start` and `MPC`, the float64 restatement tests/mpc_reference.py against its own properties, and the closed loop on a point mass."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib, planning

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_reference as MR  # noqa: E402
import plan_reference as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'pivp_cem_update_ex', 'pivp_cem_shift'}


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_mpc_header_library_and_ctypes_table_agree():
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_mpc.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.MPC_SIGNATURES) == NEW and declared <= exported
    assert not any(declared & set(table) for header, table in _lib.HEADER_SIGNATURES.items() if header != 'pivp_mpc.h')
    lib = _lib.load()
    # pivp_hip.h is what it was: 118 symbols, version 17
    assert lib.pivp_abi_version() == 17 and len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)
    assert 'mpc.hip' in build.SOURCES and 'pivp_mpc.h' in [os.path.basename(p) for p in _digest.source_files()]
    assert 'cem_noise.h' in [os.path.basename(p) for p in _digest.source_files()]
    # the header's prototypes, argument by argument; pivp_cem_update_ex is pivp_cem_update's plus keep, kept_in, add_mean, beta
    header = open(os.path.join(ROOT, 'include', 'pivp_mpc.h')).read()
    i, f, vp, ull = _lib._i, _lib._f, _lib._vp, ctypes.c_ulonglong
    for name in NEW:
        proto = re.search(r'int %s\(([^)]*)\);' % name, header).group(1)
        kinds = [vp if '*' in a else (f if a.strip().startswith('float') else (ull if 'unsigned long long' in a else i)) for a in proto.split(',')]
        res, args = _lib.MPC_SIGNATURES[name]
        assert res is i and kinds == args, name
        fn = getattr(lib, name)                                                # load() bound the new table too
        assert fn.argtypes == args and fn.restype is i
    old = _lib.SIGNATURES['pivp_cem_update'][1]
    assert _lib.MPC_SIGNATURES['pivp_cem_update_ex'][1] == old[:-1] + [i, i, i, f] + old[-1:]
    assert int(re.search(r'#define PIVP_CEM_MAX_COLORED_STEPS (\d+)', header).group(1)) == planning.MAX_COLORED_HORIZON == 64
    # the two kernels share the random numbers through a header instead of two copies
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc')
    for src in ('cem.hip', 'mpc.hip'):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "cem_noise.h"' in text and 'philox4x32_10(unsigned c0' not in text, src


def test_the_ops_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    good = dict(cost=p, actions=p, mean=p, std=p, best_actions=p, best_cost=p, low=p, high=p, el=p, K=8, steps=4, t0=1, elites=3, alpha=0.0,
                min_std=1e-3, seed=1, it=0, keep=2, kept_in=0, add_mean=1, beta=1.0)

    def ex(**over):
        a = dict(good, **over)
        return lib.pivp_cem_update_ex(a['cost'], a['actions'], a['mean'], a['std'], a['best_actions'], a['best_cost'], a['low'], a['high'], a['el'], a['K'],
                                      a['steps'], a['t0'], a['elites'], a['alpha'], a['min_std'], ctypes.c_ulonglong(a['seed']), a['it'], a['keep'],
                                      a['kept_in'], a['add_mean'], a['beta'], None)
    nan, inf = float('nan'), float('inf')
    bad = [dict(actions=None), dict(mean=None), dict(std=None), dict(best_actions=None), dict(best_cost=None), dict(low=None), dict(high=None),
           dict(K=0), dict(K=1025), dict(steps=0), dict(t0=-1), dict(t0=4), dict(it=-1), dict(elites=0), dict(elites=9), dict(alpha=-0.1), dict(alpha=1.5),
           dict(alpha=nan), dict(min_std=-1.0), dict(keep=-1), dict(keep=4), dict(kept_in=2), dict(kept_in=-1), dict(add_mean=2), dict(add_mean=-1),
           dict(K=3, keep=3, add_mean=1), dict(K=1, elites=1, keep=1, add_mean=1),            # keep + add_mean > K
           dict(beta=-0.5), dict(beta=nan), dict(beta=inf), dict(steps=66, t0=1, beta=0.5), dict(steps=65, t0=0, beta=2.0)]      # n = 65 with colored noise
    for over in bad:
        assert ex(**over) == -1, over

    sgood = dict(mean=p, std=p, actions=p, best_actions=p, best_cost=p, low=p, high=p, tail_mean=p, tail_std=p, floor=p, K=8, steps=5, t0=1, keep=2, shift=1)

    def sh(**over):
        a = dict(sgood, **over)
        return lib.pivp_cem_shift(a['mean'], a['std'], a['actions'], a['best_actions'], a['best_cost'], a['low'], a['high'], a['tail_mean'], a['tail_std'],
                                  a['floor'], a['K'], a['steps'], a['t0'], a['keep'], a['shift'], None)
    sbad = [dict(mean=None), dict(std=None), dict(tail_mean=None), dict(tail_std=None), dict(floor=None), dict(low=None), dict(high=None),
            dict(actions=None), dict(K=0), dict(K=1025), dict(keep=-1), dict(keep=9), dict(t0=-1), dict(t0=5), dict(shift=0), dict(shift=4), dict(shift=-1),
            dict(steps=2, t0=1), dict(steps=70000, t0=0)]                                      # n = 1: nothing to shift; n > 65536
    for over in sbad:
        assert sh(**over) == -1, over


def _good(**over):
    kw = dict(context_images=np.zeros((2, 1, 3, 64, 64), np.float32), state=np.zeros((1, 5), np.float32), designated_rc=[[32, 32]], goal_rc=[[40, 24]],
              horizon=3, past_actions=np.zeros((1, 5), np.float32), samples=8, elites=3)
    kw.update(over)
    return kw


def _warm(horizon=3, keep=2, **over):
    kw = dict(mean=torch.zeros(horizon, 5), std=torch.ones(horizon, 5), kept=torch.zeros(horizon, keep, 5) if keep else None)
    kw.update(over)
    return planning.PlanWarmStart(**kw)


def test_cem_plan_option_errors_come_before_the_library():
    m = pivp_amd.Model(10, num_frame_before_prediction=2)
    sig = inspect.signature(planning.cem_plan).parameters
    assert [(sig[k].default) for k in ('keep_elites', 'add_mean', 'noise_beta', 'warm', 'designated_planes')] == [0, False, 0.0, None, None]
    one_hot = planning.one_hot_planes([[[32, 32]]], 64, 64)[0]
    neg, nan = one_hot.clone(), one_hot.clone()
    neg[0, 0, 0], nan[0, 1, 1] = -1.0, float('nan')
    bad = [dict(keep_elites=-1), dict(keep_elites=4), dict(keep_elites=1.0), dict(keep_elites=True), dict(add_mean=1), dict(add_mean='yes'),
           dict(samples=3, elites=3, keep_elites=3, add_mean=True),                            # no slot left for the mean
           dict(noise_beta=-1.0), dict(noise_beta=float('nan')), dict(noise_beta=float('inf')), dict(noise_beta='1'), dict(noise_beta=True),
           dict(noise_beta=0.5, horizon=65),
           dict(warm=(torch.zeros(3, 5), torch.ones(3, 5))), dict(warm=_warm(horizon=4), keep_elites=2), dict(warm=_warm(keep=2), keep_elites=3),
           dict(warm=_warm(keep=2)),                                                           # kept sequences, but keep_elites = 0
           dict(designated_planes=one_hot),                                                    # with designated_rc: one or the other
           dict(designated_rc=None, designated_planes=one_hot[0]), dict(designated_rc=None, designated_planes=torch.zeros(1, 32, 64)),
           dict(designated_rc=None, designated_planes=torch.zeros(9, 64, 64)), dict(designated_rc=None, designated_planes=neg),
           dict(designated_rc=None, designated_planes=nan), dict(designated_rc=None, designated_planes=torch.zeros(1, 64, 64, dtype=torch.int32)),
           dict(designated_rc=None, designated_planes=one_hot, goal_rc=[[1, 2], [3, 4]]), dict(designated_rc=None, designated_planes=one_hot, goal_rc=None)]
    calls = []
    real, _lib.load = _lib.load, lambda: calls.append(1) or real()
    try:
        for over in bad:
            with pytest.raises(ValueError):
                planning.cem_plan(m, **_good(**over))
        for kw in (dict(mean=np.zeros((3, 5)), std=torch.ones(3, 5)), dict(mean=torch.zeros(3, 5), std=torch.ones(3, 4)), dict(mean=torch.zeros(3, 4), std=torch.ones(3, 4)),
                   dict(mean=torch.zeros(3, 5, dtype=torch.float64), std=torch.ones(3, 5)), dict(mean=torch.zeros(3, 5), std=torch.ones(3, 5), kept=torch.zeros(3, 5)),
                   dict(mean=torch.zeros(3, 5), std=torch.ones(3, 5), kept=torch.zeros(2, 2, 5)), dict(mean=torch.zeros(3, 5), std=torch.ones(3, 5), kept=torch.zeros(3, 0, 5))):
            with pytest.raises(ValueError):
                planning.PlanWarmStart(**kw)
        res = planning.PlanResult(mean=torch.zeros(3, 5), std=torch.ones(3, 5), kept=None, _low=None, _high=None, _model=None)
        for kw in (dict(shift=0), dict(shift=3), dict(shift=1.0), dict(shift=True), dict(tail_mean=np.zeros(4)), dict(tail_mean=float('nan')), dict(tail_std=-1.0),
                   dict(std_floor=-0.5), dict(std_floor=np.full(5, np.inf))):
            with pytest.raises(ValueError):
                res.warm_start(**kw)
        # the options through _check_cem_args: what the loop reads
        kw = _good(iterations=2)
        ctx, st = kw.pop('context_images'), kw.pop('state')
        check = lambda **over: planning._check_cem_args(m, ctx, st, **dict(kw, **over))
        off = check()
        assert (off.keep, off.add_mean, off.beta, off.warm, off.planes, off.ex, off.belief, off.image) == (0, False, 0.0, None, None, False, None, None)
        a = check(keep_elites=2, add_mean=True, noise_beta=1.5)
        assert (a.keep, a.add_mean, a.beta, a.ex) == (2, True, 1.5, True)
        w = _warm()
        assert check(keep_elites=2, warm=w).warm is w
        assert check(warm=_warm(keep=0)).ex is True      # a warm start alone
        a = check(designated_rc=None, designated_planes=one_hot)
        assert a.P == 1 and a.planes is one_hot and a.ex is False and a.goals.tolist() == [[40.0, 24.0]]
        # one shape of checked values, whoever asks and whatever is switched on
        train = pivp_amd.Model(10, num_frame_before_prediction=2, keep_activations=True)
        g64 = np.zeros((3, 64, 64), np.float32)
        on = check(keep_elites=2, add_mean=True, noise_beta=1.5, warm=w, goal_image=g64, designated_rc=None, designated_planes=one_hot)
        refine = planning._check_cem_refine_args(train, ctx, st, 3, g64, kw['past_actions'], 2, 0.05, dict(samples=8, elites=3)).cem
        ctl = planning.MPC(pivp_amd.Model(10, carry_state=True), 3, goal_rc=[[40, 24]], samples=8, elites=3, keep_elites=2)
        reset = ctl._check_reset_args(ctx, st, kw['past_actions'], [[32, 32]]).cem
        assert set(vars(off)) == set(vars(on)) == set(vars(refine)) == set(vars(reset))
        assert (refine.keep, refine.add_mean, refine.beta, refine.warm, refine.planes, refine.ex, refine.belief, refine.P) == (0, False, 0.0, None, None, False, None, 0)
        assert (reset.keep, reset.ex, reset.warm, reset.P, reset.goals.tolist()) == (2, True, None, 1, [[40.0, 24.0]]) and reset.planes.shape == (1, 64, 64)
        assert reset.belief is planning._BELIEF_TO_COME and not hasattr(ctl, '_cem') and not hasattr(ctl, '_options') and not hasattr(planning, '_check_plan_args')
        # cem_refine refuses what it does not serve instead of dropping it
        for over in (dict(keep_elites=1), dict(add_mean=True), dict(noise_beta=1.0), dict(warm=w), dict(designated_planes=one_hot)):
            with pytest.raises(ValueError, match='closed-loop'):
                planning.cem_refine(train, ctx, st, 3, g64, past_actions=kw['past_actions'], **over)
    finally:
        _lib.load = real
    assert not calls


def test_mpc_argument_errors_come_before_the_library():
    on, off = pivp_amd.Model(10, carry_state=True), pivp_amd.Model(10)
    M = planning.MPC
    calls = []
    real, _lib.load = _lib.load, lambda: calls.append(1) or real()
    try:
        for kw in (dict(model=off), dict(planner=off), dict(horizon=1), dict(horizon=2.0), dict(horizon=True), dict(warm_iterations=0), dict(warm_iterations=1.5),
                   dict(renormalize=1), dict(seed=-1), dict(seed=2 ** 63), dict(seed=0.5), dict(goal_rc=None), dict(tail_mean=np.zeros(3)),
                   dict(tail_std=-1.0), dict(std_floor=float('nan')), dict(init_std=np.ones((2, 5)))):
            with pytest.raises(ValueError):
                M(**dict(dict(model=on, horizon=3, goal_rc=[[40, 24]]), **kw))
        c = M(on, 3, goal_rc=[[40, 24]], samples=8, elites=3, init_mean=[0.1, 0, 0, 0, 0], init_std=0.5)
        assert c.tail_mean.tolist() == [0.1, 0, 0, 0, 0] and c.tail_std.tolist() == [0.5] * 5 and c.std_floor.tolist() == [0.5] * 5
        assert M(on, 3, goal_rc=[[40, 24]], tail_std=2.0, std_floor=0.25).std_floor.tolist() == [0.25] * 5
        for method in (c.act, lambda: c.observe(np.zeros((3, 64, 64)), np.zeros(5))):
            with pytest.raises(RuntimeError, match='reset'):
                method()
        frames, st = np.zeros((2, 1, 3, 64, 64), np.float32), np.zeros((1, 5), np.float32)
        r = c._check_reset_args(frames, st, np.zeros((1, 5)), [[32, 32]])
        assert (r.n, r.H, r.W, r.cem.P, r.cem.ctx, r.cem.horizon, r.cem.K) == (2, 64, 64, 1, 1, 3, 8) and r.planes.shape == (1, 1, 64, 64)
        assert float(r.planes.sum()) == 1.0 and float(r.planes[0, 0, 32, 32]) == 1.0
        assert c._check_reset_args(frames[:1], st, None, [[32, 32]]).n == 1
        for args in ((frames[:, 0], st, np.zeros((1, 5)), [[32, 32]]), (frames[:0], st, None, [[32, 32]]), (frames, np.zeros(5), np.zeros((1, 5)), [[32, 32]]),
                     (frames, st, None, [[32, 32]]), (frames, st, np.zeros((2, 5)), [[32, 32]]), (frames, st, np.full((1, 5), np.nan), [[32, 32]]),
                     (frames[:1], st, np.zeros((1, 5)), [[32, 32]]), (frames, st, np.zeros((1, 5)), None), (frames, st, np.zeros((1, 5)), [[64, 0]]),
                     (frames, st, np.zeros((1, 5)), [[1, 2], [3, 4]])):
            with pytest.raises(ValueError):
                c.reset(*args)
        image_only = M(on, 3, goal_image=np.zeros((3, 64, 64), np.float32), samples=8, elites=3)
        assert image_only._check_reset_args(frames, st, np.zeros((1, 5)), None).cem.P == 0
        with pytest.raises(ValueError):
            image_only.reset(frames, st, np.zeros((1, 5)), [[32, 32]])                       # pixels without goals
        for kw in (dict(keep_elites=4), dict(add_mean=1), dict(noise_beta=-1.0), dict(samples=0), dict(chunk=3)):      # cem_plan's own complaints, at reset
            with pytest.raises(ValueError):
                M(on, 3, goal_rc=[[40, 24]], **dict(dict(samples=8, elites=3), **kw)).reset(frames, st, np.zeros((1, 5)), [[32, 32]])
    finally:
        _lib.load = real
    assert not calls


# ---- the restatement's own properties -------------------------------------------------------------------------------------------------------
def test_color_matrix_rows_have_unit_norm():
    for n in list(range(1, 13)) + [64]:
        for beta in (0.5, 1.0, 2.0, 3.0):
            Q = MR.color_matrix(n, beta)
            assert Q.shape == (n, n) and np.abs(np.diag(Q @ Q.T) - 1.0).max() < 1e-12, (n, beta)
        assert np.abs(MR.color_matrix(n, 0.0) @ MR.color_matrix(n, 0.0).T - np.eye(n)).max() < 1e-12      # white: orthogonal (but not the identity)
    C = MR.color_matrix(9, 1.0) @ MR.color_matrix(9, 1.0).T
    assert C[0, 1] > 0.3 and MR.color_matrix(9, 2.0)[0] @ MR.color_matrix(9, 2.0)[1] > C[0, 1]      # neighbours correlate, the more the larger beta


def _state(rs, K, n, t0):
    actions = (rs.randn(t0 + n, K, 5) * 0.7)
    return actions, rs.randn(n, 5) * 0.5, 0.3 + rs.rand(n, 5), rs.permutation(K) * 0.37 + 1.0, rs.randn(n, 5)


def test_restatement_defaults_are_cem_update_and_the_options_do_what_the_header_says():
    rs = np.random.RandomState(4)
    K, n, t0, M = 7, 4, 1, 3
    actions, mean, std, cost, best = _state(rs, K, n, t0)
    low, high = np.full(5, -1.2), np.full(5, 1.2)
    kw = dict(t0=t0, elites=M, alpha=0.25, min_std=0.05, seed=77, iteration=2)
    for c in (cost, None):
        a, b = MR.cem_update_ex(c, actions, mean, std, best, np.inf, low, high, **kw), PR.cem_update(c, actions, mean, std, best, np.inf, low, high, **kw)
        assert all(np.array_equal(a[k], b[k]) for k in ('actions', 'mean', 'std', 'best_actions')) and a['best_cost'] == b['best_cost']
    base = PR.cem_update(cost, actions, mean, std, best, np.inf, low, high, **kw)
    got = MR.cem_update_ex(cost, actions, mean, std, best, np.inf, low, high, keep=2, add_mean=1, **kw)      # beta = 0: the identity by definition
    el = base['elites']
    assert np.array_equal(got['actions'][t0:, 0], actions[t0:, el[0]]) and np.array_equal(got['actions'][t0:, 1], actions[t0:, el[1]])
    assert np.array_equal(got['actions'][t0:, 2], np.clip(base['mean'], low, high)) and np.array_equal(got['actions'][t0:, 3:], base['actions'][t0:, 3:])
    assert np.array_equal(got['actions'][:t0], actions[:t0]) and np.array_equal(got['mean'], base['mean'])
    warm = MR.cem_update_ex(None, actions, mean, std, best, np.inf, low, high, keep=2, kept_in=1, **kw)
    cold = MR.cem_update_ex(None, actions, mean, std, best, np.inf, low, high, keep=2, kept_in=0, **kw)
    plain = PR.cem_update(None, actions, mean, std, best, np.inf, low, high, **kw)
    assert np.array_equal(warm['actions'][t0:, :2], actions[t0:, :2]) and np.array_equal(warm['actions'][t0:, 2:], plain['actions'][t0:, 2:])
    assert np.array_equal(cold['actions'], plain['actions'])
    col = MR.cem_update_ex(None, actions, mean, std, best, np.inf, -np.inf, np.inf, beta=1.0, **kw)
    assert not np.array_equal(col['actions'][t0:], plain['actions'][t0:]) and np.array_equal(col['actions'][:t0], actions[:t0])
    # the shift
    sh = MR.cem_shift(mean, std, actions, best, low, high, [3.0, 0, 0, 0, -3.0], 0.7, 0.5, t0, 2, 1)
    assert np.array_equal(sh['mean'][:-1], mean[1:]) and sh['mean'][-1].tolist() == [3.0, 0, 0, 0, -3.0]
    assert np.array_equal(sh['std'][:-1], np.maximum(std[1:], 0.5)) and (sh['std'][-1] == 0.7).all() and sh['best_cost'] == np.inf
    assert np.array_equal(sh['actions'][t0:-1, :2], actions[t0 + 1:, :2]) and sh['actions'][-1, 0].tolist() == [1.2, 0, 0, 0, -1.2]
    assert np.array_equal(sh['actions'][:, 2:], actions[:, 2:]) and np.array_equal(sh['actions'][:t0], actions[:t0])
    assert np.array_equal(sh['best_actions'][:-1], best[1:]) and sh['best_actions'][-1].tolist() == [1.2, 0, 0, 0, -1.2]
    far = MR.cem_shift(mean, std, None, None, None, None, 0.0, 1.0, 0.0, 0, 0, n - 1)
    assert np.array_equal(far['mean'][0], mean[-1]) and (far['mean'][1:] == 0).all() and far['actions'] is None


def test_colored_noise_statistics_of_the_restatement():
    worst, r = MR.colored_noise_statistics(MR.colored_draws(MR.cem_update_ex), 1.0)
    print('restatement, K = 1024, 8 iterations, n = 9, beta = 1: worst deviation %.2f standard errors; lag-1 correlation %.4f' % (worst, r[0]))
    assert worst < 5.0 and r[0] > 0.3
    white, _ = MR.colored_noise_statistics(MR.colored_draws(MR.cem_update_ex, beta=0.0), 1.0)      # the check can fail: white noise is not colored
    assert white > 5.0


def test_warm_starts_win_the_point_mass_closed_loop():
    """Horizon 12, 32 samples, 8 elites, one CEM iteration per control step, 10 control steps, 30 targets from N(0, 8^2) per dimension."""
    targets = np.random.RandomState(7).randn(30, 5) * 8.0
    cold = np.array([MR.point_mass_episode(g, False, seed=100 * i) for i, g in enumerate(targets)])
    warm = np.array([MR.point_mass_episode(g, True, seed=100 * i) for i, g in enumerate(targets)])
    wins = int((warm < cold).sum())
    print('closed-loop cost, median over 30 targets: cold %.1f, warm %.1f; warm better on %d of 30' % (np.median(cold), np.median(warm), wins))
    assert np.median(warm) < np.median(cold) and wins > 15
