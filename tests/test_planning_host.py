"""CPU-side tests of on-device CEM planning: the float64 restatement of the two ops (tests/plan_reference.py) against known answers, the argument
checks of `planning.cem_plan`, and the C-ABI surface of pivp_plan_cost / pivp_cem_update.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib, planning
from pivp_amd.planning import cem_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pivp_plan_cost', 'pivp_cem_update')


def test_header_library_and_ctypes_table_agree_on_the_planning_ops():
    import __graft_entry__ as g
    g.build()
    header = open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', header)) - {'pivp_config', 'pivp_plan'}
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert declared == set(_lib.SIGNATURES) and declared <= exported
    assert _lib.load().pivp_abi_version() == 17                       # added without a version change: nothing else moved
    assert len(_lib.SIGNATURES['pivp_plan_cost'][1]) == 14 and len(_lib.SIGNATURES['pivp_cem_update'][1]) == 18
    from pivp_amd import build
    assert 'cem.hip' in build.SOURCES


def test_philox4x32_10_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in PR.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))) == want
    # vectorised over leading dimensions
    out = PR.philox4x32_10(np.array([k[0] for k in kat], np.uint64), np.array([k[1] for k in kat], np.uint64))
    assert out.shape == (3, 4) and [tuple(int(v) for v in r) for r in out] == [k[2] for k in kat]


def test_uniform_lies_strictly_inside_the_unit_interval_and_normals_are_standard():
    assert PR.uniform(0) == 2.0 ** -25 and PR.uniform(2 ** 32 - 1) == 1.0 - 2.0 ** -25
    assert 0.0 < PR.uniform(0) and PR.uniform(2 ** 32 - 1) < 1.0
    assert PR.uniform(0xff) == PR.uniform(0) and PR.uniform(0x100) == 1.5 * 2.0 ** -24       # the low eight bits are dropped
    z = PR.normals(1000, range(20), 3, 12345)                    # 10^5 normals
    assert z.shape == (20, 1000, 5) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    for d in range(5):
        assert abs(z[..., d].mean()) < 0.03 and abs(z[..., d].std() - 1.0) < 0.03
    # streams: the same (seed, iteration) repeats, another iteration or seed does not; rows are addressed by their index, not their position
    assert np.array_equal(PR.normals(8, range(2, 5), 1, 7), PR.normals(8, range(0, 5), 1, 7)[2:])
    assert not np.array_equal(PR.normals(8, range(3), 1, 7), PR.normals(8, range(3), 2, 7))
    assert not np.array_equal(PR.normals(8, range(3), 1, 7), PR.normals(8, range(3), 1, 7 + 2 ** 32))


def test_reference_loop_converges_on_a_sum_target():
    """K = 64, M = 8, 5 iterations on ||sum_t a_t - g||: the final best cost is below a tenth of the first iteration's best.

    What the remaining choices follow from.  The refit is a FACTORISED Gaussian: selecting on the sum shrinks the sum's variance to a fraction s,
    but refitting each step on its own drops the negative correlation between steps that the selection induced, so the refitted sum keeps the
    fraction 1 - (1 - s) / horizon.  Only a one-step horizon contracts at the selection's own rate (the elite 8 of 64 in five dimensions roughly
    halve the std per refit; four refits are evaluated: 0.5^4 = 0.06), and the mean can travel about 3 std in total, so the target lies about one
    initial std from the initial mean (|g| = 4.2, init_std 4).  The ratio depends on nothing else (|g| / std and the horizon).  Measured over
    seeds 0..15 in that setting: 0.031 .. 0.128, median 0.075, 13 of 16 below 0.1; seed 0 gives 0.080.  A single seed is one draw of that spread, so the
    same criterion is also asserted on the median over the sixteen seeds, which does not hang on any one of them.  At horizon 4 the same loop reaches
    0.22 .. 0.39 of the first best (seeds 0..7): asserted below only as an improvement."""
    g = np.array([1.5, -2.0, 0.5, 3.0, -1.0])
    fn = lambda actions: np.linalg.norm(actions.sum(axis=0) - g, axis=1)
    out = PR.cem_loop(fn, horizon=1, samples=64, elites=8, iterations=5, seed=0, init_std=4.0)
    first = out['trace'][0]['cost'].min()
    print('final / first best: %.4f' % (out['cost'] / first))
    assert out['best_cost_per_iteration'].shape == (5,) and out['best_cost_per_iteration'][0] == first
    assert (np.diff(out['best_cost_per_iteration']) <= 0).all() and out['cost'] == out['best_cost_per_iteration'][-1]
    assert out['cost'] < 0.1 * first, (out['cost'], first)
    assert abs(fn(out['actions'][:, None])[0] - out['cost']) < 1e-12        # the returned sequence is the one that was scored
    ratios = []
    for seed in range(16):
        o = PR.cem_loop(fn, horizon=1, samples=64, elites=8, iterations=5, seed=seed, init_std=4.0)
        ratios.append(o['cost'] / o['trace'][0]['cost'].min())
    print('final / first best over seeds 0..15: median %.4f, %d below 0.1' % (np.median(ratios), sum(r < 0.1 for r in ratios)))
    assert np.median(ratios) < 0.1
    out4 = PR.cem_loop(fn, horizon=4, samples=64, elites=8, iterations=5, seed=0)
    assert (np.diff(out4['best_cost_per_iteration']) <= 0).all() and out4['cost'] < out4['trace'][0]['cost'].min()
    assert abs(fn(out4['actions'][:, None])[0] - out4['cost']) < 1e-12
    # past rows are carried, never resampled
    past = np.arange(10.0).reshape(2, 5)
    out = PR.cem_loop(lambda a: np.linalg.norm(a[2:].sum(axis=0) - g, axis=1), horizon=3, samples=16, elites=4, iterations=2, seed=2, past=past)
    for rec in out['trace']:
        assert (rec['actions'][:2] == past[:, None]).all()


def test_ties_and_nan_costs_rank_as_specified():
    c = np.array([3.0, 1.0, np.nan, 1.0, np.inf, 0.5, 3.0])
    r, cc = PR.ranks(c)
    assert r.tolist() == [3, 1, 5, 2, 6, 0, 4] and cc[2] == np.inf    # ties to the lower index; NaN as +inf, ahead of the later +inf
    assert PR.elite_indices(c, 4).tolist() == [5, 1, 3, 0]
    assert PR.elite_indices(np.full(5, np.nan), 2).tolist() == [0, 1]
    # the refit: by hand on two elites
    actions = np.zeros((1, 3, 5)); actions[0, :, 0] = [1.0, 5.0, 3.0]
    out = PR.cem_update(np.array([2.0, 9.0, 1.0]), actions, np.zeros((1, 5)), np.ones((1, 5)), np.zeros((1, 5)), np.inf, -np.inf, np.inf,
                        t0=0, elites=2, alpha=0.5, min_std=0.25, seed=0, iteration=1)
    assert out['elites'].tolist() == [2, 0] and out['mean'][0, 0] == 0.5 * 2.0 and out['std'][0, 0] == 0.5 + 0.5 * 1.0
    assert out['std'][0, 1] == 0.5 and out['best_cost'] == 1.0 and out['best_actions'][0, 0] == 3.0
    out2 = PR.cem_update(np.array([2.0, 9.0, 1.5]), out['actions'], out['mean'], out['std'], out['best_actions'], out['best_cost'], -0.1, 0.1,
                         t0=0, elites=3, alpha=0.0, min_std=0.25, seed=0, iteration=2)
    assert out2['best_cost'] == 1.0 and out2['best_actions'][0, 0] == 3.0          # not better: the record stays
    assert (out2['std'] >= 0.25).all() and np.abs(out2['actions']).max() <= 0.1      # floor and clamp
    # the cost: a two-point plane by hand, and the miss rule
    t = np.zeros((1, 3, 1, 6, 6)); t[0, 0, 0, 0, 0], t[0, 0, 0, 3, 4] = 0.5, 1.5; t[0, 2, 0, 1, 1] = np.nan
    cost, mass, edist = PR.plan_cost(t, [[0, 0]], [2.0], [1.0], 9.0)
    assert mass[0, 0, 0] == 2.0 and edist[0, 0, 0] == 3.75 and cost.tolist() == [7.5, 18.0, 18.0] and np.isnan(mass[0, 2, 0])


def _good(**kw):
    a = dict(context_images=np.zeros((2, 1, 3, 64, 64), np.float32), state=np.zeros((1, 5), np.float32), designated_rc=[[32, 32]],
             goal_rc=[[40.5, 24]], horizon=4, past_actions=np.zeros((1, 5), np.float32))
    a.update(kw)
    return a


def test_cem_plan_argument_errors_need_no_gpu():
    m = pivp_amd.Model(10, num_frame_before_prediction=2)
    bad = [
        dict(context_images=np.zeros((2, 2, 3, 64, 64), np.float32)),          # a batch of contexts
        dict(context_images=np.zeros((1, 1, 3, 64, 64), np.float32)),          # ctx mismatch
        dict(context_images=np.zeros((2, 1, 2, 64, 64), np.float32)),          # not RGB
        dict(context_images=np.zeros((2, 3, 64, 64), np.float32)),
        dict(state=np.zeros((5,), np.float32)),
        dict(state=np.zeros((2, 5), np.float32)),
        dict(past_actions=None),                                               # required with ctx > 1
        dict(past_actions=np.zeros((2, 5), np.float32)),
        dict(past_actions=np.zeros((1, 4), np.float32)),
        dict(past_actions=np.full((1, 5), np.nan)),
        dict(horizon=0), dict(horizon=2.5), dict(iterations=0), dict(samples=0), dict(samples=2048),
        dict(elites=0), dict(elites=33), dict(samples=8, elites=9),            # elites > samples
        dict(samples=32, chunk=5), dict(samples=32, chunk=64), dict(chunk=0),  # samples % chunk != 0
        dict(designated_rc=np.zeros((0, 2))), dict(designated_rc=np.zeros((9, 2)), goal_rc=np.zeros((9, 2))),     # P outside 1..8
        dict(designated_rc=[[1, 2, 3]]), dict(designated_rc=[[1.5, 2]]),
        dict(designated_rc=[[64, 0]]), dict(designated_rc=[[0, 64]]), dict(designated_rc=[[-1, 3]]),              # outside the frame
        dict(goal_rc=[[63.5, 0]]), dict(goal_rc=[[0, -0.5]]), dict(goal_rc=[[np.nan, 0]]),
        dict(goal_rc=[[1, 1], [2, 2]]),                                        # one goal per designated pixel
        dict(init_mean=np.zeros((3, 5))), dict(init_std=np.zeros((4, 4))), dict(init_std=-1.0), dict(init_mean=np.inf),
        dict(min_std=-1e-3), dict(min_std=np.nan), dict(alpha=1.5), dict(alpha=-0.1),
        dict(action_low=np.zeros(4)), dict(action_low=1.0, action_high=-1.0), dict(action_high=np.nan),
        dict(step_weights=np.ones(3)), dict(step_weights=np.full(4, np.inf)), dict(plane_weights=np.ones(2)),
        dict(miss_cost=np.inf), dict(miss_cost='far'), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            cem_plan(m, **_good(**kw))
    # tensors are read the same way
    with pytest.raises(ValueError):
        cem_plan(m, **_good(context_images=torch.zeros(2, 2, 3, 64, 64)))
    with pytest.raises(ValueError):
        cem_plan(m, **_good(designated_rc=torch.tensor([[70, 2]])))
    # one context frame: there is no past step
    m1 = pivp_amd.Model(10, num_frame_before_prediction=1)
    with pytest.raises(ValueError):
        cem_plan(m1, **_good(context_images=np.zeros((1, 1, 3, 64, 64), np.float32)))
    if not torch.cuda.is_available():
        # good arguments get as far as the GPU requirement: there is no CPU fallback
        for kw in (dict(), dict(samples=32, chunk=8, elites=32), dict(designated_rc=[[1, 2], [3, 4]], goal_rc=[[5, 6], [7, 8]], plane_weights=[1, 2]),
                   dict(designated_rc=(3, 4), goal_rc=(5.5, 6))):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                cem_plan(m, **_good(**kw))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            cem_plan(m1, **_good(context_images=np.zeros((1, 1, 3, 64, 64), np.float32), past_actions=None))
    # the checked values
    good = _good()
    a = planning._check_cem_args(m, good.pop('context_images'), good.pop('state'), **good)      # (everything else: `cem_plan`'s defaults)
    assert abs(a.miss_cost - np.sqrt(2 * 63.0 ** 2)) < 1e-12 and a.chunk == 32 and a.mean.shape == (4, 5) and (a.std == 1).all()
    assert a.low.tolist() == [-np.inf] * 5 and a.step_w.tolist() == [1.0] * 4


def test_score_actions_and_the_helpers_are_still_there():
    assert 'optimiser' in planning.__doc__ and "is the caller's" not in planning.__doc__
    with pytest.raises(ValueError):
        planning.score_actions(None, np.zeros((2, 2, 3, 8, 8)), np.zeros((1, 5)), np.zeros((4, 3, 5)), (1, 1), (2, 2))


def test_this_module_loaded_no_second_copy_of_the_package_s_modules():
    # `from pivp_amd.planning import` hands out the package's own planning.py, whose `config` is the one `pivp_amd.using_config` sets -- and so does
    # every other import through the alias, whichever test module made it
    assert sys.modules['pivp_amd.planning'] is planning is pivp_amd.planning and planning.using_config is pivp_amd.using_config
    own = pivp_amd.__name__
    assert own != 'pivp_amd' and all(mod is sys.modules[own + name[len('pivp_amd'):]] for name, mod in list(sys.modules.items()) if name.startswith('pivp_amd.'))
