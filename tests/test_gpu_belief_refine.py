"""GPU tests of gradient refinement from a belief: `planning.refine_actions(belief=)`, `planning.cem_refine(belief=)` and `planning.MPC(refine_steps=)`.

Bounds.  (a), (b): the project's model-level input-gradient gate, 2e-3 relative under input_grad_reference.rel_errors -- what
tests/test_gpu_state_grad.py::test_input_gradients_after_a_carried_start holds the same sweep to; the float64 reference and its batch seeds are
tests/belief_refine_reference.py's.  (b)'s iteration-0 cost and everything in (c) and (e) are bit for bit: copies, or the same launches on the same
values -- the models of (c) and (e) are built with deterministic=True, because a default model's sweep adds with atomics and a second Adam step would
carry that spread into the actions.  (d): 1e-6 relative, the gate tests/test_gpu_goal_cost.py holds this cost to.

Measured on an MI355X (profiles/r20/NOTES.md):
  (a) d cost / d actions against float64, relative L2 / largest element: CDNA 1.2e-6 / 1.3e-6, STP 1.1e-5 / 8.4e-6, DNA 1.2e-6 / 1.8e-6
      (plain float32 autograd of the restatement on the CPU: 8.9e-7 / 9.9e-7, 8.9e-6 / 5.9e-6, 1.1e-6 / 9.5e-7)
  (b) belief route against frame route: iteration-0 cost equal bits; free rows' gradient 4.6e-7 / 4.7e-7
  (d) score_actions(belief=) against the returned cost: 0 (equal bits on this fixture; not a contract, the gate is the bound)"""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import belief_refine_reference as BR  # noqa: E402
import track_reference as TR  # noqa: E402
from input_grad_reference import rel_errors  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FLAGS = dict(carry_state=True, keep_activations=True, state_backward=True, num_frame_before_prediction=1)
COST_GATE = 1e-6


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _random_model(pivp_amd, case, **kw):
    m = pivp_amd.Model(case['nm'], prefix='t', **dict(case['mkw'], **kw))
    m.load_state_dict_reference(case['P'])
    return m


def _bits(a, b):
    """two tensors hold the same bits (a float32 is compared as its int32 pattern)"""
    import torch
    raw = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


# ---- (a) d cost / d actions of one iteration against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cdna', 'stp', 'dna'])
def test_action_gradient_from_a_belief_matches_float64(name):
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    case, ref = BR.case_inputs(name), BR.reference(name)
    m = _random_model(pivp_amd, case, carry_state=True, keep_activations=True, state_backward=True)
    m.imagine(*case['observed'], observed=1)                  # one observed frame: the belief, one state per sample
    belief = m.recurrent_state()
    assert (belief.batch, belief.hw) == (BR.B, (BR.H, BR.W))
    spec = planning.GoalImageCost(case['goal'], **BR.GOAL)
    refined, costs = planning.refine_actions(m, case['frame'], case['state'], case['actions'], goal_image=spec, steps=1, lr=0.0, belief=belief)
    got = m.action_grad.cpu().numpy()                         # the sweep of iteration 0 (the rollout that scores the result has none)
    e = rel_errors(got, ref['action_grad'])
    ec = np.abs(costs.cpu().numpy().astype(np.float64) / ref['cost'] - 1).max()
    print('refine_actions(belief=) %s: d cost / d actions against float64 rel L2 %.2e max %.2e (max |ref| %.1e); cost %.2e (relative)'
          % (name, e[0], e[1], np.abs(ref['action_grad']).max(), ec))
    assert got.shape == (BR.HORIZON, BR.B, 5) and np.isfinite(got).all()
    assert np.abs(ref['action_grad']).max() > 0 and max(e) < BR.GATE
    assert np.array_equal(refined.cpu().numpy().view(np.uint32), case['actions'].view(np.uint32))      # lr = 0: the input's bits
    assert torch.equal(costs[0], costs[1])


# ---- (b) the belief route against the frame route -----------------------------------------------------------------------------------------------------
def test_the_belief_route_is_the_frame_route():
    """One set of weights in two models: a ctx = 2 model refines from both frames with the step between them as past_actions; a ctx = 1 carrying
    model observes frame 0 (`imagine(observed=1)`) and refines from the belief and frame 1.  A split rollout is the whole one bit for bit, so the
    iteration-0 costs are equal bits; the sweeps differ in where they stop (the belief is a constant), not in what the free rows receive."""
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    case = BR.case_inputs('cdna')
    frame0, action0, state0 = case['observed']
    spec = planning.GoalImageCost(case['goal'], **BR.GOAL)
    two = _random_model(pivp_amd, dict(case, mkw=dict(case['mkw'], num_frame_before_prediction=2)), keep_activations=True)
    _, costs2 = planning.refine_actions(two, np.concatenate((frame0, case['frame'])), state0, np.concatenate((action0, case['actions'])),
                                        goal_image=spec, steps=1, lr=0.0, past_actions=action0)
    g2 = two.action_grad.cpu().numpy()
    one = _random_model(pivp_amd, case, carry_state=True, keep_activations=True, state_backward=True)
    one.imagine(frame0, action0, state0, observed=1)
    belief, state1 = one.recurrent_state(), one.gen_states[-1].clone()
    _, costs1 = planning.refine_actions(one, case['frame'], state1, case['actions'], goal_image=spec, steps=1, lr=0.0, belief=belief)
    g1 = one.action_grad.cpu().numpy()
    e = rel_errors(g1, g2[1:])
    dc = float((costs1[0] - costs2[0]).abs().max())
    print('belief route against frame route: iteration-0 cost differs by %.3g (%s); free rows\' gradient rel L2 %.2e max %.2e'
          % (dc, costs1[0].cpu().numpy().tolist(), e[0], e[1]))
    assert (g2[:1] == 0).all() and np.abs(g2[1:]).max() > 0
    assert _bits(costs1[0], costs2[0])
    assert max(e) < BR.GATE


# ---- the trained fixture ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """The trained CDNA fixture on the moving batch of tests/test_gpu_planning.py: two observed frames, one past action; the goal is a later true frame."""
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    return P, nm, imgs[:2], stas[0], acts[:1, 0], np.ascontiguousarray(imgs[4, 0])


def _trained(pivp_amd, **kw):
    P, nm = _scene()[:2]
    m = pivp_amd.Model(nm, is_cdna=True, prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _spec(planning):
    roi = np.zeros((64, 64), np.float32)
    roi[8:56, 8:56] = 1.0
    roi[24:40, 24:40] = 2.0
    return planning.GoalImageCost(_scene()[5], mse=1.0, l1=0.25, pixel_weight=roi, weight=2.0)


def _observe_first_frame(m):
    """-> (belief, newest frame (1, 1, 3, 64, 64), its robot state (1, 5)): the model has seen frame 0 and the step to frame 1."""
    _, _, ctx_imgs, state0, past, _ = _scene()
    m.reset_state()
    m.imagine(ctx_imgs[:1], past[:, None], state0, observed=1)
    return m.recurrent_state(), ctx_imgs[1:2], m.gen_states[-1].clone()


def _no_sync(torch, fn):
    """fn() under torch.cuda.set_sync_debug_mode('error'); the mode must flag a synchronising call on this build for the run to mean anything."""
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
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
    assert detects, 'torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build'
    return out


# ---- (c) the states are left untouched ----------------------------------------------------------------------------------------------------------------
def test_refinement_from_a_belief_leaves_every_state_untouched():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    m = _trained(pivp_amd, deterministic=True, **FLAGS)
    belief, frame, state = _observe_first_frame(m)
    held, before, belief_before = m._state, m.recurrent_state().data.clone(), belief.data.clone()
    frame2, state2 = np.repeat(frame, 2, axis=1), state.expand(2, -1)
    starts = (0.2 * np.random.RandomState(3).standard_normal((3, 2, 5))).astype(np.float32)
    kw = dict(goal_image=_spec(planning), steps=2, lr=0.02, bounds=(-1.0, 1.0))
    refined, costs = (t.clone() for t in planning.refine_actions(m, frame2, state2, starts, belief=belief, **kw))
    c = costs.cpu().numpy()
    print('refine_actions(belief=) on the trained fixture: costs %s' % (c.tolist(),))
    assert m._state is held and _bits(m.recurrent_state().data, before) and _bits(belief.data, belief_before)
    assert np.isfinite(c).all() and (c[2] < c[0]).all() and (refined.cpu().numpy() != starts).any() and float(refined.abs().max()) <= 1.0
    # one belief per sample is used where it lies, and not written either; the same values give the same bits
    per_sample = belief.expand(2)
    kept = per_sample.data.clone()
    refined_b, costs_b = planning.refine_actions(m, frame2, state2, starts, belief=per_sample, **kw)
    assert _bits(per_sample.data, kept) and _bits(refined_b, refined) and _bits(costs_b, costs)
    assert m._state is held and _bits(m.recurrent_state().data, before)
    # an exception that leaves the loop: the state is what it was

    def failing(gen):
        raise KeyError('the caller\'s cost failed')

    with pytest.raises(KeyError):
        planning.refine_actions(m, frame2, state2, starts, cost_fn=failing, steps=2, lr=0.02, belief=belief)
    assert m._state is held and _bits(m.recurrent_state().data, before) and _bits(belief.data, belief_before)
    # belief=None on the same model: the same call twice, a belief call in between -- the same bits

    def plain():
        m.reset_state()
        return tuple(t.clone() for t in planning.refine_actions(m, frame2, state2, starts, **kw))

    first = plain()
    m.reset_state()
    planning.refine_actions(m, frame2, state2, starts, belief=belief, **kw)
    assert m._state is None                                     # (as on entry here too: nothing carried)
    second = plain()
    assert _bits(first[0], second[0]) and _bits(first[1], second[1])
    assert not _bits(first[1], costs)                           # (from zeros, not from the belief: another rollout)


# ---- (d) cem_refine(belief=) ----------------------------------------------------------------------------------------------------------------------------
def test_cem_refine_from_a_belief_returns_the_cheapest_of_three():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    spec = _spec(planning)
    m = _trained(pivp_amd, **FLAGS)
    belief, frame, state = _observe_first_frame(m)
    held, before, belief_before = m._state, m.recurrent_state().data.clone(), belief.data.clone()
    kw = dict(iterations=2, samples=8, elites=2, init_std=0.5, seed=3, action_low=-1.0, action_high=1.0)
    res = planning.cem_refine(m, frame, state, 2, spec, belief=belief, refine_steps=2, lr=0.02, **kw)
    source = int(res.source)
    three = [float(res.cem.cost)] + res.refine_costs[-1].cpu().numpy().tolist()
    print('cem_refine(belief=): CEM best %.6g, refined best %.6g, refined mean %.6g -> source %d; refine costs %s'
          % (three[0], three[1], three[2], source, res.refine_costs.cpu().numpy().tolist()))
    assert source in (0, 1, 2) and res.actions.shape == (2, 5) and res.refine_costs.shape == (3, 2)
    assert float(res.cost) <= float(res.cem.cost) and float(res.cost) == min(three) and source == int(np.argmin(three))
    acts = res.actions.cpu().numpy()
    assert np.abs(acts).max() <= 1.0
    assert m._state is held and _bits(m.recurrent_state().data, before) and _bits(belief.data, belief_before)
    # CEM's stage is cem_plan(belief=)'s: the same seed, the same plan
    plain = planning.cem_plan(_trained(pivp_amd, carry_state=True), frame, state, None, None, 2, goal_image=spec, belief=belief, **kw)
    assert torch.equal(plain.actions, res.cem.actions) and torch.equal(plain.cost, res.cem.cost) and torch.equal(plain.mean, res.cem.mean)
    # the returned actions score the returned cost
    scored = float(planning.score_actions(_trained(pivp_amd, carry_state=True), frame, state, acts[None], None, None, belief=belief, goal_image=spec)[0])
    d_score = abs(scored / float(res.cost) - 1)
    print('cem_refine(belief=): score_actions(belief=) against the returned cost %.2e (relative)' % d_score)
    assert d_score < COST_GATE
    # the loop under sync debug mode, its uploads in front
    a = planning._check_cem_refine_args(m, frame, state, 2, spec, None, 2, 0.02, dict(kw), belief)
    b = planning._cem_refine_upload(m, a, frame, state)
    quiet = _no_sync(torch, lambda: planning._cem_refine_iterate(m, a, b))
    assert torch.equal(quiet.cem.actions, res.cem.actions) and torch.isfinite(quiet.actions).all()


# ---- (e) the controller -------------------------------------------------------------------------------------------------------------------------------
MPC_SETUP = dict(horizon=3, iterations=2, samples=8, elites=3, init_std=0.5, keep_elites=2, warm_iterations=1, action_low=-1.0, action_high=1.0)
PLAN_FIELDS = ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration', 'kept')


def _episode(torch, pivp_amd, refine=None, seed=5, steps=3, check=False, quiet=False):
    """`steps` control steps of `planning.MPC` on a goal image in an environment that is a second model with the same weights.  refine: None (a
    controller built without the keywords) or refine_steps.  check: every step against the manual composition on a third model.  quiet: act() and
    observe() run under the sync debug mode.  -> (actions, per step the plan's fields as copies)."""
    from pivp_amd import planning
    _, _, ctx_imgs, state0, past, _ = _scene()
    spec = _spec(planning)
    env, m = _trained(pivp_amd, carry_state=True), _trained(pivp_amd, deterministic=True, **FLAGS)
    extra = {} if refine is None else dict(refine_steps=refine, refine_lr=0.02)
    ctl = planning.MPC(m, goal_image=spec, seed=seed, **dict(MPC_SETUP, **extra))
    ctl.reset(ctx_imgs, state0, past)
    run = (lambda fn: _no_sync(torch, fn)) if quiet else (lambda fn: fn())
    env.imagine(ctx_imgs[:1], past[:, None], state0, observed=1)                        # the world has seen what the robot has
    frame, state = torch.from_numpy(ctx_imgs[1:2]).to(DEV), env.gen_states[-1].clone()
    if check:
        man = _trained(pivp_amd, deterministic=True, **FLAGS)
        man.imagine(ctx_imgs[:1], past[:, None], state0, observed=1)
        warm = None
    actions, plans = [], []
    for step in range(steps):
        action = run(ctl.act)
        plan = ctl.last_plan
        assert action.shape == (5,) and action.is_cuda and ctl.step == step and torch.equal(action, plan.actions[0])
        actions.append(action.clone())
        plans.append({k: getattr(plan, k).clone() for k in PLAN_FIELDS + (('source', 'refine_costs') if refine else ())})
        assert hasattr(plan, 'source') == bool(refine)
        if check:
            res = planning.cem_plan(man, frame, state, None, None, 3, iterations=2 if step == 0 else 1, samples=8, elites=3, init_std=0.5, keep_elites=2,
                                    action_low=-1.0, action_high=1.0, seed=seed + step, belief=man.recurrent_state(), warm=warm, goal_image=spec)
            refined, costs = planning.refine_actions(man, frame.expand(-1, 2, -1, -1, -1), state.expand(2, -1), torch.stack((res.actions, res.mean), dim=1),
                                                     goal_image=spec, steps=refine, lr=0.02, bounds=(-1.0, 1.0), belief=man.recurrent_state())
            three_costs = torch.cat((res.cost.view(1), costs[-1]))
            three = torch.cat((res.actions.unsqueeze(0), refined.transpose(0, 1)))
            source = int(torch.argmin(three_costs))
            print('MPC(refine_steps=%d) step %d: CEM best %.6g, refined best %.6g, refined mean %.6g -> source %d'
                  % ((refine, step) + tuple(three_costs.cpu().numpy().tolist()) + (source,)))
            if source > 0:
                res.kept[:, 0] = three[source]
            got = plans[-1]
            assert int(got['source']) == source and _bits(got['refine_costs'], costs)
            assert _bits(got['actions'], three[source]) and _bits(got['cost'], three_costs[source]) and _bits(action, three[source][0])
            for name in ('mean', 'std', 'best_cost_per_iteration', 'kept'):
                assert _bits(got[name], getattr(res, name)), (step, name)
            assert float(got['cost']) <= float(res.cost)
        env.imagine(frame, action.view(1, 1, 5), state, observed=1)                     # the world moves
        new_frame, new_state = env.gen_images[-1].clone().view(1, 1, 3, 64, 64), env.gen_states[-1].clone()
        run(lambda: ctl.observe(new_frame, new_state))
        if check:
            man.imagine(frame, action.view(1, 1, 5), state, observed=1)
            assert _bits(man.recurrent_state().data, m.recurrent_state().data)              # the belief: the polish left it alone
            warm = res.warm_start(shift=1, tail_mean=0.0, tail_std=0.5, std_floor=0.5)
            assert all(_bits(getattr(warm, k), getattr(ctl._warm, k)) for k in ('mean', 'std', 'kept'))      # the polished plan travels on
        frame, state = new_frame, new_state
    return torch.stack(actions), plans


def test_mpc_with_refinement_is_the_manual_composition_bit_for_bit():
    torch, pivp_amd = _gpu()
    a, plans = _episode(torch, pivp_amd, refine=2, check=True)
    assert torch.isfinite(a).all() and float(a.abs().max()) <= 1.0
    # the same steps never synchronise with the host after reset(), and give the same bits
    b, plans_b = _episode(torch, pivp_amd, refine=2, quiet=True)
    assert _bits(a, b) and all(_bits(p[k], q[k]) for p, q in zip(plans, plans_b) for k in p)


def test_mpc_without_refinement_is_the_controller_it_was():
    torch, pivp_amd = _gpu()
    off, plans_off = _episode(torch, pivp_amd, refine=0, steps=2)
    without, plans_without = _episode(torch, pivp_amd, refine=None, steps=2)
    assert _bits(off, without) and all(_bits(p[k], q[k]) for p, q in zip(plans_off, plans_without) for k in PLAN_FIELDS)
