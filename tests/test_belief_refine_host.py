"""CPU-side tests of gradient refinement from a belief: the new keywords of `planning.refine_actions`, `planning.cem_refine` and `planning.MPC`
and their defaults, every refusal (raised before the GPU or the library is needed), `_refine_iterate`'s handling of the start state with a stub in
the model's place (tests/test_input_grad_host.py's manner), and the default controller's arguments.  No GPU."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import planning
from pivp_amd.state import RecurrentState, state_layout

H = W = 16
z = np.zeros


def _belief(batch=1, hw=(H, W)):
    return RecurrentState(torch.zeros(batch * state_layout(*hw)[1]), batch, hw)


def _model(ctx=1, **kw):
    flags = dict(carry_state=True, keep_activations=True, state_backward=True)
    flags.update(kw)
    return pivp_amd.Model(3, num_frame_before_prediction=ctx, **flags)


def _refine_args(**over):
    kw = dict(model=_model(), context_images=z((1, 2, 3, H, W), np.float32), state=z((2, 5), np.float32), actions=z((3, 2, 5), np.float32),
              goal_image=z((3, H, W), np.float32), cost_fn=None, steps=2, lr=0.1, past_actions=None, bounds=None, belief=_belief())
    kw.update(over)
    return kw


# ---- the interface -----------------------------------------------------------------------------------------------------------------------------
def test_the_new_keywords_and_their_defaults():
    sig = lambda f: inspect.signature(f).parameters
    assert sig(planning.refine_actions)['belief'].default is None
    assert sig(planning.cem_refine)['belief'].default is None and sig(planning.cem_refine)['belief'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    mpc = sig(planning.MPC.__init__)
    assert [mpc[k].default for k in ('refine_steps', 'refine_lr', 'refiner')] == [0, 0.05, None]
    assert sig(planning._check_refine_args)['belief'].default is None and sig(planning._check_cem_refine_args)['belief'].default is None
    # the earlier parameters keep their places: what was called by position still is
    assert list(sig(planning.refine_actions))[:10] == ['model', 'context_images', 'state', 'actions', 'goal_image', 'cost_fn', 'steps', 'lr', 'past_actions',
                                                       'bounds']
    assert list(sig(planning.cem_refine))[:8] == ['model', 'context_images', 'state', 'horizon', 'goal_image', 'past_actions', 'refine_steps', 'lr']
    for f in (planning.refine_actions, planning.cem_refine, planning.MPC):
        assert 'belief' in f.__doc__ and 'state_backward=True' in f.__doc__
    assert 'refine_actions(belief=)' in planning.__doc__ and 'MPC(refine_steps=)' in planning.__doc__
    assert 'same checkpoint' in planning.MPC.__doc__


def test_refine_actions_accepts_a_belief_of_batch_one_or_b():
    a = planning._check_refine_args(**_refine_args())
    assert (a.ctx, a.B, a.H, a.W, a.steps_T, a.n_past, a.iters) == (1, 2, H, W, 3, 0, 2) and a.belief.batch == 1
    assert planning._check_refine_args(**_refine_args(belief=_belief(2))).belief.batch == 2
    assert planning._check_refine_args(**_refine_args(belief=None)).belief is None
    wide = _model(action_dim=3, state_dim=7)      # any width the model has
    a = planning._check_refine_args(**_refine_args(model=wide, state=z((2, 7), np.float32), actions=z((3, 2, 3), np.float32)))
    assert a.steps_T == 3


@pytest.mark.parametrize('flag', planning.REFINE_BELIEF_FLAGS)
def test_refine_actions_names_the_missing_model_flag(flag):
    kw = {'carry_state': dict(carry_state=False, state_backward=False), 'keep_activations': dict(keep_activations=False, state_backward=False),
          'state_backward': dict(state_backward=False)}[flag]
    with pytest.raises(ValueError, match='%s=True is missing' % flag):
        planning._check_refine_args(**_refine_args(model=_model(**kw)))
    with pytest.raises(ValueError, match='%s=True is missing' % flag):      # the public function: before the GPU or the library is needed
        planning.refine_actions(_model(**kw), z((1, 2, 3, H, W)), z((2, 5)), z((3, 2, 5)), goal_image=z((3, H, W)), belief=_belief())
    assert planning.REFINE_BELIEF_FLAGS == ('carry_state', 'keep_activations', 'state_backward')


def test_refine_actions_belief_refusals():
    with pytest.raises(ValueError, match='num_frame_before_prediction=1'):
        planning._check_refine_args(**_refine_args(model=_model(ctx=2), context_images=z((2, 2, 3, H, W)), actions=z((4, 2, 5))))
    with pytest.raises(ValueError, match='num_frame_before_prediction=1'):
        planning._check_refine_args(**_refine_args(model=_model(ctx=2)))
    with pytest.raises(ValueError, match='newest frame only'):
        planning._check_refine_args(**_refine_args(context_images=z((2, 2, 3, H, W))))
    for past in (z((0, 5)), z((1, 5)), z((1, 2, 5))):
        with pytest.raises(ValueError, match='past_actions given with a belief'):
            planning._check_refine_args(**_refine_args(past_actions=past))
    with pytest.raises(ValueError, match='32x32 frames'):
        planning._check_refine_args(**_refine_args(belief=_belief(1, (32, 32))))
    with pytest.raises(ValueError, match='holds 3 samples'):
        planning._check_refine_args(**_refine_args(belief=_belief(3)))
    look_alike = SimpleNamespace(data=torch.zeros(4), batch=1, hw=(H, W))
    for bad in (look_alike, object(), _belief().data, 1):
        with pytest.raises(ValueError, match='belief must be a RecurrentState'):
            planning._check_refine_args(**_refine_args(belief=bad))
    # what was refused without a belief still is
    for over in (dict(state=z((1, 5))), dict(actions=z((3, 2, 4))), dict(goal_image=None), dict(steps=0), dict(bounds=(1.0, 0.0)),
                 dict(goal_image=z((3, 8, 8)))):
        with pytest.raises(ValueError):
            planning._check_refine_args(**_refine_args(**over))


def test_cem_refine_belief_refusals():
    frame, st, goal = z((1, 1, 3, H, W), np.float32), z((1, 5), np.float32), z((3, H, W), np.float32)
    a = planning._check_cem_refine_args(_model(), frame, st, 3, goal, None, 2, 0.02, dict(samples=8, elites=2), _belief())
    assert (a.cem.ctx, a.cem.horizon, a.refine.B, a.refine.steps_T, a.refine.n_past) == (1, 3, 2, 3, 0)
    assert a.cem.belief is a.refine.belief and a.cem.image is a.spec
    plain = planning._check_cem_refine_args(_model(ctx=2, carry_state=False, state_backward=False), z((2, 1, 3, H, W)), st, 3, goal, z((1, 5)), 2, 0.02,
                                            dict(samples=8, elites=2))
    assert sorted(vars(plain.cem)) == sorted(vars(a.cem))      # `_check_cem_args`' result keeps one shape for every caller
    assert plain.cem.belief is None and plain.refine.belief is None
    run = lambda model=None, **kw: planning.cem_refine(model if model is not None else _model(), kw.pop('frame', frame), st, 3, goal,
                                                       **dict(dict(belief=_belief()), **kw))
    with pytest.raises(ValueError, match='past_actions given with a belief'):
        run(past_actions=z((0, 5)))
    with pytest.raises(ValueError, match='belief must be a RecurrentState'):
        run(belief=object())
    with pytest.raises(ValueError, match='batch-1'):
        run(belief=_belief(2))
    with pytest.raises(ValueError, match='32x32'):
        run(belief=_belief(1, (32, 32)))
    with pytest.raises(ValueError, match='newest frame only'):
        run(frame=z((2, 1, 3, H, W)))
    with pytest.raises(ValueError, match='keep_activations'):
        run(_model(keep_activations=False, state_backward=False))
    with pytest.raises(ValueError, match='carry_state=True'):
        run(_model(carry_state=False, state_backward=False))
    with pytest.raises(ValueError, match='state_backward=True is missing'):
        run(_model(state_backward=False))
    with pytest.raises(ValueError, match='num_frame_before_prediction'):
        run(_model(ctx=2))
    for kw in (dict(designated_rc=[[1, 2]]), dict(goal_rc=[[1, 2]]), dict(keep_elites=1), dict(add_mean=True), dict(noise_beta=1.0),
               dict(warm=object())):
        with pytest.raises(ValueError, match='not served|does not serve'):
            run(**kw)


def test_mpc_refine_refusals_and_the_default_controller():
    goal = z((3, H, W), np.float32)
    m = _model()
    with pytest.raises(ValueError, match='give goal_image'):
        planning.MPC(m, 3, goal_rc=[[4, 4]], refine_steps=2)
    with pytest.raises(ValueError, match='not served with goal_rc'):
        planning.MPC(m, 3, goal_image=goal, goal_rc=[[4, 4]], refine_steps=2)
    for flag, kw in (('carry_state', None), ('keep_activations', dict(keep_activations=False, state_backward=False)),
                     ('state_backward', dict(state_backward=False))):
        refiner = pivp_amd.Model(3, num_frame_before_prediction=1, keep_activations=True) if kw is None else _model(**kw)
        with pytest.raises(ValueError, match='refiner.*%s=True is missing' % flag):
            planning.MPC(m, 3, goal_image=goal, refine_steps=2, refiner=refiner)
    with pytest.raises(ValueError, match='keep_activations=True is missing'):      # the refiner defaults to the model
        planning.MPC(_model(keep_activations=False, state_backward=False), 3, goal_image=goal, refine_steps=1)
    with pytest.raises(ValueError, match='num_frame_before_prediction=1'):
        planning.MPC(m, 3, goal_image=goal, refine_steps=2, refiner=_model(ctx=2))
    for bad in (dict(refine_steps=-1), dict(refine_steps=1.0), dict(refine_steps=True), dict(refine_lr=-0.1), dict(refine_lr=float('nan'))):
        with pytest.raises(ValueError):
            planning.MPC(m, 3, goal_image=goal, **bad)
    with pytest.raises(ValueError, match='five-column'):      # the controller stays five wide
        planning.MPC(_model(action_dim=4), 3, goal_image=goal, refine_steps=2)._check_reset_args(z((1, 1, 3, H, W)), z((1, 5)), None, None)
    # refine_steps = 0 is the controller without the keyword: the same plan arguments, no refiner, nothing checked for the polish
    plain_model = pivp_amd.Model(3, carry_state=True)      # (neither keep_activations nor state_backward: today's controller asks for neither)
    off, without = planning.MPC(plain_model, 3, goal_image=goal, refine_steps=0, samples=8, elites=2), planning.MPC(plain_model, 3, goal_image=goal,
                                                                                                                  samples=8, elites=2)
    assert off._plan_arguments == without._plan_arguments and sorted(vars(off)) == sorted(vars(without))
    assert (off.refine_steps, off.refiner, without.refine_steps, without.refiner) == (0, None, 0, None)
    frames2 = z((2, 1, 3, H, W), np.float32)
    r_off, r_without = (c._check_reset_args(frames2, z((1, 5)), z((1, 5)), None) for c in (off, without))
    assert r_off.refine is None and r_without.refine is None and sorted(vars(r_off.cem)) == sorted(vars(r_without.cem))
    # refine_steps > 0: the polish is checked at batch 2 under the controller's action bounds, before the GPU is needed
    ctl = planning.MPC(m, 3, goal_image=goal, refine_steps=2, refine_lr=0.01, samples=8, elites=2, action_low=-1.0, action_high=[1, 2, 3, 4, 5])
    r = ctl._check_reset_args(frames2, z((1, 5)), z((1, 5)), None)
    assert ctl.refiner is m and (r.refine.B, r.refine.steps_T, r.refine.iters, r.refine.lr, r.refine.n_past) == (2, 3, 2, 0.01, 0)
    assert r.refine.low.tolist() == [-1.0] * 5 and r.refine.high.tolist() == [1, 2, 3, 4, 5]
    assert planning.MPC(m, 3, goal_image=goal, refine_steps=1)._check_reset_args(frames2, z((1, 5)), z((1, 5)), None).refine.low is None


# ---- the loop and the start state, with a stub in the model's place ----------------------------------------------------------------------------------
class _StubCarrying(object):
    """Stands in for a state_backward model in `_refine_iterate`: frames gen[t, b] = reshape(W act[t, b]) (3 x 2 x 2), as tests/test_input_grad_host.py's
    stub.  A call starts from `_state`, leaves its final state in `_spare_state`'s buffer and keeps the start as the spare -- `Model._carried`'s hand-over."""

    def __init__(self, W):
        self.num_frame_before_prediction, self.W = 1, W
        self.scheduled_sampling_k = 7.0
        self._state, self._spare_state = 'entry state', 'entry spare'
        self.adopted, self.started, self.swept_from = [], [], []
        self.action_grad = None

    def _adopt_state(self, s):
        self.adopted.append(s)
        self._state = s

    def __call__(self, x):
        self.started.append((self._state, self._spare_state))
        self._state, self._spare_state = self._spare_state, self._state
        acts = x[1]
        self._gen = (acts[:-1] @ self.W.T).reshape(acts.shape[0] - 1, acts.shape[1], 3, 2, 2)

    def backward(self, **kw):
        self.swept_from.append(self._spare_state)      # (the sweep reads the state the last call started from)
        fg = kw['frame_grad']
        self.action_grad = fg.reshape(fg.shape[0], fg.shape[1], 12) @ self.W


def _stub_case(belief, iters=3):
    rs = np.random.RandomState(5)
    T1, B = 3, 2
    Wm = torch.from_numpy(rs.standard_normal((12, 5)).astype(np.float32))
    goal = torch.from_numpy(rs.standard_normal((3, 2, 2)).astype(np.float32))
    a = SimpleNamespace(ctx=1, B=B, H=2, W=2, steps_T=T1, n_past=0, iters=iters, lr=0.05, low=None, high=None)
    b = SimpleNamespace(actions=torch.zeros((T1 + 1, B, 5)), images=None, states=None, goal=goal, goal_cost=None, low=None, high=None)
    b.actions[:T1] = torch.from_numpy(rs.standard_normal((T1, B, 5)).astype(np.float32))
    if belief:
        b.belief, b.landing = 'the start', 'the landing buffer'
    return _StubCarrying(Wm), a, b


def _host_adam(model, p, g, m, v, lr_t):
    m += np.float32(0.1) * (g - m)
    v += np.float32(0.001) * (g * g - v)
    p -= np.float32(lr_t) * m / (v.sqrt() + np.float32(1e-8))


def test_refine_iterate_puts_the_start_state_back_in_front_of_every_rollout():
    stub, a, b = _stub_case(belief=True)
    refined, costs = planning._refine_iterate(stub, a, b, adam=_host_adam)
    # iters rollouts with a sweep and the one that scores the result: each starts from the start, with the landing buffer to write into
    assert stub.adopted == ['the start'] * 4 and stub.started == [('the start', 'the landing buffer')] * 4
    assert stub.swept_from == ['the start'] * 3
    assert (stub._state, stub._spare_state) == ('entry state', 'entry spare')      # as on entry: the objects themselves
    assert stub._swept_start == 'the start' and stub.scheduled_sampling_k == 7.0
    assert costs.shape == (4, 2) and (costs[-1] < costs[0]).all()
    # the arithmetic does not know about the state: the same numbers as the old path
    plain, a0, b0 = _stub_case(belief=False)
    refined0, costs0 = planning._refine_iterate(plain, a0, b0, adam=_host_adam)
    assert torch.equal(refined, refined0) and torch.equal(costs, costs0)


def test_refine_iterate_leaves_the_state_as_on_entry_when_the_cost_raises():
    stub, a, b = _stub_case(belief=True)
    seen = []

    def cost_fn(gen):
        seen.append(stub._state)
        if len(seen) == 2:
            raise KeyError('the caller\'s cost failed')
        return (gen * gen).mean(dim=(0, 2, 3, 4))

    with pytest.raises(KeyError):
        planning._refine_iterate(stub, a, b, cost_fn=cost_fn, adam=_host_adam)
    assert seen == ['the landing buffer'] * 2      # (inside the loop the model had moved on)
    assert (stub._state, stub._spare_state) == ('entry state', 'entry spare') and stub.scheduled_sampling_k == 7.0


def test_refine_iterate_without_a_belief_makes_no_state_call():
    class Refusing(_StubCarrying):
        def _adopt_state(self, s):
            raise AssertionError('belief=None must not touch the model\'s state')

    stub, a, b = _stub_case(belief=False)
    stub.__class__ = Refusing
    planning._refine_iterate(stub, a, b, adam=_host_adam)
    assert len(stub.started) == 4 and not hasattr(stub, '_swept_start')
    # (the stub's own calls swapped the two four times: nothing else wrote them)
    assert (stub._state, stub._spare_state) == ('entry state', 'entry spare')
    # a buffer set made by `_refine_upload` says None for both, and takes the same path
    b.belief = b.landing = None
    b.actions[:3] = 0.25
    planning._refine_iterate(stub, a, b, adam=_host_adam)
    assert len(stub.started) == 8 and not hasattr(stub, '_swept_start')
    # the caller's moments and cost table are used when it brings them (MPC.reset does), and the moments start from zero
    b.moments, b.costs = (torch.full((3, 2, 5), 9.0), torch.full((3, 2, 5), 9.0)), torch.zeros((4, 2))
    b.actions[:3] = 0.25
    again, costs = planning._refine_iterate(stub, a, b, adam=_host_adam)
    assert costs is b.costs and float(costs.abs().min()) > 0
    again = again.clone()
    b.moments = None
    b.actions[:3] = 0.25
    fresh, costs2 = planning._refine_iterate(stub, a, b, adam=_host_adam)
    assert torch.equal(again, fresh) and torch.equal(costs, costs2)
