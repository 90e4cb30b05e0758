"""CPU-side tests of the input gradients: the C-ABI surface of include/pivp_input_grad.h against `_lib.INPUT_GRAD_SIGNATURES` and the built library, the
keyword checks of `Model.backward`, the argument errors of `planning.refine_actions`, and its Adam schedule against Chainer's rule in NumPy on a
quadratic, with a stub in the rollout's place.  No GPU."""
import ctypes
import inspect
import math
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
import input_grad_reference as IR  # noqa: E402
from oracle.torch_restatement import chainer_adam_step  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_input_grad_header_library_and_ctypes_table_agree():
    """The new entry points have a header and a table of their own; the model's ABI, its version and the other headers stay as they were."""
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_input_grad.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.INPUT_GRAD_SIGNATURES) == {'pivp_plan_set_input_grad', 'pivp_plan_set_sweep_mode', 'pivp_plan_get_sweep_mode',
                                                           'pivp_action_grad'}
    assert declared <= exported
    assert not any(declared & set(table) for header, table in _lib.HEADER_SIGNATURES.items() if header != 'pivp_input_grad.h')
    assert len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)      # (as before)
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17
    i, vp = _lib._i, _lib._vp
    assert _lib.INPUT_GRAD_SIGNATURES['pivp_plan_set_input_grad'] == (i, [vp, vp, vp])
    assert _lib.INPUT_GRAD_SIGNATURES['pivp_plan_set_sweep_mode'] == (i, [vp, i]) and _lib.INPUT_GRAD_SIGNATURES['pivp_plan_get_sweep_mode'] == (i, [vp])
    assert _lib.INPUT_GRAD_SIGNATURES['pivp_action_grad'] == (i, [vp, vp, i, vp, vp, vp, vp, i, i, i, vp])
    for name, (res, args) in _lib.INPUT_GRAD_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert 'input_grad.hip' in build.SOURCES and 'pivp_input_grad.h' in [os.path.basename(f) for f in _digest.source_files()]
    header = open(os.path.join(ROOT, 'include', 'pivp_input_grad.h')).read()
    assert int(re.search(r'#define PIVP_SWEEP_PARAMS (\d+)', header).group(1)) == _lib.SWEEP_PARAMS == 1
    assert int(re.search(r'#define PIVP_SWEEP_BUILTIN_LOSS (\d+)', header).group(1)) == _lib.SWEEP_BUILTIN_LOSS == 2
    assert 'UNSPECIFIED' in header and 'REQUIRED' in header      # what a sweep without parameter gradients leaves in the registered buffers


def test_plan_setters_and_bad_arguments_need_no_gpu():
    lib = _lib.load()
    cfg = _lib.PivpConfig(batch=2, seq_len=4, height=64, width=64, num_masks=10, model_type=0, use_state=1, context_frames=2, keep_activations=1,
                          ln_eps=1e-6, stp_zero_border=0)
    h = _lib._vp()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert lib.pivp_plan_get_sweep_mode(h) == 3
        for bad in (-1, 4, 7):
            assert lib.pivp_plan_set_sweep_mode(h, bad) == -1 and lib.pivp_plan_get_sweep_mode(h) == 3
        for good in (0, 1, 2, 3):
            assert lib.pivp_plan_set_sweep_mode(h, good) == 0 and lib.pivp_plan_get_sweep_mode(h) == good
        assert lib.pivp_plan_set_input_grad(h, 4096, None) == 0 and lib.pivp_plan_set_input_grad(h, None, 4096) == 0
        assert lib.pivp_plan_set_input_grad(h, 4098, None) == -1 and lib.pivp_plan_set_input_grad(h, None, 4097) == -1
        assert lib.pivp_plan_set_input_grad(h, None, None) == 0
    finally:
        lib.pivp_plan_destroy(h)
    assert lib.pivp_plan_set_sweep_mode(None, 3) == -1 and lib.pivp_plan_get_sweep_mode(None) == -1 and lib.pivp_plan_set_input_grad(None, None, None) == -1
    assert lib.pivp_action_grad(None, None, 64, None, None, None, None, 1, 1, 1, None) == -1
    assert lib.pivp_action_grad(4096, 4096, 60, 4096, 4096, 4096, 4096, 1, 1, 1, None) == -1      # (refused before anything is launched or read)


def test_backward_keywords():
    sig = inspect.signature(pivp_amd.Model.backward).parameters
    assert [sig[k].default for k in ('on_group', 'frame_grad', 'input_grad', 'params', 'builtin_loss')] == [None, None, False, True, True]
    m = pivp_amd.Model(10, keep_activations=True)
    assert m.action_grad is None and m.state_grad is None
    # the keyword errors come first: before the model has been called, before a GPU is needed
    with pytest.raises(ValueError, match='on_group must be None'):
        m.backward(params=False, on_group=lambda g: None)
    with pytest.raises(ValueError, match='nothing to differentiate'):
        m.backward(builtin_loss=False)
    with pytest.raises(ValueError, match='nothing to differentiate'):
        m.backward(input_grad=True, params=False, builtin_loss=False)
    with pytest.raises(RuntimeError, match='call the model first'):
        m.backward(input_grad=True, params=False)
    # the mode and the registration are per call: set in front of the sweep, restored in the `finally` beside the seed's
    src = inspect.getsource(pivp_amd.Model.backward)
    fin = src[src.index('finally:'):]
    assert 'pivp_plan_set_input_grad(plan.h, None, None)' in fin and 'pivp_plan_set_sweep_mode(plan.h, 3)' in fin


def _refine_args(**over):
    m = SimpleNamespace(num_frame_before_prediction=2, keep_activations=True, _extra_loss=False)
    kw = dict(model=m, context_images=np.zeros((2, 3, 3, 8, 8), np.float32), state=np.zeros((3, 5), np.float32), actions=np.zeros((4, 3, 5), np.float32),
              goal_image=np.zeros((3, 8, 8), np.float32), cost_fn=None, steps=2, lr=0.1, past_actions=None, bounds=None)
    kw.update(over)
    return kw


def test_refine_actions_argument_errors():
    a = planning._check_refine_args(**_refine_args())
    assert (a.ctx, a.B, a.H, a.W, a.steps_T, a.n_past, a.iters, a.lr, a.low) == (2, 3, 8, 8, 4, 0, 2, 0.1, None)
    a = planning._check_refine_args(**_refine_args(past_actions=np.zeros((1, 5)), bounds=(-1.0, [1, 2, 3, 4, 5]), goal_image=np.zeros((3, 3, 8, 8))))
    assert a.n_past == 1 and a.low.tolist() == [-1.0] * 5 and a.high.tolist() == [1, 2, 3, 4, 5]
    assert planning._check_refine_args(**_refine_args(past_actions=np.zeros((1, 3, 5)), bounds=(None, 0.5))).high.tolist() == [0.5] * 5
    assert planning._check_refine_args(**_refine_args(goal_image=None, cost_fn=lambda g: g)).iters == 2
    z = np.zeros
    bad = [dict(context_images=z((2, 3, 8, 8))), dict(context_images=z((3, 3, 3, 8, 8))), dict(context_images=z((2, 3, 1, 8, 8))),
           dict(context_images=z((2, 3, 3, 1, 8))), dict(state=z((1, 5))), dict(state=z((3, 4))), dict(actions=z((4, 5))), dict(actions=z((4, 2, 5))),
           dict(actions=z((1, 3, 5))), dict(actions=z((4, 3, 4))), dict(goal_image=None), dict(cost_fn=lambda g: g), dict(goal_image=None, cost_fn=3),
           dict(goal_image=z((3, 8, 9))), dict(goal_image=z((2, 3, 8, 8))), dict(steps=0), dict(steps=2.0), dict(steps=True), dict(lr=-1.0),
           dict(lr=float('nan')), dict(lr='0.1'), dict(past_actions=z((2, 5))), dict(past_actions=z((1, 2, 5))), dict(bounds=1.0), dict(bounds=(1.0,)),
           dict(bounds=(1.0, 0.0)), dict(bounds=(z(4), None)), dict(bounds=(float('nan'), None)),
           dict(model=SimpleNamespace(num_frame_before_prediction=2, keep_activations=False, _extra_loss=False)),
           dict(model=SimpleNamespace(num_frame_before_prediction=2, keep_activations=True, _extra_loss=True)),
           dict(model=SimpleNamespace(num_frame_before_prediction=1, keep_activations=True, _extra_loss=False))]
    for over in bad:
        with pytest.raises(ValueError):
            planning._check_refine_args(**_refine_args(**over))
    one = SimpleNamespace(num_frame_before_prediction=1, keep_activations=True, _extra_loss=False)
    with pytest.raises(ValueError, match='past_actions'):      # one context frame: there is no past step
        planning._check_refine_args(**_refine_args(model=one, context_images=z((1, 3, 3, 8, 8)), past_actions=z((0, 5))))
    # every complaint is raised before the GPU or the library is needed
    with pytest.raises(ValueError, match='exactly one'):
        planning.refine_actions(pivp_amd.Model(10, keep_activations=True), z((2, 3, 3, 8, 8)), z((3, 5)), z((4, 3, 5)))
    assert 'cem_plan(' in planning.refine_actions.__doc__ and 'cem_plan' not in inspect.getsource(planning._refine_iterate)


class _StubRollout(object):
    """Stands in for the model in `_refine_iterate`: frames gen[t, b] = reshape(W act[t, b]) (3 x 2 x 2), so the default cost is a quadratic of the
    actions, and backward() hands back frame_grad pulled through W -- what the sweep does for the real model."""

    def __init__(self, ctx, W):
        self.num_frame_before_prediction, self.W = ctx, W
        self.scheduled_sampling_k, self.ks_seen, self.calls = 7.0, [], []
        self.action_grad = None

    def __call__(self, x):
        self.ks_seen.append((self.scheduled_sampling_k, pivp_amd.config.train))
        acts = x[1]
        self._gen = (acts[:-1] @ self.W.T).reshape(acts.shape[0] - 1, acts.shape[1], 3, 2, 2)

    def backward(self, **kw):
        self.calls.append({k: v for k, v in kw.items() if k != 'frame_grad'})
        fg, ctx = kw['frame_grad'], self.num_frame_before_prediction
        assert fg.dtype == torch.float32 and fg.is_contiguous()
        g = torch.full((self._gen.shape[0], fg.shape[1], 5), 3.0)      # (rows in front of the scored frames: junk that refine must zero when they are past)
        g[ctx - 1:] = fg.reshape(fg.shape[0], fg.shape[1], 12) @ self.W
        self.action_grad = g


def test_refine_actions_adam_schedule_against_numpy():
    rs = np.random.RandomState(5)
    T1, B, ctx, iters, lr = 4, 2, 2, 6, 0.05
    W = torch.from_numpy(rs.standard_normal((12, 5)).astype(np.float32))
    goal = torch.from_numpy(rs.standard_normal((3, 2, 2)).astype(np.float32))
    start = rs.standard_normal((T1, B, 5)).astype(np.float32)
    stub = _StubRollout(ctx, W)
    lrs = []

    def adam(model, p, g, m, v, lr_t):      # pivp_adam_step's arithmetic (csrc/backward.hip adam_kernel) in float32 on the host
        lrs.append(lr_t)
        omb1, omb2 = np.float32(1.0 - 0.9), np.float32(1.0 - 0.999)
        m += omb1 * (g - m)
        v += omb2 * (g * g - v)
        p -= np.float32(lr_t) * m / (v.sqrt() + np.float32(1e-8))

    a = SimpleNamespace(ctx=ctx, B=B, H=2, W=2, steps_T=T1, n_past=1, iters=iters, lr=lr, low=None, high=None)
    b = SimpleNamespace(actions=torch.zeros((T1 + 1, B, 5)), images=None, states=None, goal=goal, goal_cost=None, low=None, high=None)
    b.actions[:T1] = torch.from_numpy(start)
    with pivp_amd.using_config('train', False):
        refined, costs = planning._refine_iterate(stub, a, b, adam=adam)
        assert pivp_amd.config.train is False
    # the schedule: update t = 1, 2, ... with Chainer's bias-corrected step size, formed on the host
    assert lrs == [lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t) for t in range(1, iters + 1)]
    assert lrs[0] == pytest.approx(lr * math.sqrt(0.001) / 0.1) and planning._adam_lr_t(0.0, 3) == 0.0
    # every rollout is feed-self and in training mode whatever the model and the caller had set, and both are put back
    assert stub.ks_seen == [(-1, True)] * (iters + 1) and stub.scheduled_sampling_k == 7.0
    assert stub.calls == [dict(input_grad=True, params=False, builtin_loss=False)] * iters
    # NumPy: Chainer's Adam on the same quadratic in float64
    Wd, gd = W.double().numpy(), goal.double().numpy().reshape(12)
    P = {'a': start.astype(np.float64)}
    M, V = {'a': np.zeros_like(P['a'])}, {'a': np.zeros_like(P['a'])}
    ref_costs = []
    cost = lambda act: (((act[ctx - 1:] @ Wd.T) - gd) ** 2).mean(axis=(0, 2))
    for t in range(1, iters + 1):
        ref_costs.append(cost(P['a']))
        grad = np.zeros_like(P['a'])
        grad[ctx - 1:] = 2.0 * ((P['a'][ctx - 1:] @ Wd.T) - gd) @ Wd / (12 * (T1 + 1 - ctx))
        chainer_adam_step(P, {'a': grad}, M, V, t, alpha=lr)
    ref_costs.append(cost(P['a']))
    assert np.abs(refined.numpy() - P['a']).max() < 1e-5 and np.allclose(costs.numpy(), np.array(ref_costs), rtol=1e-5)
    assert np.array_equal(refined.numpy()[:1], start[:1]) and (costs[-1] < costs[0]).all()      # the past row never moves
    # bounds clamp the free rows after every step
    b.actions[:T1] = torch.from_numpy(start)
    b.low, b.high = torch.full((5,), -0.25), torch.full((5,), 0.5)
    clamped, _ = planning._refine_iterate(stub, a, b, adam=adam)
    assert float(clamped[1:].min()) >= -0.25 and float(clamped[1:].max()) <= 0.5 and np.array_equal(clamped.numpy()[:1], start[:1])


def test_action_grad_restatement_by_hand():
    """One sample, two pixels: the mask, the smeared-weight rows and the state predictor's transpose written out."""
    e3 = np.zeros((1, 2, 64)); de3 = np.zeros((1, 2, 64))
    e3[0, 0, 3], e3[0, 1, 3], e3[0, 1, 5] = 1.0, -1.0, 0.0
    de3[0, :, 3] = (2.0, 100.0); de3[0, 1, 5] = 50.0                    # (masked: e3 <= 0)
    w3 = np.zeros((74, 64)); w3[64 + 2, 3] = 0.5; w3[64 + 7, 3] = 9.0   # (row 71 is the state half: not an action's)
    wcs = np.zeros((5, 10)); wcs[4, 2] = 3.0; wcs[4, 8] = 11.0
    dsnew = np.zeros((1, 5)); dsnew[0, 4] = 0.25
    assert IR.action_grad(e3, de3, w3, wcs, dsnew, 1).tolist() == [[0.0, 0.0, 0.5 * 2.0 + 3.0 * 0.25, 0.0, 0.0]]
    assert IR.action_grad(e3, de3, w3, wcs, dsnew, 0).tolist() == [[0.0, 0.0, 0.75, 0.0, 0.0]]
