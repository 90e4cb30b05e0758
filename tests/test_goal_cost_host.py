"""CPU-side tests of the goal-image cost: the C-ABI surface of include/pivp_goal_cost.h against `_lib.GOAL_COST_SIGNATURES` and the built library,
every ValueError of `planning.GoalImageCost` and the new complaints of `cem_plan` / `score_actions` / `cem_refine`, and the float64 restatement
tests/goal_cost_reference.py against torch autograd and against `refine_actions`' closed form."""
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
import goal_cost_reference as GR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_goal_cost_header_library_and_ctypes_table_agree():
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_goal_cost.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.GOAL_COST_SIGNATURES) == {'pivp_goal_image_cost'}
    assert declared <= exported
    assert not any(declared & set(table) for header, table in _lib.HEADER_SIGNATURES.items() if header != 'pivp_goal_cost.h')
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17 and len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)
    i, f, vp = _lib._i, _lib._f, _lib._vp
    assert _lib.GOAL_COST_SIGNATURES['pivp_goal_image_cost'] == (i, [vp, vp, i, vp, f, vp, f, f, f, f, i, vp, vp, vp, i, i, i, i, vp])
    fn = lib.pivp_goal_image_cost                                              # load() bound the new table too
    assert fn.argtypes == _lib.GOAL_COST_SIGNATURES['pivp_goal_image_cost'][1] and fn.restype is i
    assert 'goal_cost.hip' in build.SOURCES and 'pivp_goal_cost.h' in [os.path.basename(p) for p in _digest.source_files()]
    # the header's prototype, argument by argument
    header = open(os.path.join(ROOT, 'include', 'pivp_goal_cost.h')).read()
    proto = re.search(r'int pivp_goal_image_cost\(([^)]*)\);', header).group(1)
    kinds = [vp if '*' in a else (f if a.strip().startswith('float') else i) for a in proto.split(',')]
    assert kinds == _lib.GOAL_COST_SIGNATURES['pivp_goal_image_cost'][1]


def test_bad_arguments_are_refused_without_a_gpu():
    """Sizes, null pointers and the scalars are checked before anything is launched: the calls return on a machine without a device."""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    good = dict(frames=p, goal=p, G=1, pixel_w=None, inv_norm=1.0 / 768, step_w=p, w_mse=1.0, w_l1=0.0, bad=1.0, scale=1.0, acc=0, cost=p, per_step=p,
                grad=None, S=2, K=3, H=16, W=16)

    def rc(**over):
        a = dict(good, **over)
        return lib.pivp_goal_image_cost(a['frames'], a['goal'], a['G'], a['pixel_w'], a['inv_norm'], a['step_w'], a['w_mse'], a['w_l1'], a['bad'],
                                        a['scale'], a['acc'], a['cost'], a['per_step'], a['grad'], a['S'], a['K'], a['H'], a['W'], None)
    nan, inf = float('nan'), float('inf')
    bad = [dict(frames=None), dict(goal=None), dict(step_w=None), dict(cost=None), dict(per_step=None), dict(S=0), dict(K=0), dict(K=-1), dict(H=1),
           dict(W=1), dict(W=253), dict(H=32769), dict(G=2), dict(G=0), dict(inv_norm=0.0), dict(inv_norm=-1.0), dict(inv_norm=nan), dict(inv_norm=inf),
           dict(w_mse=nan), dict(w_l1=inf), dict(bad=nan), dict(bad=-inf), dict(scale=inf), dict(scale=nan), dict(frames=p + 2), dict(grad=p + 1)]
    for over in bad:
        assert rc(**over) == -1, over


def test_goal_image_cost_spec_errors():
    G = planning.GoalImageCost
    z = np.zeros
    s = G(z((3, 8, 12)))
    assert (s.mse, s.l1, s.weight, s.bad_cost, s.hw, s.batch) == (1.0, 0.0, 1.0, 1.0, (8, 12), None) and s.inv_norm() == 1.0 / (3 * 8 * 12)
    assert s.steps(4).tolist() == [0.25] * 4 and s.steps(4).dtype == np.float32
    s = G(z((5, 3, 8, 12)), mse=0.5, l1=2.0, pixel_weight=np.full((8, 12), 0.5), step_weights=[0, 0, 1.0], weight=3.0)
    assert s.batch == 5 and s.bad_cost == 2.5 and s.inv_norm() == 1.0 / (3 * 48.0) and s.steps(3).tolist() == [0, 0, 1.0]
    assert G(torch.zeros(3, 8, 12), bad_cost=-2.0).bad_cost == -2.0 and 'GoalImageCost(' in repr(s)
    w_neg, w_zero, w_nan = np.ones((8, 12)), z((8, 12)), np.ones((8, 12))
    w_neg[0, 0], w_nan[1, 1] = -1.0, np.nan
    bad = [dict(goal_image=z((8, 12))), dict(goal_image=z((1, 8, 12))), dict(goal_image=z((2, 2, 3, 8, 12))), dict(goal_image=z((3, 1, 12))),
           dict(goal_image=z((0, 3, 8, 12))), dict(goal_image=np.full((3, 8, 12), np.nan)), dict(goal_image='frame'),
           dict(goal_image=torch.zeros(3, 8, 12, dtype=torch.int32)),
           dict(mse=-1.0), dict(mse=np.nan), dict(mse='1'), dict(mse=True), dict(l1=-0.5), dict(l1=np.inf), dict(mse=0.0, l1=0.0), dict(mse=1e39),
           dict(pixel_weight=np.ones((8, 8))), dict(pixel_weight=np.ones(96)), dict(pixel_weight=w_neg), dict(pixel_weight=w_zero),
           dict(pixel_weight=w_nan), dict(pixel_weight=np.full((8, 12), np.inf)), dict(pixel_weight='all'),
           dict(step_weights=np.ones((2, 2))), dict(step_weights=[]), dict(step_weights=[1.0, np.nan]), dict(step_weights=[np.inf]), dict(step_weights=1.0),
           dict(weight=np.nan), dict(weight=np.inf), dict(weight='2'), dict(bad_cost=np.inf), dict(bad_cost=np.nan), dict(bad_cost=None, mse=np.inf)]
    for over in bad:
        with pytest.raises(ValueError):
            G(**dict(dict(goal_image=z((3, 8, 12))), **over))
    # the frames it is asked to score
    s = G(z((3, 8, 12)), step_weights=[1.0, 2.0])
    s.check_frames(2, 7, 8, 12)
    for args in ((3, 7, 8, 12), (2, 7, 8, 8), (2, 7, 12, 8)):
        with pytest.raises(ValueError):
            s.check_frames(*args)
    per = G(z((7, 3, 8, 12)))
    per.check_frames(2, 7, 8, 12, per_sample=True)
    for args, kw in (((2, 7, 8, 12), {}), ((2, 6, 8, 12), dict(per_sample=True))):
        with pytest.raises(ValueError):
            per.check_frames(*args, **kw)
    with pytest.raises(ValueError):
        G(z((3, 8, 300))).check_frames(1, 1, 8, 300)
    # the wrapper's own complaints come before the GPU is needed
    with pytest.raises(ValueError, match='GoalImageCost'):
        planning.goal_image_cost(torch.zeros(2, 3, 3, 8, 12), np.zeros((3, 8, 12)))
    for frames in (np.zeros((2, 3, 3, 8, 12), np.float32), torch.zeros(2, 3, 3, 8), torch.zeros(2, 3, 3, 8, 12, dtype=torch.float64),
                   torch.zeros(2, 3, 2, 8, 12), torch.zeros(2, 3, 3, 8, 8)):
        with pytest.raises(ValueError):
            planning.goal_image_cost(frames, G(z((3, 8, 12))))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        planning.goal_image_cost(torch.zeros(2, 3, 3, 8, 12), G(z((3, 8, 12))))


def _good(**over):
    kw = dict(context_images=np.zeros((2, 1, 3, 64, 64), np.float32), state=np.zeros((1, 5), np.float32), designated_rc=None, goal_rc=None,
              horizon=4, past_actions=np.zeros((1, 5), np.float32), goal_image=np.zeros((3, 64, 64), np.float32))
    kw.update(over)
    return kw


def test_cem_plan_goal_image_argument_errors():
    m = pivp_amd.Model(10, num_frame_before_prediction=2)
    sig = inspect.signature(planning.cem_plan).parameters
    assert list(sig)[-2:] == ['belief', 'goal_image'] and sig['goal_image'].default is None
    # the checker: three positional arguments, then `cem_plan`'s own keywords (all but trace, which is no checked value) with `cem_plan`'s defaults
    own = {n: q for n, q in sig.items() if n not in ('model', 'context_images', 'state', 'trace')}
    checker = inspect.signature(planning._check_cem_args).parameters
    assert list(checker)[:3] == ['model', 'context_images', 'state'] and list(checker)[3:] == list(own)
    assert all(checker[n].kind is inspect.Parameter.KEYWORD_ONLY and checker[n].default == own[n].default for n in own)
    assert [n for n in own if own[n].default is inspect.Parameter.empty] == ['designated_rc', 'goal_rc', 'horizon']
    assert inspect.signature(planning.score_actions).parameters['goal_image'].default is None
    G = planning.GoalImageCost
    g64 = np.zeros((3, 64, 64), np.float32)
    bad = [dict(goal_image=None),                                                        # neither goal
           dict(plane_weights=[1.0]), dict(miss_cost=10.0), dict(step_weights=np.ones(4)),    # they belong to the planes
           dict(goal_image=np.zeros((3, 32, 64))), dict(goal_image=np.zeros((64, 64))), dict(goal_image=np.zeros((1, 3, 64, 64))),
           dict(goal_image=G(np.zeros((32, 3, 64, 64)))), dict(goal_image=G(g64, step_weights=np.ones(3))), dict(goal_image='goal'),
           dict(designated_rc=[[1, 2]]), dict(goal_rc=[[1, 2]]),                         # half a pixel goal
           dict(designated_rc=[[1, 2]], goal_rc=[[3, 4]], plane_weights=[1.0, 2.0])]
    for over in bad:
        with pytest.raises(ValueError):
            planning.cem_plan(m, **_good(**over))
    with pytest.raises(ValueError, match='no goal'):
        planning.cem_plan(m, **_good(goal_image=None))
    with pytest.raises(ValueError, match='plane_weights'):
        planning.cem_plan(m, **_good(plane_weights=[1.0]))
    kw = _good()
    ctx, st = kw.pop('context_images'), kw.pop('state')
    a = planning._check_cem_args(m, ctx, st, **kw)                                      # (goal_image=g64; the rest: the defaults)
    assert a.P == 0 and a.designated.shape == (0, 2) and isinstance(a.image, G) and a.image.weight == 1.0 and a.plane_w.shape == (0,)
    spec = G(g64, l1=0.5, step_weights=np.arange(4.0), weight=2.0)
    kw.update(designated_rc=[[3, 4]], goal_rc=[[5.5, 6]])
    a = planning._check_cem_args(m, ctx, st, **dict(kw, goal_image=spec))
    assert a.P == 1 and a.image is spec
    assert planning._check_cem_args(m, ctx, st, **dict(kw, goal_image=None)).image is None
    for args, over in (((kw['designated_rc'],), {}), ((), dict(trace=False)), ((), dict(no_such_argument=1))):      # a fourth positional; unknown names
        with pytest.raises(TypeError):
            planning._check_cem_args(m, ctx, st, *args, **dict(kw, **over))
    if not torch.cuda.is_available():
        for over in (dict(), dict(goal_image=spec), dict(goal_image=spec, designated_rc=[[3, 4]], goal_rc=[[5, 6]])):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                planning.cem_plan(m, **_good(**over))
    # score_actions: the same rules
    ctx, st, cand = np.zeros((2, 1, 3, 64, 64), np.float32), np.zeros((1, 5), np.float32), np.zeros((4, 3, 5), np.float32)
    for kw in (dict(), dict(goal_image=np.zeros((3, 32, 32))), dict(goal_image=G(g64, step_weights=np.ones(3))), dict(goal_image=G(np.zeros((4, 3, 64, 64))))):
        with pytest.raises(ValueError):
            planning.score_actions(m, ctx, st, cand, None, None, **kw)
    with pytest.raises(ValueError):
        planning.score_actions(m, ctx, st, np.zeros((4, 1, 5), np.float32), None, None, goal_image=g64)      # no predicted step
    # refine_actions: a spec of another size, horizon or batch
    tm = SimpleNamespace(num_frame_before_prediction=2, keep_activations=True, _extra_loss=False)
    rk = dict(model=tm, context_images=np.zeros((2, 3, 3, 8, 8), np.float32), state=np.zeros((3, 5), np.float32), actions=np.zeros((4, 3, 5), np.float32),
              cost_fn=None, steps=2, lr=0.1, past_actions=None, bounds=None)
    assert planning._check_refine_args(goal_image=G(np.zeros((3, 8, 8)), step_weights=np.ones(3)), **rk).B == 3
    assert planning._check_refine_args(goal_image=G(np.zeros((3, 3, 8, 8))), **rk).B == 3
    for g in (G(np.zeros((3, 8, 9))), G(np.zeros((2, 3, 8, 8))), G(np.zeros((3, 8, 8)), step_weights=np.ones(4))):
        with pytest.raises(ValueError):
            planning._check_refine_args(goal_image=g, **rk)


def test_cem_refine_argument_errors():
    ctx, st = np.zeros((2, 1, 3, 64, 64), np.float32), np.zeros((1, 5), np.float32)
    g64, past = np.zeros((3, 64, 64), np.float32), np.zeros((1, 5), np.float32)
    train = pivp_amd.Model(10, num_frame_before_prediction=2, keep_activations=True)
    with pytest.raises(ValueError, match='keep_activations'):
        planning.cem_refine(pivp_amd.Model(10, num_frame_before_prediction=2), ctx, st, 4, g64, past_actions=past)
    with pytest.raises(ValueError, match='belief'):
        planning.cem_refine(train, ctx, st, 4, g64, past_actions=past, belief=object())
    for kw in (dict(designated_rc=[[1, 2]]), dict(goal_rc=[[1, 2]]), dict(plane_weights=[1.0]), dict(samples=0), dict(no_such_argument=1)):
        with pytest.raises((ValueError, TypeError)):
            planning.cem_refine(train, ctx, st, 4, g64, past_actions=past, **kw)
    for goal in (None, np.zeros((2, 3, 64, 64)), np.zeros((3, 32, 32))):
        with pytest.raises(ValueError):
            planning.cem_refine(train, ctx, st, 4, goal, past_actions=past)
    assert 'cem_refine' in planning.refine_actions.__doc__ and 'goal_image' in planning.__doc__


def _case(rs, S, K, H, W, G):
    frames = rs.rand(S, K, 3, H, W)
    goal = rs.rand(G, 3, H, W)
    frames[0, 0, :, 0, :3] = goal[0, :, 0, :3]                                  # d == 0: sign(0) = 0
    w = rs.rand(H, W) * (rs.rand(H, W) > 0.3)
    f64 = lambda a: a.astype(np.float32).astype(np.float64)                     # float32 values, as the entry point receives them
    return f64(frames), f64(goal), f64(w), f64(rs.rand(S) + 0.25)


def test_the_restatement_gradient_is_autograd_s():
    rs = np.random.RandomState(5)
    for S, K, H, W, G, w_mse, w_l1 in ((3, 4, 5, 6, 1, 1.0, 0.0), (2, 3, 4, 7, 3, 0.0, 1.5), (2, 2, 6, 5, 1, 0.75, 0.5)):
        frames, goal, w, sw = _case(rs, S, K, H, W, G)
        inv = GR.inv_norm(w, H, W)
        scale, cost_in = 1.75, rs.rand(K)
        cost, per_step, grad = GR.goal_image_cost(frames, goal, w, inv, sw, w_mse, w_l1, 9.0, scale, cost_in=cost_in)
        f = torch.tensor(frames, dtype=torch.float64, requires_grad=True)
        d = f - torch.tensor(goal)[None]
        ps = float(np.float32(inv)) * (torch.tensor(w.astype(np.float32).astype(np.float64)) * (w_mse * d * d + w_l1 * d.abs())).sum(dim=(2, 3, 4))
        c = torch.tensor(cost_in) + float(np.float32(scale)) * (torch.tensor(sw)[:, None] * ps).sum(dim=0)
        c.sum().backward()
        assert np.abs(per_step / ps.detach().numpy() - 1).max() < 1e-6            # (per_step carries the header's one rounding to float32)
        assert np.abs(cost / c.detach().numpy() - 1).max() < 1e-6
        assert np.abs(grad - f.grad.numpy()).max() <= 1e-12 * np.abs(grad).max()
        assert (grad[0, 0, :, 0, :3] == 0).all()
    # a frame that is not finite: bad_cost, and a zero gradient
    frames, goal, w, sw = _case(rs, 2, 3, 4, 4, 1)
    frames[1, 2, 0, 1, 1] = np.nan
    cost, per_step, grad = GR.goal_image_cost(frames, goal, None, GR.inv_norm(None, 4, 4), sw, 1.0, 1.0, 9.0, 1.0)
    assert per_step[1, 2] == 9.0 and (grad[1, 2] == 0).all() and np.isfinite(cost).all() and np.isfinite(grad).all()
    assert np.abs(grad[1, 1]).max() > 0


def test_the_defaults_are_refine_actions_formula():
    """GoalImageCost's defaults restate `refine_actions`' bare goal_image cost: the squared error averaged over steps and pixels, and its closed-form
    gradient diff * 2 / (nf * 3 * H * W)."""
    rs = np.random.RandomState(6)
    for shape in ((3, 8, 12), (4, 3, 8, 12)):
        nf, B, H, W = 5, 4, 8, 12
        gen = rs.rand(nf, B, 3, H, W).astype(np.float32)
        goal = rs.rand(*shape).astype(np.float32)
        spec = planning.GoalImageCost(goal)
        cost, per_step, grad = GR.spec_cost(gen, spec, want_grad=True)
        diff = gen.astype(np.float64) - goal.astype(np.float64)
        assert np.abs(cost / (diff * diff).mean(axis=(0, 2, 3, 4)) - 1).max() < 1e-6
        want = diff * (2.0 / (nf * 3 * H * W))
        assert np.abs(grad - want).max() < 1e-6 * np.abs(want).max()
    src = inspect.getsource(planning._refine_iterate)
    assert '(diff * diff).mean(dim=(0, 2, 3, 4))' in src and '2.0 / (nf * 3 * a.H * a.W)' in src      # the bare array keeps its closed form
