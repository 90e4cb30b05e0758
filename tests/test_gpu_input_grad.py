"""GPU tests of the input gradients (include/pivp_input_grad.h): pivp_action_grad against its float64 restatement, `Model.backward(input_grad=True,
params=, builtin_loss=)` against float64 autograd through the torch restatement of the model, the neutrality of the new switches, and
`planning.refine_actions`.  References: tests/input_grad_reference.py (computed once per case and shared)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_grad_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GATE = 2e-3          # the project's gradient gate at these shapes (tests/test_gpu_train.py): relative L2, and largest element relative to max |ref|
OP_GATE = 1e-6       # of the tensor's largest reference element: the project's gate for fp64-accumulated reductions (one rounding of the result: 6e-8)


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


# ---- per-op --------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _action_grad(pivp, d, ldd3, use_state, B, HW8):
    lib = pivp._lib.load()
    t = {k: _dev(v) for k, v in d.items()}
    out = torch.full((B, 5), float('nan'), dtype=torch.float32, device=DEV)
    rc = lib.pivp_action_grad(t['e3'].data_ptr(), t['de3'].data_ptr(), ldd3, t['w3'].data_ptr(), t['wcs'].data_ptr(), t['dsnew'].data_ptr(),
                              out.data_ptr(), B, HW8, use_state, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize('use_state', [0, 1])
@pytest.mark.parametrize('ldd3', [64, 192])
@pytest.mark.parametrize('HW8', [1, 63, 64, 65, 256])
def test_action_grad_matches_float64(pivp, HW8, ldd3, use_state):
    """HW8: under, at and over one pass of the sixteen row groups x four rows (64), and the 128 x 128 frame's 16 x 16 map."""
    B = 3
    d = IR.action_grad_inputs(B, HW8, ldd3, seed=HW8 + ldd3 + use_state)
    ref = IR.action_grad(d['e3'], d['de3'], d['w3'], d['wcs'], d['dsnew'], use_state)
    rc, got = _action_grad(pivp, d, ldd3, use_state, B, HW8)
    assert rc == 0
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print('pivp_action_grad HW8 %d ldd3 %d use_state %d: worst error %.2e of the largest element' % (HW8, ldd3, use_state, worst))
    assert np.isfinite(got).all() and worst <= OP_GATE
    rc2, again = _action_grad(pivp, d, ldd3, use_state, B, HW8)
    assert rc2 == 0 and np.array_equal(got.view(np.uint32), again.view(np.uint32)), 'same bytes, other bits'


@pytest.mark.parametrize('HW8', [65, 256])
def test_action_grad_mixed_magnitudes(pivp, HW8):
    """d e3 of magnitudes around 1e4 and 1e-3 side by side: an fp32 running sum of the columns drops the small terms (1e4 carries an ulp of 1e-3)."""
    B = 3
    d = IR.action_grad_inputs(B, HW8, 192, seed=11, mixed=True)
    ref = IR.action_grad(d['e3'], d['de3'], d['w3'], d['wcs'], d['dsnew'], 1)
    rc, got = _action_grad(pivp, d, 192, 1, B, HW8)
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print('pivp_action_grad mixed magnitudes HW8 %d: worst error %.2e of the largest element' % (HW8, worst))
    assert rc == 0 and worst <= OP_GATE


def test_action_grad_bad_arguments_launch_nothing(pivp):
    lib = pivp._lib.load()
    d = {k: _dev(v) for k, v in IR.action_grad_inputs(2, 8, 64, seed=1).items()}
    out = torch.full((2, 5), 7.0, dtype=torch.float32, device=DEV)
    p = lambda k: d[k].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    good = [p('e3'), p('de3'), 64, p('w3'), p('wcs'), p('dsnew'), out.data_ptr(), 2, 8, 1, st]
    for at, bad in ((0, None), (1, None), (2, 60), (2, 66), (3, None), (4, None), (5, None), (6, None), (7, 0), (8, 0), (0, p('e3') + 4), (1, p('de3') + 8),
                    (6, out.data_ptr() + 2)):
        args = list(good)
        args[at] = bad
        assert lib.pivp_action_grad(*args) == -1, (at, bad)
    args = list(good); args[3] = None; args[9] = 0      # w3 is not read without use_state
    assert lib.pivp_action_grad(*args) == 0
    torch.cuda.synchronize()
    assert lib.pivp_plan_set_input_grad(None, None, None) == -1 and lib.pivp_plan_set_sweep_mode(None, 3) == -1 and lib.pivp_plan_get_sweep_mode(None) == -1


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, l1=False):
    return IR.input_grads(name, torch.float64, l1)


def _ctx(name):
    return IR.MODEL_CASES[name][0].get('num_frame_before_prediction', 2)


def _model(pivp, name, **kw):
    mkw, nm, P, imgs, acts, stas = IR.case_inputs(name)
    m = pivp.Model(nm, prefix='t', keep_activations=True, **dict(mkw, **kw))
    m.load_state_dict_reference(P)
    return m, (imgs, acts, stas)


def _l1_seed(m, name):
    """d l1_cost / d gen_images[ctx-1:] by torch autograd on the device, as a caller would form it"""
    gen = m._gen[_ctx(name) - 1:].detach().requires_grad_(True)
    g, = torch.autograd.grad(IR.l1_cost(gen, torch.from_numpy(IR.l1_target()).to(gen.device)), gen)
    return g


def _sweep(m, x, name, l1=False, **kw):
    m(list(x), 0)
    m.cleargrads()
    if l1:
        m.backward(frame_grad=_l1_seed(m, name), input_grad=True, builtin_loss=False, **kw)
    else:
        m.backward(input_grad=True, **kw)
    return m.action_grad.clone(), m.state_grad.clone()


def _check(name, ag, sg, l1=False, what=''):
    a_ref, s_ref = _reference(name, l1)
    T = IR.MODEL_CASES[name][3]
    ag, sg = ag.cpu().numpy(), sg.cpu().numpy()
    assert ag.shape == (T - 1, 2, 5) and sg.shape == (2, 5) and ag.dtype == np.float32
    ea, es = IR.rel_errors(ag, a_ref[:T - 1]), IR.rel_errors(sg, s_ref[0])
    print('%s%s%s: action_grad rel L2 %.2e, largest element %.2e; state_grad rel L2 %.2e, largest element %.2e'
          % (name, ' (L1 seed)' if l1 else '', what, ea[0], ea[1], es[0], es[1]))
    assert max(ea) < GATE, 'action_grad: relative L2 %.3e, largest element %.3e of max |ref|' % ea
    assert max(es) < GATE, 'state_grad: relative L2 %.3e, largest element %.3e of max |ref|' % es


@pytest.mark.parametrize('name', list(IR.MODEL_CASES))
def test_input_gradients_match_float64_autograd(pivp, name):
    """Measured on the MI355X (rel L2 / largest element of action_grad; of state_grad): profiles/r14/NOTES.md."""
    a_ref, s_ref = _reference(name)
    T, ctx = IR.MODEL_CASES[name][3], _ctx(name)
    # what the reference says about the rows the model never reads: the last action and the states between the context frames get no gradient
    assert not a_ref[T - 1].any() and not s_ref[1:ctx].any() and np.abs(a_ref[:T - 1]).max() > 0 and np.abs(s_ref[0]).max() > 0
    m, x = _model(pivp, name)
    ag, sg = _sweep(m, x, name)
    _check(name, ag, sg)


def test_seed_hook_alone_differentiates_the_callers_cost(pivp):
    name = IR.L1_CASE
    m, x = _model(pivp, name)
    ag, sg = _sweep(m, x, name, l1=True)
    _check(name, ag, sg, l1=True)
    with pytest.raises(ValueError, match='builtin_loss'):
        m.backward(input_grad=True, builtin_loss=False)
    with pytest.raises(ValueError, match='on_group'):
        m.backward(params=False, on_group=lambda g: None)
    # the C ABI says the same: no seed and no own loss is a state error, and the mode is the plan's until it is set back
    plan, lib = m._active, pivp._lib.load()
    assert lib.pivp_plan_get_sweep_mode(plan.h) == 3 and lib.pivp_plan_set_sweep_mode(plan.h, 4) == -1 and lib.pivp_plan_set_sweep_mode(plan.h, 1) == 0
    images, actions, states = m._inputs
    rc = lib.pivp_rollout_backward(plan.h, images.data_ptr(), actions.data_ptr(), states.data_ptr(), None, m._gen.data_ptr(), m._gen_states.data_ptr(),
                                   m._stream())
    assert rc == -3 and lib.pivp_plan_set_sweep_mode(plan.h, 3) == 0


def test_switches_are_neutral_on_a_deterministic_model(pivp):
    name = 'cdna_T5'
    m, x = _model(pivp, name, deterministic=True)
    m(list(x), 0)
    m.cleargrads(); m.backward()
    plain = m._flat_grads.clone()
    m.cleargrads(); m.backward(input_grad=True)
    ag, sg = m.action_grad.clone(), m.state_grad.clone()
    assert torch.equal(m._flat_grads, plain), 'parameter gradients differ in %d elements with input gradients registered' % int((m._flat_grads != plain).sum())
    _check(name, ag, sg, what=' deterministic')
    m.action_grad.fill_(float('nan')); m.state_grad.fill_(float('nan'))
    m.backward(input_grad=True, params=False)
    assert torch.equal(m.action_grad, ag) and torch.equal(m.state_grad, sg), 'params=False changed the input gradients'
    only_a = m.action_grad.clone()
    # one of the two alone (the C ABI admits either pointer null)
    plan, lib = m._active, pivp._lib.load()
    images, actions, states = m._inputs
    sweep = lambda: lib.pivp_rollout_backward(plan.h, images.data_ptr(), actions.data_ptr(), states.data_ptr(), None, m._gen.data_ptr(),
                                              m._gen_states.data_ptr(), m._stream())
    only_s = torch.full_like(sg, float('nan'))
    only_a.fill_(float('nan'))
    assert lib.pivp_plan_set_input_grad(plan.h, only_a.data_ptr(), None) == 0 and sweep() == 0
    assert lib.pivp_plan_set_input_grad(plan.h, None, only_s.data_ptr()) == 0 and sweep() == 0
    assert lib.pivp_plan_set_input_grad(plan.h, None, None) == 0
    assert torch.equal(only_a, ag) and torch.equal(only_s, sg)


def test_params_false_on_a_default_model_and_no_state_leaks(pivp):
    from test_gpu_train import _autograd, _check_grads
    name = 'cdna_T3'
    m, x = _model(pivp, name)
    ag, sg = _sweep(m, x, name, params=False)
    _check(name, ag, sg, what=' params=False')      # (atomics in the K-split data gradients: no bit comparison on a default model)
    ag, sg = _sweep(m, x, name, l1=True, params=False)
    _check(name, ag, sg, l1=True, what=' params=False')
    # a plain sweep afterwards is the parent's again
    mkw, nm, P, imgs, acts, stas = IR.case_inputs(name)
    _, gref = _autograd(P, imgs, acts, stas)
    m.cleargrads(); m.backward()
    print('after a params=False sweep, worst relative parameter-gradient error', _check_grads(m.grads_reference(), gref, 2e-3))


def test_bf16_action_grad_tracks_fp32(pivp):
    """The bound is tests/test_gpu_bf16.py's for the bf16 mode's parameter gradients against the fp32 path's (relative L2 < 5e-2)."""
    name = 'cdna_T3'
    out = {}
    for prec in ('fp32', 'bf16'):
        m, x = _model(pivp, name, precision=prec)
        out[prec] = _sweep(m, x, name)[0]
    rel = float((out['bf16'] - out['fp32']).norm() / out['fp32'].norm())
    print('bf16 action_grad against fp32: relative L2 %.2e' % rel)
    assert torch.isfinite(out['bf16']).all() and rel < 5e-2


# ---- refine_actions ------------------------------------------------------------------------------------------------------------------------
def _refine_scene(pivp, deterministic=False):
    """B = 2, T = 4: the goal is the last frame the model itself predicts under the batch's own actions; the start is those actions moved by 0.2 * N(0, 1)
    on the free rows."""
    name = 'cdna_T5'
    mkw, nm, P, imgs, acts, stas = IR.case_inputs(name)
    imgs, acts, stas = imgs[:4], acts[:4], stas[:4]
    m = pivp.Model(nm, prefix='t', keep_activations=True, deterministic=deterministic)
    m.load_state_dict_reference(P)
    m([imgs, acts, stas], 0)
    goal = m._gen[-1].clone()
    start = acts[:3].copy()
    start[1:] += (0.2 * np.random.RandomState(3).standard_normal(start[1:].shape)).astype(np.float32)
    return m, imgs[:2], stas[0], start, acts[:1], goal


def test_refine_actions_lowers_the_cost(pivp):
    from pivp_amd import planning
    m, ctx_imgs, state, start, past, goal = _refine_scene(pivp, deterministic=True)
    kw = dict(goal_image=goal, steps=3, lr=0.02, past_actions=past)
    refined, costs = planning.refine_actions(m, ctx_imgs, state, start, **kw)
    c = costs.cpu().numpy()
    print('refine_actions cost per iteration and sample:', c.tolist())
    assert refined.shape == (3, 2, 5) and costs.shape == (4, 2) and refined.device.type == 'cuda' and np.isfinite(c).all()
    assert (c[3] < c[0]).all(), 'cost after three steps %s, before %s' % (c[3], c[0])
    r = refined.cpu().numpy()
    assert np.array_equal(r[:1], past), 'past_actions rows moved'
    assert (r[1:] != start[1:]).any()
    refined = refined.clone()
    # a deterministic model: the same bits again
    again, costs2 = planning.refine_actions(m, ctx_imgs, state, start, **kw)
    assert torch.equal(again, refined) and torch.equal(costs2, costs)
    # lr = 0: the actions come back bit-identical; bounds clamp the free rows only
    same, _ = planning.refine_actions(m, ctx_imgs, state, start, **dict(kw, lr=0.0))
    assert np.array_equal(same.cpu().numpy().view(np.uint32), start.view(np.uint32))
    clamped, _ = planning.refine_actions(m, ctx_imgs, state, start, **dict(kw, bounds=(-0.05, 0.05)))
    cl = clamped.cpu().numpy()
    assert np.abs(cl[1:]).max() <= np.float32(0.05) and np.array_equal(cl[:1], r[:1])
    # cost_fn: the same cost written by the caller and differentiated by autograd instead of the closed form
    fn = lambda gen: ((gen - goal) ** 2).mean(dim=(0, 2, 3, 4))
    _, cfn = planning.refine_actions(m, ctx_imgs, state, start, cost_fn=fn, steps=3, lr=0.02, past_actions=past)
    assert torch.allclose(cfn[0], costs[0], rtol=1e-5) and bool((cfn[3] < cfn[0]).all())


def test_refine_actions_never_synchronises_with_the_host(pivp):
    from pivp_amd import planning
    m, ctx_imgs, state, start, past, goal = _refine_scene(pivp)
    kw = dict(goal_image=goal, steps=2, lr=0.02, past_actions=past)
    planning.refine_actions(m, ctx_imgs, state, start, **kw)            # plans, workspaces and allocator blocks exist from here on
    torch.cuda.synchronize()
    args = [_dev(ctx_imgs), _dev(state), _dev(start)]
    kw['past_actions'] = _dev(past)
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            a = planning._check_refine_args(m, args[0], args[1], args[2], goal, None, 2, 0.02, past, None)
            torch.cuda.set_sync_debug_mode('default')
            b = planning._refine_upload(m, a, args[0], args[1], args[2], goal, kw['past_actions'])      # the uploads, once, in front of the loop
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode('error')
            res, costs = planning._refine_iterate(m, a, b)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not detects:
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made')
    assert torch.isfinite(res).all() and torch.isfinite(costs).all()
