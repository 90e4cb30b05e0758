"""GPU tests of planning on a goal image: pivp_goal_image_cost (include/pivp_goal_cost.h) against the float64 restatement
tests/goal_cost_reference.py, its bit-level properties, and `planning.cem_plan(goal_image=)`, `score_actions(goal_image=)`,
`refine_actions(goal_image=GoalImageCost)` and `cem_refine` end to end on the trained CDNA fixture.

Bounds.  The op: 1e-6 relative on per_step and cost, 1e-6 of the gradient's largest element -- the gate the project holds its other fp64-sum,
round-once ops to (pivp_image_loss, pivp_grad_stats); an fp64 sum rounded to fp32 once errs by 6e-8.  `cem_refine`'s cost against
`score_actions` on the returned actions: the two roll one sequence out on the training plan at batch 2 and on the inference plan at batch 1; the
margin is stated at the test.  The loops run under torch's sync debug mode with their uploads in front, as the project's other no-sync tests do."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import goal_cost_reference as GR  # noqa: E402
import track_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 1e-6


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (np.abs(want) + 1e-30)).max())


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _data(seed, S, K, H, W, G):
    rs = np.random.RandomState(seed)
    frames = rs.rand(S, K, 3, H, W).astype(np.float32)
    goal = rs.rand(G, 3, H, W).astype(np.float32)
    frames[0, 0, :, 0, :5] = goal[0, :, 0, :5]                                  # bit-equal pixels: sign(0) = 0
    frames[S - 1, K - 1, 1, H - 1, W - 3:] = goal[G - 1, 1, H - 1, W - 3:]      # ... and in the last group of a channel
    pixel_w = (rs.rand(H, W) * (rs.rand(H, W) > 0.25)).astype(np.float32)       # a quarter of the weights are zero
    step_w = (rs.rand(S) + 0.25).astype(np.float32)
    return frames, goal, pixel_w, step_w


# (S, K, H, W): 8 x 12 -- one partial round of the vector form; 7 x 10 -- a frame is 210 floats, so its base is off 16 bytes and the element-wise form
# runs, with a partial last group; 64 x 64 -- twelve full requests per thread; 72 x 64 and 67 x 63 -- more than 1024 groups per channel, the
# looping path, in the vector and the element-wise form
SHAPES = [(3, 5, 8, 12), (2, 3, 7, 10), (2, 4, 64, 64), (2, 3, 72, 64), (1, 2, 67, 63)]


@pytest.mark.parametrize('S,K,H,W', SHAPES)
def test_goal_cost_matches_the_float64_restatement(S, K, H, W):
    _gpu()
    import goal_cost_ops as ops
    worst = dict(per_step=0.0, cost=0.0, grad=0.0)
    n = 0
    for G in (1, K):
        frames, goal, pixel_w, step_w = _data(1000 * H + W + G, S, K, H, W, G)
        for pw in (None, pixel_w):
            inv = GR.inv_norm(pw, H, W)
            for w_mse, w_l1 in ((1.0, 0.0), (0.0, 1.0), (0.75, 0.4)):
                for accumulate, scale in ((0, 1.0), (1, 1.75), (0, 0.3)):
                    cost_in = (np.arange(K) * 0.37 + 0.5).astype(np.float32) if accumulate else None
                    cost, per_step, grad = ops.goal_cost(frames, goal, pw, inv, step_w, w_mse, w_l1, 2.0, scale, cost_in=cost_in)
                    rcost, rstep, rgrad = GR.goal_image_cost(frames, goal, pw, inv, step_w, w_mse, w_l1, 2.0, scale, cost_in=cost_in)
                    e = dict(per_step=_rel(per_step, rstep), cost=_rel(cost, rcost), grad=float(np.abs(grad - rgrad).max() / np.abs(rgrad).max()))
                    for k in worst:
                        worst[k] = max(worst[k], e[k])
                    assert e['per_step'] < GATE and e['cost'] < GATE and e['grad'] < GATE, (G, pw is not None, w_mse, w_l1, accumulate, scale, e)
                    assert (grad[0, 0, :, 0, :5] == 0).all() and (grad[S - 1, K - 1, 1, H - 1, W - 3:] == 0).all()      # sign(0) = 0, exactly
                    if pw is not None:
                        assert (grad[:, :, :, pw == 0] == 0).all() and np.abs(grad).max() > 0
                    n += 1
    print('goal cost %dx%dx%dx%d: %d variants, worst per_step %.2e  cost %.2e (relative)  grad %.2e (of the largest element)'
          % (S, K, H, W, n, worst['per_step'], worst['cost'], worst['grad']))


@pytest.mark.parametrize('H,W', [(8, 12), (64, 64), (72, 64)])
def test_goal_cost_bits_do_not_depend_on_the_launch(H, W):
    """K = 7 against each candidate alone at K = 1; G = K with the goal repeated against G = 1; with and without grad; a second launch; the vector form
    against the same data at a base shifted by 4 bytes (the element-wise form): all bit-identical."""
    _gpu()
    import goal_cost_ops as ops
    S, K = 2, 7
    frames, goal, pixel_w, step_w = _data(7 * H + W, S, K, H, W, 1)
    inv = GR.inv_norm(pixel_w, H, W)
    args = (pixel_w, inv, step_w, 0.75, 0.4, 2.0, 1.75)
    cost, per_step, grad = ops.goal_cost(frames, goal, *args)
    assert np.isfinite(cost).all() and np.abs(grad).max() > 0
    for k in range(K):
        c1, p1, g1 = ops.goal_cost(np.ascontiguousarray(frames[:, k:k + 1]), goal, *args)
        assert _bits(c1, cost[k:k + 1]) and _bits(p1, per_step[:, k:k + 1]) and _bits(g1, grad[:, k:k + 1]), k
    for other in (ops.goal_cost(frames, np.repeat(goal, K, axis=0), *args),          # G = K, the goal repeated
                  ops.goal_cost(frames, goal, *args),                                # a second launch
                  ops.goal_cost(frames, goal, *args, shift=1)):                      # the element-wise form
        assert _bits(other[0], cost) and _bits(other[1], per_step) and _bits(other[2], grad)
    for shift in (0, 1):
        c0, p0, g0 = ops.goal_cost(frames, goal, *args, want_grad=False, shift=shift)
        assert g0 is None and _bits(c0, cost) and _bits(p0, per_step)
    c2, p2, g2 = ops.goal_cost(frames, goal, None, GR.inv_norm(None, H, W), step_w, 1.0, 0.0, 2.0, 1.0)      # no pixel weights: both forms again
    c3, p3, g3 = ops.goal_cost(frames, goal, None, GR.inv_norm(None, H, W), step_w, 1.0, 0.0, 2.0, 1.0, shift=3)
    assert _bits(c2, c3) and _bits(p2, p3) and _bits(g2, g3)


@pytest.mark.parametrize('S,K,H,W', [(2, 3, 7, 10), (2, 4, 64, 64), (2, 3, 72, 64)])
def test_a_frame_that_is_not_finite_costs_bad_cost_and_has_no_gradient(S, K, H, W):
    _gpu()
    import goal_cost_ops as ops
    frames, goal, pixel_w, step_w = _data(11 * H + W, S, K, H, W, 1)
    args = (goal, pixel_w, GR.inv_norm(pixel_w, H, W), step_w, 0.75, 0.4, 2.5, 1.75)
    clean = ops.goal_cost(frames, *args)
    for value in (np.nan, np.inf):
        broken = frames.copy()
        broken[1, 2, 1, H // 2, W // 3] = value
        for shift in (0, 1):
            cost, per_step, grad = ops.goal_cost(broken, *args, shift=shift)
            assert per_step[1, 2] == np.float32(2.5) and (grad[1, 2] == 0).all() and np.isfinite(cost).all() and np.isfinite(grad).all()
            keep = np.ones((S, K), bool); keep[1, 2] = False
            assert _bits(per_step[keep], clean[1][keep]) and _bits(grad[keep], clean[2][keep])
            others = np.arange(K) != 2
            assert _bits(cost[others], clean[0][others])
            rcost, rstep, _ = GR.goal_image_cost(broken, *args)
            assert _rel(cost, rcost) < GATE and _rel(per_step, rstep) < GATE
        c0, p0, _ = ops.goal_cost(broken, *args, want_grad=False)
        assert _bits(c0, cost) and _bits(p0, per_step)


def test_goal_cost_bad_arguments_launch_nothing():
    _gpu()
    import goal_cost_ops as ops
    frames, goal, pixel_w, step_w = _data(0, 2, 3, 16, 16, 1)
    good = dict(pixel_w=pixel_w, inv_norm=GR.inv_norm(pixel_w, 16, 16), step_w=step_w, w_mse=1.0, w_l1=0.5, bad_cost=2.0, scale=1.0)
    assert ops.goal_cost_rc(frames, goal, **good)[0] == 0

    def refused(**over):
        kw = dict(good)
        call = {k: over.pop(k) for k in list(over) if k in ('null', 'S', 'K', 'H', 'W', 'G')}
        kw.update(over)
        rc, (cost, per_step, grad) = ops.goal_cost_rc(frames, goal, **kw, **call)
        untouched = (cost == ops.SENTINEL).all() and (per_step == ops.SENTINEL).all() and (grad == ops.SENTINEL).all()
        return rc == -1 and untouched
    for null in ('frames', 'goal', 'step_w', 'cost', 'per_step'):
        assert refused(null=null), null
    for over in (dict(S=0), dict(K=0), dict(K=-1), dict(H=1), dict(W=1), dict(W=253), dict(H=0), dict(H=32769), dict(G=2), dict(G=0), dict(G=-1)):
        assert refused(**over), over
    for name in ('inv_norm', 'w_mse', 'w_l1', 'bad_cost', 'scale'):
        for v in (np.nan, np.inf, -np.inf):
            assert refused(**{name: v}), (name, v)
    assert refused(inv_norm=0.0) and refused(inv_norm=-1.0 / 768)


# ---- the planner on a goal image -----------------------------------------------------------------------------------------------------------------
SETUP = dict(horizon=2, iterations=2, samples=8, elites=2, init_std=0.5, seed=3)


@functools.lru_cache(maxsize=None)
def _scene():
    """The trained CDNA fixture on the moving batch of tests/test_gpu_planning.py: two context frames, one past action; the goal is a later true frame."""
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    return P, nm, imgs[:2], stas[0], acts[:1, 0], np.ascontiguousarray(imgs[4, 0])


def _model(pivp_amd, **kw):
    P, nm = _scene()[:2]
    m = pivp_amd.Model(nm, is_cdna=True, prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _spec(planning, goal):
    H, W = goal.shape[1:]
    roi = np.zeros((H, W), np.float32)
    roi[8:56, 8:56] = 1.0
    roi[24:40, 24:40] = 2.0
    return planning.GoalImageCost(goal, mse=1.0, l1=0.25, pixel_weight=roi, step_weights=[0.5, 1.5], weight=2.0)


def _no_sync(torch, fn):
    """fn() under torch.cuda.set_sync_debug_mode('error'); the mode must flag a synchronising call on this build for the run to mean anything."""
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda:0')
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


def _check_image_trace(torch, pivp_amd, res, spec, ctx_imgs, state, past, chunk, setup=SETUP):
    """Every record: a fresh `imagine` of its candidates at the batch the loop used gives the frames; their restatement is `image_cost` and `cost`;
    the elites are the cheapest by the device's cost."""
    K, M, Hh = setup['samples'], setup['elites'], setup['horizon']
    fresh = _model(pivp_amd)
    worst = 0.0
    for rec in res.trace:
        cand = rec['actions'].cpu().numpy()
        assert cand.shape == (1 + Hh, K, 5) and (cand[:1] == past[:, None]).all()
        assert rec['mass'].shape == (Hh, K, 0) and rec['image_cost'].shape == (Hh, K)
        cost, image_cost = rec['cost'].cpu().numpy(), rec['image_cost'].cpu().numpy()
        for k0 in range(0, K, chunk):
            sl = slice(k0, k0 + chunk)
            gen = fresh.imagine(np.repeat(ctx_imgs, chunk, axis=1), np.ascontiguousarray(cand[:, sl]), np.repeat(state, chunk, axis=0))
            frames = gen[1:].cpu().numpy()
            assert frames.shape == (Hh, chunk, 3, 64, 64)
            rcost, rstep, _ = GR.spec_cost(frames, spec)
            worst = max(worst, _rel(image_cost[:, sl], rstep), _rel(cost[sl], rcost))
        assert np.isfinite(cost).all() and cost.min() > 0
        assert rec['elites'].cpu().numpy().tolist() == np.argsort(cost, kind='stable')[:M].tolist()
    print('cem_plan(goal_image=) chunk %d: image_cost / cost against the restatement, worst %.2e (relative)' % (chunk, worst))
    assert worst < GATE
    return fresh


def test_cem_plan_on_a_goal_image_alone():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past, goal = _scene()
    spec = _spec(planning, goal)
    m = _model(pivp_amd)
    run = lambda model, **kw: planning.cem_plan(model, ctx_imgs, state, None, None, past_actions=past, goal_image=spec, trace=True, **dict(SETUP, **kw))
    res = run(m)
    assert res.actions.shape == (2, 5) and len(res.trace) == 2 and res.cost.is_cuda
    per = res.best_cost_per_iteration.cpu().numpy()
    assert np.isfinite(per).all() and (np.diff(per) <= 0).all() and float(res.cost) == per[-1] == min(float(r['cost'].min()) for r in res.trace)
    last_frames = torch.stack(m.gen_images).clone()
    fresh = _check_image_trace(torch, pivp_amd, res, spec, ctx_imgs, state, past, chunk=8)
    fresh.imagine(np.repeat(ctx_imgs, 8, axis=1), res.trace[-1]['actions'], np.repeat(state, 8, axis=0))
    assert torch.equal(torch.stack(fresh.gen_images), last_frames)                      # imagine gives the rollout's frames, bit for bit
    # the same seed: the same bits (another model, and the first one again); a bare array is the spec's defaults
    for other in (run(_model(pivp_amd)), run(m)):
        for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
            assert torch.equal(getattr(res, name), getattr(other, name)), name
        assert all(torch.equal(a[k], b[k]) for a, b in zip(res.trace, other.trace) for k in a)
    bare = planning.cem_plan(m, ctx_imgs, state, None, None, past_actions=past, goal_image=goal, trace=True, **SETUP)
    dflt = planning.cem_plan(m, ctx_imgs, state, None, None, past_actions=past, goal_image=planning.GoalImageCost(goal), trace=True, **SETUP)
    assert torch.equal(bare.cost, dflt.cost) and torch.equal(bare.trace[1]['image_cost'], dflt.trace[1]['image_cost'])
    assert torch.equal(bare.trace[0]['actions'], res.trace[0]['actions'])               # the sampler does not see the cost
    # chunked: the same candidates in the first iteration, the same checks per chunk
    ch = run(m, chunk=4)
    assert torch.equal(ch.trace[0]['actions'], res.trace[0]['actions'])
    _check_image_trace(torch, pivp_amd, ch, spec, ctx_imgs, state, past, chunk=4)
    # the loop under sync debug mode, its uploads in front
    kw = dict(SETUP, chunk=4)
    a = planning._check_cem_args(m, ctx_imgs, state, designated_rc=None, goal_rc=None, past_actions=past, goal_image=spec, **kw)
    b = planning._cem_upload(m, a, ctx_imgs, state)
    quiet = _no_sync(torch, lambda: planning._cem_iterate(m, a, b, trace=False))
    assert torch.equal(quiet.actions, ch.actions) and torch.equal(quiet.best_cost_per_iteration, ch.best_cost_per_iteration)


def test_cem_plan_with_both_goals_adds_the_image_cost():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past, goal = _scene()
    spec = _spec(planning, goal)
    m = _model(pivp_amd)
    pix = dict(designated_rc=[[32, 32], [20, 40]], goal_rc=[[40, 24], [20, 44]], plane_weights=[1.0, 0.5], step_weights=[0.25, 1.0])
    kw = dict(SETUP, past_actions=past, trace=True, **pix)
    alone = planning.cem_plan(m, ctx_imgs, state, **kw)
    both = planning.cem_plan(m, ctx_imgs, state, goal_image=spec, **kw)
    assert 'image_cost' not in alone.trace[0] and torch.equal(alone.trace[0]['actions'], both.trace[0]['actions'])
    assert torch.equal(alone.trace[0]['mass'], both.trace[0]['mass']) and torch.equal(alone.trace[0]['edist'], both.trace[0]['edist'])
    image = both.trace[0]['image_cost'].cpu().numpy().astype(np.float64)
    want = alone.trace[0]['cost'].cpu().numpy().astype(np.float64) + spec.weight * (spec.steps(2).astype(np.float64)[:, None] * image).sum(axis=0)
    err = _rel(both.trace[0]['cost'].cpu().numpy(), want)
    print('both goals: cost against pixel cost + weight * image cost, %.2e (relative); image share %.3g of %.3g'
          % (err, float((want - alone.trace[0]['cost'].cpu().numpy()).mean()), float(want.mean())))
    assert err < GATE and (image > 0).all()
    # goal_image=None: the bits of a call without the argument
    again = planning.cem_plan(m, ctx_imgs, state, goal_image=None, **kw)
    assert torch.equal(again.cost, alone.cost) and all(torch.equal(a[k], b[k]) for a, b in zip(alone.trace, again.trace) for k in a)


def test_score_actions_on_a_goal_image():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past, goal = _scene()
    spec = planning.GoalImageCost(goal, mse=0.5, l1=1.0, step_weights=[1.0, 0.5, 0.25], weight=1.5)
    K = 4
    cand = (np.random.RandomState(2).randn(K, 4, 5) * 0.5).astype(np.float32)
    cand[:, 0] = past[0]
    m = _model(pivp_amd)
    cost = planning.score_actions(m, ctx_imgs, state, cand, None, None, goal_image=spec)
    frames = torch.stack(m.gen_images)[1:].cpu().numpy()
    rcost, _, _ = GR.spec_cost(frames, spec)
    assert cost.shape == (K,) and _rel(cost.cpu().numpy(), rcost) < GATE
    fresh = _model(pivp_amd)
    gen = fresh.imagine(np.repeat(ctx_imgs, K, axis=1), np.ascontiguousarray(cand.transpose(1, 0, 2)), np.repeat(state, K, axis=0))
    assert torch.equal(gen[1:], torch.from_numpy(frames).to(gen.device))
    # with a pixel goal as well: the two costs add
    pixel = planning.score_actions(m, ctx_imgs, state, cand, (32, 32), (40, 24))
    both = planning.score_actions(m, ctx_imgs, state, cand, (32, 32), (40, 24), goal_image=spec)
    assert torch.equal(both, pixel + cost)


def _refine_scene(pivp_amd):
    P, nm, ctx_imgs, state, past, goal = _scene()
    m = _model(pivp_amd, keep_activations=True)
    B = 2
    start = np.zeros((3, B, 5), np.float32)
    start[0] = past[0]
    start[1:] = (0.2 * np.random.RandomState(3).standard_normal((2, B, 5))).astype(np.float32)
    return m, np.repeat(ctx_imgs, B, axis=1), np.repeat(state, B, axis=0), start, past, goal


def test_refine_actions_on_a_default_spec_is_the_bare_array_cost():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    m, ctx2, state2, start, past, goal = _refine_scene(pivp_amd)
    spec = planning.GoalImageCost(goal)
    kw = dict(steps=2, lr=0.02, past_actions=past)
    r_bare, c_bare = planning.refine_actions(m, ctx2, state2, start, goal_image=goal, **kw)
    r_spec, c_spec = planning.refine_actions(m, ctx2, state2, start, goal_image=spec, **kw)
    cb, cs = c_bare.cpu().numpy(), c_spec.cpu().numpy()
    print('refine_actions costs, bare array %s, GoalImageCost %s' % (cb.tolist(), cs.tolist()))
    assert _rel(cs[0], cb[0]) < GATE and np.isfinite(cs).all() and (cs[2] < cs[0]).all()
    assert np.array_equal(r_spec.cpu().numpy()[:1], start[:1]) and (r_spec.cpu().numpy()[1:] != start[1:]).any()
    # one (B, 3, H, W) goal per sample
    per = planning.GoalImageCost(np.stack([goal, goal]))
    _, c_per = planning.refine_actions(m, ctx2, state2, start, goal_image=per, **dict(kw, steps=1))
    assert _rel(c_per.cpu().numpy()[0], cb[0]) < GATE
    # lr = 0 returns the input's bits on either path
    for g in (goal, spec):
        same, _ = planning.refine_actions(m, ctx2, state2, start, goal_image=g, **dict(kw, lr=0.0))
        assert np.array_equal(same.cpu().numpy().view(np.uint32), start.view(np.uint32))
    # the loop under sync debug mode, its uploads in front
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')
    args = [dev(ctx2), dev(state2), dev(start)]
    a = planning._check_refine_args(m, args[0], args[1], args[2], spec, None, 2, 0.02, past, None)
    b = planning._refine_upload(m, a, args[0], args[1], args[2], spec, dev(past))
    res, costs = _no_sync(torch, lambda: planning._refine_iterate(m, a, b))
    assert torch.equal(costs, c_spec) or _rel(costs.cpu().numpy(), cs) < 1e-4      # (a default model's sweep is not bit-reproducible)
    assert torch.isfinite(res).all()


def test_cem_refine_returns_the_cheapest_of_three():
    """MARGIN: `cost` comes from a training-plan rollout at batch 2 (or, source 0, CEM's inference-plan rollout at batch 8), `score_actions` from an
    inference-plan rollout at batch 1.  The project bounds the batch dependence of a planning cost by 1e-4 absolute on costs of order 10
    (tests/test_gpu_planning.py, chunk 8 against 16): 1e-5 relative, which is the gate here.  Measured on this fixture: 0 for both distances (equal
    bits, profiles/r17/NOTES.md) -- not a contract, so the gate is the bound and not the measurement."""
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, ctx_imgs, state, past, goal = _scene()
    spec = _spec(planning, goal)
    m = _model(pivp_amd, keep_activations=True)
    kw = dict({k: v for k, v in SETUP.items() if k != 'horizon'}, action_low=-1.0, action_high=1.0)
    res = planning.cem_refine(m, ctx_imgs, state, 2, spec, past_actions=past, refine_steps=2, lr=0.02, **kw)
    source = int(res.source)
    three = [float(res.cem.cost)] + res.refine_costs[-1].cpu().numpy().tolist()
    print('cem_refine: CEM best %.6g, refined best %.6g, refined mean %.6g -> source %d; refine costs %s'
          % (three[0], three[1], three[2], source, res.refine_costs.cpu().numpy().tolist()))
    assert source in (0, 1, 2) and res.actions.shape == (2, 5) and res.refine_costs.shape == (3, 2)
    assert float(res.cost) <= float(res.cem.cost) and float(res.cost) == min(three) and source == int(np.argmin(three))
    acts = res.actions.cpu().numpy()
    assert np.abs(acts).max() <= 1.0
    if source == 0:
        assert torch.equal(res.actions, res.cem.actions)
    # CEM's stage is cem_plan's: the same seed, the same plan
    plain = planning.cem_plan(_model(pivp_amd), ctx_imgs, state, None, None, 2, past_actions=past, goal_image=spec, **kw)
    assert torch.equal(plain.actions, res.cem.actions) and torch.equal(plain.cost, res.cem.cost) and torch.equal(plain.mean, res.cem.mean)
    # the refinement started from CEM's best: its first cost is CEM's, to the distance between the two plans
    first = res.refine_costs[0].cpu().numpy()
    d_plans = abs(first[0] / float(res.cem.cost) - 1)
    # score_actions on the returned actions
    cand = np.concatenate((past, acts))[None]
    scored = float(planning.score_actions(_model(pivp_amd), ctx_imgs, state, cand, None, None, goal_image=spec)[0])
    d_score = abs(scored / float(res.cost) - 1)
    print('cem_refine: training-plan against inference-plan cost of CEM\'s best %.2e, score_actions against cost %.2e (relative)' % (d_plans, d_score))
    assert d_plans < 1e-5 and d_score < 1e-5
    # the loop under sync debug mode, its uploads in front
    a = planning._check_cem_refine_args(m, ctx_imgs, state, 2, spec, past, 2, 0.02, dict(kw))
    b = planning._cem_refine_upload(m, a, ctx_imgs, state)
    quiet = _no_sync(torch, lambda: planning._cem_refine_iterate(m, a, b))
    assert torch.equal(quiet.cem.actions, res.cem.actions) and torch.isfinite(quiet.cost) and float(quiet.cost) <= float(quiet.cem.cost)
