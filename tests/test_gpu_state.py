"""GPU tests of the recurrent state across calls (include/pivp_state.h): `Model(carry_state=True)`, `imagine(observed=, advance=)`,
`RecurrentState`, pivp_state_copy and planning from a belief.

Bounds.  Against the reference's semantics the gate is the project's own: max per-pixel L2 < 1e-4 against the float64 oracle called the same way
(tests/test_gpu_model.py).  On the inputs used here -- two consecutive six-frame windows of R.moving_batch(2, 12, 64, 64, seed=31), widened random
weights for CDNA / DNA, the trained ones for STP -- the float32 NumPy oracle is within 9.8e-6 / 7.3e-6 (CDNA, first / second call), 1.0e-6 / 1.3e-6
(STP) and 2.3e-5 / 2.1e-5 (DNA) of the float64 one, so plain float32 meets the gate with a margin of four or more, and a second call that
forgot the state would be off by 0.5 .. 4.3 (the float64 oracle, carried against fresh).  Everything else is bit equality: a split rollout is the
whole rollout, a restored snapshot replays, a copy is a copy.  The planning cost from a belief is held to ten times max(the float32 oracle's own
relative cost error, 1e-5) -- 1e-5 being the bound of a ratio of two fp32 sums over a plane (tests/test_gpu_planning.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reference as PR  # noqa: E402
import track_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
GATE = 1e-4


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _model(pivp_amd, model_type, nm, P, **kw):
    m = pivp_amd.Model(nm, is_cdna=model_type == 'CDNA', is_stp=model_type == 'STP', is_dna=model_type == 'DNA', prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _random_params(model_type, size=64, seed=4):
    nm = 1 if model_type == 'DNA' else 10
    return R.init_params_widened(seed=seed, scale=1.0, num_masks=nm, model_type=model_type, height=size, width=size), nm


def _registration(plan):
    a, b, o = ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_int(-1)
    assert plan.lib.pivp_plan_get_rollout_state(plan.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o)) == 0
    return a.value, b.value, o.value


# ---- 1. against the reference's semantics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model_type', ['CDNA', 'STP', 'DNA'])
def test_a_second_call_continues_from_the_first_as_the_reference_does(model_type):
    torch, pivp_amd = _gpu()
    P, nm = TR.load_trained('STP') if model_type == 'STP' else _random_params(model_type)
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, 12, 64, 64, seed=31))
    windows = [slice(0, 6), slice(6, 12)]
    ref = R.Model(nm, params=P, dtype=np.float64, prefix='x', **TR.FLAGS[model_type]); ref.train = False
    want = []
    for w in windows:                                    # no reset_state() in between: TM:254-257 keeps c and h
        ref([imgs[w], acts[w], stas[w]], 0)
        want.append(np.stack(ref.gen_images))
    m = _model(pivp_amd, model_type, nm, P, carry_state=True)
    got = []
    with pivp_amd.using_config('train', False):
        for w in windows:
            m([imgs[w], acts[w], stas[w]], 0)
            got.append(torch.stack(m.gen_images).cpu().numpy())
        fresh = _model(pivp_amd, model_type, nm, P)
        fresh([imgs[windows[1]], acts[windows[1]], stas[windows[1]]], 0)
        forgot = torch.stack(fresh.gen_images).cpu().numpy()
    err = [R.per_pixel_l2(g, w).max() for g, w in zip(got, want)]
    apart = R.per_pixel_l2(got[1], forgot).max()
    print('%s: max per-pixel L2, first call %.3e, second call %.3e; second call against a fresh start %.3e' % (model_type, err[0], err[1], apart))
    assert got[0].shape == (5, 2, 3, 64, 64) and all(R.per_pixel_l2(g, w).max() < GATE for g, w in zip(got, want))      # every frame of both calls
    assert apart > 1000 * GATE                           # ... and the state matters: a model that forgot it would be nowhere near
    assert _registration(m._active) == (None, None, 0)   # the registration was the call's own


# ---- 2. a split rollout is the whole rollout, bit for bit -----------------------------------------------------------------------------------------
SPLIT = [('CDNA', 'fp32', 64, 4, 5), ('STP', 'fp32', 64, 4, 5), ('DNA', 'fp32', 64, 4, 5), ('CDNA', 'bf16', 64, 4, 5), ('CDNA', 'fp16x3', 64, 4, 5),
         ('CDNA', 'fp32', 128, 2, 2)]


@pytest.mark.parametrize('model_type,precision,size,n1,n2', SPLIT, ids=['%s-%s-%d-%d+%d' % c for c in SPLIT])
def test_a_split_rollout_is_the_whole_rollout(model_type, precision, size, n1, n2):
    torch, pivp_amd = _gpu()
    P, nm = _random_params(model_type, size)
    n = n1 + n2
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, n + 1, size, size, seed=31))
    planes = np.random.RandomState(1).rand(2, 3, size, size).astype(np.float32)
    plain = _model(pivp_amd, model_type, nm, P, precision=precision)
    whole = plain.imagine(imgs[:2], acts[:n], stas[0], designated=planes)
    whole_states, whole_track = torch.stack(plain.gen_states), plain.pixel_distrib
    assert whole.shape == (n, 2, 3, size, size) and whole_track.shape == (n - 1, 2, 3, size, size) and torch.isfinite(whole).all()
    m = _model(pivp_amd, model_type, nm, P, precision=precision, carry_state=True)
    again = m.imagine(imgs[:2], acts[:n], stas[0], designated=planes)       # a first call of a carrying model: the plain model's bits
    assert torch.equal(again, whole) and torch.equal(m.pixel_distrib, whole_track)
    end_state = m.recurrent_state()
    m.reset_state()
    first = m.imagine(imgs[:2], acts[:n1], stas[0], designated=planes)
    first_states, first_track = torch.stack(m.gen_states), m.pixel_distrib
    assert first_track.shape == (n1 - 1, 2, 3, size, size)
    # the recipe of imagine's docstring: the last predicted frame is the one observed frame, the last predicted robot state the state, and the
    # tracked planes go on from the first call's last raw plane, given on that frame
    second = m.imagine(first[-1:], acts[n1:n], m.gen_states[-1], designated=first_track[-1], observed=1)
    assert second.shape == (n2, 2, 3, size, size) and m.pixel_distrib.shape == (n2, 2, 3, size, size)
    assert torch.equal(torch.cat((first, second)), whole)
    assert torch.equal(torch.cat((first_states, torch.stack(m.gen_states))), whole_states)
    assert torch.equal(torch.cat((first_track, m.pixel_distrib)), whole_track)
    assert torch.equal(m.recurrent_state().data, end_state.data)             # ... and both ways end in the same recurrent state
    assert (end_state.batch, end_state.hw) == (2, (size, size)) and float(end_state.data.abs().max()) > 0


def test_one_step_at_a_time_is_the_whole_rollout():
    """Streaming: a plan of T = 2 (one step, shorter than the configured context of two frames) per observed or predicted frame."""
    torch, pivp_amd = _gpu()
    P, nm = _random_params('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, 5, 64, 64, seed=31))
    whole = _model(pivp_amd, 'CDNA', nm, P).imagine(imgs[:2], acts[:4], stas[0])
    m = _model(pivp_amd, 'CDNA', nm, P, carry_state=True)
    frames, frame, state = [], imgs[0:1], stas[0]
    for t in range(4):
        out = m.imagine(frame, acts[t:t + 1], state, observed=1)
        frames.append(out)
        frame, state = (imgs[1:2] if t == 0 else out), m.gen_states[-1]       # the second observed frame, then the model's own
    assert torch.equal(torch.cat(frames), whole)


# ---- 3. reset_state(), set_recurrent_state() and advance=False ------------------------------------------------------------------------------------
def test_reset_snapshot_and_advance():
    torch, pivp_amd = _gpu()
    P, nm = _random_params('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, 8, 64, 64, seed=31))
    w1, w2 = [imgs[:4], acts[:4], stas[:4]], [imgs[4:], acts[4:], stas[4:]]
    m = _model(pivp_amd, 'CDNA', nm, P, carry_state=True)
    with pivp_amd.using_config('train', False):
        l1 = float(m(w1)); g1 = torch.stack(m.gen_images).clone()
        snap = m.recurrent_state()
        l2 = float(m(w2)); g2 = torch.stack(m.gen_images).clone()
        after = m.recurrent_state()
        assert not torch.equal(snap.data, after.data)
        # reset_state() restores a fresh start
        m.reset_state()
        assert m.recurrent_state() is None and m.loss == 0.0 and m.summaries == []
        assert float(m(w1)) == l1 and torch.equal(torch.stack(m.gen_images), g1) and torch.equal(m.recurrent_state().data, snap.data)
        # a snapshot replays, as often as wanted: the model copies it and never writes into it
        kept = snap.data.clone()
        for _ in range(2):
            m.set_recurrent_state(snap)
            assert float(m(w2)) == l2 and torch.equal(torch.stack(m.gen_images), g2) and torch.equal(m.recurrent_state().data, after.data)
        assert torch.equal(snap.data, kept)
        # a call of another T from the same state: the state is per model, not per plan
        m.set_recurrent_state(snap)
        m([imgs[4:7], acts[4:7], stas[4:7]])
        assert torch.equal(torch.stack(m.gen_images), g2[:2])
    # advance=False reads the state and leaves its bytes alone
    m.set_recurrent_state(snap)
    ptr, before = m._state.data.data_ptr(), m._state.data.clone()
    a = m.imagine(imgs[4:6], acts[4:7], stas[4], advance=False)
    assert m._state.data.data_ptr() == ptr and torch.equal(m._state.data, before)
    b = m.imagine(imgs[4:6], acts[4:7], stas[4], advance=False)
    assert torch.equal(a, b) and torch.equal(a, g2)                           # (feed-self from the same state: the second window's call)
    c = m.imagine(imgs[4:6], acts[4:7], stas[4])                              # advancing: the same frames, then the state moves on
    assert torch.equal(c, a) and torch.equal(m._state.data, after.data)
    m.reset_state()
    assert not torch.equal(m.imagine(imgs[4:6], acts[4:7], stas[4], advance=False), a) and m.recurrent_state() is None


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_call_starts_from_zeros():
    torch, pivp_amd = _gpu()
    P, nm = _random_params('CDNA')
    imgs, acts, stas = R.moving_batch(2, 4, 64, 64, seed=31)
    m = _model(pivp_amd, 'CDNA', nm, P)
    with pivp_amd.using_config('train', False):
        l1 = float(m([imgs, acts, stas])); g1 = torch.stack(m.gen_images).clone()
        assert _registration(m._active) == (None, None, 0)
        l2 = float(m([imgs, acts, stas]))                                       # no reset_state() in between
    assert l1 == l2 and torch.equal(torch.stack(m.gen_images), g1)
    assert _registration(m._active) == (None, None, 0) and m._state is None
    i1 = m.imagine(np.asarray(imgs)[:2], np.asarray(acts)[:3], np.asarray(stas)[0])
    assert torch.equal(i1, g1) and _registration(m._active) == (None, None, 0)


# ---- 5. pivp_state_copy alone ---------------------------------------------------------------------------------------------------------------------
PAD = 64


def _copy(torch, pivp_amd, src, hw, B_dst, index, offset=0, null=None, override=()):
    """src: RecurrentState -> (rc, dst RecurrentState, the PAD floats behind dst are intact).  offset: floats both buffers are shifted by; null /
    override: an argument passed as NULL / with another value than the buffers were made for."""
    from pivp_amd import _lib, state as ST
    lib = _lib.load()
    per = ST.state_layout(*hw)[1]
    dev = src.data.device
    s = torch.empty(src.data.numel() + offset, dtype=torch.float32, device=dev)
    s[offset:] = src.data
    d = torch.full((B_dst * per + offset + PAD,), -77.0, dtype=torch.float32, device=dev)
    idx = None if index is None else torch.tensor(index, dtype=torch.int32, device=dev)
    cfg = ST._config(*hw)
    args = dict(src=s.data_ptr() + 4 * offset, B_src=src.batch, dst=d.data_ptr() + 4 * offset, B_dst=B_dst, index=None if idx is None else idx.data_ptr())
    args.update(dict(override))
    if null:
        args[null] = None
    rc = lib.pivp_state_copy(ctypes.byref(cfg), args['src'], args['B_src'], args['dst'], args['B_dst'], args['index'],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = ST.RecurrentState(d[offset:offset + B_dst * per], B_dst, hw)
    return rc, out, bool((d[offset + B_dst * per:] == -77.0).all()) and bool((d[:offset] == -77.0).all())


def _random_state(torch, pivp_amd, B, hw, seed):
    from pivp_amd import state as ST
    g = torch.Generator().manual_seed(seed)
    return ST.RecurrentState(torch.randn(B * ST.state_layout(*hw)[1], generator=g).to('cuda:0'), B, hw)


COPIES = [(1, [0, 0, 0], 0), (3, [2, 1, 1, 0, 0], 0), (3, None, 0), (3, [0, 2, 1], 0), (3, [2, 1, 1, 0, 0], 1), (3, None, 1)]


@pytest.mark.parametrize('B_src,index,offset', COPIES, ids=['%d-%s-off%d' % (b, 'id' if i is None else ''.join(map(str, i)), o) for b, i, o in COPIES])
def test_state_copy_is_torch_indexing_of_the_cells(B_src, index, offset):
    """16 x 16 frames (512 .. 2,048 floats per sample and segment: short runs); offset 1 puts both buffers off 16 bytes -> the element-wise form."""
    torch, pivp_amd = _gpu()
    hw = (16, 16)
    src = _random_state(torch, pivp_amd, B_src, hw, 5)
    B_dst = B_src if index is None else len(index)
    rc, dst, intact = _copy(torch, pivp_amd, src, hw, B_dst, index, offset)
    assert rc == 0 and intact
    pick = torch.arange(B_src) if index is None else torch.tensor(index)
    for (sc, sh), (dc, dh) in zip(src.cells(), dst.cells()):
        assert torch.equal(dc, sc[pick.to(sc.device)]) and torch.equal(dh, sh[pick.to(sh.device)])
    if offset == 0 and index is not None:               # the Python surface is the same launch
        sel = src.select(index)
        assert torch.equal(sel.data, dst.data) and (sel.batch, sel.hw) == (B_dst, hw)
        if B_src == 1:
            assert torch.equal(src.expand(B_dst).data, dst.data)


def test_state_copy_at_1024_samples_of_64x64():
    """1.27 GB of state: offsets past 2^31 bytes.  The first and the last sample of every segment."""
    torch, pivp_amd = _gpu()
    hw = (64, 64)
    src = _random_state(torch, pivp_amd, 2, hw, 6)
    index = [(3 * b // 2) % 2 for b in range(1024)]
    index[0], index[-1] = 1, 0
    rc, dst, intact = _copy(torch, pivp_amd, src, hw, 1024, index)
    assert rc == 0 and intact and dst.data.numel() * 4 > 2 ** 30
    for (sc, sh), (dc, dh) in zip(src.cells(), dst.cells()):
        for s, d in ((sc, dc), (sh, dh)):
            assert torch.equal(d[0], s[1]) and torch.equal(d[-1], s[0]) and torch.equal(d[511], s[index[511]])


def test_state_copy_refusals():
    torch, pivp_amd = _gpu()
    hw = (16, 16)
    src = _random_state(torch, pivp_amd, 2, hw, 7)
    for kw in (dict(null='dst'), dict(null='src'), dict(override=dict(B_dst=0)), dict(override=dict(B_dst=-1)), dict(override=dict(B_src=0))):
        rc, dst, intact = _copy(torch, pivp_amd, src, hw, 3, [0, 1, 0], **kw)
        assert rc == -1 and intact and bool((dst.data == -77.0).all()), kw       # PIVP_ERR_BADARG, nothing written
    rc, dst, intact = _copy(torch, pivp_amd, src, hw, 3, None)                  # the identity needs equal batches
    assert rc == -1 and bool((dst.data == -77.0).all())
    rc, dst, intact = _copy(torch, pivp_amd, src, hw, 3, [0, 1, 0])             # the same call with good arguments runs
    assert rc == 0 and intact and not bool((dst.data == -77.0).any())


# ---- 6. planning from a belief --------------------------------------------------------------------------------------------------------------------
def _belief_scene(torch, pivp_amd, precision='fp32'):
    """The trained CDNA model has seen frame 0 (and taken action 0): its state is the belief, frame 1 the newest frame, the predicted robot state
    the state -- what steps 1 .. of a rollout over both context frames start from.  The observer is an fp32 model (the state is fp32 in every mode;
    the bf16 gate kernels do not take batch 1 at this size); with another precision the model returned is a planner of that mode that has seen nothing."""
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a, dtype=np.float32) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    m = _model(pivp_amd, 'CDNA', nm, P, carry_state=True)
    m.imagine(imgs[:1], acts[:1], stas[0], observed=1)
    belief, state1 = m.recurrent_state(), m.gen_states[-1].clone()
    if precision != 'fp32':
        m = _model(pivp_amd, 'CDNA', nm, P, carry_state=True, precision=precision)
    return P, nm, imgs, acts, stas, m, belief, state1


def test_score_actions_from_a_belief_against_the_oracle():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, imgs, acts, stas, m, belief, state1 = _belief_scene(torch, pivp_amd)
    K, Hh = 4, 4
    rs = np.random.RandomState(2)
    cand = (acts[1:1 + Hh, 0][None] + rs.randn(K, Hh, 5) * 0.5).astype(np.float32)
    cand[0] = acts[1:1 + Hh, 0]
    carried = m.recurrent_state()
    cost = planning.score_actions(m, imgs[1:2], state1, cand, (32, 32), (40, 24), belief=belief)
    got = torch.stack(m.gen_images).cpu().numpy()
    assert cost.shape == (K,) and got.shape == (Hh, K, 3, 64, 64)
    assert torch.equal(m.recurrent_state().data, carried.data) and m.recurrent_state().batch == 1      # the model's own state is what it was
    # the oracle at batch 4 on the replicated context: both frames, action 0 in front of every candidate
    T = Hh + 2
    images = np.zeros((T, K, 3, 64, 64)); images[:2] = imgs[:2]
    actions = np.zeros((T, K, 5)); actions[0] = acts[0]; actions[1:1 + Hh] = cand.transpose(1, 0, 2)
    states = np.zeros((T, K, 5)); states[0] = stas[0]
    D0 = np.zeros((K, 1, 64, 64)); D0[:, 0, 32, 32] = 1.0
    costs = {}
    for dt in (np.float64, np.float32):
        ref = TR.run_oracle(P, 'CDNA', nm, (images, actions, states), dtype=dt)
        track = TR.advect_rollout(ref, D0, 1)
        costs[dt] = PR.plan_cost(track, [[40, 24]], np.ones(Hh), np.ones(1), 89.0)[0]
        if dt is np.float64:
            want = np.stack(ref.gen_images)[1:]
    l2 = R.per_pixel_l2(got, want).max()
    rel = np.abs(cost.cpu().numpy() / costs[np.float64] - 1).max()
    own = np.abs(costs[np.float32] / costs[np.float64] - 1).max()
    print('score_actions(belief): max per-pixel L2 %.3e; cost %s, relative error %.2e (float32 oracle %.2e)' % (l2, costs[np.float64], rel, own))
    assert l2 < GATE and rel < 10 * max(own, 1e-5)
    assert costs[np.float64].max() - costs[np.float64].min() > 1e-3 * costs[np.float64].min()      # the candidates differ: the comparison means something


SETUP = dict(designated_rc=[[32, 32]], goal_rc=[[40, 24]], horizon=4, iterations=3, samples=16, elites=4, init_std=0.5, seed=3)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_cem_plan_from_a_belief_is_reproducible(precision):
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, imgs, acts, stas, m, belief, state1 = _belief_scene(torch, pivp_amd, precision)
    kept = belief.data.clone()
    a = planning.cem_plan(m, imgs[1:2], state1, belief=belief, trace=True, **SETUP)
    b = planning.cem_plan(m, imgs[1:2], state1, belief=belief, trace=True, chunk=16, **SETUP)
    m2 = _belief_scene(torch, pivp_amd, precision)[5]
    c = planning.cem_plan(m2, imgs[1:2], state1, belief=belief, **SETUP)      # another model, the same belief
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
        assert torch.isfinite(getattr(a, name)).all() and torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name)), name
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a.trace, b.trace) for k in x)
    assert a.actions.shape == (4, 5) and a.trace[0]['actions'].shape == (4, 16, 5)      # horizon steps: no past rows in front
    assert (np.diff(a.best_cost_per_iteration.cpu().numpy()) <= 0).all()
    own = m.recurrent_state()                                                 # the planner's own state is what it was: the observer's, or none
    assert torch.equal(belief.data, kept) and (torch.equal(own.data, kept) if precision == 'fp32' else own is None) and len(m.gen_images) == 4
    other = planning.cem_plan(m, imgs[1:2], state1, belief=belief, trace=True, **dict(SETUP, seed=4))
    assert not torch.equal(other.trace[0]['actions'], a.trace[0]['actions'])


def test_planning_from_the_frames_is_untouched_by_a_carried_state():
    """`belief=None` on a carrying model: every candidate starts from zeros over the context frames -- the plain model's bits -- and the carried
    state is neither read nor written."""
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, imgs, acts, stas, m, belief, state1 = _belief_scene(torch, pivp_amd)
    plain = _model(pivp_amd, 'CDNA', nm, P)
    kw = dict(SETUP, iterations=2, past_actions=acts[:1, 0])
    a, b = planning.cem_plan(m, imgs[:2], stas[0], **kw), planning.cem_plan(plain, imgs[:2], stas[0], **kw)
    for name in ('actions', 'cost', 'mean', 'std', 'best_cost_per_iteration'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    cand = np.random.RandomState(3).randn(4, 5, 5).astype(np.float32) * 0.3
    assert torch.equal(planning.score_actions(m, imgs[:2], stas[0], cand, (32, 32), (40, 24)),
                       planning.score_actions(plain, imgs[:2], stas[0], cand, (32, 32), (40, 24)))
    assert m.carry_state is True and torch.equal(m.recurrent_state().data, belief.data)


def test_the_belief_loop_never_synchronises_with_the_host():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm, imgs, acts, stas, m, belief, state1 = _belief_scene(torch, pivp_amd)
    kw = dict(SETUP, samples=32, elites=8, chunk=16)
    warm = planning.cem_plan(m, imgs[1:2], state1, belief=belief, **kw)        # plans, workspaces and allocator blocks exist from here on
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
            a = planning._check_cem_args(m, imgs[1:2], state1, belief=belief, **kw)
            torch.cuda.set_sync_debug_mode('default')
            b = planning._cem_upload(m, a, imgs[1:2], state1)                 # the uploads and the ONE expansion of the belief, in front of the loop
            assert b.belief.batch == 16
            torch.cuda.set_sync_debug_mode('error')
            res = planning._cem_iterate(m, a, b, trace=False)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not detects:
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made')
    assert torch.equal(res.actions, warm.actions) and torch.equal(res.best_cost_per_iteration, warm.best_cost_per_iteration)


# ---- 7. the state machine -------------------------------------------------------------------------------------------------------------------------
def test_what_a_carried_state_does_not_serve():
    torch, pivp_amd = _gpu()
    from pivp_amd import _lib
    P, nm = _random_params('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(3, 8, 64, 64, seed=31))
    w1, w2 = [imgs[:4, :2], acts[:4, :2], stas[:4, :2]], [imgs[4:, :2], acts[4:, :2], stas[4:, :2]]
    m = _model(pivp_amd, 'CDNA', nm, P, carry_state=True, keep_activations=True, deterministic=True)      # (fixed-order sums: gradients compare bit for bit)
    m(w1)
    m.cleargrads()
    m.backward()                                          # a call that started from zeros back-propagates as ever
    g1 = m._flat_grads.clone()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    m(w2)                                                 # ... one that started from a carried state does not
    with pytest.raises(RuntimeError, match='truncated BPTT'):
        m.backward()
    plan = m._active
    rc = plan.lib.pivp_rollout_backward(plan.h, m._inputs[0].data_ptr(), m._inputs[1].data_ptr(), m._inputs[2].data_ptr(), None, m._gen.data_ptr(),
                                        m._gen_states.data_ptr(), m._stream())
    assert rc == -3 and _lib._ERR[rc] == 'PIVP_ERR_STATE'
    torch.cuda.synchronize()
    assert torch.equal(m._flat_grads, g1)                 # the refused sweep launched nothing
    with pytest.raises(ValueError, match='carries the recurrent state of batch 2'):
        m([imgs[:4], acts[:4], stas[:4]])                 # another batch size while a state is carried
    m.reset_state()
    m(w1)
    m.cleargrads()
    m.backward()
    assert torch.equal(m._flat_grads, g1)                 # after reset_state(): the first call's gradients, bit for bit
