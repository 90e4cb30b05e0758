"""Models whose actions and robot states are not five wide (Model(action_dim=, state_dim=), pivp_config_t::action_dim / state_dim), against the float64
oracles, which take the widths from their parameters and inputs: forward in a training and in an inference plan, parameter gradients, input gradients,
the rollout and planning surface, checkpoints, bf16 -- and 5 / 5 given explicitly against the default, bit for bit.

Parameters: R.init_params_widened with enc3/W, current_state/W and current_state/b drawn anew at the case's widths (LeCunNormal weights, 0.1 N(0, 1) bias,
rounded to float32 and widened, like every other entry).  Inputs: synthetic_batch (smooth_batch for STP) frames, actions and states 0.1 N(0, 1).
The float32 autograd of the restatement is within 8.6e-6 relative L2 of its float64 autograd on these inputs (every parameter tensor, actions, states;
seeds 1 .. 3), so the gradient gates are free for a correct implementation."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import restatement as R
from input_grad_reference import rel_errors
from train_reference import _autograd_zero_filled, _check_grads, _oracle_pass

pytestmark = pytest.mark.gpu

HEAD_KW = {'CDNA': dict(is_cdna=True), 'STP': dict(is_cdna=False, is_stp=True), 'DNA': dict(is_cdna=False, is_dna=True)}
GATE = {'CDNA': 2e-3, 'STP': 5e-3, 'DNA': 5e-3}      # the gradient gates of tests/test_gpu_train_shapes.py
INPUT_GATE = 2e-3                                    # tests/test_gpu_input_grad.py: relative L2, and largest element relative to max |ref|
FRAME_GATE, STATE_GATE, LOSS_GATE = 1e-4, 1e-5, 1e-6      # tests/test_gpu_model.py; the loss as the gradient tests hold it
WIDTH_KEYS = ('enc3/W', 'current_state/W', 'current_state/b')

# name -> (head, masks, A, S, H, W, B, T, use_state)
CASES = OrderedDict([
    ('cdna_4_3', ('CDNA', 3, 4, 3, 16, 16, 2, 4, True)),
    ('stp_7_5', ('STP', 2, 7, 5, 16, 16, 2, 4, True)),
    ('dna_1_1', ('DNA', 1, 1, 1, 16, 16, 2, 4, True)),
    ('cdna_16_16', ('CDNA', 10, 16, 16, 16, 16, 2, 4, True)),
    ('cdna_4_3_64', ('CDNA', 3, 4, 3, 64, 64, 2, 3, True)),
    ('cdna_4_3_no_state', ('CDNA', 3, 4, 3, 16, 16, 2, 4, False)),
])
SMALL = [n for n in CASES if n != 'cdna_4_3_64']


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def _params(head, nm, A, S, H, W, use_state, seed=1):
    P = R.init_params_widened(seed=seed, scale=1.0, num_masks=nm, model_type=head, use_state=use_state, height=H, width=W)
    rs = np.random.RandomState(1000 + seed)
    draw = lambda shape, std: (std * rs.standard_normal(shape)).astype(np.float32).astype(np.float64)
    if use_state:
        P['enc3/W'] = draw((64, 64 + A + S, 1, 1), math.sqrt(1.0 / (64 + A + S)))
    P['current_state/W'] = draw((S, A + S), math.sqrt(1.0 / (A + S)))
    P['current_state/b'] = draw((S,), 0.1)
    return P


def _inputs(name, seed=1):
    head, nm, A, S, H, W, B, T, use_state = CASES[name]
    P = _params(head, nm, A, S, H, W, use_state, seed)
    imgs = (R.smooth_batch if head == 'STP' else R.synthetic_batch)(B, T, H, W)[0]
    rs = np.random.RandomState(2000 + seed)
    acts = (0.1 * rs.standard_normal((T, B, A))).astype(np.float32)
    stas = (0.1 * rs.standard_normal((T, B, S))).astype(np.float32)
    return P, (imgs, acts, stas)


def _kw(name):
    head, nm, A, S, H, W, B, T, use_state = CASES[name]
    return dict(HEAD_KW[head], use_state=use_state)


_FORWARD, _GRADS = {}, {}


def _oracle_forward(name):
    """frames, predicted states and loss of the float64 restatement, computed once per session and left unchanged"""
    if name not in _FORWARD:
        P, batch = _inputs(name)
        ref = R.Model(CASES[name][1], params=P, dtype=np.float64, prefix='t', **_kw(name))
        ref.train = False
        loss = float(ref(list(batch), 0))
        out = (np.stack(ref.gen_images), np.stack(ref.gen_states), loss)
        for a in out[:2]:
            a.setflags(write=False)
        _FORWARD[name] = out
    return _FORWARD[name]


def _oracle_grads(name):
    """float64 autograd: (loss, parameter gradients by _autograd_zero_filled, (d loss / d actions, d loss / d states) with the inputs as leaves)"""
    if name not in _GRADS:
        P, batch = _inputs(name)
        loss, grads = _autograd_zero_filled(P, *batch, num_masks=CASES[name][1], **_kw(name))
        _, loss_in, _, (da, ds) = _oracle_pass(P, batch, wrt_inputs=True, num_masks=CASES[name][1], **_kw(name))
        assert abs(loss_in - loss) < 1e-12
        for g in list(grads.values()) + [da, ds]:
            g.setflags(write=False)
        _GRADS[name] = (loss, grads, (da, ds))
    return _GRADS[name]


def _model(pivp, name, P, widths=True, **kw):
    head, nm, A, S = CASES[name][:4]
    if widths:
        kw = dict(kw, action_dim=A, state_dim=S)
    m = pivp.Model(nm, prefix='t', **dict(_kw(name), **kw))
    m.load_state_dict_reference(P)
    return m


def _frames(m):
    return torch.stack(m.gen_images).cpu().numpy(), torch.stack(m.gen_states).cpu().numpy()


def _check_forward(name, what, m, loss):
    head, nm, A, S, H, W, B, T, use_state = CASES[name]
    gen_ref, gs_ref, loss_ref = _oracle_forward(name)
    gen, gs = _frames(m)
    assert gen.shape == (T - 1, B, 3, H, W) and gs.shape == (T - 1, B, S)
    l2 = R.per_pixel_l2(gen, gen_ref).reshape(T - 1, -1).max(axis=1)
    es = np.abs(gs - gs_ref).max()
    print('%s %s: per-pixel L2 by step %s, gen_states %.3e, loss hip %.9f oracle %.9f' % (name, what, ' '.join('%.2e' % v for v in l2), es, loss, loss_ref))
    assert (l2 < FRAME_GATE).all() and es < STATE_GATE and abs(loss - loss_ref) < LOSS_GATE


@pytest.mark.parametrize('name', list(CASES))
def test_forward_in_a_training_and_an_inference_plan(pivp, name):
    P, batch = _inputs(name)
    m = _model(pivp, name, P, keep_activations=True)
    _check_forward(name, 'training plan', m, float(m(list(batch), 0)))
    out = {}
    for fuse in (1, 0):      # (widths the fused epilogue does not serve take the separate launch under either value: the bits must not know the option)
        mi = _model(pivp, name, P, keep_activations=False, plan_options={'fuse_enc3': fuse})
        with pivp.using_config('train', False):
            loss = float(mi(list(batch), 0))
        _check_forward(name, 'inference plan, fuse_enc3=%d' % fuse, mi, loss)
        out[fuse] = (loss,) + _frames(mi)
    assert out[1][0] == out[0][0] and np.array_equal(out[1][1], out[0][1]) and np.array_equal(out[1][2], out[0][2])


def _check_input_grads(name, m):
    head, nm, A, S, H, W, B, T, use_state = CASES[name]
    _, _, (a_ref, s_ref) = _oracle_grads(name)
    ag, sg = m.action_grad.cpu().numpy(), m.state_grad.cpu().numpy()
    assert ag.shape == (T - 1, B, A) and sg.shape == (B, S) and ag.dtype == np.float32 and sg.dtype == np.float32
    assert a_ref.shape == (T, B, A) and s_ref.shape == (T, B, S) and not a_ref[T - 1].any() and not s_ref[1:2].any()
    ea, es = rel_errors(ag, a_ref[:T - 1]), rel_errors(sg, s_ref[0])
    print('%s: action_grad rel L2 %.2e, largest element %.2e; state_grad rel L2 %.2e, largest element %.2e' % (name, ea[0], ea[1], es[0], es[1]))
    assert np.abs(a_ref[:T - 1]).max() > 0 and np.abs(s_ref[0]).max() > 0
    assert max(ea) < INPUT_GATE, 'action_grad: relative L2 %.3e, largest element %.3e of max |ref|' % ea
    assert max(es) < INPUT_GATE, 'state_grad: relative L2 %.3e, largest element %.3e of max |ref|' % es


def _print_width_keys(name, got, gref):
    for k in WIDTH_KEYS:
        d = got[k].astype(np.float64) - gref[k]
        print('  %s: %s %s relative L2 error %.3e' % (name, k, got[k].shape, np.linalg.norm(d) / (np.linalg.norm(gref[k]) + 1e-30)))


@pytest.mark.parametrize('name', SMALL)
def test_parameter_and_input_gradients_match_float64_autograd(pivp, name):
    P, batch = _inputs(name)
    loss_ref, gref, _ = _oracle_grads(name)
    m = _model(pivp, name, P, keep_activations=True)
    loss = float(m(list(batch), 0))
    m.cleargrads(); m.backward(input_grad=True)
    got = m.grads_reference()
    _print_width_keys(name, got, gref)
    assert abs(loss - loss_ref) < LOSS_GATE
    for k in WIDTH_KEYS:
        assert got[k].shape == gref[k].shape, k
    worst = _check_grads(got, gref, GATE[CASES[name][0]])
    print('%s: worst relative gradient error %.3e (%s)' % (name, worst[0], worst[1]))
    _check_input_grads(name, m)


def test_a_deterministic_sweep_on_64x64_frames(pivp):
    name = 'cdna_4_3_64'
    P, batch = _inputs(name)
    loss_ref, gref, _ = _oracle_grads(name)
    m = _model(pivp, name, P, keep_activations=True, deterministic=True)
    runs = []
    for _ in range(2):
        loss = float(m(list(batch), 0))
        m.cleargrads(); m.backward(input_grad=True)
        runs.append((loss, m._flat_grads.clone(), m.action_grad.clone(), m.state_grad.clone()))
    got = m.grads_reference()
    _print_width_keys(name, got, gref)
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:])), 'two deterministic steps differ'
    assert abs(runs[0][0] - loss_ref) < LOSS_GATE
    worst = _check_grads(got, gref, GATE['CDNA'])
    print('%s deterministic: worst relative gradient error %.3e (%s)' % (name, worst[0], worst[1]))
    _check_input_grads(name, m)
    # ... and the default sweep (atomics) inside the same gates
    md = _model(pivp, name, P, keep_activations=True)
    md(list(batch), 0)
    md.cleargrads(); md.backward(input_grad=True)
    _check_grads(md.grads_reference(), gref, GATE['CDNA'])
    _check_input_grads(name, md)


def test_imagine_scoring_and_refinement_at_4_3(pivp):
    from pivp_amd import planning
    name = 'cdna_4_3'
    head, nm, A, S, H, W, B, T, _ = CASES[name]
    P, (imgs, acts, stas) = _inputs(name)
    m = _model(pivp, name, P)
    with pivp.using_config('train', False):
        m([imgs, acts, stas], 0)
    gen, gs = _frames(m)
    out = m.imagine(imgs[:2], acts[:T - 1], stas[0])
    assert np.array_equal(out.cpu().numpy(), gen) and np.array_equal(_frames(m)[1], gs), 'imagine differs from the feed-self call on its context'
    rs = np.random.RandomState(5)
    cand = (0.1 * rs.standard_normal((4, T - 1, A))).astype(np.float32)
    cost = planning.score_actions(m, imgs[:2, :1], stas[0, :1], cand, (8, 8), (4, 4))
    assert tuple(cost.shape) == (4,) and bool(torch.isfinite(cost).all())
    mt = _model(pivp, name, P, keep_activations=True)
    past = acts[:1]
    refined, costs = planning.refine_actions(mt, imgs[:2], stas[0], acts[:T - 1], goal_image=np.full((3, H, W), 0.5, np.float32), steps=1,
                                             past_actions=past, bounds=(np.full(A, -1.0), 1.0))
    r = refined.cpu().numpy()
    assert r.shape == (T - 1, B, A) and tuple(costs.shape) == (2, B) and bool(torch.isfinite(costs).all())
    assert np.array_equal(r[:1], past), 'past_actions rows moved'
    assert (r[1:] != acts[1:T - 1]).any()
    assert mt.action_grad.shape == (T - 1, B, A) and mt.state_grad.shape == (B, S)


def test_checkpoints_keep_the_model_s_widths(pivp, tmp_path):
    name = 'cdna_4_3'
    head, nm, A, S = CASES[name][:4]
    P, batch = _inputs(name)
    m = _model(pivp, name, P)
    with pivp.using_config('train', False):
        loss = float(m(list(batch), 0))
    gen = _frames(m)[0]
    path = str(tmp_path / 'training-0')
    pivp.save_npz(path, m)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(P.keys())
        for k in P:
            assert z[k].shape == P[k].shape and np.array_equal(z[k], P[k].astype(np.float32)), k
        assert z['enc3/W'].shape == (64, 64 + A + S, 1, 1) and z['current_state/W'].shape == (S, A + S) and z['current_state/b'].shape == (S,)
    m2 = pivp.Model(nm, prefix='t', action_dim=A, state_dim=S)
    pivp.load_npz(path, m2)
    with pivp.using_config('train', False):
        loss2 = float(m2(list(batch), 0))
    assert loss2 == loss and np.array_equal(_frames(m2)[0], gen)
    five = R.synthetic_batch(2, 4, 16, 16)
    with pytest.raises(ValueError, match='enc3/W'):
        m3 = pivp.Model(nm, prefix='t')
        pivp.load_npz(path, m3)
        with pivp.using_config('train', False):
            m3(list(five), 0)


@pytest.mark.parametrize('head,nm', [('CDNA', 10), ('STP', 10), ('DNA', 1)])
def test_5_5_given_explicitly_is_the_default_bit_for_bit(pivp, head, nm):
    B, T = 2, 3
    P = R.init_params_widened(seed=1, scale=1.0, num_masks=nm, model_type=head)
    batch = (R.smooth_batch if head == 'STP' else R.synthetic_batch)(B, T)
    out = {}
    for widths in (False, True):
        kw = dict(action_dim=5, state_dim=5) if widths else {}
        mi = pivp.Model(nm, prefix='t', **HEAD_KW[head], **kw)
        mi.load_state_dict_reference(P)
        with pivp.using_config('train', False):
            li = float(mi(list(batch), 0))
        mt = pivp.Model(nm, prefix='t', keep_activations=True, deterministic=True, **HEAD_KW[head], **kw)
        mt.load_state_dict_reference(P)
        lt = float(mt(list(batch), 0))
        mt.cleargrads(); mt.backward(input_grad=True)
        out[widths] = (li, lt) + tuple(torch.from_numpy(a) for a in _frames(mi) + _frames(mt)) + (mt._flat_grads.clone().cpu(), mt.action_grad.cpu(), mt.state_grad.cpu())
        assert mi._active.lib.pivp_plan_workspace_bytes(mi._active.h) > 0
    assert out[True][:2] == out[False][:2]
    for a, b in zip(out[True][2:], out[False][2:]):
        assert torch.equal(a, b)


def test_a_bf16_train_step_at_4_3_tracks_fp32(pivp):
    """The comparison and the gate of tests/test_gpu_bf16.py::test_train_step_in_bf16_mode_tracks_fp32."""
    name = 'cdna_4_3_64'
    P, batch = _inputs(name)
    outs = {}
    for prec in ('fp32', 'bf16'):
        m = _model(pivp, name, P, keep_activations=True, precision=prec)
        with pivp.using_config('train', True):
            loss = float(m(list(batch), 0))
            m.cleargrads(); m.backward()
        outs[prec] = (loss, m._flat_grads.clone())
    g32, g16 = outs['fp32'][1], outs['bf16'][1]
    rel = float((g16 - g32).norm() / g32.norm())
    print('bf16-forward train step at 4 / 3: loss %.6f vs %.6f, relative gradient difference %.2e' % (outs['bf16'][0], outs['fp32'][0], rel))
    assert abs(outs['bf16'][0] - outs['fp32'][0]) < 1e-3
    assert 1e-6 < rel < 5e-2
