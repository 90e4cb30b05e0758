"""Whole-model gradients against float64 autograd on the frames the other model-level tests do not reach: heights and widths that differ, that are no
powers of two, the smallest frame, every head, mask counts from 1 to 10 -- and the contract of the accepted domain: a configuration trains, or it is
refused before anything is enqueued.

What each fp32 case puts under the sweep (maps of the cells lstm1..7 at frame H x W: H/2 x W/2 (1, 2, 7), H/4 x W/4 (3, 4, 6), H/8 x W/8 (5)):
  72 x 40   36x20, 18x10, 9x5: every ConvLSTM weight gradient through igemm_wgrad_kernel's per-lane addressing, the enc layers through its partial planes
  24 x 32   12x16, 6x8, 3x4: wgrad5x5_kernel<16> on 12 rows, and 6x8 at B = 2 -- where 4-row chunks would run over the end of a sample
  72 x 64   36x32 (wgrad5x5_kernel<32>), 18x16 (<16>), and lstm5 on 9x8 at B = 4
  24 x 40, 16 x 16, 96 x 48, 40 x 24, 48 x 80, 32 x 96: odd batches, M below one chunk (2x2 maps), the nine-tap wgrad3x3s2 instances on non-square maps
The norms' ln_bwd_* kernels and lstm_gates_bwd run at all of them with n = C*H*W no multiple of their slice."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from train_reference import _autograd_zero_filled, _check_grads

pytestmark = pytest.mark.gpu

HEAD_KW = {'CDNA': dict(is_cdna=True), 'STP': dict(is_cdna=False, is_stp=True), 'DNA': dict(is_cdna=False, is_dna=True)}
GATE = {'CDNA': 2e-3, 'STP': 5e-3, 'DNA': 5e-3}      # the gradient gates of tests/test_gpu_train.py


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def _inputs(head, H, W, nm, B, T, seed=1):
    P = R.init_params_widened(seed=seed, scale=1.0, num_masks=nm, model_type=head, height=H, width=W)
    batch = (R.smooth_batch if head == 'STP' else R.synthetic_batch)(B, T, H, W)
    return P, batch


_ORACLE = {}


def _oracle(head, H, W, nm, B, T, seed=1):
    """float64 autograd of the case, computed once per session and left unchanged"""
    key = (head, H, W, nm, B, T, seed)
    if key not in _ORACLE:
        P, (imgs, acts, stas) = _inputs(*key)
        loss, grads = _autograd_zero_filled(P, imgs, acts, stas, num_masks=nm, **HEAD_KW[head])
        for g in grads.values():
            g.setflags(write=False)
        _ORACLE[key] = (loss, grads)
    return _ORACLE[key]


def _model(pivp, head, nm, P, **kw):
    m = pivp.Model(nm, prefix='t', keep_activations=True, **HEAD_KW[head], **kw)
    m.load_state_dict_reference(P)
    return m


# The parameters' seed is 1 but for 24 x 32.  There seeds 1 and 2 put a ReLU unit within fp32 rounding of zero: the oracle ITSELF, run in float32 against its
# float64 run, then differs by 3.5e-4 / 6.4e-4 relative L2 in the median tensor (8.3e-4 / 1.3e-3 in the worst) -- the footprint _check_grads' docstring
# describes, on a frame so small that one unit's share is a thousandth of every sum; the HIP path, with other roundings, measured 1e-3 .. 2.5e-3 at seed 1
# against the 2e-3 gate.  At seed 3 the float32 oracle is within 2.5e-6 in every tensor, so the gate is free for a correct implementation.
@pytest.mark.parametrize('H,W,head,nm,B,T,seed', [(72, 40, 'CDNA', 10, 2, 4, 1), (24, 32, 'CDNA', 10, 2, 4, 3), (72, 64, 'CDNA', 3, 4, 3, 1),
                                                  (24, 40, 'CDNA', 7, 3, 4, 1), (16, 16, 'CDNA', 10, 2, 4, 1), (96, 48, 'CDNA', 1, 2, 3, 1),
                                                  (40, 24, 'STP', 10, 2, 4, 1), (48, 80, 'STP', 2, 3, 3, 1), (32, 96, 'DNA', 1, 2, 4, 1)])
def test_bptt_gradients_off_the_square_grid(pivp, H, W, head, nm, B, T, seed):
    P, (imgs, acts, stas) = _inputs(head, H, W, nm, B, T, seed)
    loss_ref, gref = _oracle(head, H, W, nm, B, T, seed)
    m = _model(pivp, head, nm, P)
    loss = float(m([imgs, acts, stas], 0))
    m.cleargrads(); m.backward()
    got = m.grads_reference()
    print('%s %dx%d nm %d B %d T %d: loss hip %.9f oracle %.9f' % (head, H, W, nm, B, T, loss, loss_ref))
    for k in ('lstm3/conv/W', 'lstm5/conv/W', 'lstm5/conv/b', 'lstm6/conv/W'):
        d = got[k].astype(np.float64) - gref[k]
        print('  %s: relative L2 error %.3e' % (k, np.linalg.norm(d) / (np.linalg.norm(gref[k]) + 1e-30)))
    assert abs(loss - loss_ref) < 1e-6
    worst = _check_grads(got, gref, GATE[head])
    print('%s %dx%d nm %d B %d T %d: worst relative gradient error %.3e (%s)' % (head, H, W, nm, B, T, worst[0], worst[1]))


def _train_step(pivp, precision, H, W, B, T):
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=10, model_type='CDNA', height=H, width=W)
    imgs, acts, stas = R.synthetic_batch(B, T, H, W)
    m = pivp.Model(10, prefix='t', keep_activations=True, precision=precision)
    m.load_state_dict_reference(P)
    with pivp.using_config('train', True):
        loss = float(m([imgs, acts, stas], 0))
        m.backward()
    return m, loss, m._flat_grads.clone()


_FP32_STEP = {}


@pytest.mark.parametrize('H,W', [(72, 64), (72, 40), (80, 64)])
@pytest.mark.parametrize('precision', ['fp16x3', 'bf16x6'])
def test_split_modes_train_on_frames_they_serve_in_part(pivp, precision, H, W):
    """The packed-operand tiles are 8 rows deep.  72 x 64 and 72 x 40 at B = 2: the cells' maps are 36, 18 and 9 rows high (widths a multiple of 8 with an even
    batch at 72 x 64, not even that at 72 x 40), so the forward runs every cell on the fp32 kernel and only the transposed convs in the mode's form; 80 x 64:
    lstm1/2/7 (40 x 32) run in the mode's form, lstm3/4/6 (20 x 16) and lstm5 (10 x 8) fall back.  The sweep must choose as the forward did, cell by cell, for
    the data gradient and for the weight gradient.  The comparison of test_gpu_bf16.py::test_train_step_in_fp16x3_mode_matches_the_fp32_gradients against the
    fp32 plan."""
    from test_gpu_bf16 import _relu_mismatches
    B, T = 2, 3
    if (H, W) not in _FP32_STEP:
        _FP32_STEP[(H, W)] = _train_step(pivp, 'fp32', H, W, B, T)
    m32, loss32, g32 = _FP32_STEP[(H, W)]
    m, loss, g = _train_step(pivp, precision, H, W, B, T)
    rel = float((g - g32).norm() / g32.norm())
    flips = _relu_mismatches(m32, m, T - 1)
    print('%s train step at %dx%d: loss %.8f vs %.8f, relative gradient difference %.2e, ReLU units on different sides of zero: %d' % (precision, H, W, loss, loss32, rel, flips))
    assert abs(loss - loss32) < 1e-6 and rel < (1e-4 if flips == 0 else 2e-3)


def test_bf16_precision_is_refused_on_a_72x40_frame(pivp):
    """the bf16 mode has no per-layer fall-back: a frame whose maps its tiles do not serve is refused at pivp_plan_set_precision, in front of the workspace"""
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=10, model_type='CDNA', height=72, width=40)
    imgs, acts, stas = R.synthetic_batch(2, 3, 72, 40)
    m = pivp.Model(10, prefix='t', keep_activations=True, precision='bf16')
    m.load_state_dict_reference(P)
    with pytest.raises(RuntimeError, match='pivp_plan_set_precision'):
        m([imgs, acts, stas], 0)


# ---- the accepted domain ------------------------------------------------------------------------------------------------------------------------------------
# What include/pivp_hip.h documents (pivp_plan_create, pivp_rollout_backward): where each configuration of the grid must end
def _documented(head, nm, H, W):
    if W + 4 > 256 or (head == 'CDNA' and 25 * nm > 256):
        return 'create'
    if (head == 'CDNA' and nm > 10) or (head == 'STP' and not 2 <= nm <= 10):
        return 'backward'
    return 'served'


DOMAIN = [(head, nm, H, W) for head in ('CDNA', 'STP', 'DNA') for nm in (1, 2, 10, 11) for (H, W) in ((16, 16), (24, 40), (16, 256), (16, 264))
          if head != 'DNA' or nm == 1]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('head,nm,H,W', DOMAIN)
def test_every_accepted_plan_trains_or_is_refused_at_the_door(pivp, head, nm, H, W):
    B, T = (1 if W >= 256 else 2), 3
    want = _documented(head, nm, H, W)
    P, (imgs, acts, stas) = _inputs(head, H, W, nm, B, T)
    m = _model(pivp, head, nm, P)
    if want == 'create':
        with pytest.raises(RuntimeError, match=r'pivp_plan_create failed: PIVP_ERR_BADARG'):
            m([imgs, acts, stas], 0)
        assert m._active is None or m._results is None      # nothing ran
    else:
        loss_ref, gref = _oracle(head, H, W, nm, B, T)
        loss = float(m([imgs, acts, stas], 0))
        print('%s nm %d %dx%d: loss hip %.9f oracle %.9f' % (head, nm, H, W, loss, loss_ref))
        assert abs(loss - loss_ref) < 1e-5
        m.cleargrads()
        if want == 'served':
            m.backward()
            worst = _check_grads(m.grads_reference(), gref, GATE[head])
            print('%s nm %d %dx%d: worst relative gradient error %.3e (%s)' % (head, nm, H, W, worst[0], worst[1]))
            return
        # a limit of the backward kernels alone: refused at the entry of pivp_rollout_backward -- neither the gradients nor a byte of the workspace (where the
        # sweep's first launches would have left the loss's seed) may have changed
        flat = m._ensure_grads()
        flat.copy_(torch.arange(flat.numel(), dtype=torch.float32, device=flat.device) * 1e-3)
        torch.cuda.synchronize()
        grads0, ws0 = _bits(flat).clone(), _bits(m._active.workspace).clone()
        with pytest.raises(RuntimeError, match=r'pivp_rollout_backward failed: PIVP_ERR_BADARG'):
            m.backward()
        torch.cuda.synchronize()
        assert torch.equal(_bits(flat), grads0)
        assert torch.equal(_bits(m._active.workspace), ws0)
    # ... and the process goes on: a served model's sweep still works
    Ps, (si, sa, ss) = _inputs('CDNA', 16, 16, 10, 2, 3)
    loss_ref, gref = _oracle('CDNA', 16, 16, 10, 2, 3)
    ms = _model(pivp, 'CDNA', 10, Ps)
    loss = float(ms([si, sa, ss], 0))
    ms.cleargrads(); ms.backward()
    assert abs(loss - loss_ref) < 1e-5
    _check_grads(ms.grads_reference(), gref, GATE['CDNA'])
