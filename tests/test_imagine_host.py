"""CPU-side tests of open-loop prediction with designated-pixel tracking: the C-ABI surface, `Model.imagine`'s argument checks, the planning
helpers, known answers of the float64 tracking rule (tests/track_reference.py) and the conditions the GPU gates of tests/test_gpu_imagine.py
rely on, checked on the oracle alone."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib, planning
from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pivp_pixel_track', 'pivp_rollout_predict')


def test_header_library_and_ctypes_table_agree_on_the_new_symbols():
    import __graft_entry__ as g
    g.build()
    header = open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', header)) - {'pivp_config', 'pivp_plan'}
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert declared == set(_lib.SIGNATURES) and declared <= exported
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17                       # added without a version change: nothing else moved
    assert len(_lib.SIGNATURES['pivp_pixel_track'][1]) == 12 and len(_lib.SIGNATURES['pivp_rollout_predict'][1]) == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pivp_rollout_predict')


def _args(ctx=2, B=2, steps=5, H=64, W=64):
    return (np.zeros((ctx, B, 3, H, W), np.float32), np.zeros((steps, B, 5), np.float32), np.zeros((B, 5), np.float32))


def test_imagine_argument_errors_need_no_gpu():
    m = pivp_amd.Model(10, num_frame_before_prediction=2)
    ci, ac, st = _args()
    planes = np.zeros((2, 3, 64, 64), np.float32)
    bad = [
        dict(context_images=ci[:1]),                                           # ctx mismatch
        dict(context_images=np.zeros((3, 2, 3, 64, 64), np.float32)),
        dict(context_images=ci[:, :, :2]),                                     # not RGB
        dict(context_images=ci[0]),                                            # not time-major
        dict(actions=ac[:1]),                                                  # T - 1 < ctx
        dict(actions=ac[:, :1]),                                               # batch mismatch
        dict(actions=ac[:, :, :4]),
        dict(state=np.zeros((5, 2, 5), np.float32)),                           # states of every frame instead of frame 0's
        dict(state=st[:1]),
        dict(designated=np.zeros((2, 9, 64, 64), np.float32)),                 # P > 8
        dict(designated=np.zeros((2, 0, 64, 64), np.float32)),
        dict(designated=np.zeros((1, 3, 64, 64), np.float32)),
        dict(designated=np.zeros((2, 3, 32, 64), np.float32)),
        dict(designated=planes[0]),
        dict(designated=planes, designated_frame=2),                           # f out of range
        dict(designated=planes, designated_frame=-1),
        dict(designated=planes, designated_frame=0.5),
        dict(designated_frame=1),                                              # a frame without planes
    ]
    for kw in bad:
        a = dict(context_images=ci, actions=ac, state=st)
        a.update(kw)
        with pytest.raises(ValueError):
            m.imagine(**a)
    # tensors and lists are read the same way
    with pytest.raises(ValueError):
        m.imagine(torch.zeros(3, 2, 3, 64, 64), torch.zeros(5, 2, 5), torch.zeros(2, 5))
    with pytest.raises(ValueError):
        m.imagine([torch.zeros(2, 3, 64, 64)] * 3, ac, st)
    if not torch.cuda.is_available():
        # good arguments get as far as the GPU requirement: there is no CPU fallback
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.imagine(ci, ac, st, designated=planes, designated_frame=0)
    assert m.pixel_distrib is None and m.pixel_mass is None and m.summaries == []
    with pytest.raises(RuntimeError, match='call the model first'):
        m.backward()


def test_planning_helpers_by_hand():
    coords = np.array([[[3, 5], [0, 0]], [[7, 15], [4, 4]]])
    p = planning.one_hot_planes(coords, 8, 16)
    assert p.shape == (2, 2, 8, 16) and p.dtype == torch.float32
    assert float(p.sum()) == 4.0 and p[0, 0, 3, 5] == 1 and p[1, 0, 7, 15] == 1 and p[0, 1, 0, 0] == 1
    assert torch.equal(planning.expected_position(p), torch.tensor(coords, dtype=torch.float32))     # one-hot -> its own coordinates
    # two-point distribution: 1/4 at (0, 0), 3/4 at (3, 4); goal (0, 0): distances 0 and 5 -> 3.75; position (2.25, 3)
    d = np.zeros((6, 6))
    d[0, 0], d[3, 4] = 0.25, 0.75
    assert float(planning.expected_distance(d, (0, 0))) == 3.75
    assert planning.expected_position(d).tolist() == [2.25, 3.0]
    assert abs(float(planning.expected_distance(d, (3, 0))) - (0.25 * 3 + 0.75 * 4)) < 1e-15
    # goals broadcast against the leading dimensions
    both = planning.expected_distance(np.stack([d, d]), np.array([[0, 0], [3, 0]]))
    assert both.tolist() == [3.75, 3.75]
    for bad in ([[[8, 0]]], [[[0, 16]]], [[[-1, 0]]], [[0, 0]], [[[0.5, 0]]]):
        with pytest.raises(ValueError):
            planning.one_hot_planes(bad, 8, 16)
    with pytest.raises(ValueError):
        planning.score_actions(None, np.zeros((2, 2, 3, 8, 8)), np.zeros((1, 5)), np.zeros((4, 3, 5)), (1, 1), (2, 2))   # context at batch 2


def test_predict_cli_flag_parses_and_defaults_to_off():
    from pivp_amd import predict as Pm
    args = Pm.build_parser().parse_args(['d', 'm', '3'])
    assert args.designated_pixel == ''                       # off: the CLI is what it was
    args = Pm.build_parser().parse_args(['d', 'm', '3', '--designated_pixel', '12,50'])
    assert Pm.parse_designated_pixel(args.designated_pixel, 64, 64) == (12, 50)
    for bad in ('12', '12,50,1', 'a,b', '64,0', '0,64', '-1,3', '1.5,2'):
        with pytest.raises(ValueError):
            Pm.parse_designated_pixel(bad, 64, 64)


def _masks(rs, B, NM, H, W):
    m = rs.rand(B, NM + 1, H, W) + 0.1
    return m / m.sum(axis=1, keepdims=True)


def test_advect_step_known_answers():
    rs = np.random.RandomState(5)
    B, NM, H, W = 2, 4, 12, 16
    D = rs.rand(B, 3, H, W)
    masks = _masks(rs, B, NM, H, W)
    masks[:, 1] += masks[:, 0]
    masks[:, 0] = 0.0                                          # m_0 = 0
    delta = np.zeros((B, NM, 5, 5)); delta[:, :, 2, 2] = 1.0
    # identity transforms: D times the sum of the masks that pair with a transform (CDNA: m_2 .. m_NM, the last KERNEL is dropped)
    want = D * masks[:, 2:].sum(axis=1, keepdims=True)
    assert np.allclose(TR.advect_step(D, masks, 'CDNA', delta), want, atol=1e-15)
    theta = np.tile(np.array([[1.0, 0, 0, 0, 1.0, 0]]), (B, 1))
    for border in ('clamp', 'zeros'):
        assert np.allclose(TR.advect_step(D, masks, 'STP', theta, border), want, atol=1e-13)
    # ... and the dropped kernel really has no say
    odd = delta.copy(); odd[:, NM - 1] = rs.rand(B, 5, 5)
    assert np.array_equal(TR.advect_step(D, masks, 'CDNA', odd), TR.advect_step(D, masks, 'CDNA', delta))
    # a one-pixel shift, in the orientation test_oracle_kat pins for the frame: a delta at (i, j) gives out[y, x] = prev[y + i - 2, x + j - 2]
    hot = np.zeros((B, 1, H, W)); hot[:, 0, 5, 7] = 1.0
    only = np.zeros((B, NM + 1, H, W)); only[:, 2] = 1.0       # all mass on the first transform
    k = np.zeros((B, NM, 5, 5)); k[:, 0, 2, 3] = 1.0          # out[y, x] = prev[y, x + 1]: the pixel moves one column to the left
    out = TR.advect_step(hot, only, 'CDNA', k)
    assert out[0, 0, 5, 6] == 1.0 and out.sum() == B
    k = np.zeros((B, NM, 5, 5)); k[:, 0, 1, 2] = 1.0          # out[y, x] = prev[y - 1, x]: one row down
    out = TR.advect_step(hot, only, 'CDNA', k)
    assert out[1, 0, 6, 7] == 1.0 and out.sum() == B
    # DNA: the same tap as a per-pixel kernel (enc7 plane index = i * 5 + j)
    e7 = np.zeros((B, 25, H, W)); e7[:, 2 * 5 + 3] = 1.0
    m2 = np.zeros((B, 2, H, W)); m2[:, 1] = 1.0
    out = TR.advect_step(hot, m2, 'DNA', e7)
    assert abs(out[0, 0, 5, 6] - 1.0) < 1e-10 and abs(out.sum() - B) < 1e-10
    # all mass on m_1, the synthesised layer: painted pixels carry nothing
    synth = np.zeros((B, NM + 1, H, W)); synth[:, 1] = 1.0
    assert not TR.advect_step(D, synth, 'CDNA', rs.rand(B, NM, 5, 5)).any()
    assert not TR.advect_step(D, synth, 'STP', theta).any()
    # linear: advecting a sum is the sum of the advected planes
    k = rs.rand(B, NM, 5, 5); masks = _masks(rs, B, NM, H, W)
    a, b = TR.advect_step(D[:, :1], masks, 'CDNA', k), TR.advect_step(D[:, 1:2], masks, 'CDNA', k)
    assert np.allclose(TR.advect_step(D[:, :1] + D[:, 1:2], masks, 'CDNA', k), a + b, atol=1e-14)


@pytest.mark.parametrize('model_type', ['CDNA', 'STP', 'DNA'])
def test_advect_step_is_the_oracle_step_without_the_synthesised_layer(model_type):
    """On a full oracle step with D := the RGB frame, advect_step plus m_1 * sigmoid(enc7) is the oracle's own `output`: the rule is `_step`'s."""
    nm = 1 if model_type == 'DNA' else 10
    P = R.init_params_widened(seed=2, scale=1.0, num_masks=nm, model_type=model_type)
    batch = R.moving_batch(2, 4, 64, 64, seed=9)
    m = TR.run_oracle(P, model_type, nm, batch, np.float64)
    for t in (0, 2):                                            # a ground-truth-fed and a fed-back step
        taps = m.taps[t]
        prev = np.asarray(batch[0][t], dtype=np.float64) if t < 2 else m.gen_images[t - 1]
        out = TR.advect_step(prev, taps['masks'], model_type, TR.head_aux(m, taps))
        if model_type != 'DNA':
            out = out + taps['masks'][:, 1:2] * R.sigmoid(taps['enc7'])
        assert np.abs(out - taps['output']).max() < 1e-12
        # the form the rollout check uses (the oracle's own heads, three planes at a time) is the same map; five planes exercise the chunking
        D = np.random.RandomState(t).rand(2, 5, 64, 64)
        assert np.abs(TR.advect_with_oracle_heads(m, taps, D) - TR.advect_step(D, taps['masks'], model_type, TR.head_aux(m, taps))).max() < 1e-12


@pytest.mark.parametrize('model_type,T,planes,keeps_signal', TR.ROLLOUT_CASES, ids=['%s-T%d' % (c[0], c[1]) for c in TR.ROLLOUT_CASES])
def test_gpu_gate_conditions_hold_on_the_oracle(model_type, T, planes, keeps_signal):
    """What tests/test_gpu_imagine.py's rollout gate relies on, on the reference alone: on the trained weights the float32 oracle stays within 1e-6
    of float64 on every step, and every gated plane keeps a maximum of at least 1e-3, so that the absolute bound of 1e-5 means something.

    The second condition cannot hold for the trained STP model over the five steps of the six-frame batch: it explains most of every pixel by
    the synthesised layer, and a plane's maximum shrinks 6-10x per step (smallest at step 5: 2.8e-6; at step 4 of f = 1: 1.7e-5).  That case stays --
    the GPU gate on it is absolute and is applied unchanged -- and is marked here as the one that does not keep its signal; the four-frame STP case
    (TR.stp_short_planes) is the one that satisfies both conditions, asserted below."""
    P, nm = TR.load_trained(model_type)
    batch = R.moving_batch(2, T, 64, 64, seed=123)
    D0 = planes(2)
    assert D0.min() >= 0 and D0.max() <= 1
    m64 = TR.run_oracle(P, model_type, nm, batch, np.float64)
    m32 = TR.run_oracle(P, model_type, nm, batch, np.float32)
    for f in (0, 1):
        d64, d32 = TR.advect_rollout(m64, D0, f), TR.advect_rollout(m32, D0, f)
        assert d64.shape == (T - 1 - f, 2, 3, 64, 64) and d32.dtype == np.float32
        pmax = d64.max(axis=(3, 4))
        err = np.abs(d32.astype(np.float64) - d64).max(axis=(1, 2, 3, 4))
        print(model_type, 'T=%d f=%d' % (T, f), 'smallest plane maximum per step', ['%.1e' % v for v in pmax.min(axis=(1, 2))],
              'float32-oracle error per step', ['%.1e' % v for v in err], 'mean mass', ['%.2g' % v for v in d64.sum(axis=(3, 4)).mean(axis=(1, 2))])
        assert err.max() < 1e-6
        assert (d64 >= 0).all()
        if keeps_signal:
            assert pmax.min() >= 1e-3
        else:
            assert pmax[0].min() >= 1e-3 and pmax.min() < 1e-3      # the record of why the four-frame case exists: drop it if this ever changes
