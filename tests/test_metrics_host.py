"""CPU-side tests of the evaluation metrics: the float64 restatement (tests/metrics_reference.py) against analytic answers and an independent
filter, the argument checks of `metrics.frame_metrics`, `StepCurves` against NumPy, the `evaluate` argument parser and the C-ABI surface of
pivp_frame_metrics.  No GPU."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib, StepCurves, frame_metrics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as MR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 1e-4, 9e-4


def test_reference_constant_images_have_the_closed_form():
    """Two constant images a, b: every variance and the covariance vanish, S = (2ab + C1) / (a^2 + b^2 + C1).
    In float64 the computed variances are rounding residue of the moments, about 2^-53 * 0.5 each, standing over C2 = 9e-4: 1e-13 of S;
    the bound is 1e-12."""
    a, b = 0.7, 0.3
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert abs(want - 0.72419) < 1e-5
    for win, sigma in ((11, 1.5), (7, 1.5), (3, 0.0)):
        s, m = MR.ssim_mse(np.full((2, 3, 13, 17), a), np.full((2, 3, 13, 17), b), win, sigma)
        assert s.shape == (2,) and np.abs(s - want).max() < 1e-12
        assert np.abs(m - 0.16).max() < 1e-15
    # another data range scales C1 and C2 with L^2: the same image pair at 255 times the range gives the same value
    s255, _ = MR.ssim_mse(np.full((1, 1, 11, 11), 255 * a), np.full((1, 1, 11, 11), 255 * b), 11, 1.5, data_range=255.0)
    assert abs(s255[0] - want) < 1e-12


def test_reference_identical_images_give_one_and_mse_is_the_squared_offset():
    rs = np.random.RandomState(0)
    x = rs.rand(3, 3, 16, 20)
    s, m = MR.ssim_mse(x, x)
    assert np.abs(s - 1.0).max() < 1e-14 and (m == 0).all() and np.isinf(MR.psnr(m)).all()
    d = 0.125
    _, m = MR.ssim_mse(x, x + d)
    assert np.abs(m - d * d).max() < 1e-15
    assert np.abs(MR.psnr(m) - 10 * np.log10(1 / (d * d))).max() < 1e-12


def test_reference_3x3_uniform_window_by_hand():
    """x = i / 10, i = 0..8 row-major, y = x reversed; win = 3 uniform: one window position holding the whole image.
    mean 0.4 for both, E[x^2] = 204 / 900, var = 204/900 - 0.16 = 1/15, E[xy] = 84 / 900, cov = -1/15:
    S = ((0.32 + C1)(-2/15 + C2)) / ((0.32 + C1)(2/15 + C2)) = (C2 - 2/15) / (C2 + 2/15) = -0.98659..."""
    x = (np.arange(9.0) / 10).reshape(1, 1, 3, 3)
    y = x[..., ::-1, ::-1]
    s, m = MR.ssim_mse(x, y, win=3, sigma=0.0)
    want = (C2 - 2.0 / 15) / (C2 + 2.0 / 15)
    assert abs(want - (-0.98659)) < 1e-5
    assert abs(s[0] - want) < 1e-13
    assert abs(m[0] - np.mean((np.arange(9.0) / 10 - np.arange(9.0)[::-1] / 10) ** 2)) < 1e-15
    # the Gaussian window by hand at win = 3, sigma = 1: weights e^-0.5 : 1 : e^-0.5
    w = MR.window(3, 1.0)
    e = np.exp(-0.5)
    assert np.abs(w - np.array([e, 1, e]) / (1 + 2 * e)).max() < 1e-16 and abs(w.sum() - 1) < 1e-15
    assert np.abs(MR.window(11, 1.5) - MR.window(11, 1.5)[::-1]).max() == 0 and (MR.window(5, 0.0) == 0.2).all()


def test_reference_agrees_with_an_independent_filter():
    ndi = pytest.importorskip('scipy.ndimage')
    rs = np.random.RandomState(1)
    worst = 0.0
    for (H, W), win, sigma in (((37, 53), 11, 1.5), ((12, 27), 7, 1.5), ((11, 11), 11, 1.5), ((9, 14), 3, 0.0)):
        x, y = rs.rand(2, 3, H, W), rs.rand(2, 3, H, W)
        w = MR.window(win, sigma)
        p = win // 2

        def f(a):
            a = ndi.correlate1d(ndi.correlate1d(a, w, axis=-1, mode='constant'), w, axis=-2, mode='constant')
            return a[..., p:H - p, p:W - p]
        mx, my = f(x), f(y)
        sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
        got, _ = MR.ssim_mse(x, y, win, sigma)
        worst = max(worst, np.abs(got - S.mean(axis=(1, 2, 3))).max())
        assert MR.ssim_map(x, y, win, sigma).shape == (2, 3, H - win + 1, W - win + 1)
    print('restatement vs scipy.ndimage.correlate1d: %.3e' % worst)
    assert worst <= 1e-12


def test_frame_metrics_argument_errors_need_no_gpu(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_library)
    z = np.zeros((2, 3, 16, 16), np.float32)
    bad = [
        dict(truth=np.zeros((2, 3, 16, 15), np.float32)),                    # shape mismatch
        dict(truth=np.zeros((3, 16, 16), np.float32)),
        dict(pred=np.zeros((16, 16), np.float32), truth=np.zeros((16, 16), np.float32)),      # fewer than 3 dimensions
        dict(pred=np.zeros((3, 10, 16), np.float32), truth=np.zeros((3, 10, 16), np.float32)),    # H below win
        dict(pred=np.zeros((3, 16, 10), np.float32), truth=np.zeros((3, 16, 10), np.float32)),    # W below win
        dict(pred=np.zeros((0, 3, 16, 16), np.float32), truth=np.zeros((0, 3, 16, 16), np.float32)),
        dict(win=10), dict(win=1), dict(win=13), dict(win=0), dict(win=-3), dict(win=7.0), dict(win=True),
        dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=np.inf), dict(data_range=np.nan), dict(data_range='wide'),
        dict(sigma=np.nan), dict(sigma=np.inf),
    ]
    for kw in bad:
        a = dict(pred=z, truth=z)
        a.update(kw)
        with pytest.raises(ValueError):
            frame_metrics(**a)
    with pytest.raises(ValueError):                                           # tensors are read the same way
        frame_metrics(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))
    # Model.evaluate checks before it rolls out
    m = pivp_amd.Model(10, num_frame_before_prediction=2)
    x = [np.zeros((4, 1, 3, 64, 64), np.float32), np.zeros((4, 1, 5), np.float32), np.zeros((4, 1, 5), np.float32)]
    for kw in (dict(win=4), dict(win=65), dict(data_range=0)):
        with pytest.raises(ValueError):
            m.evaluate(x, **kw)
    with pytest.raises(ValueError):
        m.evaluate([np.zeros((2, 1, 3, 64, 64), np.float32), x[1][:2], x[2][:2]])          # no frame after the context
    with pytest.raises(ValueError):
        m.evaluate([np.zeros((4, 3, 64, 64), np.float32), x[1], x[2]])
    monkeypatch.undo()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):            # good arguments get as far as the GPU requirement
            frame_metrics(z, z)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            frame_metrics(z, z, win=3, sigma=0)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.evaluate(x)


def test_step_curves_match_numpy_over_uneven_batches():
    rs = np.random.RandomState(3)
    S = 4
    batches = []
    for B in (5, 1, 7):
        mse = rs.rand(S, B) * 1e-2 + 1e-4
        batches.append(dict(mse=mse, psnr=10 * np.log10(1 / mse), ssim=1 - rs.rand(S, B) * 0.3))
    batches[1]['psnr'][2, 0] = np.inf                          # a frame identical to its ground truth
    batches[2]['psnr'][2, 3] = np.inf
    batches[2]['psnr'][0, 6] = np.inf
    cur = StepCurves()
    for b in batches:
        cur.add(SimpleNamespace(**{k: torch.from_numpy(v.astype(np.float32)) for k, v in b.items()}))
    r = cur.result()
    for k in ('mse', 'psnr', 'ssim'):
        cat = np.concatenate([b[k].astype(np.float32).astype(np.float64) for b in batches], axis=1)
        for s in range(S):
            v = cat[s][np.isfinite(cat[s])]
            assert r[k]['count'][s] == len(v) and r[k]['n_inf'][s] == 13 - len(v)
            for f, fn in (('mean', np.mean), ('std', np.std), ('min', np.min), ('max', np.max)):
                assert abs(r[k][f][s] - fn(v)) <= 1e-12 * max(1.0, abs(fn(v))), (k, f, s, r[k][f][s], fn(v))
    assert r['psnr']['n_inf'].tolist() == [1, 0, 2, 0] and r['mse']['n_inf'].tolist() == [0] * 4
    assert np.isfinite(r['psnr']['mean']).all() and np.isfinite(r['psnr']['max']).all()      # the +inf did not poison anything
    # a step that never saw a finite value reports NaN, not a number
    c2 = StepCurves()
    c2.add(SimpleNamespace(mse=torch.zeros(1, 2), psnr=torch.full((1, 2), np.inf), ssim=torch.ones(1, 2)))
    r2 = c2.result()
    assert r2['psnr']['count'][0] == 0 and r2['psnr']['n_inf'][0] == 2 and np.isnan(r2['psnr']['mean'][0]) and r2['ssim']['mean'][0] == 1.0
    with pytest.raises(ValueError):
        cur.add(SimpleNamespace(mse=torch.zeros(3, 2), psnr=torch.zeros(3, 2), ssim=torch.zeros(3, 2)))      # another number of steps
    with pytest.raises(ValueError):
        cur.add(SimpleNamespace(mse=torch.zeros(4), psnr=torch.zeros(4), ssim=torch.zeros(4)))
    with pytest.raises(RuntimeError):
        StepCurves().result()


def test_evaluate_parser_accepts_predicts_arguments():
    from pivp_amd import evaluate as E
    from pivp_amd.predict import build_parser as pred_parser
    argv = ['20240101-000000-STP-32', 'training-5', '3', '--models_dir', 'm', '--data_dir', 'd', '--context_frames', '3', '--num_masks', '8',
            '--image_height', '128', '--image_width', '128', '--use_state', '0', '--gpu', '1']
    a, p = E.build_parser().parse_args(argv), pred_parser().parse_args(argv)
    for k in ('model_dir', 'model_name', 'data_index', 'models_dir', 'data_dir', 'model_type', 'schedsamp_k', 'context_frames', 'use_state',
              'num_masks', 'image_height', 'image_width', 'gpu', 'out'):
        assert getattr(a, k) == getattr(p, k), k
    assert (a.batch_size, a.max_sequences, a.win, a.sigma) == (32, 0, 11, 1.5) and E.model_type_of(a) == 'STP'
    b = E.build_parser().parse_args(['d', 'n', '--batch_size', '4', '--max_sequences', '10', '--win', '7', '--sigma', '1.0', '--model_type', 'DNA'])
    assert (b.data_index, b.batch_size, b.max_sequences, b.win, b.sigma) == (0, 4, 10, 7, 1.0) and E.model_type_of(b) == 'DNA'
    with pytest.raises(ValueError):
        E.model_type_of(b.__class__(model_dir='nodashes', model_type=''))
    # what goes into the npz
    r = {k: dict(mean=np.ones(2), std=np.zeros(2), min=np.ones(2), max=np.ones(2), count=np.array([3, 3]), n_inf=np.array([0, 1]))
         for k in ('mse', 'psnr', 'ssim')}
    arr = E.curves_to_arrays(r)
    assert sorted(arr) == sorted(['%s_%s' % (k, f) for k in ('mse', 'psnr', 'ssim') for f in ('mean', 'std', 'min', 'max')] + ['count', 'psnr_n_inf'])


def test_header_library_and_ctypes_table_agree_on_frame_metrics():
    import subprocess
    import __graft_entry__ as g
    g.build()
    header = open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', header)) - {'pivp_config', 'pivp_plan'}
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert 'pivp_frame_metrics' in declared and 'pivp_frame_metrics' in exported and 'pivp_frame_metrics' in _lib.SIGNATURES
    assert declared == set(_lib.SIGNATURES) and declared <= exported and len(declared) == 118
    assert _lib.load().pivp_abi_version() == 17                       # added without a version change: nothing else moved
    res, args = _lib.SIGNATURES['pivp_frame_metrics']
    assert res is _lib._i and args == [_lib._vp, _lib._vp] + [_lib._i] * 5 + [_lib._f] * 2 + [_lib._vp] * 3
    from pivp_amd import build
    assert 'metrics.hip' in build.SOURCES
    assert pivp_amd.metrics.frame_metrics is frame_metrics and pivp_amd.metrics.StepCurves is StepCurves and hasattr(pivp_amd.Model, 'evaluate')
