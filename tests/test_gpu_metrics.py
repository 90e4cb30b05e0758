"""GPU tests of pivp_frame_metrics (per-sample MSE / SSIM in one launch) against the float64 restatement of tests/metrics_reference.py, of its
structural promises (same bits run to run, an image's result independent of its neighbours, the grid and the other output), and of
`Model.evaluate` / `metrics.frame_metrics` on top of it.

Gates.  |ssim - float64| <= 1e-6 per image on every input: the kernel accumulates the five window moments and their differences in fp64 and
rounds numerator and denominator to fp32 once, so what is left is a few fp32 roundings (6e-8 each) of a value of magnitude <= 1.  The plain
float32 formulation (metrics_reference with dtype=float32) is printed beside it and never gated: it misses the gate on `const` and `bright flat`,
which is what those inputs are for.  mse: relative 1e-6 (the kernel sums exact fp64 squares; the fp32 result is one rounding, 6e-8)."""
import os
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ops as MO  # noqa: E402
import metrics_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-6
MSE_RTOL = 1e-6
BADARG = -1
INPUTS = ('noise', 'smooth+eps', 'const', 'bright flat', 'halves', 'same')


def make_input(kind, N, C, H, W, seed):
    """-> (pred, truth) float32 (N, C, H, W); `same` returns one array twice."""
    rs = np.random.RandomState(seed)
    shp = (N, C, H, W)
    if kind == 'noise':
        x, y = rs.rand(*shp), rs.rand(*shp)
    elif kind == 'smooth+eps':
        yy, xx = np.arange(H).reshape(1, 1, H, 1), np.arange(W).reshape(1, 1, 1, W)
        fy, fx = rs.uniform(0.05, 0.6, (N, C, 1, 1)), rs.uniform(0.05, 0.6, (N, C, 1, 1))
        py, px = rs.uniform(0, 2 * np.pi, (N, C, 1, 1)), rs.uniform(0, 2 * np.pi, (N, C, 1, 1))
        x = 0.5 + 0.5 * np.sin(fy * yy + py) * np.sin(fx * xx + px)
        y = np.clip(x + rs.normal(0.0, 0.02, shp), 0.0, 1.0)
    elif kind == 'const':
        x, y = np.full(shp, 0.7), np.full(shp, 0.3)
    elif kind == 'bright flat':
        x = 0.95 + 0.001 * rs.rand(*shp)
        y = x + 0.001
    elif kind == 'halves':
        x = np.full(shp, 0.05)
        x[..., W // 2:] = 0.95
        x = x + 0.001 * rs.rand(*shp)
        y = x + 0.002 * rs.rand(*shp)
    elif kind == 'same':
        x = rs.rand(*shp)
        y = x
    else:
        raise KeyError(kind)
    x = x.astype(np.float32)
    return x, (x if kind == 'same' else y.astype(np.float32))


_REF = {}


def reference(kind, N, C, H, W, win, sigma):
    """(pred, truth, float64 ssim, float64 mse, float32 ssim, float32 mse), computed once per case and shared."""
    key = (kind, N, C, H, W, win, sigma)
    if key not in _REF:
        x, y = make_input(kind, N, C, H, W, seed=len(kind) * 1000 + H * 7 + W)
        s64, m64 = MR.ssim_mse(x, y, win, sigma, 1.0, np.float64)
        s32, m32 = MR.ssim_mse(x, y, win, sigma, 1.0, np.float32)
        for a in (x, y, s64, m64, s32, m32):
            a.setflags(write=False)
        _REF[key] = (x, y, s64, m64, s32, m32)
    return _REF[key]


SIZES = [(11, 11, 9), (12, 27, 9), (37, 53, 9), (64, 64, 2), (128, 128, 2)]          # (H, W, N)
WINDOWS = [(11, 1.5), (7, 1.5), (3, 0.0)]
CASES = [(H, W, N, 3, win, sigma) for (H, W, N) in SIZES for (win, sigma) in WINDOWS] + [(37, 53, 9, 1, 11, 1.5)]


@pytest.mark.parametrize('H,W,N,C,win,sigma', CASES, ids=['%dx%d-n%d-c%d-win%d-s%g' % c for c in CASES])
def test_frame_metrics_against_float64(H, W, N, C, win, sigma):
    fails = []
    for kind in INPUTS:
        x, y, s64, m64, s32, m32 = reference(kind, N, C, H, W, win, sigma)
        mse, ssim = MO.frame_metrics(x, y, win, sigma, same=kind == 'same')
        assert mse.dtype == np.float32 and ssim.dtype == np.float32 and mse.shape == (N,) and ssim.shape == (N,)
        es = np.abs(ssim.astype(np.float64) - s64).max()
        es32 = np.abs(s32.astype(np.float64) - s64).max()
        with np.errstate(invalid='ignore', divide='ignore'):
            em = np.where(m64 > 0, np.abs(mse.astype(np.float64) - m64) / m64, np.abs(mse)).max()
            em32 = np.where(m64 > 0, np.abs(m32.astype(np.float64) - m64) / m64, np.abs(m32)).max()
        print('%-12s %3dx%-3d win %2d: ssim err %.2e (plain float32 %.2e)   mse rel err %.2e (plain float32 %.2e)' % (kind, H, W, win, es, es32, em, em32))
        if not es <= SSIM_TOL:
            fails.append('%s: ssim off by %.3e' % (kind, es))
        if not em <= MSE_RTOL:
            fails.append('%s: mse off by %.3e (relative)' % (kind, em))
        if kind == 'same':
            if not (mse == 0).all():
                fails.append('same: mse is not exactly 0: %r' % mse)
            if not np.abs(ssim.astype(np.float64) - 1.0).max() <= SSIM_TOL:
                fails.append('same: ssim is not 1: %r' % ssim)
    assert not fails, fails


def test_frame_metrics_same_bits_run_to_run():
    x, y = reference('smooth+eps', 9, 3, 37, 53, 11, 1.5)[:2]
    a, b = MO.frame_metrics(x, y), MO.frame_metrics(x, y)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('N,picks', [(300, (0, 1, 255, 256, 299)), (700, (0, 511, 512, 699))], ids=['n300', 'n700'])
def test_an_images_result_depends_on_nothing_but_the_image(N, picks):
    """More images than CUs (256) and than blocks in the grid (two per CU): the block loop wraps.  Image i inside the batch and image i alone
    (N = 1, block 0, first pass of the loop) give the same bits."""
    rs = np.random.RandomState(11)
    x = rs.rand(N, 3, 16, 24).astype(np.float32)
    y = np.clip(x + rs.normal(0, 0.05, x.shape), 0, 1).astype(np.float32)
    mse, ssim = MO.frame_metrics(x, y)
    assert len(np.unique(mse)) > N // 2 and len(np.unique(ssim)) > N // 2           # distinct images
    for i in picks:
        m1, s1 = MO.frame_metrics(x[i:i + 1], y[i:i + 1])
        assert m1.tobytes() == mse[i:i + 1].tobytes() and s1.tobytes() == ssim[i:i + 1].tobytes(), i
    s64, m64 = MR.ssim_mse(x, y)
    assert np.abs(ssim - s64).max() <= SSIM_TOL and (np.abs(mse - m64) <= MSE_RTOL * m64).all()


def test_a_null_output_leaves_the_other_unchanged():
    x, y = reference('noise', 9, 3, 12, 27, 7, 1.5)[:2]
    mse, ssim = MO.frame_metrics(x, y, 7, 1.5)
    rc, (m_only, s_untouched) = MO.frame_metrics_rc(x, y, 7, 1.5, null='ssim')
    assert rc == 0 and m_only.tobytes() == mse.tobytes() and (s_untouched == -7).all()
    rc, (m_untouched, s_only) = MO.frame_metrics_rc(x, y, 7, 1.5, null='mse')
    assert rc == 0 and s_only.tobytes() == ssim.tobytes() and (m_untouched == -7).all()


def test_bad_arguments_are_refused_and_nothing_is_written():
    x = np.random.RandomState(5).rand(2, 3, 12, 14).astype(np.float32)
    bad = [dict(N=0), dict(N=-1), dict(C=0), dict(win=4), dict(win=10), dict(win=2), dict(win=1), dict(win=13), dict(win=-3),
           dict(H=10), dict(W=10), dict(H=0), dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=float('nan')),
           dict(null=('mse', 'ssim')), dict(null='pred'), dict(null='truth')]
    for kw in bad:
        kw = dict(kw)
        args = dict(win=kw.pop('win', 11), sigma=1.5, data_range=kw.pop('data_range', 1.0))
        rc, (mse, ssim) = MO.frame_metrics_rc(x, x, null=kw.pop('null', None), **args, **kw)
        assert rc == BADARG, (kw, args, rc)
        assert (mse == -7).all() and (ssim == -7).all(), (kw, args)
    rc, (mse, ssim) = MO.frame_metrics_rc(x, x, win=11)                    # the same call with good arguments runs
    assert rc == 0 and (mse == 0).all() and np.abs(ssim - 1).max() <= SSIM_TOL


def test_module_frame_metrics_shapes_inputs_and_psnr():
    x, y, s64, m64 = reference('smooth+eps', 9, 3, 12, 27, 7, 1.5)[:4]
    xs, ys = x.reshape(3, 3, 3, 12, 27), y.reshape(3, 3, 3, 12, 27)
    got = pivp_amd.frame_metrics(xs, torch.from_numpy(ys).cuda(), win=7)                  # host array against device tensor
    assert got.mse.shape == got.psnr.shape == got.ssim.shape == (3, 3) and got.ssim.is_cuda and got.ssim.dtype == torch.float32
    assert np.abs(got.ssim.cpu().numpy().reshape(9) - s64).max() <= SSIM_TOL
    assert (np.abs(got.mse.cpu().numpy().reshape(9) - m64) <= MSE_RTOL * m64).all()
    assert np.abs(got.psnr.cpu().numpy().reshape(9) - MR.psnr(m64)).max() <= 1e-4        # 10 log10 of a value good to 1e-6: 4e-6 dB + fp32 log
    one = pivp_amd.frame_metrics(x[0], x[0], win=7)                                       # a single (C, H, W) frame against itself
    assert one.mse.shape == () and float(one.mse) == 0.0 and float(one.psnr) == float('inf') and abs(float(one.ssim) - 1) <= SSIM_TOL


def _setup(model_type):
    nm = 10
    P = R.init_params_widened(seed=1, scale=1.0) if model_type == 'CDNA' else \
        R.init_params_widened(seed=1, scale=1.0, num_masks=nm, model_type=model_type, height=64, width=64)
    x = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in R.synthetic_batch(2, 4)]
    m = pivp_amd.Model(nm, is_cdna=model_type == 'CDNA', is_stp=model_type == 'STP', prefix='ev', device='cuda:0')
    m.load_state_dict_reference(P)
    return m, x


@pytest.mark.parametrize('model_type', ['CDNA', 'STP'])
def test_model_evaluate(model_type):
    m, x = _setup(model_type)
    ctx = 2
    with pivp_amd.using_config('train', False):
        loss = m(x).clone()
    psnr_all, gen = m.psnr_all.clone(), torch.stack(m.gen_images).clone()
    m.reset_state()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')         # a host synchronisation inside evaluate() raises
    try:
        out = m.evaluate(x)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out is m.metrics
    for t in (out.mse, out.psnr, out.ssim):
        assert tuple(t.shape) == (2, 2) and t.is_cuda and t.dtype == torch.float32
    # the rollout is the plain feed-self __call__
    assert torch.equal(m.loss, loss) and torch.equal(m.psnr_all, psnr_all) and torch.equal(torch.stack(m.gen_images), gen)
    # pairing and layout: the restatement on the host, on the GPU's own frames
    g = gen.cpu().numpy()[ctx - 1:]
    truth = x[0].cpu().numpy()[ctx:]
    s64, m64 = MR.ssim_mse(g, truth)
    s32, _ = MR.ssim_mse(g, truth, dtype=np.float32)
    mse, ssim, psnr = out.mse.cpu().numpy(), out.ssim.cpu().numpy(), out.psnr.cpu().numpy()
    print('%s: ssim %s  err %.2e (plain float32 %.2e)  mse rel err %.2e' % (model_type, ssim.ravel(), np.abs(ssim - s64).max(), np.abs(s32 - s64).max(),
                                                                             (np.abs(mse - m64) / m64).max()))
    assert np.abs(ssim - s64).max() <= SSIM_TOL and (np.abs(mse - m64) <= MSE_RTOL * m64).all()
    assert np.abs(psnr - MR.psnr(m64)).max() <= 1e-4
    # wiring: the step's recon_cost is the batch mean of the same squared errors (two fp32-grade sums of the same 24,576 terms)
    recon = [float(s.split(': ')[1]) for s in m.summaries if '_recon_cost' in s]
    assert len(recon) == 2
    for t in range(2):
        assert abs(mse[t].astype(np.float64).mean() - recon[t]) <= 1e-5 * recon[t], (t, mse[t], recon[t])
    # another window through the same door
    m.reset_state()
    out3 = m.evaluate(x, win=3, sigma=0)
    assert np.abs(out3.ssim.cpu().numpy() - MR.ssim_mse(g, truth, 3, 0.0)[0]).max() <= SSIM_TOL
    assert torch.equal(out3.mse, out.mse) and torch.equal(torch.stack(m.gen_images), gen)


def test_evaluate_entry_point_walks_a_dataset(tmp_path, capsys):
    """`python -m pivp_amd.evaluate` on a five-sequence data set in the reference's on-disk format, from sequence 1, three sequences in batches of
    two: the npz holds what the same batches give through `Model.evaluate` + `StepCurves` by hand."""
    from pivp_amd import dataset as ds, evaluate as E
    from pivp_amd.predict import resize_images
    data = tmp_path / 'data'; data.mkdir()
    mdir = tmp_path / 'models' / '20240101-000000-CDNA-2'; mdir.mkdir(parents=True)
    rs = np.random.RandomState(0)
    rows = []
    for j in range(5):
        np.save(str(data / ('action_%d' % j)), (rs.randn(4, 5) * 0.1).astype(np.float32))
        np.save(str(data / ('state_%d' % j)), (rs.randn(4, 5) * 0.1).astype(np.float32))
        np.save(str(data / ('pred_%d' % j)), (rs.rand(4, 96, 120, 3) * 255).astype(np.uint8))
        rows.append([j, '', 'pred_%d.npy' % j, 'action_%d.npy' % j, 'state_%d.npy' % j, '', 'pred_%d.npy' % j])
    ds.write_map(str(data), rows)
    P = R.init_params_widened(seed=1, scale=1.0)
    m = pivp_amd.Model(10, prefix='e')
    m.load_state_dict_reference(P)
    pivp_amd.save_npz(str(mdir / 'training-0'), m)
    E.main([mdir.name, 'training-0', '1', '--models_dir', str(tmp_path / 'models'), '--data_dir', str(data), '--batch_size', '2', '--max_sequences', '3'])
    printed = capsys.readouterr().out
    assert printed.count('step ') == 2 and '3 sequences' in printed
    with np.load(str(mdir / 'metrics-training-0.npz')) as z:
        got = {k: z[k] for k in z.files}
    assert sorted(got) == sorted(['%s_%s' % (k, f) for k in ('mse', 'psnr', 'ssim') for f in ('mean', 'std', 'min', 'max')] + ['count', 'psnr_n_inf'])
    assert got['count'].tolist() == [3, 3] and got['psnr_n_inf'].tolist() == [0, 0]
    cur = pivp_amd.StepCurves()
    for idx in ((1, 2), (3,)):
        batch = []
        for i in idx:
            _, raw, _, act, sta = ds.get_data_info(str(data), i)
            batch.append([raw, act, sta])
        img, act, sta = pivp_amd.concat_examples(batch)
        frames = torch.stack([resize_images(img[t], (64, 64), 'cuda:0', 1.0 / 255.0) for t in range(4)])
        cur.add(m.evaluate([frames, act, sta]))
        m.reset_state()
    want = E.curves_to_arrays(cur.result())
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-6, atol=0), (k, got[k], want[k])
    assert (got['ssim_min'] <= got['ssim_mean']).all() and (got['ssim_mean'] <= got['ssim_max']).all() and (got['mse_std'] >= 0).all()
