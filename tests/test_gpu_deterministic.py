"""Model(deterministic=True): a training step gives the same bits every time (include/pivp_hip.h, pivp_plan_set_deterministic) -- across
sweeps of one Model, fresh Models, the side-stream schedule, processes and Adam steps -- and its gradients are as accurate as the default
mode's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle.torch_restatement import TorchModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def _sweep(m, x):
    """one forward + backward from cleared gradients: (flat gradient, loss, generated frames), all copied"""
    m.reset_state()
    loss = m(x, 0)
    m.cleargrads(); m.backward()
    torch.cuda.synchronize()
    return m._flat_grads.clone(), loss.detach().clone(), torch.stack(m.gen_images).clone()


def _fresh(pivp, P, x, n, kw):
    kw = dict(kw)
    m = pivp.Model(kw.pop('num_masks', 10), prefix='d', keep_activations=True, deterministic=True, **kw)
    m.load_state_dict_reference(P)
    return [_sweep(m, x) for _ in range(n)], m


def _determinism(pivp, P, x, n_one=5, n_fresh=2, **kw):
    """n_one sweeps in one Model, n_fresh in a fresh one, one more each with the side stream off and on: all bit-identical"""
    runs, m = _fresh(pivp, P, x, n_one, kw)
    assert m.deterministic is True
    runs += _fresh(pivp, P, x, n_fresh, kw)[0]
    for side in (0, 1):
        r, ms = _fresh(pivp, P, x, 1, dict(kw, plan_options={'side_stream': side}))
        assert ms.effective_plan_options()['side_stream'] == side
        runs += r
    g0, l0, i0 = runs[0]
    for j, (g, l, i) in enumerate(runs[1:], 1):
        assert torch.equal(g, g0), 'run %d: flat gradient differs in %d elements' % (j, int((g != g0).sum()))
        assert torch.equal(l, l0), 'run %d: loss differs' % j
        assert torch.equal(i, i0), 'run %d: gen_images differ' % j
    return runs[0], m


def _default_grads(pivp, P, x, **kw):
    m = pivp.Model(kw.pop('num_masks', 10), prefix='d', keep_activations=True, **kw)
    m.load_state_dict_reference(P)
    return _sweep(m, x)[0]


def _agree(g_det, g_def, tol):
    """the soak scripts' measure (scripts/soak_side_stream.py): relative L2 difference of the flat gradients"""
    rel = float((g_det.double() - g_def.double()).norm() / g_def.double().norm())
    assert rel < tol, 'deterministic vs default flat gradient: relative L2 difference %.3e' % rel
    return rel


# ---- the float64 autograd gates of tests/test_gpu_train.py (copied: that file stays as it is) ----
MAX_OVER_TOL_NORM = 4 * 128
MAX_OVER_TOL = 16


def _check_grads(got, ref, tol, relu_flips=2):
    worst = []
    for kname, g in ref.items():
        scale = np.abs(g).max() + 1e-12
        d = got[kname].astype(np.float64) - g
        e = np.sort(np.abs(d).ravel() / scale)
        if g.size >= 32768 and '/norm/' in kname:
            e = e[:-relu_flips]
        p99 = e[int(0.99 * (e.size - 1))]
        rel_l2 = np.linalg.norm(d) / (np.linalg.norm(g) + 1e-30)
        worst.append((max(p99, rel_l2), kname))
        assert p99 < tol, '%s: 99th-percentile relative gradient error %.3e (scale %.3e)' % (kname, p99, scale)
        assert rel_l2 < tol, '%s: relative L2 gradient error %.3e' % (kname, rel_l2)
        assert e[-1] < 10 * tol, '%s: largest relative gradient error %.3e (scale %.3e)' % (kname, e[-1], scale)
        n_over = int((e > tol).sum())
        allowed = MAX_OVER_TOL_NORM if '/norm/' in kname else MAX_OVER_TOL
        assert n_over <= allowed, '%s: %d elements above tol %.1e (allowed %d)' % (kname, n_over, tol, allowed)
    return max(worst)


def _config2():
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(32, 10)
    return P, [imgs, acts, stas]


def test_config2_fp32_is_bit_identical_and_matches_golden(pivp):
    P, x = _config2()
    (g, loss, _), m = _determinism(pivp, P, x)
    # the gates of test_config2_batch32_gradients_match_golden against the float64 autograd fixture
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'cdna_b32_t10_grads.npz'))
    assert abs(float(loss) - float(gold['loss'])) < 1e-5
    got = m.grads_reference()
    ns = int(gold['samples'])
    assert len(got) == 54
    for k, v in got.items():
        key = k.replace('/', '.')
        f = v.ravel().astype(np.float64)
        ref = gold['val:' + key]
        val = f[::max(1, f.size // ns)][:ns]
        rel = np.linalg.norm(val - ref) / (np.linalg.norm(ref) + 1e-30)
        nrm = abs(np.linalg.norm(f) - float(gold['norm:' + key])) / (float(gold['norm:' + key]) + 1e-30)
        assert rel < 5e-4, '%s: relative L2 error of the sampled entries %.3e' % (k, rel)
        assert nrm < 2e-4, '%s: gradient norm off by %.3e' % (k, nrm)
        assert abs(f.sum() - float(gold['sum:' + key])) < 2e-3 * float(gold['norm:' + key]) * np.sqrt(f.size) + 1e-9, k
    print('config 2 fp32: deterministic vs default %.2e' % _agree(g, _default_grads(pivp, P, x), 1e-5))


def test_config3_bf16_is_bit_identical(pivp):
    P, x = _config2()
    (g, _, _), _m = _determinism(pivp, P, x, precision='bf16')
    print('config 3 bf16: deterministic vs default %.2e' % _agree(g, _default_grads(pivp, P, x, precision='bf16'), 1e-3))


@pytest.mark.parametrize('case', ['stp_b2_t4', 'stp_b32_t10', 'dna_b2_t4', 'cdna_b3_t4', 'cdna_128_b2_t3'])
def test_other_models_and_shapes_are_bit_identical(pivp, case):
    if case.startswith('stp'):      # feed-self: d prev of the fed-back frames goes through the bilinear sampler's scatter
        kw = dict(is_cdna=False, is_stp=True)
        P = R.init_params_widened(seed=1, scale=1.0, model_type='STP')
        x = list(R.synthetic_batch(2, 4) if case == 'stp_b2_t4' else R.synthetic_batch(32, 10))
    elif case == 'dna_b2_t4':
        kw = dict(num_masks=1, is_cdna=False, is_dna=True)
        P = R.init_params_widened(seed=1, scale=1.0, model_type='DNA', num_masks=1)
        x = list(R.synthetic_batch(2, 4))
    elif case == 'cdna_b3_t4':
        kw = {}
        P = R.init_params_widened(seed=1, scale=1.0)
        x = list(R.synthetic_batch(3, 4))
    else:
        kw = {}
        P = R.init_params_widened(seed=1, scale=1.0, height=128, width=128)
        x = list(R.synthetic_batch(2, 3, 128, 128))
    _determinism(pivp, P, x, n_one=3, n_fresh=1, **kw)


def test_gradients_match_float64_autograd(pivp):
    P = R.init_params_widened(seed=1, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(2, 5)
    tm = TorchModel(10, params=P, requires_grad=True)
    loss_t = tm([imgs, acts, stas], 0)
    loss_t.backward()
    loss_ref = float(loss_t.detach())
    gref = {k: v.grad.numpy() for k, v in tm.p.items()}
    m = pivp.Model(10, prefix='d', keep_activations=True, deterministic=True)
    m.load_state_dict_reference(P)
    loss = float(m([imgs, acts, stas], 0))
    m.cleargrads(); m.backward()
    assert abs(loss - loss_ref) < 1e-6
    print('worst relative gradient error', _check_grads(m.grads_reference(), gref, 2e-3))


def test_adam_steps_are_bit_identical(pivp):
    P = R.init_params_widened(seed=1, scale=1.0)
    x = list(R.synthetic_batch(4, 5))
    out = []
    for _ in range(2):
        m = pivp.Model(10, prefix='d', keep_activations=True, deterministic=True)
        m.load_state_dict_reference(P)
        opt = pivp.Adam(alpha=0.001).setup(m)
        for itr in range(3):
            opt.update(m, x, itr)
            m.reset_state()
        torch.cuda.synchronize()
        out.append((m._flat_params.clone(), opt._m.clone(), opt._v.clone(), opt.t))
    assert out[0][3] == out[1][3] == 3
    for a, b, what in zip(out[0][:3], out[1][:3], ('parameters', 'Adam m', 'Adam v')):
        assert torch.equal(a, b), '%s differ after three steps' % what


_CHILD = r'''
import hashlib, sys
import torch
sys.path.insert(0, %r)
import pivp_amd
from oracle import restatement as R
P = R.init_params_widened(seed=1, scale=1.0)
m = pivp_amd.Model(10, prefix='c', keep_activations=True, deterministic=True)
m.load_state_dict_reference(P)
m(list(R.synthetic_batch(4, 5)), 0)
m.cleargrads(); m.backward(); torch.cuda.synchronize()
print('SHA', hashlib.sha256(m._flat_grads.cpu().numpy().tobytes()).hexdigest())
'''


def test_two_processes_give_the_same_gradient_bits(pivp):
    hashes = []
    for _ in range(2):      # one child at a time, each under a time limit
        p = subprocess.run([sys.executable, '-c', _CHILD % ROOT], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        hashes.append([ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith('SHA ')][-1])
    assert hashes[0] == hashes[1]


def _make_dataset(root, n=6, T=4):
    """tests/test_gpu_pipeline.py's generated data set (copied)"""
    from pivp_amd import dataset as ds
    rs = np.random.RandomState(0)
    rows = []
    for j in range(n):
        np.save(os.path.join(root, 'image_batch_%d' % j), rs.rand(T, 64, 64, 3).astype(np.float32))
        np.save(os.path.join(root, 'action_batch_%d' % j), (rs.randn(T, 5) * 0.1).astype(np.float32))
        np.save(os.path.join(root, 'state_batch_%d' % j), (rs.randn(T, 5) * 0.1).astype(np.float32))
        np.save(os.path.join(root, 'image_batch_pred_%d' % j), (rs.rand(T, 96, 120, 3) * 255).astype(np.uint8))
        rows.append([j, '', 'image_batch_%d.npy' % j, 'action_batch_%d.npy' % j, 'state_batch_%d.npy' % j, '', 'image_batch_pred_%d.npy' % j])
    ds.write_map(root, rows)


def _checkpoints(d):
    return sorted(f for f in os.listdir(d) if f.split('-')[0] in ('training', 'state') and f.split('-', 1)[1][:1].isdigit())


def test_train_main_twice_writes_identical_checkpoints(pivp, tmp_path):
    from pivp_amd import train as T
    data = tmp_path / 'data'
    data.mkdir()
    _make_dataset(str(data))
    dirs = []
    for r in range(2):
        out = tmp_path / ('models%d' % r)
        out.mkdir()
        dirs.append(T.main(['--data_dir', str(data), '--output_dir', str(out), '--num_iterations', '4', '--batch_size', '2',
                            '--schedsamp_k', '900', '--save_interval', '2', '--validation_interval', '2', '--train_val_split', '0.7',
                            '--deterministic', '1']))
    files = _checkpoints(dirs[0])
    assert files and files == _checkpoints(dirs[1])
    for f in files:
        with np.load(os.path.join(dirs[0], f)) as a, np.load(os.path.join(dirs[1], f)) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in a.files:
                assert np.array_equal(a[k], b[k]), '%s: %s differs between the two runs' % (f, k)


def test_stp_gradients_match_float64_autograd(pivp):
    # tests/test_gpu_train.py::test_bptt_gradients_stp's case and gate, deterministic (d prev through the integer accumulator)
    from numpy.lib.stride_tricks import sliding_window_view
    P = R.init_params_widened(seed=1, scale=1.0, model_type='STP')
    imgs, acts, stas = R.synthetic_batch(2, 4)
    pad = np.pad(imgs, ((0, 0), (0, 0), (0, 0), (5, 5), (5, 5)), mode='reflect')
    imgs = np.ascontiguousarray(sliding_window_view(pad, (11, 11), axis=(3, 4)).mean(axis=(-1, -2))).astype(np.float32)
    tm = TorchModel(10, params=P, requires_grad=True, is_cdna=False, is_stp=True)
    loss_t = tm([imgs, acts, stas], 0)
    loss_t.backward()
    gref = {k: v.grad.numpy() for k, v in tm.p.items()}
    m = pivp.Model(10, is_cdna=False, is_stp=True, prefix='d', keep_activations=True, deterministic=True)
    m.load_state_dict_reference(P)
    loss = float(m([imgs, acts, stas], 0))
    m.cleargrads(); m.backward()
    assert abs(loss - float(loss_t.detach())) < 1e-6
    print('STP worst relative gradient error', _check_grads(m.grads_reference(), gref, 5e-3))


def test_refused_combinations_raise(pivp):
    for prec in ('bf16x6', 'fp16x3'):
        with pytest.raises(ValueError, match=prec):
            pivp.Model(10, keep_activations=True, precision=prec, deterministic=True)
    # a shape the fixed-order weight gradients do not serve (ConvLSTM maps not a power of two): refused when the plan is made
    m = pivp.Model(10, keep_activations=True, deterministic=True)
    with pytest.raises(ValueError, match='48x48'):
        m(list(R.synthetic_batch(2, 3, 48, 48)), 0)
