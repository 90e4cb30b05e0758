"""GPU tests of pivp_image_loss (L1 / gradient-difference / DSSIM / extra-MSE terms with their gradient, include/pivp_loss.h) against the float64
restatement of tests/loss_reference.py, of its structural promises (same bits run to run, an image's outputs independent of its neighbours, the
grid and the gradient being asked for), of the backward sweep's seed hook (pivp_plan_set_frame_grad, `Model.backward(frame_grad=...)`) and of
`Model(image_loss=...)` on top of both.

Gates.  dssim: 1e-6 absolute per image (the metric's gate).  mse / l1 / gdl: 1e-6 relative (fp64 sums of exact differences, one rounding).
Gradient: every element within 1e-6 of float64 autograd, relative to that image's largest reference element -- the kernel keeps moments, maps and
the transposed window in fp64 and rounds once (6e-8; twice when the DSSIM part and the pointwise part are added); the loss composed in plain
float32 autograd is printed beside it and never gated: it misses the gate on the flat inputs, which is what those inputs are for.  For L1 / GDL
the pixels lie on a 2^-10 grid: every difference is exact in fp32 and fp64, kernel and reference take the same `sign` branches -- many of them the
exact zero, which pins sign(0) = 0 -- and no element is excluded anywhere.  weighted total: 1e-6 of sum |w_k term_k| (each term's own gate)."""
import os
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from oracle import restatement as R
from oracle.torch_restatement import TorchModel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ops as LO  # noqa: E402
import loss_reference as LR  # noqa: E402

pytestmark = pytest.mark.gpu

DSSIM_TOL = 1e-6
VALUE_RTOL = 1e-6
GRAD_RTOL = 1e-6
BADARG = -1
INPUTS = ('noise', 'bright flat', 'const truth', 'ramp')
ALONE = {'mse': (1.0, 0, 0, 0), 'l1': (0, 1.0, 0, 0), 'gdl': (0, 0, 1.0, 0), 'dssim': (0, 0, 0, 1.0)}
ALL = (0.5, 0.2, 0.1, 0.3)


def make_input(kind, N, C, H, W, seed, grid):
    """-> (pred, truth) float32 (N, C, H, W); grid: every pixel a multiple of 2^-10."""
    rs = np.random.RandomState(seed)
    shp = (N, C, H, W)
    if kind == 'noise':
        y, x = rs.rand(*shp), rs.rand(*shp)
    elif kind == 'bright flat':
        x = 0.9 + 0.02 * rs.rand(*shp)
        y = x + 0.01 * rs.randn(*shp)
    elif kind == 'const truth':
        x = np.full(shp, 0.75)
        y = x + 1e-3 * rs.randn(*shp)
    elif kind == 'ramp':
        x = rs.rand(*shp)
        y = np.broadcast_to((np.arange(H).reshape(H, 1) + np.arange(W).reshape(1, W)) / float(H + W), shp).copy()
    else:
        raise KeyError(kind)
    if grid:
        y, x = np.round(y * 1024.0) / 1024.0, np.round(x * 1024.0) / 1024.0
    return y.astype(np.float32), x.astype(np.float32)


_REF = {}


def reference(kind, shape, weights, win, sigma, grid):
    """(pred, truth, float64 result, plain-float32-autograd result), computed once per case and shared, write-protected."""
    key = (kind, shape, weights, win, sigma, grid)
    if key not in _REF:
        y, x = make_input(kind, *shape, seed=len(kind) * 1000 + shape[2] * 7 + shape[3], grid=grid)
        r64 = LR.loss_and_grad(y, x, weights, win, sigma, 1.0, torch.float64)
        r32 = LR.loss_and_grad(y, x, weights, win, sigma, 1.0, torch.float32)
        for a in (y, x) + tuple(r64.values()) + tuple(r32.values()):
            a.setflags(write=False)
        _REF[key] = (y, x, r64, r32)
    return _REF[key]


def grad_err(g, ref):
    """largest element error per image, relative to that image's largest reference element"""
    N = ref.shape[0]
    scale = np.abs(ref).reshape(N, -1).max(axis=1)
    err = np.abs(g.astype(np.float64) - ref).reshape(N, -1).max(axis=1)
    assert (scale > 0).all()
    return (err / scale).max()


def check_against(out, r64, r32, weights, label, fails):
    """values, means, total and gradient of one call against float64; prints each figure beside plain float32 autograd's"""
    N = r64['values'].shape[1]
    line = [label]
    for k, name in enumerate(LR.TERMS):
        got, ref = out['values'][k].astype(np.float64), r64['values'][k]
        if weights[k] == 0:
            if not ((out['values'][k] == 0).all() and out['terms'][k] == 0):
                fails.append('%s: %s has weight 0 but is not written as 0' % (label, name))
            continue
        if name == 'dssim':
            e, e_mean, tol = np.abs(got - ref).max(), abs(float(out['terms'][k]) - r64['terms'][k]), DSSIM_TOL
        else:
            with np.errstate(invalid='ignore', divide='ignore'):
                e = np.where(ref > 0, np.abs(got - ref) / ref, np.abs(got)).max()
            e_mean = abs(float(out['terms'][k]) - r64['terms'][k]) / r64['terms'][k] if r64['terms'][k] > 0 else abs(float(out['terms'][k]))
            tol = VALUE_RTOL
        line.append('%s %.1e / mean %.1e' % (name, e, e_mean))
        if not (e <= tol and e_mean <= tol):
            fails.append('%s: %s off by %.3e per image, %.3e in the mean (gate %.0e)' % (label, name, e, e_mean, tol))
    budget = sum(abs(w * t) for w, t in zip(weights, r64['terms'][:4]))
    e_tot = abs(float(out['terms'][4]) - r64['terms'][4])
    if not e_tot <= 1e-6 * budget:
        fails.append('%s: total off by %.3e (budget %.3e)' % (label, e_tot, 1e-6 * budget))
    eg, eg32 = grad_err(out['grad'], r64['grad']), grad_err(r32['grad'], r64['grad'])
    line.append('grad %.2e (plain float32 autograd %.2e)' % (eg, eg32))
    print('   '.join(line))
    if not eg <= GRAD_RTOL:
        fails.append('%s: gradient off by %.3e of the image\'s largest element' % (label, eg))


SHAPES = [(1, 1, 11, 11), (3, 3, 16, 24), (2, 3, 13, 37), (5, 3, 64, 64), (1, 3, 128, 128)]
CASES = [(s, 11, 1.5) for s in SHAPES] + [((3, 3, 16, 24), 3, 1.5), ((3, 3, 16, 24), 7, 1.5), ((3, 3, 16, 24), 7, 0.0)]


@pytest.mark.parametrize('shape,win,sigma', CASES, ids=['n%dc%d-%dx%d-win%d-s%g' % (s + (w, g)) for s, w, g in CASES])
def test_image_loss_against_float64(shape, win, sigma):
    """Each term alone and all four together, on every input.  mse and dssim alone on the raw float32 inputs; l1, gdl and the combination on the
    2^-10 grid (see the module docstring)."""
    fails = []
    for kind in INPUTS:
        for name, weights, grid in [('mse', ALONE['mse'], False), ('dssim', ALONE['dssim'], False), ('l1', ALONE['l1'], True),
                                    ('gdl', ALONE['gdl'], True), ('all', ALL, True)]:
            y, x, r64, r32 = reference(kind, shape, weights, win, sigma, grid)
            out = LO.image_loss(y, x, weights, win, sigma)
            check_against(out, r64, r32, weights, '%-11s %-5s %s win %d' % (kind, name, 'x'.join(map(str, shape)), win), fails)
    assert not fails, fails


@pytest.mark.parametrize('shape', [(2, 3, 13, 37), (2, 3, 64, 64)], ids=['13x37', '64x64'])
def test_identical_frames_have_no_gradient(shape):
    """pred == truth: every term sits at its minimum (l1 / gdl at sign(0) = 0).  DSSIM's three per-pixel terms cancel there in exact arithmetic;
    what fp64 leaves is bounded absolutely."""
    N, C, H, W = shape
    y = make_input('noise', *shape, seed=4, grid=False)[0]
    for weights in (ALONE['dssim'], ALL):
        for same in (True, False):
            out = LO.image_loss(y, y.copy(), weights, same=same)
            bound = 1e-9 / (C * (H - 10) * (W - 10))
            g = np.abs(out['grad']).max()
            print('identical %s weights %s: max |grad| %.2e (bound %.2e), dssim %s' % ('x'.join(map(str, shape)), weights, g, bound, out['values'][3]))
            assert g <= bound
            assert np.abs(out['values'][3]).max() <= DSSIM_TOL and (out['values'][:3] == 0).all() and abs(out['terms'][4]) <= DSSIM_TOL


def test_same_bits_run_to_run():
    y, x = reference('bright flat', (2, 3, 13, 37), ALL, 11, 1.5, True)[:2]
    a, b = LO.image_loss(y, x, ALL), LO.image_loss(y, x, ALL)
    for k in ('values', 'terms', 'grad'):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_an_images_outputs_depend_on_nothing_but_the_image():
    """More images than CUs (256): the block loop of the DSSIM kernel wraps (two blocks per CU at the most).  Image i inside the batch and image i
    alone (N = 1, block 0) give the same values bit for bit, and the same gradient when the weights keep w_k / N what it was: 75 at N = 300 against
    0.25 at N = 1, both exact in fp32 -- the gradient is d terms[4] / d pred, which carries 1 / N by definition."""
    N = 300
    rs = np.random.RandomState(11)
    x = (np.round(rs.rand(N, 3, 16, 24) * 1024) / 1024).astype(np.float32)
    y = np.clip(x + np.round(rs.normal(0, 0.05, x.shape) * 1024) / 1024, 0, 1).astype(np.float32)
    big = LO.image_loss(y, x, (75.0, 75.0, 75.0, 75.0))
    assert len(np.unique(big['values'][3])) > N // 2
    for i in (0, 1, 255, 256, 299):
        one = LO.image_loss(y[i:i + 1], x[i:i + 1], (0.25, 0.25, 0.25, 0.25))
        assert one['values'].tobytes() == big['values'][:, i:i + 1].tobytes(), i
        assert one['grad'].tobytes() == big['grad'][i:i + 1].tobytes(), i
    r64 = LR.loss_and_grad(y, x, (75.0, 75.0, 75.0, 75.0))
    assert np.abs(big['values'][3] - r64['values'][3]).max() <= DSSIM_TOL and grad_err(big['grad'], r64['grad']) <= GRAD_RTOL
    assert (np.abs(big['terms'][:3] - r64['terms'][:3]) <= VALUE_RTOL * r64['terms'][:3]).all() and abs(big['terms'][3] - r64['terms'][3]) <= DSSIM_TOL


def test_a_null_gradient_leaves_the_values_unchanged():
    y, x = reference('noise', (2, 3, 13, 37), ALL, 11, 1.5, True)[:2]
    full = LO.image_loss(y, x, ALL)
    rc, vo = LO.image_loss_rc(y, x, ALL, want_grad=False)
    assert rc == 0 and vo['values'].tobytes() == full['values'].tobytes() and vo['terms'].tobytes() == full['terms'].tobytes()
    assert (vo['grad'] == LO.FILL).all()


def test_a_zero_weight_leaves_zeros():
    y, x = reference('noise', (2, 3, 13, 37), ALL, 11, 1.5, True)[:2]
    full = LO.image_loss(y, x, ALL)
    for k in range(4):
        w = tuple(0.0 if j == k else ALL[j] for j in range(4))
        out = LO.image_loss(y, x, w)
        assert (out['values'][k] == 0).all() and out['terms'][k] == 0
        for j in range(4):
            if j != k:      # the other terms do not notice
                assert out['values'][j].tobytes() == full['values'][j].tobytes() and out['terms'][j] == full['terms'][j]
    none = LO.image_loss(y, x, (0.0, 0.0, 0.0, 0.0))      # nothing to compute: zeros everywhere, the gradient included (every element is written)
    assert (none['values'] == 0).all() and (none['terms'] == 0).all() and (none['grad'] == 0).all()


def test_bad_arguments_are_refused_and_nothing_is_written():
    y = np.random.RandomState(5).rand(2, 3, 12, 14).astype(np.float32)
    nan, inf = float('nan'), float('inf')
    bad = [dict(N=0), dict(N=-1), dict(C=0), dict(H=0), dict(W=0), dict(win=4), dict(win=10), dict(win=1), dict(win=13), dict(win=-3),
           dict(H=10), dict(W=10), dict(weights=(0, 0, 1.0, 0), H=1), dict(weights=(0, 0, 1.0, 0), W=1),
           dict(weights=(nan, 0, 0, 0)), dict(weights=(0, inf, 0, 0)), dict(weights=(0, 0, -inf, 0)), dict(weights=(0, 0, 0, nan)),
           dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=nan), dict(sigma=nan),
           dict(null='pred'), dict(null='truth'), dict(null='spec'), dict(null='values'), dict(null='terms'), dict(null='ws')]
    for kw in bad:
        kw = dict(kw)
        args = dict(weights=kw.pop('weights', ALL), win=kw.pop('win', 11), sigma=kw.pop('sigma', 1.5), data_range=kw.pop('data_range', 1.0))
        rc, out = LO.image_loss_rc(y, y, null=kw.pop('null', ()), **args, **kw)
        assert rc == BADARG, (kw, args, rc)
        assert all((out[k] == LO.FILL).all() for k in ('values', 'terms', 'grad')), (kw, args)
    # smaller than the window is fine while DSSIM is off, one row is fine while the GDL is off
    rc, out = LO.image_loss_rc(y, y, (1.0, 1.0, 1.0, 0.0), H=10)
    assert rc == 0
    rc, out = LO.image_loss_rc(y, y, (1.0, 1.0, 0.0, 0.0), H=1)
    assert rc == 0 and (out['values'] == 0).all()


def test_module_image_loss_shapes_and_inputs():
    y, x, r64, _ = reference('noise', (2, 3, 13, 37), ALL, 11, 1.5, True)
    spec = pivp_amd.ImageLoss(*ALL)
    ys, xs = y.reshape(2, 1, 3, 13, 37), x.reshape(2, 1, 3, 13, 37)
    got = pivp_amd.image_loss(ys, torch.tensor(xs).cuda(), spec, want_grad=True)            # host array against device tensor
    assert got.values.shape == (4, 2, 1) and got.terms.shape == (5,) and got.grad.shape == ys.shape and got.grad.is_cuda and got.total.dim() == 0
    assert grad_err(got.grad.cpu().numpy().reshape(y.shape), r64['grad']) <= GRAD_RTOL and abs(float(got.total) - r64['terms'][4]) <= 1e-6
    assert pivp_amd.image_loss(y[0], x[0], spec).grad is None


# ---- the seed hook and the model ------------------------------------------------------------------------------------------------------------

MAX_OVER_TOL_NORM = 4 * 128      # per-element LayerNorm parameters: up to four flipped units x 128 channels at their pixel
MAX_OVER_TOL = 16                # every other tensor


def _check_grads(got, ref, tol, relu_flips=2):
    """The rule of test_gpu_train._check_grads (see there for the why).  Per tensor, relative to max |ref|: the 99th percentile of the element errors
    < tol, the relative L2 error < tol, no element beyond 10 x tol, and at most a few flipped units' footprint between tol and 10 x tol; the
    per-element LayerNorm parameters directly behind a ReLU drop their `relu_flips` largest elements from the 10 x tol bound."""
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


def _masks(model_type):
    return 1 if model_type == 'DNA' else 10      # (the DNA head takes one mask, TM:390)


def _params(model_type):
    return R.init_params_widened(seed=1, scale=1.0) if model_type == 'CDNA' else \
        R.init_params_widened(seed=1, scale=1.0, num_masks=_masks(model_type), model_type=model_type, height=64, width=64)


def _kinds(model_type):
    return dict(is_cdna=model_type == 'CDNA', is_stp=model_type == 'STP', is_dna=model_type == 'DNA')


def _autograd(P, batch, model_type='CDNA', weights=None, seed_tensor=None, k=-1, it=0, rng_seed=None):
    """float64 autograd on TorchModel of: its own loss + the image terms with `weights` (the MSE weight beyond the reference's 1) + sum(seed * gen[ctx-1:]).
    -> (total loss, {term: mean}, gradients)"""
    imgs, acts, stas = batch
    tm = TorchModel(_masks(model_type), params=P, requires_grad=True, scheduled_sampling_k=k, **_kinds(model_type))
    if rng_seed is not None:
        tm.rng = np.random.RandomState(rng_seed)
    loss = tm([imgs, acts, stas], it)
    ctx = 2
    gen = torch.stack(tm.gen_images[ctx - 1:])                                   # (T-ctx, B, 3, H, W), keeps the graph
    means = {}
    if weights is not None:
        truth = torch.tensor(np.asarray(imgs[ctx:]), dtype=torch.float64)
        extra, _, means = LR.total(gen.reshape((-1,) + tuple(gen.shape[2:])), truth.reshape((-1,) + tuple(truth.shape[2:])),
                                   (weights[0] - 1.0,) + tuple(weights[1:]))
        loss = loss + extra
        means = {k_: float(v.detach()) for k_, v in means.items()}
    if seed_tensor is not None:
        loss = loss + (torch.tensor(seed_tensor, dtype=torch.float64) * gen).sum()
    loss.backward()
    return float(loss.detach()), means, {kk: v.grad.numpy() for kk, v in tm.p.items()}


def _flat(m):
    return m._flat_grads.clone()


def test_seed_hook_matches_autograd_and_clears():
    """CDNA, B = 2, T = 5, 64 x 64: backward(frame_grad=R) against float64 autograd of loss + sum(R * gen[ctx-1:]); then, with the seed cleared, the
    sweep is the plain one again, bit for bit under deterministic=True."""
    P = _params('CDNA')
    batch = R.synthetic_batch(2, 5)
    Rs = (np.random.RandomState(21).randn(3, 2, 3, 64, 64) * 1e-5).astype(np.float32)      # the size of the loss's own seed: 2 (gen - x) / (24576 * 3) ~ 8e-6
    _, _, gref = _autograd(P, batch, seed_tensor=Rs)
    m = pivp_amd.Model(10, prefix='t', keep_activations=True, deterministic=True)
    m.load_state_dict_reference(P)
    m(list(batch), 0)
    m.cleargrads(); m.backward(frame_grad=torch.from_numpy(Rs).cuda())
    worst = _check_grads(m.grads_reference(), gref, 2e-3)
    print('seed hook: worst relative gradient error', worst)
    m.reset_state()
    m(list(batch), 0)
    m.cleargrads(); m.backward()
    after = _flat(m)
    plain = pivp_amd.Model(10, prefix='t', keep_activations=True, deterministic=True)
    plain.load_state_dict_reference(P)
    plain(list(batch), 0)
    plain.cleargrads(); plain.backward()
    assert torch.equal(after, _flat(plain))
    for bad in (torch.zeros(3, 2, 3, 64, 64), torch.zeros(2, 2, 3, 64, 64).cuda(), torch.zeros(3, 2, 3, 64, 64, dtype=torch.float64).cuda(), Rs):
        with pytest.raises(ValueError, match='frame_grad'):
            m.backward(frame_grad=bad)


@pytest.mark.parametrize('model_type,sched', [('CDNA', False), ('STP', False), ('DNA', False), ('CDNA', True)],
                         ids=['CDNA', 'STP', 'DNA', 'CDNA-scheduled-sampling'])
def test_model_with_an_image_loss(model_type, sched):
    P = _params(model_type)
    batch = R.synthetic_batch(2, 5)
    spec = pivp_amd.ImageLoss(mse=0.5, l1=0.2, gdl=0.1, dssim=0.3)
    k, it = (2.0, 1.0) if sched else (-1, 0)
    loss_ref, means, gref = _autograd(P, batch, model_type, spec.weights(), k=k, it=it, rng_seed=5 if sched else None)
    m = pivp_amd.Model(_masks(model_type), prefix='t', keep_activations=True, image_loss=spec, scheduled_sampling_k=k, **_kinds(model_type))
    m.load_state_dict_reference(P)
    np.random.seed(5)
    with pivp_amd.using_config('train', True):
        loss = m(list(batch), it)
    m.cleargrads(); m.backward()
    assert loss.is_cuda and loss.dim() == 0 and loss is m.loss and sorted(m.loss_terms) == ['dssim', 'extra', 'gdl', 'l1', 'mse']
    print('%s%s: loss %.8f (float64 %.8f)  terms %s  float64 %s' % (model_type, ' scheduled' if sched else '', float(loss), loss_ref,
                                                                     {k_: float(v) for k_, v in m.loss_terms.items()}, means))
    assert abs(float(loss) - loss_ref) <= 1e-6
    assert abs(float(m.loss_terms['extra']) - (float(loss) - float(m._results[0]))) <= 1e-7
    worst = _check_grads(m.grads_reference(), gref, 2e-3)
    print('worst relative gradient error', worst)
    # the term the user is shown: 1 - mean of the per-sample SSIM the evaluation reports, on the same frames
    fm = pivp_amd.frame_metrics(torch.stack(m.gen_images)[1:], torch.from_numpy(np.asarray(batch[0], np.float32)).cuda()[2:])
    assert abs(float(m.loss_terms['dssim']) - (1.0 - float(fm.ssim.double().mean()))) <= 1e-6
    # summaries, psnr_all and the frames are the rollout's own
    assert len(m.summaries) == 3 * 3 + 2 and m.summaries[-1] == 't_loss: ' + str(m._results.cpu().numpy()[0])
    # without training mode nothing is kept for a sweep
    m.reset_state()
    with pivp_amd.using_config('train', False):
        m(list(batch), it)
    assert m._loss_grad is None and m.loss_terms is not None
    with pytest.raises(RuntimeError, match='training mode'):
        m.backward()


def _step(m, opt, batch):
    loss = opt.update(m, list(batch), 0).clone()
    out = (loss, _flat(m), m._flat_params.clone())
    m.reset_state()
    return out


def test_deterministic_steps_repeat_and_the_off_switch_changes_no_bit():
    P = _params('CDNA')
    batch = R.synthetic_batch(2, 5)
    spec = pivp_amd.ImageLoss(mse=0.5, l1=0.2, gdl=0.1, dssim=0.3)

    def run(**kw):
        m = pivp_amd.Model(10, prefix='t', keep_activations=True, deterministic=True, **kw)
        m.load_state_dict_reference(P)
        opt = pivp_amd.Adam(alpha=0.001); opt.setup(m)
        return _step(m, opt, batch)
    a, b = run(image_loss=spec), run(image_loss=spec)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # None and the reference's own weights: loss, gradients and the Adam step of a model built without the argument
    base = run()
    for kw in (dict(image_loss=None), dict(image_loss=pivp_amd.ImageLoss())):
        for u, v in zip(run(**kw), base):
            assert torch.equal(u, v)
    assert not torch.equal(a[1], base[1])
