"""The float64 autograd oracle of the model-level gradient tests and their gate, shared by tests/test_gpu_train.py (64 x 64 and 128 x 128 frames) and
tests/test_gpu_train_shapes.py (every other frame size and mask count the plan accepts)."""
import numpy as np

from oracle.torch_restatement import TorchModel


def _autograd(P, imgs, acts, stas, k=-1, it=0, seed=None, **kw):
    tm = TorchModel(kw.pop('num_masks', 10), params=P, requires_grad=True, scheduled_sampling_k=k, **kw)
    if seed is not None:
        tm.rng = np.random.RandomState(seed)
    loss = tm([imgs, acts, stas], it)
    loss.backward()
    return float(loss), {kk: v.grad.numpy() for kk, v in tm.p.items()}


MAX_OVER_TOL_NORM = 4 * 128      # per-element LayerNorm parameters: up to four flipped units x 128 channels at their pixel
MAX_OVER_TOL = 16                # every other tensor


def _check_grads(got, ref, tol, relu_flips=2):
    """Per tensor, relative to max |ref|: the 99th percentile of the element errors < tol, the relative L2 error < tol, and
    no element beyond 10 x tol.  Why not simply max < tol: an activation within fp32 rounding of zero has its ReLU mask decided
    differently in fp32 and in the float64 oracle, which moves the gradient of everything in that unit's footprint by one sample's
    dy -- e.g. one flipped enc5 unit shows up at ONE pixel position in all 64 channels of hidden6's gamma/beta (7e-3 there, 5e-7
    median: scripts/debug_grad_errors_stp.py), one flipped enc6 unit in one element of norm_enc6 (scripts/debug_dna_grad.py).
    Which unit flips changes with any rounding change in the forward pass; a wrong kernel moves the bulk, which the percentile and
    the L2 norm see.  The per-element LayerNorm parameters directly behind a ReLU (norm_enc0, norm_enc6) additionally drop their
    `relu_flips` largest elements from the 10 x tol bound."""
    worst = []
    over_counts = []
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
        # ... and HOW MANY elements may sit between tol and 10 x tol: the footprint of a few flipped units, not a flat 1 % of the tensor
        # (a tile-edge bug in a partial-sum reduce or a column-limited data gradient is wrong on a stripe of the tensor: hundreds to
        # thousands of elements).  A flipped unit moves ONE pixel position of the per-element LayerNorm parameters above it in all of its
        # <= 128 channels, and nothing else by more than one sample's share of a sum over >= 2048 pixels.
        n_over = int((e > tol).sum())
        allowed = MAX_OVER_TOL_NORM if '/norm/' in kname else MAX_OVER_TOL
        over_counts.append((n_over, kname))
        assert n_over <= allowed, '%s: %d elements above tol %.1e (allowed %d)' % (kname, n_over, tol, allowed)
    print('elements above tol, worst tensors:', sorted(over_counts, reverse=True)[:3])
    return max(worst)


def _autograd_zero_filled(P, imgs, acts, stas, **kw):
    """_autograd for configurations in which the oracle leaves a parameter out of the graph (num_masks = 1: cdna_kerns in CDNA, stp_input and
    identity_params in STP -- the single transformed image is dropped, TM:726): its `.grad` is None, which counts as a gradient of zeros."""
    tm = TorchModel(kw.pop('num_masks', 10), params=P, requires_grad=True, scheduled_sampling_k=-1, **kw)
    loss = tm([imgs, acts, stas], 0)
    loss.backward()
    return float(loss), {kk: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for kk, v in tm.p.items()}


# ---- the tight gate: float64 autograd on the branch the device took --------------------------------------------------------------------------
# _check_grads above is as wide as one flipped ReLU unit (its docstring).  The helpers below take the flip out of the comparison instead: the oracle's ReLUs
# are forced to the masks read from the device's own activations (TorchModel(relu_masks=...)), so that the float64 gradient is the gradient of the function
# the device evaluated, and the gate is a multiple of what the SAME oracle in float32 loses against float64 on that branch.
TAPPED_SITES = ('enc0', 'enc1', 'enc2', 'enc3', 'enc4', 'enc5', 'enc6')      # Model.tap gives the post-ReLU activation itself; + 'enc7' for CDNA / DNA
UNTAPPED_SITES = ('masks', 'kern', 'kn', 's1')                               # mask logits, CDNA kernel shift, DNA kernel shift, STP hidden layer: the oracle's own ReLU
TIGHT_MARGIN = 10.0
TIGHT_FACTOR_CAP = 50.0


def _tapped_sites(model_type):
    return TAPPED_SITES + (('enc7',) if model_type in ('CDNA', 'DNA') else ())


def _oracle_pass(P, batch, masks=None, dtype=None, record=False, k=-1, it=0, seed=None, wrt_inputs=False, backward=True, tm=None, **kw):
    """One pass of the torch restatement, optionally on forced ReLU masks -> (tm, loss, grads, (d loss / d actions, d loss / d states)).  Parameters and
    inputs left out of the graph count as zero gradients (_autograd_zero_filled).  `tm`: continue on this model's carried state (no reset_state())."""
    import torch
    dtype = dtype or torch.float64
    if tm is None:
        tm = TorchModel(kw.pop('num_masks', 10), params=P, requires_grad=backward, scheduled_sampling_k=k, dtype=dtype, record=record, relu_masks=masks, **kw)
    if seed is not None:
        tm.rng = np.random.RandomState(seed)
    imgs, acts, stas = batch
    a = torch.tensor(np.asarray(acts), dtype=dtype, requires_grad=wrt_inputs)
    s = torch.tensor(np.asarray(stas), dtype=dtype, requires_grad=wrt_inputs)
    with torch.set_grad_enabled(backward):
        loss = tm([torch.tensor(np.asarray(imgs), dtype=dtype), a, s], it)
    if not backward:
        return tm, float(loss.detach()), None, None
    for v in tm.p.values():
        v.grad = None
    loss.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy().copy()
    return tm, float(loss.detach()), {kk: zero(v) for kk, v in tm.p.items()}, (zero(a), zero(s))


def _autograd_masked(P, batch, masks, dtype, **kw):
    """loss and zero-filled parameter gradients of the oracle run in `dtype` with the ReLUs listed in `masks` forced ({(site, step): bool array})"""
    _, loss, grads, _ = _oracle_pass(P, batch, masks=masks, dtype=dtype, **kw)
    return loss, grads


def _oracle_preactivations(P, batch, **kw):
    """{(site, step): pre-activation} of the unforced float64 oracle (forward only)"""
    tm = _oracle_pass(P, batch, record=True, backward=False, **kw)[0]
    return {key: v.numpy() for key, v in tm.pre.items()}


def _device_relu_masks(model, steps, pre64=None, step0=0):
    """-> ({(site, step0 + step): tap > 0}, n): the masks of every ReLU site whose post-ReLU activation Model.tap exposes, for the first `steps` timesteps of
    the model's last call, and (with the unforced float64 oracle's pre-activations `pre64`) how many of these units the oracle has on the other side of zero.
    Every tap must be a post-ReLU tensor: no negative entry."""
    masks, n = {}, (0 if pre64 is not None else None)
    for site in _tapped_sites(model.model_type):
        for st in range(steps):
            a = model.tap(site, st)
            a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
            assert a.min() >= 0, 'tap %s of step %d is no post-ReLU tensor (min %.3e)' % (site, st, a.min())
            masks[(site, step0 + st)] = a > 0
            if pre64 is not None:
                n += int(((pre64[(site, step0 + st)] > 0) != masks[(site, step0 + st)]).sum())
    return masks, n


def _near_zero_untapped(pre, eps=1e-5):
    """how many units of the sites left to the oracle have |pre-activation| < eps: the candidates for a flip the forced masks do not remove.  (DNA's `kn` is
    relu(enc7) - RELU_SHIFT: where enc7's own, forced, ReLU gave zero it is -RELU_SHIFT exactly and no candidate.)"""
    from oracle.torch_restatement import RELU_SHIFT
    n = 0
    for (site, _), v in pre.items():
        if site in UNTAPPED_SITES:
            v = np.asarray(v)
            n += int(((np.abs(v) < eps) & ((v != -RELU_SHIFT) if site == 'kn' else True)).sum())
    return n


def _rel_errors(got, ref):
    d = np.asarray(got, dtype=np.float64) - ref
    return np.linalg.norm(d) / np.linalg.norm(ref), np.abs(d).max() / np.abs(ref).max()


def _e32(ref64, ref32):
    """the float32 oracle's own error against the float64 one, worst over the tensors: (relative L2, largest element error relative to max |ref|)"""
    errs = [_rel_errors(ref32[k], g) for k, g in ref64.items() if np.any(g)]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def _check_grads_tight(got, ref64, ref32, factors=None, margin=TIGHT_MARGIN):
    """Every tensor, no percentile, no outliers: relative L2 error <= M x e32_L2 and max |error| / max |ref| <= M x e32_max, with e32_* the same measures of
    the float32 oracle `ref32` against `ref64` (same forced masks), worst over the case's tensors, and M = `margin` -- or `factors[name]` (<= 50) for a tensor
    the test file's table names.  A tensor whose float64 gradient is identically zero must be exactly zero.  -> (worst ratio to e32, tensor name)."""
    factors = factors or {}
    assert all(f <= TIGHT_FACTOR_CAP for f in factors.values()) and set(factors) <= set(ref64), factors
    e32_l2, e32_max = _e32(ref64, ref32)
    worst, failures = (0.0, ''), []
    for kname, g in ref64.items():
        x = np.asarray(got[kname])
        assert x.shape == g.shape, (kname, x.shape, g.shape)
        if not np.any(g):
            if np.any(x):
                failures.append('%s: the float64 gradient is identically zero, got max |g| %.3e' % (kname, np.abs(x).max()))
            continue
        l2, mx = _rel_errors(x, g)
        ratio = max(l2 / e32_l2, mx / e32_max)
        worst = max(worst, (ratio, kname))
        m = factors.get(kname, margin)
        if not (np.isfinite(x).all() and l2 <= m * e32_l2 and mx <= m * e32_max):
            failures.append('%s: relative L2 %.3e (%.1f x e32), max %.3e (%.1f x e32), allowed %g x' % (kname, l2, l2 / e32_l2, mx, mx / e32_max, m))
    print('tight gate: e32 L2 %.3e max %.3e; worst ratio to e32 %.2f (%s)' % (e32_l2, e32_max, worst[0], worst[1]))
    assert not failures, '%d tensors outside the tight gate (e32 L2 %.3e, max %.3e):\n  ' % (len(failures), e32_l2, e32_max) + '\n  '.join(failures)
    return worst
