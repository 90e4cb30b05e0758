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
