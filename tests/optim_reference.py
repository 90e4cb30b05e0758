"""Float64 NumPy restatement of the guarded Adam step (include/pivp_optim.h): the L2 norms of gscale * g per segment, per gradient group and over
the whole flat buffer, Chainer's GradientClipping rate rounded to float32, the non-finite flag, and the clipped gradient fed to Chainer's Adam rule
(oracle.torch_restatement.chainer_adam_step).  Written from the definitions, not from the kernels: np.sum's pairwise order, no granules."""
import numpy as np

from oracle.torch_restatement import chainer_adam_step

GRAD_GROUPS = 6


def segments(seg_end):
    """[(start, end)] of a segment table (ascending ends, the first segment starts at 0)."""
    ends = [int(e) for e in seg_end]
    return list(zip([0] + ends[:-1], ends))


def grad_stats(g, seg_end, seg_group, ngroups=GRAD_GROUPS, gscale=1.0, threshold=0.0):
    """-> dict(norm, rate (np.float32), nonfinite (0 / 1), group_norms [ngroups], seg_norms [nseg]), norms in float64."""
    with np.errstate(all='ignore'):
        x = np.asarray(g, dtype=np.float64) * np.float64(gscale)
        assert x.ndim == 1 and int(seg_end[-1]) == x.size
        seg_sq = np.array([np.sum(x[a:b] * x[a:b]) for a, b in segments(seg_end)], dtype=np.float64)
        grp = np.asarray(seg_group)
        group_sq = np.array([np.sum(seg_sq[grp == k]) for k in range(ngroups)], dtype=np.float64)
        total = np.sum(seg_sq)
        norm = np.sqrt(total)
        rate = np.float32(1.0)
        if threshold > 0:                      # chainer.optimizer.GradientClipping: rate = threshold / norm; if rate < 1: grad *= rate
            r = np.float64(threshold) / norm
            if r < 1:
                rate = np.float32(r)
        return dict(norm=norm, rate=rate, nonfinite=0 if np.isfinite(total) else 1, group_norms=np.sqrt(group_sq), seg_norms=np.sqrt(seg_sq))


def clipped(g, rate, gscale=1.0):
    """The gradient Adam sees, in float64: (g * gscale) * rate."""
    return (np.asarray(g, dtype=np.float64) * np.float64(gscale)) * np.float64(rate)


def guarded_adam_steps(p, grads, rates, gscale=1.0, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8):
    """Float64 Chainer Adam from zero state over the flat arrays grads[0], grads[1], ... clipped with rates[t] -> (p, m, v) after the last step."""
    P = {'x': np.asarray(p, dtype=np.float64).copy()}
    M, V = {'x': np.zeros_like(P['x'])}, {'x': np.zeros_like(P['x'])}
    for t, (g, rate) in enumerate(zip(grads, rates)):
        chainer_adam_step(P, {'x': clipped(g, rate, gscale)}, M, V, t + 1, alpha=alpha, beta1=beta1, beta2=beta2, eps=eps)
    return P['x'], M['x'], V['x']
