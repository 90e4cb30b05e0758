"""Thin callers of pivp_grad_stats / pivp_adam_step_guarded / pivp_adam_step on torch device tensors, for the GPU tests (like metrics_ops.py)."""
import math

import torch

from pivp_amd import _lib
from hip_ops import DEV, stream

HEAD = 3      # norm, rate, nonfinite in front of the group norms
FILL = -7.0   # what the outputs hold before a call: a call that returns BADARG must leave it there


def tables(seg_end, seg_group):
    return (torch.tensor([int(e) for e in seg_end], dtype=torch.int64, device=DEV),
            torch.tensor([int(k) for k in seg_group], dtype=torch.int32, device=DEV))


def grad_stats_rc(g, seg_end, seg_group, ngroups=6, gscale=1.0, threshold=0.0, null=(), **override):
    """g: device float32 tensor [n]; seg_end / seg_group: host lists -> (return code, stats as a NumPy array [3 + ngroups + nseg] out of a buffer
    pre-filled with FILL).  null: names among g / seg_end / seg_group / ws / stats passed as NULL; override: n / nseg / ngroups given to the call."""
    lib = _lib.load()
    n, nseg = g.numel(), len(seg_end)
    ends, groups = tables(seg_end, seg_group)
    nbytes = lib.pivp_grad_stats_ws_bytes(n, nseg)
    assert nbytes == ((n + 63) // 64 + nseg) * 8
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    stats = torch.full((HEAD + max(ngroups, 6) + nseg,), FILL, dtype=torch.float32, device=DEV)
    ptr = dict(g=g.data_ptr(), seg_end=ends.data_ptr(), seg_group=groups.data_ptr(), ws=ws.data_ptr(), stats=stats.data_ptr())
    for k in null:
        ptr[k] = None
    a = dict(n=n, nseg=nseg, ngroups=ngroups)
    a.update(override)
    rc = lib.pivp_grad_stats(ptr['g'], a['n'], ptr['seg_end'], ptr['seg_group'], a['nseg'], a['ngroups'], float(gscale), float(threshold),
                             ptr['ws'], ptr['stats'], stream())
    torch.cuda.synchronize()
    out = stats.cpu().numpy()
    return rc, (out[:HEAD + ngroups + nseg] if rc == 0 else out)      # a refused call: the whole pre-filled buffer


def grad_stats(g, seg_end, seg_group, ngroups=6, gscale=1.0, threshold=0.0):
    """-> dict(norm, rate, nonfinite, group_norms, seg_norms, raw) of float32 values as the kernel wrote them."""
    rc, s = grad_stats_rc(g, seg_end, seg_group, ngroups, gscale, threshold)
    _lib.check(rc, 'pivp_grad_stats')
    return dict(norm=s[0], rate=s[1], nonfinite=s[2], group_norms=s[HEAD:HEAD + ngroups], seg_norms=s[HEAD + ngroups:], raw=s)


def stats_buffer(rate=1.0, nonfinite=0.0):
    """A statistics buffer as pivp_adam_step_guarded reads it (only rate and nonfinite matter to it)."""
    return torch.tensor([0.0, rate, nonfinite], dtype=torch.float32, device=DEV)


def adam_guarded_rc(p, g, m, v, stats, t, skip_nonfinite=0, skipped=None, gscale=1.0, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8, null=(),
                    **override):
    """One guarded step on device tensors, in place; t: the 1-based step count (the host forms lr_t from it, as Adam.lr does)."""
    lib = _lib.load()
    lr_t = alpha * math.sqrt(1.0 - math.pow(beta2, t)) / (1.0 - math.pow(beta1, t))
    ptr = dict(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), stats=stats.data_ptr(),
               skipped=None if skipped is None else skipped.data_ptr())
    for k in null:
        ptr[k] = None
    a = dict(n=p.numel(), skip_nonfinite=skip_nonfinite)
    a.update(override)
    rc = lib.pivp_adam_step_guarded(ptr['p'], ptr['g'], ptr['m'], ptr['v'], a['n'], lr_t, beta1, beta2, eps, float(gscale), ptr['stats'],
                                    a['skip_nonfinite'], ptr['skipped'], stream())
    torch.cuda.synchronize()
    return rc


def adam_plain(p, g, m, v, t, gscale=1.0, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8):
    lib = _lib.load()
    lr_t = alpha * math.sqrt(1.0 - math.pow(beta2, t)) / (1.0 - math.pow(beta1, t))
    _lib.check(lib.pivp_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr_t, beta1, beta2, eps, float(gscale), stream()),
               'pivp_adam_step')
    torch.cuda.synchronize()
