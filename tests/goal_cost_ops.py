"""NumPy-in / NumPy-out wrapper around pivp_goal_image_cost, for the GPU tests (like plan_ops.py)."""
import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, _t, stream

SENTINEL = -7.0


def _shifted(a, shift):
    """A device copy of `a` whose base lies `shift` floats behind a 16-byte boundary (torch's allocations are aligned far beyond 16 bytes)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    view = buf[shift:shift + a.size]
    view.copy_(torch.from_numpy(a.ravel()))
    return view


def goal_cost_rc(frames, goal, pixel_w, inv_norm, step_w, w_mse, w_l1, bad_cost, scale, cost_in=None, want_grad=True, shift=0, null=None, **override):
    """frames (S, K, 3, H, W), goal (G, 3, H, W) -> (return code, (cost, per_step, grad or None)); the outputs are returned on a bad return code too, so
    that their sentinel fill can be checked.  cost_in: accumulate onto it; shift: the big buffers' base in floats past 16 bytes; null: name of a pointer
    passed as NULL; override: S / K / H / W / G."""
    lib = _lib.load()
    S, K, _, H, W = frames.shape
    d = dict(frames=_shifted(frames, shift), goal=_shifted(goal, shift), step_w=_t(np.asarray(step_w, np.float32)),
             cost=torch.full((K,), SENTINEL, device=DEV) if cost_in is None else _t(np.asarray(cost_in, np.float32)),
             per_step=torch.full((S, K), SENTINEL, device=DEV))
    if pixel_w is not None:
        d['pixel_w'] = _shifted(pixel_w, shift)
    if want_grad:
        d['grad'] = torch.full((frames.size + 4,), SENTINEL, device=DEV)[shift:shift + frames.size]
    ptr = {k: v.data_ptr() for k, v in d.items()}
    ptr.setdefault('pixel_w', None)
    ptr.setdefault('grad', None)
    if null is not None:
        ptr[null] = None
    n = dict(S=S, K=K, H=H, W=W, G=goal.shape[0])
    n.update(override)
    rc = lib.pivp_goal_image_cost(ptr['frames'], ptr['goal'], n['G'], ptr['pixel_w'], float(inv_norm), ptr['step_w'], float(w_mse), float(w_l1),
                                  float(bad_cost), float(scale), 0 if cost_in is None else 1, ptr['cost'], ptr['per_step'], ptr['grad'], n['S'], n['K'],
                                  n['H'], n['W'], stream())
    torch.cuda.synchronize()
    grad = d['grad'].cpu().numpy().reshape(frames.shape) if want_grad else None
    return rc, (d['cost'].cpu().numpy(), d['per_step'].cpu().numpy(), grad)


def goal_cost(*args, **kw):
    rc, out = goal_cost_rc(*args, **kw)
    _lib.check(rc, 'pivp_goal_image_cost')
    return out
