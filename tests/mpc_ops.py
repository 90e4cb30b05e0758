"""NumPy-in / NumPy-out wrappers around pivp_cem_update_ex and pivp_cem_shift, for the GPU tests (like plan_ops.py)."""
import ctypes

import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, _t, stream


def cem_update_ex_rc(cost, actions, mean, std, best_actions, best_cost, low, high, t0, elites, alpha, min_std, seed, iteration, keep=0, kept_in=0,
                     add_mean=0, beta=0.0, null=None, **override):
    """One pivp_cem_update_ex on copies of the arrays -> (return code, dict(actions, mean, std, best_actions, best_cost, elites) or None), as
    plan_ops.cem_update_rc."""
    lib = _lib.load()
    steps, K, _ = np.shape(actions)
    d = dict(actions=_t(actions), mean=_t(mean), std=_t(std), best_actions=_t(best_actions), best_cost=_t(np.reshape(best_cost, (1,))),
             low=_t(np.broadcast_to(low, (5,))), high=_t(np.broadcast_to(high, (5,))))
    if cost is not None:
        d['cost'] = _t(cost)
    el = torch.full((max(int(elites), 1),), -1, dtype=torch.int32, device=DEV)
    ptr = {k: v.data_ptr() for k, v in d.items()}
    ptr.setdefault('cost', None)
    ptr['elites'] = el.data_ptr()
    if null is not None:
        ptr[null] = None
    n = dict(K=K, steps=steps)
    n.update(override)
    rc = lib.pivp_cem_update_ex(ptr['cost'], ptr['actions'], ptr['mean'], ptr['std'], ptr['best_actions'], ptr['best_cost'], ptr['low'], ptr['high'],
                                ptr['elites'], n['K'], n['steps'], int(t0), int(elites), float(alpha), float(min_std), ctypes.c_ulonglong(int(seed)),
                                int(iteration), int(keep), int(kept_in), int(add_mean), float(beta), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    out = {k: d[k].cpu().numpy() for k in ('actions', 'mean', 'std', 'best_actions')}
    out['best_cost'] = float(d['best_cost'].cpu().numpy()[0])
    out['elites'] = el.cpu().numpy()
    return rc, out


def cem_update_ex(*args, **kw):
    rc, out = cem_update_ex_rc(*args, **kw)
    _lib.check(rc, 'pivp_cem_update_ex')
    return out


def cem_shift_rc(mean, std, actions, best_actions, low, high, tail_mean, tail_std, std_floor, t0, keep, shift, best_cost=0.25, **override):
    """One pivp_cem_shift on copies -> (return code, dict(mean, std, actions, best_actions, best_cost) or None); actions / best_actions may be None."""
    lib = _lib.load()
    f5 = lambda v: _t(np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (5,))))
    d = dict(mean=_t(mean), std=_t(std), low=f5(low), high=f5(high), tail_mean=f5(tail_mean), tail_std=f5(tail_std), std_floor=f5(std_floor),
             best_cost=_t(np.reshape(np.float32(best_cost), (1,))))
    if actions is not None:
        d['actions'] = _t(actions)
    if best_actions is not None:
        d['best_actions'] = _t(best_actions)
    ptr = {k: v.data_ptr() for k, v in d.items()}
    ptr.setdefault('actions', None)
    ptr.setdefault('best_actions', None)
    n = dict(K=np.shape(actions)[1] if actions is not None else 1, steps=t0 + np.shape(mean)[0])
    n.update(override)
    rc = lib.pivp_cem_shift(ptr['mean'], ptr['std'], ptr['actions'], ptr['best_actions'], ptr['best_cost'], ptr['low'], ptr['high'], ptr['tail_mean'],
                            ptr['tail_std'], ptr['std_floor'], n['K'], n['steps'], int(t0), int(keep), int(shift), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    out = {k: (d[k].cpu().numpy() if k in d else None) for k in ('mean', 'std', 'actions', 'best_actions')}
    out['best_cost'] = float(d['best_cost'].cpu().numpy()[0])
    return rc, out


def cem_shift(*args, **kw):
    rc, out = cem_shift_rc(*args, **kw)
    _lib.check(rc, 'pivp_cem_shift')
    return out
