"""NumPy-in / NumPy-out wrappers around pivp_plan_cost and pivp_cem_update, for the GPU tests (like track_ops.py)."""
import ctypes

import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, _t, stream


def plan_cost_rc(track, goals, step_w, plane_w, miss_cost, null=None, **override):
    """track (S, K, P, H, W) -> (return code, (cost, mass, edist) or None).  null: name of a pointer passed as NULL; override: S / K / P / H / W."""
    lib = _lib.load()
    S, K, P, H, W = track.shape
    d = dict(track=_t(track), goals=_t(np.asarray(goals).reshape(-1, 2)), step_w=_t(step_w), plane_w=_t(plane_w),
             cost=torch.full((K,), -7.0, device=DEV), mass=torch.full((S, K, P), -7.0, device=DEV), edist=torch.full((S, K, P), -7.0, device=DEV))
    ptr = {k: v.data_ptr() for k, v in d.items()}
    if null is not None:
        ptr[null] = None
    n = dict(S=S, K=K, P=P, H=H, W=W)
    n.update(override)
    rc = lib.pivp_plan_cost(ptr['track'], ptr['goals'], ptr['step_w'], ptr['plane_w'], float(miss_cost), ptr['cost'], ptr['mass'], ptr['edist'],
                            n['S'], n['K'], n['P'], n['H'], n['W'], stream())
    torch.cuda.synchronize()
    return rc, (tuple(d[k].cpu().numpy() for k in ('cost', 'mass', 'edist')) if rc == 0 else None)


def plan_cost(track, goals, step_w, plane_w, miss_cost):
    rc, out = plan_cost_rc(track, goals, step_w, plane_w, miss_cost)
    _lib.check(rc, 'pivp_plan_cost')
    return out


def cem_update_rc(cost, actions, mean, std, best_actions, best_cost, low, high, t0, elites, alpha, min_std, seed, iteration, null=None, **override):
    """One pivp_cem_update on copies of the arrays -> (return code, dict(actions, mean, std, best_actions, best_cost, elites) or None).
    cost None: the sample-only mode; override: K / steps."""
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
    rc = lib.pivp_cem_update(ptr['cost'], ptr['actions'], ptr['mean'], ptr['std'], ptr['best_actions'], ptr['best_cost'], ptr['low'], ptr['high'],
                             ptr['elites'], n['K'], n['steps'], int(t0), int(elites), float(alpha), float(min_std), ctypes.c_ulonglong(int(seed)),
                             int(iteration), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    out = {k: d[k].cpu().numpy() for k in ('actions', 'mean', 'std', 'best_actions')}
    out['best_cost'] = float(d['best_cost'].cpu().numpy()[0])
    out['elites'] = el.cpu().numpy()
    return rc, out


def cem_update(*args, **kw):
    rc, out = cem_update_rc(*args, **kw)
    _lib.check(rc, 'pivp_cem_update')
    return out
