"""Helpers for planning with `Model.imagine` (Finn & Levine 2017, "Deep visual foresight for planning robot motion"): designate pixels of the
current frame, roll the model forward under candidate action sequences, and score each candidate by where the model expects the pixels to end up.

Only the scoring is here; the optimiser over action sequences (CEM, MPPI) is the caller's.  Everything is plain torch on whatever device the
planes live on: the arithmetic that matters runs inside `imagine`."""
import numpy as np
import torch

from .model import Model


def one_hot_planes(coords, H, W, device=None):
    """coords (B, P, 2) integer (row, col) -> float32 planes (B, P, H, W), each zero but for a 1 at its pixel."""
    c = coords if torch.is_tensor(coords) else torch.from_numpy(np.array(coords))
    if c.dim() != 3 or c.shape[2] != 2:
        raise ValueError('coords must be (B, P, 2) of (row, col), got shape %s' % (tuple(c.shape),))
    if c.is_floating_point():
        if not bool((c == c.round()).all()):
            raise ValueError('coords must be whole pixels')
    c = c.to(torch.int64).cpu()
    r, q = c[..., 0], c[..., 1]
    if c.numel() and (int(r.min()) < 0 or int(r.max()) >= H or int(q.min()) < 0 or int(q.max()) >= W):
        raise ValueError('coords outside the %d x %d frame' % (H, W))
    B, P = c.shape[:2]
    planes = torch.zeros((B, P, H * W), dtype=torch.float32)
    planes.scatter_(2, (r * W + q).unsqueeze(2), 1.0)
    planes = planes.view(B, P, H, W)
    return planes.to(device) if device is not None else planes


def _as_planes(distrib):
    d = distrib if torch.is_tensor(distrib) else torch.as_tensor(np.asarray(distrib))
    if d.dim() < 2:
        raise ValueError('a distribution is (..., H, W), got shape %s' % (tuple(d.shape),))
    return d


def expected_position(distrib):
    """distrib (..., H, W), each plane summing to 1 (`imagine(..., normalize=True)`) -> (..., 2): the expected (row, col).
    The planes are taken as they are: an unnormalised plane gives mass * position."""
    d = _as_planes(distrib)
    H, W = d.shape[-2:]
    rows = torch.arange(H, dtype=d.dtype, device=d.device)
    cols = torch.arange(W, dtype=d.dtype, device=d.device)
    er = (d.sum(dim=-1) * rows).sum(dim=-1)
    ec = (d.sum(dim=-2) * cols).sum(dim=-1)
    return torch.stack((er, ec), dim=-1)


def expected_distance(distrib, goal_rc):
    """distrib (..., H, W) -> (...): sum over pixels of distrib * Euclidean distance (in pixels) from the pixel to goal_rc, a (row, col) pair or
    anything that broadcasts against (..., 2).  The cost of Finn & Levine 2017, eq. 2, for one designated pixel and one step."""
    d = _as_planes(distrib)
    H, W = d.shape[-2:]
    g = torch.as_tensor(np.asarray(goal_rc, dtype=np.float64) if not torch.is_tensor(goal_rc) else goal_rc).to(device=d.device, dtype=d.dtype)
    if g.shape[-1:] != (2,):
        raise ValueError('goal_rc must end in a (row, col) pair, got shape %s' % (tuple(g.shape),))
    rows = torch.arange(H, dtype=d.dtype, device=d.device).view(H, 1)
    cols = torch.arange(W, dtype=d.dtype, device=d.device).view(1, W)
    dist = torch.sqrt((rows - g[..., 0, None, None]) ** 2 + (cols - g[..., 1, None, None]) ** 2)
    return (d * dist).sum(dim=(-2, -1))


def score_actions(model, context_images, state, candidates, designated_rc, goal_rc):
    """Cost of K candidate action sequences for moving one designated pixel to a goal.

    context_images (ctx, 1, 3, H, W), state (1, 5): what the robot sees now; candidates (K, T-1, 5); designated_rc, goal_rc: (row, col) on the
    last context frame.  The context is replicated K times and ONE `imagine` runs at batch K with normalised distributions; the cost of
    candidate k is the sum over the predicted frames of `expected_distance` to the goal.  -> (K,) tensor on the model's device."""
    ctx_shape = Model._host_shape(context_images)
    if len(ctx_shape) != 5 or ctx_shape[1] != 1:
        raise ValueError('context_images must be (ctx, 1, 3, H, W), got shape %s' % (ctx_shape,))
    cand_shape = Model._host_shape(candidates)
    if len(cand_shape) != 3 or cand_shape[2] != 5 or cand_shape[0] < 1:
        raise ValueError('candidates must be (K, T-1, 5), got shape %s' % (cand_shape,))
    if Model._host_shape(state) != (1, 5):
        raise ValueError('state must be (1, 5), got shape %s' % (Model._host_shape(state),))
    K = cand_shape[0]
    H, W = ctx_shape[3:]
    to_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    ctx_k = to_t(context_images).expand(-1, K, -1, -1, -1)
    state_k = to_t(state).expand(K, -1)
    actions = to_t(candidates).transpose(0, 1)
    rc = np.asarray(designated_rc).reshape(1, 1, 2)
    planes = one_hot_planes(np.broadcast_to(rc, (K, 1, 2)), H, W)
    model.imagine(ctx_k, actions, state_k, designated=planes, normalize=True)
    return expected_distance(model.pixel_distrib[:, :, 0], goal_rc).sum(dim=0)
