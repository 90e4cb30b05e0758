"""A float64 NumPy restatement of pivp_goal_image_cost, written from the text of include/pivp_goal_cost.h alone; shared by
tests/test_goal_cost_host.py and tests/test_gpu_goal_cost.py."""
import numpy as np


def goal_image_cost(frames, goal, pixel_w, inv_norm, step_w, w_mse, w_l1, bad_cost, scale, cost_in=None, want_grad=True):
    """frames (S, K, 3, H, W), goal (G, 3, H, W) with G in (1, K), pixel_w (H, W) or None, step_w (S,) -> (cost (K,), per_step (S, K), grad or None).
    The scalars are taken at the float32 values the entry point receives; everything else is float64.  per_step is rounded to float32 (the
    header's single rounding) before the steps are folded; cost_in: the cost to accumulate onto (accumulate = 1), or None."""
    f = np.asarray(frames, dtype=np.float64)
    g = np.asarray(goal, dtype=np.float64)
    S, K, C, H, W = f.shape
    assert C == 3 and g.shape in ((1, 3, H, W), (K, 3, H, W))
    w = np.ones((H, W)) if pixel_w is None else np.asarray(pixel_w, dtype=np.float64)
    inv_norm, w_mse, w_l1, bad_cost, scale = (float(np.float32(v)) for v in (inv_norm, w_mse, w_l1, bad_cost, scale))
    sw = np.asarray(step_w, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        d = f - g[None]                                                        # G = 1 broadcasts over k
        per_step = (inv_norm * (w * (w_mse * d * d + w_l1 * np.abs(d))).sum(axis=(2, 3, 4))).astype(np.float32)
    bad = ~np.isfinite(per_step)
    per_step = np.where(bad, np.float32(bad_cost), per_step)
    total = np.zeros(K)
    for s in range(S):                                                         # s ascending, in double
        total += sw[s] * per_step[s].astype(np.float64)
    cost = (np.zeros(K) if cost_in is None else np.asarray(cost_in, dtype=np.float64)) + scale * total
    grad = None
    if want_grad:
        with np.errstate(invalid='ignore', over='ignore'):
            grad = scale * sw[:, None, None, None, None] * inv_norm * w * (2.0 * w_mse * d + w_l1 * np.sign(d))
        grad[bad] = 0.0
    return cost, per_step.astype(np.float64), grad


def inv_norm(pixel_w, H, W):
    """1 / (3 * sum(pixel_w)) in double, of the float32 weights; None: 1 / (3 H W)."""
    if pixel_w is None:
        return 1.0 / (3.0 * H * W)
    return 1.0 / (3.0 * float(np.asarray(pixel_w, dtype=np.float32).sum(dtype=np.float64)))


def spec_cost(frames, spec, want_grad=False):
    """The restatement under a `planning.GoalImageCost` (host-side fields only) -> (cost, per_step, grad)."""
    S = np.shape(frames)[0]
    goal = np.asarray(spec.goal_image if not hasattr(spec.goal_image, 'cpu') else spec.goal_image.cpu().numpy(), dtype=np.float64)
    goal = goal.reshape((-1,) + goal.shape[-3:])
    return goal_image_cost(frames, goal, spec.pixel_weight, spec.inv_norm(), spec.steps(S), spec.mse, spec.l1, spec.bad_cost, spec.weight,
                           want_grad=want_grad)
