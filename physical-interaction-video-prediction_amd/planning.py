"""Planning with `Model.imagine` (Finn & Levine 2017, "Deep visual foresight for planning robot motion"): designate pixels of the current frame,
roll the model forward under candidate action sequences, score each candidate by where the model expects the pixels to end up, and optimise the
action sequence.

`cem_plan` is the optimiser: the cross-entropy method over action sequences, on the device from the first sample to the returned plan.  Its loop
body is three stream-ordered calls -- pivp_cem_update (refit + Philox resample, one workgroup), pivp_rollout_predict (the rollout with raw
tracked planes) and pivp_plan_cost (expected distance to the goals, each plane read once) -- with every input uploaded before the loop, no host
synchronisation and no host-to-device copy inside it.  It knows about PAST actions: the steps before the last observed frame are fixed, only the
horizon is optimised (the MPC case).  `cem_refine` and `MPC` reach the same loop through the same checker, `_check_cem_args`: called by `cem_plan`'s
keywords, with `cem_plan`'s defaults, and returning one shape of checked values whoever asks.

`refine_actions` is the gradient-based counterpart: Adam on an action sequence, with d cost / d actions from the model's own backward sweep
(`Model.backward(input_grad=True, params=False, builtin_loss=False)`, include/pivp_input_grad.h) and any torch cost of the predicted frames.

`score_actions` scores a given set of candidates with one `imagine` and plain torch (`one_hot_planes`, `expected_position`,
`expected_distance`); it is kept as it was for callers that bring their own optimiser.

Closed-loop control: `cem_plan(..., belief=)` and `score_actions(..., belief=)` start every candidate from ONE recurrent state (`state.RecurrentState`,
what a `Model(carry_state=True)` holds after it has seen the frames so far) and the newest frame, instead of re-encoding the observed frames for every
candidate in every iteration.

Planning on a goal image: `GoalImageCost` specifies the task as a frame to reach (weighted squared / absolute error of the predicted frames, with an
optional region of interest and step weights); `goal_image_cost` is one call of pivp_goal_image_cost (include/pivp_goal_cost.h), value and gradient
on the device.  `cem_plan(goal_image=)`, `score_actions(goal_image=)` and `refine_actions(goal_image=)` share it, and `cem_refine` composes the two
optimisers on that one cost: CEM chooses a plan, gradient descent polishes it, the cheapest sequence is returned.

The closed loop: `MPC` plans once per control step from the model's belief, executes the first action and observes; the next plan starts from this
one moved on by one action (`PlanResult.warm_start`, pivp_cem_shift of include/pivp_mpc.h) and the designated pixels travel as the planes `imagine`
advected (`cem_plan(designated_planes=)`).  `cem_plan(keep_elites=, add_mean=, noise_beta=)` are the population options of iCEM (Pinneri et al. 2020)
in pivp_cem_update_ex; all default to off, and then `cem_plan` launches what it always did.

Gradient refinement from a belief: `refine_actions(belief=)` starts the rollout of every iteration from a `RecurrentState` instead of re-encoding context
frames from zeros -- in a closed loop those frames exist as the belief only -- and takes d cost / d actions from the sweep through that carried start,
the state a constant (`Model(carry_state=True, keep_activations=True, state_backward=True)`, include/pivp_state_grad.h).  `cem_refine(belief=)` composes
it with `cem_plan(belief=)`, and `MPC(refine_steps=)` runs that composition inside every `act()`, the polished plan entering the next step's warm start.
No new kernel and no new entry point: the existing rollout, sweep, cost and state-copy launches, in a new order.  All off by default."""
import contextlib
import ctypes
import inspect
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .model import Model, using_config
from .state import RecurrentState
from .state import _config as _state_config


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


def _check_belief(model, belief, ctx_shape, past_actions=None):
    """The complaints about `belief` (a batch-1 RecurrentState of the frames' size on a carry_state model, with ONE context frame and no past actions)."""
    if not isinstance(belief, RecurrentState):
        raise ValueError('belief must be a RecurrentState (Model.recurrent_state()), not %r' % (type(belief).__name__,))
    if not getattr(model, 'carry_state', False):
        raise ValueError('belief: the model must be built with carry_state=True')
    if belief.batch != 1:
        raise ValueError('belief must be a batch-1 state (what the robot believes now), this one holds %d samples' % belief.batch)
    if ctx_shape[0] != 1:
        raise ValueError('with a belief, context_images is (1, 1, 3, H, W): the newest frame only (the belief holds the frames before it), got shape %s'
                         % (ctx_shape,))
    if belief.hw != tuple(ctx_shape[3:]):
        raise ValueError('belief is of %dx%d frames, context_images of %dx%d' % (belief.hw + tuple(ctx_shape[3:])))
    if past_actions is not None and _host_array(past_actions, 'past_actions').size:
        raise ValueError('past_actions given with a belief: the belief has consumed the past steps, past_actions must be empty')


@contextlib.contextmanager
def _starting_from(model, state):
    """Inside: the model's carried recurrent state is `state` (taken as it is, not copied); behind it: what it was before.  None: the rollouts inside
    start from zeros and leave no state behind, on a carry_state model too -- planning from the context frames is the same with and without the flag."""
    if state is None:
        carries = getattr(model, 'carry_state', False)
        if carries:
            model.carry_state = False
        try:
            yield
        finally:
            if carries:
                model.carry_state = True
        return
    kept = model._state
    model._adopt_state(state)
    try:
        yield
    finally:
        model._state = kept


def score_actions(model, context_images, state, candidates, designated_rc, goal_rc, belief=None, goal_image=None):
    """Cost of K candidate action sequences for moving one designated pixel to a goal.

    belief: a batch-1 `RecurrentState` (carry_state=True models).  context_images is then (1, 1, 3, H, W), the newest frame only; `state` its robot
    state; candidates (K, horizon, action_dim).  The belief is expanded to K and every candidate runs `horizon` steps from it (`imagine(observed=1,
    advance=False)`); the model's own carried state is what it was afterwards.  None: the path below, with the bits it always had.

    context_images (ctx, 1, 3, H, W), state (1, state_dim): what the robot sees now; candidates (K, T-1, action_dim) -- the model's widths, 5 / 5
    unless it was built otherwise; designated_rc, goal_rc: (row, col) on the last context frame.  The context is replicated K times and ONE `imagine` runs at batch K with normalised distributions; the cost of
    candidate k is the sum over the predicted frames of `expected_distance` to the goal.  -> (K,) tensor on the model's device.

    goal_image: a `GoalImageCost` or a bare (3, H, W) array (its defaults): `goal_image_cost` of the predicted frames -- the cost `cem_plan(goal_image=)`
    ranks by -- is added to the pixel term, or, with designated_rc and goal_rc both None, returned instead of it (the rollout then runs without
    planes).  None: the path and the bits of a call without the argument."""
    ctx_shape = Model._host_shape(context_images)
    if len(ctx_shape) != 5 or ctx_shape[1] != 1:
        raise ValueError('context_images must be (ctx, 1, 3, H, W), got shape %s' % (ctx_shape,))
    if belief is not None:
        _check_belief(model, belief, ctx_shape)
    cand_shape = Model._host_shape(candidates)
    A, S = _widths(model)
    if len(cand_shape) != 3 or cand_shape[2] != A or cand_shape[0] < 1:
        raise ValueError('candidates must be (K, T-1, %d), got shape %s' % (A, cand_shape))
    if Model._host_shape(state) != (1, S):
        raise ValueError('state must be (1, %d), got shape %s' % (S, Model._host_shape(state)))
    K = cand_shape[0]
    H, W = ctx_shape[3:]
    image = _as_goal_cost(goal_image)
    pixels = designated_rc is not None or goal_rc is not None
    if image is not None:
        n_ctx = 1 if belief is not None else int(model.num_frame_before_prediction)
        if cand_shape[1] < n_ctx:
            raise ValueError('candidates cover %d steps; at least the %d context steps are needed' % (cand_shape[1], n_ctx))
        image.check_frames(cand_shape[1] - (n_ctx - 1), K, H, W)
    elif not pixels:
        raise ValueError('no goal: give designated_rc and goal_rc (a pixel to move), goal_image (a frame to reach), or both')
    to_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    ctx_k = to_t(context_images).expand(-1, K, -1, -1, -1)
    state_k = to_t(state).expand(K, -1)
    actions = to_t(candidates).transpose(0, 1)
    planes = None
    if pixels:
        rc = np.asarray(designated_rc).reshape(1, 1, 2)
        planes = one_hot_planes(np.broadcast_to(rc, (K, 1, 2)), H, W)
    with _starting_from(model, belief.expand(K) if belief is not None else None):
        if belief is not None:
            gen = model.imagine(ctx_k, actions, state_k, designated=planes, normalize=True, observed=1, advance=False)
        else:
            gen = model.imagine(ctx_k, actions, state_k, designated=planes, normalize=True)
    cost = expected_distance(model.pixel_distrib[:, :, 0], goal_rc).sum(dim=0) if pixels else None
    if image is not None:
        c_image = goal_image_cost(gen[n_ctx - 1:], image)[0]
        cost = c_image if cost is None else cost + c_image
    return cost


MAX_CEM_SAMPLES = 1024


def _widths(model):
    """(action_dim, state_dim) of a model; 5 / 5 for an object that does not say (the reference's data)."""
    return int(getattr(model, 'action_dim', 5)), int(getattr(model, 'state_dim', 5))


def _check_cem_widths(model):
    """The CEM kernels (pivp_cem_update / _ex / _shift, include/pivp_hip.h, include/pivp_mpc.h) carry [..][K][5] action rows and the five-column Philox
    pairing in their contract, and the planner's state buffers are laid out for five numbers: `cem_plan`, `cem_refine` and `MPC` serve 5 / 5 models."""
    A, S = _widths(model)
    if (A, S) != (5, 5):
        raise ValueError('the on-device CEM samples and refits five-column actions: a model with action_dim=%d, state_dim=%d is not served '
                         '(score_actions and refine_actions are, at any width)' % (A, S))


def _host_array(a, what):
    """An argument as a float64 NumPy array on the host (tensors included), for the checks and the one upload before the loop."""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    try:
        return np.asarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s must be numeric' % what)


def _pixel_coords(rc, what, H, W, whole):
    a = _host_array(rc, what)
    if a.ndim == 1 and a.shape == (2,):
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError('%s must be (P, 2) of (row, col), got shape %s' % (what, a.shape))
    if not 1 <= a.shape[0] <= Model.MAX_TRACK_PLANES:
        raise ValueError('%s holds %d pixels; 1 to %d are served' % (what, a.shape[0], Model.MAX_TRACK_PLANES))
    if not np.isfinite(a).all() or (whole and (a != np.round(a)).any()):
        raise ValueError('%s must be %s pixel coordinates' % (what, 'whole' if whole else 'finite'))
    if (a < 0).any() or (a[:, 0] > H - 1).any() or (a[:, 1] > W - 1).any():
        raise ValueError('%s outside the %d x %d frame' % (what, H, W))
    return a


def _per_step(a, what, horizon, default):
    """None | scalar | (5,) | (horizon, 5) -> (horizon, 5) float64."""
    if a is None:
        return np.full((horizon, 5), float(default))
    a = _host_array(a, what)
    if a.shape not in ((), (5,), (horizon, 5)):
        raise ValueError('%s must be a scalar, (5,) or (%d, 5), got shape %s' % (what, horizon, a.shape))
    if not np.isfinite(a).all():
        raise ValueError('%s must be finite' % what)
    return np.ascontiguousarray(np.broadcast_to(a, (horizon, 5)))


def _finite_number(v, what, low=None):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) \
            or abs(float(v)) > float(np.finfo(np.float32).max):      # (the library takes float32 scalars)
        raise ValueError('%s must be a finite number, not %r' % (what, v))
    if low is not None and v < low:
        raise ValueError('%s must be >= %g, not %r' % (what, low, v))
    return float(v)


def _whole_number(v, what, low, high=None):
    """-> int(v): an integer (a bool is none) with low <= v, and v <= high where there is one."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low or (high is not None and v > high):
        raise ValueError('%s must be an integer %s, not %r' % (what, '>= %d' % low if high is None else 'in [%d, %d]' % (low, high), v))
    return int(v)


def _five(v, what, default, infinite=False, dim=5):
    """None | scalar | (5,) -> (5,) float64, finite (infinite=True: anything but NaN): a per-dimension value of an action (dim: of another width)."""
    a = np.full(dim, float(default)) if v is None else _host_array(v, what)
    if a.shape not in ((), (dim,)) or np.isnan(a).any() or not (infinite or np.isfinite(a).all()):
        raise ValueError('%s must be a scalar or (%d,), %s, got shape %s' % (what, dim, 'without NaN' if infinite else 'finite', a.shape))
    return np.ascontiguousarray(np.broadcast_to(a, (dim,)))


def _action_box(low, high, low_name, high_name, dim=5):
    """Each of low, high: None (no bound) | scalar | (5,), no NaN, low <= high -> (low, high), both (5,) float64 (dim: of another action width)."""
    low, high = _five(low, low_name, -np.inf, infinite=True, dim=dim), _five(high, high_name, np.inf, infinite=True, dim=dim)
    if (low > high).any():
        raise ValueError('%s exceeds %s' % (low_name, high_name))
    return low, high


# ---- the goal-image cost (include/pivp_goal_cost.h): one op on the device for CEM, scoring and refinement -----------------------------------
class GoalImageCost(object):
    """The cost of predicted frames against a goal image, the other standard task specification of visual MPC (Finn & Levine 2017; Ebert et al. 2018):

        per_step[s][k] = sum_c sum_i pixel_weight[i] * (mse * d*d + l1 * |d|) / (3 * sum(pixel_weight)),   d = frame[s][k][c][i] - goal[c][i]
        cost[k]        = weight * sum_s step_weights[s] * per_step[s][k]

    (include/pivp_goal_cost.h).  A host-validated spec: every complaint is a ValueError raised here, before the GPU or the library is needed.
    goal_image: (3, H, W) -- or (B, 3, H, W), one goal per sample, for `refine_actions`; an array, or a tensor (taken where it lies).  mse, l1:
    finite, non-negative, not both zero.  pixel_weight: (H, W), finite, non-negative with a positive sum -- the region of interest; None: all ones.
    step_weights: (horizon,), finite; None: 1 / horizon each (the mean over the steps).  weight: the factor on the whole cost (what `cem_plan` adds
    to the pixel cost when both goals are given).  bad_cost: what a frame that is not finite (a diverged rollout) costs per step; default mse + l1,
    the cost of a frame that is off by 1 everywhere.  The defaults are `refine_actions`' bare goal_image cost."""

    def __init__(self, goal_image, mse=1.0, l1=0.0, pixel_weight=None, step_weights=None, weight=1.0, bad_cost=None):
        shape = Model._host_shape(goal_image)
        if len(shape) not in (3, 4) or shape[-3] != 3 or shape[-2] < 2 or shape[-1] < 2 or shape[0] < 1:
            raise ValueError('goal_image must be (3, H, W) or (B, 3, H, W), got shape %s' % (shape,))
        if torch.is_tensor(goal_image):
            if not goal_image.is_floating_point():
                raise ValueError('goal_image must be a floating-point tensor, not %s' % (goal_image.dtype,))
            self.goal_image = goal_image.detach()
        else:
            g = _host_array(goal_image, 'goal_image')
            if not np.isfinite(g).all():
                raise ValueError('goal_image must be finite')
            self.goal_image = np.ascontiguousarray(g, dtype=np.float32)
        self.shape = tuple(int(n) for n in shape)
        self.hw = self.shape[-2:]
        self.batch = self.shape[0] if len(shape) == 4 else None
        self.mse, self.l1 = _finite_number(mse, 'mse', 0.0), _finite_number(l1, 'l1', 0.0)
        if self.mse == 0.0 and self.l1 == 0.0:
            raise ValueError('mse and l1 are both zero: the cost is empty')
        self.pixel_weight = None
        if pixel_weight is not None:
            w = _host_array(pixel_weight, 'pixel_weight')
            if w.shape != self.hw:
                raise ValueError('pixel_weight must be (%d, %d), got shape %s' % (self.hw + (w.shape,)))
            if not np.isfinite(w).all() or (w < 0).any():
                raise ValueError('pixel_weight must be finite and non-negative')
            w = np.ascontiguousarray(w, dtype=np.float32)
            if not float(w.sum(dtype=np.float64)) > 0.0:
                raise ValueError('pixel_weight sums to zero: no pixel counts')
            self.pixel_weight = w
        self.step_weights = None
        if step_weights is not None:
            sw = _host_array(step_weights, 'step_weights')
            if sw.ndim != 1 or sw.shape[0] < 1 or not np.isfinite(sw).all():
                raise ValueError('step_weights must be finite and (horizon,), got shape %s' % (sw.shape,))
            self.step_weights = np.ascontiguousarray(sw, dtype=np.float32)
        self.weight = _finite_number(weight, 'weight')
        self.bad_cost = self.mse + self.l1 if bad_cost is None else _finite_number(bad_cost, 'bad_cost')
        if not math.isfinite(self.inv_norm()) or not np.float32(self.inv_norm()) > 0:
            raise ValueError('pixel_weight is too large or too small to normalise by in float32: its sum is %r' % (1.0 / (3.0 * self.inv_norm()),))

    def inv_norm(self):
        """1 / (3 * sum(pixel_weight)), in double (the weights as the device sees them, float32)."""
        if self.pixel_weight is None:
            return 1.0 / (3.0 * self.hw[0] * self.hw[1])
        return 1.0 / (3.0 * float(self.pixel_weight.sum(dtype=np.float64)))

    def steps(self, horizon):
        """-> the (horizon,) float32 step weights; ValueError if step_weights was given for another horizon."""
        if self.step_weights is None:
            return np.full(horizon, 1.0 / horizon, dtype=np.float32)
        if self.step_weights.shape != (horizon,):
            raise ValueError('the goal image\'s step_weights must be (%d,), got shape %s' % (horizon, self.step_weights.shape))
        return self.step_weights

    def check_frames(self, horizon, K, H, W, per_sample=False):
        """ValueError if (horizon, K, 3, H, W) frames cannot be scored against this goal.  per_sample: a (K, 3, H, W) goal is served."""
        if self.hw != (H, W):
            raise ValueError('goal_image is of %dx%d frames, the frames are %dx%d' % (self.hw + (H, W)))
        if self.batch is not None and not (per_sample and self.batch == K):
            raise ValueError('goal_image must be (3, %d, %d)%s, got shape %s' % (H, W, ' or (%d, 3, %d, %d)' % (K, H, W) if per_sample else '', self.shape))
        if W + 4 > 256 or H > 32768:
            raise ValueError('%dx%d frames: the goal-image cost serves widths up to 252 and heights up to 32768' % (H, W))
        self.steps(horizon)

    def __repr__(self):
        return 'GoalImageCost(goal_image=%s, mse=%g, l1=%g, pixel_weight=%s, step_weights=%s, weight=%g, bad_cost=%g)' % (
            self.shape, self.mse, self.l1, None if self.pixel_weight is None else self.hw,
            None if self.step_weights is None else self.step_weights.shape, self.weight, self.bad_cost)


def _as_goal_cost(goal_image, what='goal_image'):
    """None | GoalImageCost | a bare (3, H, W) array (the defaults) -> None | GoalImageCost."""
    if goal_image is None or isinstance(goal_image, GoalImageCost):
        return goal_image
    spec = GoalImageCost(goal_image)
    if spec.batch is not None:
        raise ValueError('%s must be (3, H, W), got shape %s' % (what, spec.shape))
    return spec


def _goal_upload(spec, horizon, dev):
    """The goal, the pixel weights and the step weights of `spec` on the device: uploaded ONCE, in front of whatever loop launches the op."""
    to_dev = lambda v: v.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(v) else torch.from_numpy(v).to(dev)
    return SimpleNamespace(spec=spec, goal=to_dev(spec.goal_image), G=spec.batch if spec.batch is not None else 1,
                           pixel_w=None if spec.pixel_weight is None else to_dev(spec.pixel_weight), step_w=to_dev(spec.steps(horizon)),
                           inv_norm=spec.inv_norm())


def _goal_launch(d, frames_ptr, S, K, H, W, cost_ptr, per_step_ptr, grad_ptr, accumulate, stream):
    """ONE pivp_goal_image_cost on the buffers of `_goal_upload` (the caller holds the device context)."""
    sp = d.spec
    _lib.check(_lib.load().pivp_goal_image_cost(frames_ptr, d.goal.data_ptr(), d.G, None if d.pixel_w is None else d.pixel_w.data_ptr(), d.inv_norm,
                                                d.step_w.data_ptr(), sp.mse, sp.l1, sp.bad_cost, sp.weight, int(accumulate), cost_ptr, per_step_ptr,
                                                grad_ptr, S, K, H, W, stream), 'pivp_goal_image_cost')


def goal_image_cost(frames, spec, want_grad=False):
    """The cost of predicted frames (S, K, 3, H, W), a float32 tensor on the device (`imagine`'s return value from the first predicted frame on),
    under the `GoalImageCost` spec: one pivp_goal_image_cost call (include/pivp_goal_cost.h), a thin wrapper as `losses.image_loss` is for its op.
    -> (cost (K,), per_step (S, K), grad (S, K, 3, H, W) = d cost[k] / d frames, or None).  The goal is (3, H, W) or (K, 3, H, W).  Stream-ordered
    on the frames' device; no host synchronisation (the spec's arrays are uploaded by this call: `cem_plan` and `refine_actions` do that once)."""
    if not isinstance(spec, GoalImageCost):
        raise ValueError('spec must be a GoalImageCost, not %r' % (spec,))
    if not torch.is_tensor(frames) or frames.dim() != 5 or frames.shape[2] != 3 or frames.dtype != torch.float32 or frames.shape[0] < 1 or frames.shape[1] < 1:
        raise ValueError('frames must be a float32 tensor (S, K, 3, H, W), got %s' % (tuple(frames.shape) if torch.is_tensor(frames) else type(frames).__name__,))
    S, K, _, H, W = frames.shape
    spec.check_frames(S, K, H, W, per_sample=True)
    if not frames.is_cuda:
        raise RuntimeError('frames must be on the GPU: this path has no CPU fallback')
    _lib.load()
    dev = frames.device
    with torch.cuda.device(dev):
        frames = frames.contiguous()
        d = _goal_upload(spec, S, dev)
        cost = torch.empty((K,), dtype=torch.float32, device=dev)
        per_step = torch.empty((S, K), dtype=torch.float32, device=dev)
        grad = torch.empty_like(frames) if want_grad else None
        _goal_launch(d, frames.data_ptr(), S, K, H, W, cost.data_ptr(), per_step.data_ptr(), grad.data_ptr() if want_grad else None, 0,
                     torch.cuda.current_stream(dev).cuda_stream)
    return cost, per_step, grad


MAX_COLORED_HORIZON = 64      # PIVP_CEM_MAX_COLORED_STEPS (include/pivp_mpc.h)
_BELIEF_TO_COME = object()      # stands for a batch-1 belief of the frames' size in `_check_cem_args`, where the belief itself does not exist yet


class PlanWarmStart(object):
    """What one planning call hands to the next (`cem_plan(warm=)`): the sampling distribution `mean`, `std` (horizon, 5) and the `kept`
    sequences (horizon, keep_elites, 5) or None, as float32 device tensors.  Made by a plan result's `warm_start()`."""

    def __init__(self, mean, std, kept=None):
        for name, t in (('mean', mean), ('std', std), ('kept', kept)):
            if t is None and name == 'kept':
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise ValueError('PlanWarmStart.%s must be a float32 tensor, not %r' % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if mean.dim() != 2 or mean.shape[1] != 5 or mean.shape[0] < 1 or std.shape != mean.shape:
            raise ValueError('PlanWarmStart: mean and std must both be (horizon, 5), got %s and %s' % (tuple(mean.shape), tuple(std.shape)))
        if kept is not None and (kept.dim() != 3 or kept.shape[0] != mean.shape[0] or kept.shape[2] != 5 or kept.shape[1] < 1):
            raise ValueError('PlanWarmStart: kept must be (%d, keep_elites, 5), got %s' % (mean.shape[0], tuple(kept.shape)))
        self.mean, self.std, self.kept = mean, std, kept

    def check(self, horizon, keep):
        """The complaints of `cem_plan(horizon=, keep_elites=, warm=self)`."""
        if self.mean.shape[0] != horizon:
            raise ValueError('warm holds a distribution over %d steps, horizon = %d' % (self.mean.shape[0], horizon))
        if self.kept is not None and self.kept.shape[1] != keep:
            raise ValueError('warm holds %d kept sequences, keep_elites = %d' % (self.kept.shape[1], keep))


class PlanResult(SimpleNamespace):
    """What `cem_plan` returns: the attributes its docstring lists, and the step to the next control step's plan."""

    def warm_start(self, shift=1, tail_mean=None, tail_std=None, std_floor=None):
        """The receding-horizon step: -> the `PlanWarmStart` of the next planning call, `shift` executed actions later.  mean, std and the kept
        sequences move up by `shift` rows (exact copies); the freed rows take tail_mean (default 0) / tail_std (default 1) -- the kept sequences
        tail_mean clamped to the action box --, and every std is raised to std_floor (default: tail_std, so that a distribution that has collapsed
        onto the last plan explores again).  Each of the three is a scalar or (5,), or a (5,) float32 device tensor, which is used as it is: with
        device tensors the call is one pivp_cem_shift on copies of this result's tensors and never synchronises.  This result is left unchanged."""
        Hh = int(self.mean.shape[0])
        shift = _whole_number(shift, 'shift (it stays below the horizon of %d)' % Hh, 1, Hh - 1)
        dev = self.mean.device
        vals = []
        for name, v, default in (('tail_mean', tail_mean, 0.0), ('tail_std', tail_std, 1.0), ('std_floor', std_floor, None)):
            if torch.is_tensor(v) and v.is_cuda:
                if v.dtype != torch.float32 or tuple(v.shape) != (5,):
                    raise ValueError('%s as a device tensor must be float32 (5,), got %s %s' % (name, v.dtype, tuple(v.shape)))
                vals.append(v.contiguous())
            elif v is None and default is None:
                vals.append(None)
            else:
                a = _five(v, name, default)
                if name != 'tail_mean' and (a < 0).any():
                    raise ValueError('%s must be non-negative' % name)
                vals.append(a)
        if vals[2] is None:
            vals[2] = vals[1]
        host = [i for i, v in enumerate(vals) if not torch.is_tensor(v)]
        if host:      # ONE host-to-device copy for what came from the host
            up = torch.from_numpy(np.concatenate([vals[i] for i in host]).astype(np.float32)).to(dev)
            for n, i in enumerate(host):
                vals[i] = up[5 * n:5 * n + 5]
        with torch.cuda.device(dev):
            mean, std = self.mean.clone(), self.std.clone()
            kept = self.kept.clone() if self.kept is not None else None
            keep = int(kept.shape[1]) if kept is not None else 0
            _lib.check(_lib.load().pivp_cem_shift(mean.data_ptr(), std.data_ptr(), kept.data_ptr() if keep else None, None, None, self._low.data_ptr(),
                                                  self._high.data_ptr(), vals[0].data_ptr(), vals[1].data_ptr(), vals[2].data_ptr(), max(keep, 1), Hh, 0,
                                                  keep, int(shift), self._model._stream()), 'pivp_cem_shift')
        return PlanWarmStart(mean, std, kept)


def _check_cem_args(model, context_images, state, *, designated_rc, goal_rc, horizon, past_actions, iterations, samples, elites, init_mean, init_std,
                    min_std, alpha, action_low, action_high, step_weights, plane_weights, miss_cost, chunk, seed, keep_elites, add_mean, noise_beta,
                    warm, designated_planes, belief, goal_image):
    """Every complaint of `cem_plan`, those about the closed-loop options (include/pivp_mpc.h) included, is a ValueError raised here, before the GPU
    or the library is needed.  Everything behind `state` goes by `cem_plan`'s keyword; what is left out takes `cem_plan`'s default (the line below
    `cem_plan` hands them over: they are written once, in its signature), and a name `cem_plan` does not have is a TypeError.
    -> the checked host-side values, the same attributes whoever asks -- `cem_plan`, `cem_refine` or `MPC.reset`.  With the options off keep,
    add_mean, beta, warm, planes, ex, belief and image are 0, False, 0.0, None, None, False, None and None; ex: the loop calls pivp_cem_update_ex."""
    _check_cem_widths(model)
    ctx = int(model.num_frame_before_prediction)
    si = Model._host_shape(context_images)
    if len(si) != 5 or si[1] != 1 or si[2] != 3:
        raise ValueError('context_images must be (ctx, 1, 3, H, W), got shape %s' % (si,))
    if belief is not None:      # one observed frame on top of the belief, whatever the model's context length
        if belief is _BELIEF_TO_COME:      # (`MPC.reset` checks its arguments before the frames that make the belief are consumed)
            if not getattr(model, 'carry_state', False):
                raise ValueError('belief: the model must be built with carry_state=True')
        else:
            _check_belief(model, belief, si, past_actions)
        ctx = 1
    if ctx < 1 or si[0] != ctx:
        raise ValueError('context_images holds %d frames, the model was built with num_frame_before_prediction=%d' % (si[0], ctx))
    H, W = si[3:]
    if H < 2 or W < 2:
        raise ValueError('context_images is empty: shape %s' % (si,))
    if Model._host_shape(state) != (1, 5):
        raise ValueError('state must be (1, 5), got shape %s' % (Model._host_shape(state),))
    if designated_planes is not None:
        if designated_rc is not None:
            raise ValueError('designated_planes and designated_rc are two forms of one argument: give one of them')
        sp = Model._host_shape(designated_planes)
        if len(sp) != 3 or sp[1:] != (H, W) or not 1 <= sp[0] <= Model.MAX_TRACK_PLANES:
            raise ValueError('designated_planes must be (P, H, W) of the frames\' size with 1 <= P <= %d, got shape %s for frames of shape %s'
                             % (Model.MAX_TRACK_PLANES, sp, si))
        if torch.is_tensor(designated_planes) and not designated_planes.is_floating_point():
            raise ValueError('designated_planes must be floating point, not %s' % (designated_planes.dtype,))
        if not (torch.is_tensor(designated_planes) and designated_planes.is_cuda):      # (a device tensor is taken as it is: looking at it would synchronise)
            host = _host_array(designated_planes, 'designated_planes')
            if not np.isfinite(host).all() or (host < 0).any():
                raise ValueError('designated_planes must be finite and non-negative')
        designated_rc = np.zeros((sp[0], 2))      # (P pixels as far as the checks of goal_rc and the weights are concerned)
    horizon, iterations, samples, elites = (_whole_number(v, name, 1) for name, v in (('horizon', horizon), ('iterations', iterations),
                                                                                      ('samples', samples), ('elites', elites)))
    if samples > MAX_CEM_SAMPLES:
        raise ValueError('samples = %d: the refit runs in one workgroup and serves at most %d' % (samples, MAX_CEM_SAMPLES))
    if elites > samples:
        raise ValueError('elites = %d exceeds samples = %d' % (elites, samples))
    chunk = samples if chunk is None else _whole_number(chunk, 'chunk', 1, samples)
    if samples % chunk:
        raise ValueError('chunk must divide samples = %d, not %r' % (samples, chunk))
    image = _as_goal_cost(goal_image)
    if image is not None:
        image.check_frames(horizon, samples, H, W)
    pixels = designated_rc is not None or goal_rc is not None
    if not pixels and image is None:
        raise ValueError('no goal: give designated_rc and goal_rc (pixels to move), goal_image (a frame to reach), or both')
    if pixels:
        designated = _pixel_coords(designated_rc, 'designated_rc', H, W, whole=True)
        goals = _pixel_coords(goal_rc, 'goal_rc', H, W, whole=False)
        P = designated.shape[0]
        if goals.shape[0] != P:
            raise ValueError('goal_rc holds %d goals for %d designated pixels' % (goals.shape[0], P))
    else:      # a goal image alone: the rollouts run without planes and pivp_plan_cost is not called
        if plane_weights is not None or miss_cost is not None or step_weights is not None:
            raise ValueError('plane_weights, miss_cost and step_weights belong to the designated pixels: without designated_rc / goal_rc they must be '
                             'None (the goal image has its own step_weights, in its GoalImageCost)')
        designated, goals, P = np.zeros((0, 2)), np.zeros((0, 2)), 0
    if ctx > 1:
        if past_actions is None:
            raise ValueError('past_actions (%d, 5) is required with %d context frames: the actions taken between the observed frames' % (ctx - 1, ctx))
        past = _host_array(past_actions, 'past_actions')
        if past.shape != (ctx - 1, 5) or not np.isfinite(past).all():
            raise ValueError('past_actions must be finite and (%d, 5), got shape %s' % (ctx - 1, past.shape))
    else:
        if past_actions is not None and _host_array(past_actions, 'past_actions').size:
            raise ValueError('past_actions given, but with one context frame there is no past step')
        past = np.zeros((0, 5))
    mean = _per_step(init_mean, 'init_mean', horizon, 0.0)
    std = _per_step(init_std, 'init_std', horizon, 1.0)
    if (std < 0).any():
        raise ValueError('init_std must be non-negative')
    min_std, alpha = _finite_number(min_std, 'min_std', 0.0), _finite_number(alpha, 'alpha', 0.0)
    if alpha > 1:
        raise ValueError('alpha must lie in [0, 1], not %r' % (alpha,))
    low, high = _action_box(action_low, action_high, 'action_low', 'action_high')
    weights = []
    for name, v, n in (('step_weights', step_weights, horizon), ('plane_weights', plane_weights, P)):
        a = np.ones(n) if v is None else _host_array(v, name)
        if a.shape != (n,) or not np.isfinite(a).all():
            raise ValueError('%s must be finite and (%d,), got shape %s' % (name, n, a.shape))
        weights.append(a)
    miss_cost = _finite_number(math.sqrt((H - 1) ** 2 + (W - 1) ** 2) if miss_cost is None else miss_cost, 'miss_cost')
    seed = _whole_number(seed, 'seed', 0, 2 ** 64 - 1)
    keep = _whole_number(keep_elites, 'keep_elites (at most elites)', 0, elites)
    if not isinstance(add_mean, (bool, np.bool_)):
        raise ValueError('add_mean must be a bool, not %r' % (add_mean,))
    if keep + int(add_mean) > samples:
        raise ValueError('keep_elites = %d and the mean need %d slots, samples = %d' % (keep, keep + 1, samples))
    beta = _finite_number(noise_beta, 'noise_beta', low=0.0)
    if beta > 0 and horizon > MAX_COLORED_HORIZON:
        raise ValueError('noise_beta > 0 is served for a horizon of at most %d steps, not %d' % (MAX_COLORED_HORIZON, horizon))
    if warm is not None:
        if not isinstance(warm, PlanWarmStart):
            raise ValueError('warm must be a PlanWarmStart (a plan result\'s warm_start()), not %r' % (type(warm).__name__,))
        warm.check(horizon, keep)
    return SimpleNamespace(ctx=ctx, H=H, W=W, P=P, K=samples, M=elites, chunk=chunk, horizon=horizon, iterations=iterations, designated=designated,
                           goals=goals, past=past, mean=mean, std=std, low=low, high=high, step_w=weights[0], plane_w=weights[1], miss_cost=miss_cost,
                           min_std=min_std, alpha=alpha, seed=seed, keep=keep, add_mean=bool(add_mean), beta=beta, warm=warm, planes=designated_planes,
                           ex=bool(keep or add_mean or beta > 0 or warm is not None), belief=belief, image=image)


def cem_plan(model, context_images, state, designated_rc, goal_rc, horizon, past_actions=None, iterations=3, samples=32, elites=8, init_mean=None,
             init_std=1.0, min_std=1e-3, alpha=0.0, action_low=None, action_high=None, step_weights=None, plane_weights=None, miss_cost=None,
             chunk=None, seed=0, trace=False, keep_elites=0, add_mean=False, noise_beta=0.0, warm=None, designated_planes=None, belief=None,
             goal_image=None):
    """Cross-entropy-method planning of `horizon` actions that move P designated pixels to their goals, entirely on the model's device.

    context_images (ctx, 1, 3, H, W), state (1, 5): what the robot sees now; designated_rc (P, 2) whole (row, col) pixels of the LAST context frame,
    goal_rc (P, 2) where each should go (1 <= P <= 8); past_actions (ctx-1, 5): the actions taken between the observed frames, required when
    ctx > 1 -- rows t < ctx-1 of every candidate are these, rows ctx-1 .. ctx-2+horizon are optimised (T-1 = ctx-1 + horizon).

    Per iteration `samples` candidates are drawn from N(mean, std) per (step, action dimension), clamped to [action_low, action_high], rolled
    out by `imagine`'s rollout at batch `chunk` (default: all at once; samples % chunk == 0) and scored by
    cost = sum_steps step_weights[s] * sum_planes plane_weights[p] * E[distance of plane (s, p) to goal p], with `miss_cost` (default: the frame
    diagonal) for a plane that lost all its mass; the `elites` cheapest refit the distribution: mean = alpha * mean + (1 - alpha) * elite mean,
    std likewise, floored at min_std.  init_mean / init_std: scalar, (5,) or (horizon, 5).  The same seed gives the same bits.

    -> an object with `actions` (horizon, 5), the best sequence ever evaluated, and its `cost`; the final `mean`, `std` (horizon, 5);
    `best_cost_per_iteration` (iterations,); and, with trace=True, `trace`: per iteration a dict of `actions` (T-1, samples, 5), `cost` (samples,),
    `elites` (elites,) int32 best first, `mass` and `edist` (horizon, samples, P).  All device tensors; nothing is synchronised.

    belief: a batch-1 `RecurrentState` -- what a `Model(carry_state=True)` holds after the frames observed so far (`model.recurrent_state()`).
    context_images is then (1, 1, 3, H, W), the newest frame only, `state` its robot state, and past_actions must be empty: the belief has consumed the
    past.  It is expanded ONCE to the chunk size, in front of the loop, and every rollout runs `horizon` steps from it (`imagine`'s observed=1,
    advance=False) instead of ctx-1 + horizon from zeros; the model's own carried state is what it was afterwards.  None: the path and the bits of
    a call without the argument.  (Belief and no-belief planning agree to rounding, not bit for bit: the observing steps ran at another batch size.)

    goal_image: a `GoalImageCost`, or a bare (3, H, W) array which gets its defaults -- the task as a frame to reach.  Each chunk's frames are then
    scored by ONE pivp_goal_image_cost call (include/pivp_goal_cost.h) behind the rollout, on the stream.  designated_rc and goal_rc may then both be
    None: the rollouts run without planes, pivp_plan_cost is not called, cost = the image cost (plane_weights, miss_cost and step_weights must be None; `mass` /
    `edist` are (horizon, samples, 0)).  With both kinds of goal pivp_plan_cost writes cost first and the image cost accumulates weight * its value
    onto it; `step_weights` weighs the pixel term, the image term has its own in the spec.  trace=True: each record also holds `image_cost`
    (horizon, samples), the per-step image costs.  The goal and its weights are uploaded once, in front of the loop.  None: the launches and the bits
    of a call without the argument.

    Closed-loop options (include/pivp_mpc.h; all off by default, and then the loop calls pivp_cem_update and returns the bits it always did):
    keep_elites: the best `keep_elites` (<= elites) candidates of an iteration stay in the population, slots 0 .. keep_elites-1 in rank order, and are
    scored again beside the new samples.  add_mean: the slot behind them holds the clamped mean instead of a sample.  noise_beta > 0: each candidate's
    noise is correlated over the horizon (power-law spectrum f^-beta, unit variance per step; horizon <= 64).  warm: a `PlanWarmStart` -- the
    previous control step's result moved on by `warm_start()` -- whose mean / std replace init_mean / init_std and whose kept sequences enter slots
    0 .. keep_elites-1 of the first iteration as they are.  The result's `kept` (horizon, keep_elites, 5) holds the final update's best sequences,
    and its `warm_start(shift=1, ...)` returns the next call's `PlanWarmStart` through one pivp_cem_shift.
    designated_planes: (P, H, W) non-negative planes on the last context frame, instead of designated_rc -- the distribution a designated pixel
    has become after the robot moved (`imagine`'s planes).  Expanded to the chunk size once, in front of the loop; one-hot planes give the bits of
    designated_rc.  A device tensor is used as it is (its values are not inspected: that would synchronise).

    Side effect: the rollouts run on `model` as `imagine` does, so afterwards `model.gen_images` / `gen_states` hold the LAST rollout (the last
    chunk of the last iteration), `pixel_distrib` / `pixel_mass` are None and `backward()` raises until the model is called again.  With
    chunk < samples every rollout copies its slice of the action buffer and allocates its own frames, on the stream, without a host round trip."""
    a = _check_cem_args(model, context_images, state, designated_rc=designated_rc, goal_rc=goal_rc, horizon=horizon, past_actions=past_actions,
                        iterations=iterations, samples=samples, elites=elites, init_mean=init_mean, init_std=init_std, min_std=min_std, alpha=alpha,
                        action_low=action_low, action_high=action_high, step_weights=step_weights, plane_weights=plane_weights, miss_cost=miss_cost,
                        chunk=chunk, seed=seed, keep_elites=keep_elites, add_mean=add_mean, noise_beta=noise_beta, warm=warm,
                        designated_planes=designated_planes, belief=belief, goal_image=goal_image)
    with torch.cuda.device(model.device) if torch.cuda.is_available() else contextlib.nullcontext():
        return _cem_iterate(model, a, _cem_upload(model, a, context_images, state), trace)


# the checker's keywords default to what `cem_plan`'s do (tests/test_goal_cost_host.py compares the two signatures)
_check_cem_args.__kwdefaults__ = {n: q.default for n, q in inspect.signature(cem_plan).parameters.items() if q.default is not q.empty and n != 'trace'}


def _cem_upload(model, a, context_images, state):
    """Everything the loop reads or writes, uploaded or built ONCE: -> the device buffers of one `cem_plan` call."""
    model._require_gpu()
    dev = model.device
    H, W, P, K, M, C, Hh = a.H, a.W, a.P, a.K, a.M, a.chunk, a.horizon
    t0, steps = a.ctx - 1, a.ctx - 1 + Hh
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    b = SimpleNamespace()
    b.context = model._as_device(context_images, ()).expand(-1, C, -1, -1, -1).contiguous()
    b.state = model._as_device(state, (5,)).expand(C, -1).contiguous()
    # the small arrays travel in ONE host-to-device copy; the buffers below are views of it
    parts = [('goals', a.goals), ('step_w', a.step_w), ('plane_w', a.plane_w), ('low', a.low), ('high', a.high), ('mean', a.mean), ('std', a.std),
             ('past', a.past), ('pixel', a.designated[:, 0] * W + a.designated[:, 1])]
    packed = torch.from_numpy(np.concatenate([np.asarray(v, dtype=np.float32).ravel() for _, v in parts])).to(dev)
    at = 0
    for name, v in parts:
        setattr(b, name, packed[at:at + np.size(v)].view(np.shape(v)))
        at += np.size(v)
    b.planes = None
    if a.planes is not None:      # the designated pixels as distributions: expanded to the chunk size here, once
        b.planes = model._as_device(a.planes, (H, W)).view(1, P, H, W).expand(C, P, H, W).contiguous()
    elif P:
        b.planes = torch.zeros((C, P, H * W), dtype=torch.float32, device=dev)
        b.planes.scatter_(2, b.pixel.to(torch.int64).view(1, P, 1).expand(C, P, 1), 1.0)      # one-hot planes, built on the device (H * W < 2^24: exact)
        b.planes = b.planes.view(C, P, H, W)
    b.image = None
    if a.image is not None:      # the goal image and its weights: uploaded here, read by every pivp_goal_image_cost of the loop
        b.image = _goal_upload(a.image, Hh, dev)
        b.image_cost = new(Hh, K)
        b.image_part = new(Hh, C) if C != K else None      # a chunk's per-step costs: [Hh][C] is not a slice of [Hh][K]
    b.actions = torch.zeros((steps, K, 5), dtype=torch.float32, device=dev)
    if t0:
        b.actions[:t0] = b.past.unsqueeze(1)
    b.best_actions, b.best_cost = new(Hh, 5), new(1)
    b.per_iter, b.cost, b.mass, b.edist = new(a.iterations), new(K), new(Hh, K, P), new(Hh, K, P)
    b.part = (new(Hh, C, P), new(Hh, C, P)) if C != K else None      # a chunk's moments: [Hh][C][P] is not a slice of [Hh][K][P]
    b.elite_idx = torch.empty((M,), dtype=torch.int32, device=dev)
    model._ensure_params(H, W)
    b.belief = None
    if a.belief is not None:      # ONE expansion to the chunk size (pivp_state_copy); every rollout of the loop reads it and leaves it untouched
        model._checked_state(a.belief)
        b.belief = a.belief.expand(C)
    model._plan_for(C, steps + 1, H, W, keep_activations=False, observed=1 if b.belief is not None else None)      # sized and bound here, not inside the loop
    _cem_arm(b, a, a.warm)
    return b


def _cem_arm(b, a, start):
    """The buffers as the first update of a `_cem_iterate` must find them.  start: a `PlanWarmStart` -- its mean / std are copied into b.mean / b.std
    (the loop writes into them) and its kept sequences, if any, into slots 0 .. keep-1, with `kept_in` saying so -- or None: the initial values
    `_cem_upload` put there.  No best sequence yet.  Device-to-device copies and fills only: `MPC.act` calls it once per control step."""
    if start is not None:
        b.mean.copy_(start.mean)
        b.std.copy_(start.std)
    b.kept_in = int(a.keep > 0 and start is not None and start.kept is not None)
    if b.kept_in:
        b.actions[a.ctx - 1:, :a.keep].copy_(start.kept)
    b.best_actions.zero_()
    b.best_cost.fill_(float('inf'))


def _cem_iterate(model, a, b, trace=False, iterations=None, seed=None, ex=None):
    """The loop of `cem_plan` on the buffers of `_cem_upload`: pivp_cem_update, the rollout, pivp_plan_cost and / or pivp_goal_image_cost --
    stream-ordered launches and device-to-device copies only (tests/test_gpu_planning.py runs it under torch's sync debug mode).  iterations, seed,
    ex: what differs from one `MPC.act` to the next on the same checked values and buffers; None: a.iterations, a.seed, a.ex."""
    lib = _lib.load()
    P, K, M, C, Hh = a.P, a.K, a.M, a.chunk, a.horizon
    t0, steps = a.ctx - 1, a.ctx - 1 + Hh
    iterations, seed, ex = (own if given is None else given for given, own in ((iterations, a.iterations), (seed, a.seed), (ex, a.ex)))
    stream = model._stream()

    def update(have_cost, it):
        shared = (b.cost.data_ptr() if have_cost else None, b.actions.data_ptr(), b.mean.data_ptr(), b.std.data_ptr(), b.best_actions.data_ptr(),
                  b.best_cost.data_ptr(), b.low.data_ptr(), b.high.data_ptr(), b.elite_idx.data_ptr(), K, steps, t0, M, a.alpha, a.min_std,
                  ctypes.c_ulonglong(seed), it)
        if ex:      # kept elites, the mean as a candidate, colored noise or a warm start: include/pivp_mpc.h
            _lib.check(lib.pivp_cem_update_ex(*shared, a.keep, 0 if have_cost else b.kept_in, int(a.add_mean), a.beta, stream), 'pivp_cem_update_ex')
        else:
            _lib.check(lib.pivp_cem_update(*shared, stream), 'pivp_cem_update')

    belief, image = b.belief, b.image
    from_belief = dict(observed=1, advance=False) if belief is not None else {}
    records = []
    with _starting_from(model, belief):      # (the expanded belief, read by every rollout and written by none; None: every rollout from zeros)
        for it in range(iterations):
            update(it > 0, it)
            if it > 0:
                b.per_iter[it - 1:it].copy_(b.best_cost)
                if trace:
                    records[-1]['elites'] = b.elite_idx.clone()
            for k0 in range(0, K, C):
                gen, track = model._rollout_predict(b.context, b.actions if C == K else b.actions[:, k0:k0 + C].contiguous(), b.state, b.planes, t0,
                                                  **from_belief)
                if P:
                    m_out, e_out = (b.mass, b.edist) if C == K else b.part
                    _lib.check(lib.pivp_plan_cost(track.data_ptr(), b.goals.data_ptr(), b.step_w.data_ptr(), b.plane_w.data_ptr(), a.miss_cost,
                                                  b.cost.data_ptr() + 4 * k0, m_out.data_ptr(), e_out.data_ptr(), Hh, C, P, a.H, a.W, stream),
                               'pivp_plan_cost')
                    if C != K and trace:
                        b.mass[:, k0:k0 + C].copy_(m_out)
                        b.edist[:, k0:k0 + C].copy_(e_out)
                if image is not None:      # the frames from the first predicted one on; onto the pixel cost where there is one
                    i_out = b.image_cost if C == K else b.image_part
                    _goal_launch(image, gen[t0:].data_ptr(), Hh, C, a.H, a.W, b.cost.data_ptr() + 4 * k0, i_out.data_ptr(), None, 1 if P else 0, stream)
                    if C != K and trace:
                        b.image_cost[:, k0:k0 + C].copy_(i_out)
            if trace:
                records.append(dict(actions=b.actions.clone(), cost=b.cost.clone(), mass=b.mass.clone(), edist=b.edist.clone()))
                if image is not None:
                    records[-1]['image_cost'] = b.image_cost.clone()
        update(True, iterations)      # the last candidates count too: best_*, mean and std reflect them (the resampled rows are not used)
        b.per_iter[iterations - 1:].copy_(b.best_cost)
        if trace:
            records[-1]['elites'] = b.elite_idx.clone()
    return PlanResult(actions=b.best_actions, cost=b.best_cost[0], mean=b.mean, std=b.std, best_cost_per_iteration=b.per_iter,
                      trace=records if trace else None, kept=b.actions[t0:, :a.keep].contiguous() if a.keep else None, _model=model, _low=b.low,
                      _high=b.high)


# ---- gradient-based refinement of an action sequence ---------------------------------------------------------------------------------------
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8      # refine_actions' Adam: the optimizer's defaults (optimizer.Adam)


def _adam_lr_t(lr, t, beta1=ADAM_BETA1, beta2=ADAM_BETA2):
    """The bias-corrected step size of Adam's update t = 1, 2, ... (optimizer.Adam.lr), formed on the host in double."""
    return lr * math.sqrt(1.0 - math.pow(beta2, t)) / (1.0 - math.pow(beta1, t))


def _adam_launch(model, p, g, m, v, lr_t):
    """ONE pivp_adam_step on the flat buffers p, g, m, v (same numel), on the model's stream."""
    _lib.check(_lib.load().pivp_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr_t, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                                          1.0, model._stream()), 'pivp_adam_step')


REFINE_BELIEF_FLAGS = ('carry_state', 'keep_activations', 'state_backward')      # what a model needs to back-propagate a rollout from a belief


def _check_refine_model(model, what):
    """The complaints about the model that refines from a belief: the three flags, each by its name, and one context frame."""
    for flag in REFINE_BELIEF_FLAGS:
        if not getattr(model, flag, False):
            raise ValueError('%s: the sweep runs through a rollout that started from a carried recurrent state, the model must be built with '
                             'carry_state=True, keep_activations=True, state_backward=True; %s=True is missing' % (what, flag))
    if int(model.num_frame_before_prediction) != 1:
        raise ValueError('%s: the model must be built with num_frame_before_prediction=1, not %d (the belief stands for every frame before the '
                         'newest one, and the training rollout feeds ground truth for its own context frames only)'
                         % (what, int(model.num_frame_before_prediction)))


def _check_refine_belief(model, belief, ctx_shape, past_actions):
    """The complaints of `refine_actions(belief=)`: a `RecurrentState` of batch 1 or B at the frames' size (or `_BELIEF_TO_COME`, which stands for a
    batch-1 one), a model that can sweep from it, the newest frame alone as context and no past actions."""
    if belief is not _BELIEF_TO_COME and not isinstance(belief, RecurrentState):
        raise ValueError('belief must be a RecurrentState (Model.recurrent_state()), not %r' % (type(belief).__name__,))
    _check_refine_model(model, 'refining from a belief')
    if ctx_shape[0] != 1:
        raise ValueError('with a belief, context_images is (1, B, 3, H, W): the newest frame only (the belief holds the frames before it), got shape %s'
                         % (ctx_shape,))
    if past_actions is not None:
        raise ValueError('past_actions given with a belief: the belief has consumed the past steps, there is none between context frames')
    if belief is _BELIEF_TO_COME:
        return
    if belief.batch not in (1, ctx_shape[1]):
        raise ValueError('belief must be a state of batch 1 (shared by every sample) or %d (one per sample), this one holds %d samples'
                         % (ctx_shape[1], belief.batch))
    if belief.hw != tuple(ctx_shape[3:]):
        raise ValueError('belief is of %dx%d frames, context_images of %dx%d' % (belief.hw + tuple(ctx_shape[3:])))


def _check_refine_args(model, context_images, state, actions, goal_image, cost_fn, steps, lr, past_actions, bounds, belief=None):
    """Every complaint of `refine_actions` is a ValueError raised here, before the GPU or the library is needed.  -> the checked host-side values."""
    ctx = int(model.num_frame_before_prediction)
    si = Model._host_shape(context_images)
    if len(si) != 5 or si[2] != 3 or si[1] < 1:
        raise ValueError('context_images must be (ctx, B, 3, H, W), got shape %s' % (si,))
    if belief is not None:
        _check_refine_belief(model, belief, si, past_actions)
    if ctx < 1 or si[0] != ctx:
        raise ValueError('context_images holds %d frames, the model was built with num_frame_before_prediction=%d' % (si[0], ctx))
    B, H, W = si[1], si[3], si[4]
    if H < 2 or W < 2:
        raise ValueError('context_images is empty: shape %s' % (si,))
    A, S = _widths(model)
    if Model._host_shape(state) != (B, S):
        raise ValueError('state must be (%d, %d), got shape %s' % (B, S, Model._host_shape(state)))
    sa = Model._host_shape(actions)
    if len(sa) != 3 or sa[1] != B or sa[2] != A or sa[0] < ctx:
        raise ValueError('actions must be (T-1, %d, %d) with T-1 >= %d (one action per rollout step, the steps between the context frames included), '
                         'got shape %s' % (B, A, ctx, sa))
    if not getattr(model, 'keep_activations', False):
        raise ValueError('refine_actions back-propagates through the rollout: the model needs keep_activations=True')
    if getattr(model, '_extra_loss', False):
        raise ValueError('refine_actions differentiates its own cost alone: the model must not carry an image loss')
    if (goal_image is None) == (cost_fn is None):
        raise ValueError('exactly one of goal_image and cost_fn must be given')
    if cost_fn is not None and not callable(cost_fn):
        raise ValueError('cost_fn must be callable: cost_fn(gen (T-ctx, B, 3, H, W)) -> (B,)')
    if isinstance(goal_image, GoalImageCost):
        goal_image.check_frames(sa[0] + 1 - ctx, B, H, W, per_sample=True)
    elif goal_image is not None:
        sg = Model._host_shape(goal_image)
        if sg not in ((3, H, W), (B, 3, H, W)):
            raise ValueError('goal_image must be (3, %d, %d) or (%d, 3, %d, %d), got shape %s' % (H, W, B, H, W, sg))
    steps, lr = _whole_number(steps, 'steps', 1), _finite_number(lr, 'lr', 0.0)
    n_past = 0
    if past_actions is not None:
        sp = Model._host_shape(past_actions)
        if ctx < 2 or sp not in ((ctx - 1, A), (ctx - 1, B, A)):
            raise ValueError('past_actions must be (%d, %d) or (%d, %d, %d): the actions taken between the %d observed frames, got shape %s'
                             % (ctx - 1, A, ctx - 1, B, A, ctx, sp))
        n_past = ctx - 1
    low = high = None
    if bounds is not None:
        if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
            raise ValueError('bounds must be a pair (low, high)')
        low, high = _action_box(bounds[0], bounds[1], 'bounds[0]', 'bounds[1]', dim=A)
    return SimpleNamespace(ctx=ctx, B=B, H=H, W=W, steps_T=sa[0], n_past=n_past, iters=steps, lr=lr, low=low, high=high, belief=belief)


def refine_actions(model, context_images, state, actions, goal_image=None, cost_fn=None, steps=10, lr=0.05, past_actions=None, bounds=None,
                   belief=None):
    """Gradient descent (Adam) on an action sequence, with the gradient from the model's own backward sweep.

    context_images (ctx, B, 3, H, W), state (B, 5): what each of B robots sees now; actions (T-1, B, 5): the sequence to start from, one action per
    rollout step (rows t < ctx-1 are the steps between the context frames) -- every 5 here is the model's action_dim, or state_dim for `state`.
    past_actions (ctx-1, 5) or (ctx-1, B, 5): when given, those first rows
    are set to it and held fixed (the MPC case: they have been executed); None: every row is free (explaining an observed video).

    Per iteration: ONE feed-self training-mode rollout (`model(...)` under config.train with scheduled sampling off, whatever the model's
    scheduled_sampling_k is; the frames after the context are zeros and play no part), the cost of the predictions gen = gen_images[ctx-1:]
    (T-ctx, B, 3, H, W) in torch -- cost_fn(gen) -> (B,), differentiated by autograd, or, with goal_image (3, H, W) / (B, 3, H, W), the squared error
    to it averaged over steps and pixels; a `GoalImageCost` as goal_image takes value and gradient from one pivp_goal_image_cost call instead (the
    cost `cem_plan(goal_image=)` ranks by; its defaults are the bare array's cost, to rounding) --, `backward(frame_grad=d sum(cost) / d gen, input_grad=True, params=False, builtin_loss=False)`, the past
    rows of the gradient zeroed, ONE pivp_adam_step on the flat action buffer (beta1 0.9, beta2 0.999, eps 1e-8, its own moments, the bias-corrected
    step size formed on the host) and the clamp to bounds = (low, high), each a scalar, (5,) or None.  Stream-ordered launches only: nothing
    synchronises with the host.  A last rollout scores the returned sequence.

    -> (actions (T-1, B, 5), costs (steps + 1, B)): the refined sequence and the cost of every sample in front of each update and behind the last;
    device tensors.  lr = 0 returns the input's bits.

    It knows nothing of `cem_plan`; refining CEM's plan on the cost that chose it is `cem_refine`, in short

        spec = GoalImageCost(goal)
        plan = cem_plan(model, context, state, None, None, horizon, past_actions=past, goal_image=spec)
        seq = torch.cat((torch.as_tensor(past, dtype=torch.float32, device=plan.actions.device).view(-1, 5), plan.actions)).unsqueeze(1)
        refined, costs = refine_actions(model, context, state, seq, goal_image=spec, past_actions=past)

    (`model`: built with keep_activations=True.)  Side effect: the model holds the last rollout; its parameter gradients are
    unspecified afterwards (`cleargrads()` before training on).

    belief: a `RecurrentState` of batch 1 or B at the frames' size -- what a carrying model holds after the frames observed so far
    (`model.recurrent_state()`), the closed-loop case, where those frames exist as the belief only.  The model must be built with carry_state=True,
    keep_activations=True, state_backward=True and num_frame_before_prediction=1; context_images is then (1, B, 3, H, W), the newest frame alone,
    `state` its robot state, actions (horizon, B, 5) with every row free, and past_actions must be None: the belief has consumed the past.  A
    batch-1 belief is expanded to B ONCE, in front of the loop (`RecurrentState.expand`, one pivp_state_copy); the rollout of every iteration starts
    from it -- a buffer hand-over, no copy -- and the sweep takes it as a constant (the truncated form of include/pivp_state_grad.h), so d cost /
    d actions is that of `horizon` steps from the belief instead of ctx-1 + horizon from zeros.  The belief is never written, and the model's own
    carried state is, bit for bit, what it was on entry: on return, and when an exception leaves the loop (`imagine(advance=False)`'s manners).
    None: the path, the launches and the bits of a call without the argument."""
    a = _check_refine_args(model, context_images, state, actions, goal_image, cost_fn, steps, lr, past_actions, bounds, belief)
    with torch.cuda.device(model.device) if torch.cuda.is_available() else contextlib.nullcontext():
        return _refine_iterate(model, a, _refine_upload(model, a, context_images, state, actions, goal_image, past_actions), cost_fn)


def _refine_upload(model, a, context_images, state, actions, goal_image, past_actions):
    """Everything the loop reads or writes, uploaded or built ONCE: -> the device buffers of one `refine_actions` call."""
    model._require_gpu()
    dev = model.device
    T = a.steps_T + 1
    b = SimpleNamespace()
    b.images = torch.zeros((T, a.B, 3, a.H, a.W), dtype=torch.float32, device=dev)
    b.images[:a.ctx] = model._as_device(context_images, ())
    A, S = _widths(model)
    b.states = torch.zeros((T, a.B, S), dtype=torch.float32, device=dev)
    b.states[0] = model._as_device(state, (S,))
    b.actions = torch.zeros((T, a.B, A), dtype=torch.float32, device=dev)      # (the rollout's action tensor is (T, B, A); row T-1 is never read)
    b.actions[:T - 1] = model._as_device(actions, (A,))
    if a.n_past:
        past = model._as_device(past_actions, (A,))
        b.actions[:a.n_past] = past if past.dim() == 3 else past.unsqueeze(1)
    b.goal, b.goal_cost = None, None
    if isinstance(goal_image, GoalImageCost):      # the spec's goal and weights: uploaded here, read by the loop's one pivp_goal_image_cost per iteration
        b.goal_cost = _goal_upload(goal_image, T - a.ctx, dev)
    elif goal_image is not None:
        b.goal = model._as_device(goal_image, ())
    to_dev = lambda v: None if v is None else torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev)
    b.low, b.high = to_dev(a.low), to_dev(a.high)
    b.belief = b.landing = None
    if getattr(a, 'belief', None) is not None:      # ONE expansion to the batch (pivp_state_copy); every rollout of the loop starts from it and leaves it untouched
        model._ensure_params(a.H, a.W)
        model._checked_state(a.belief)
        b.belief = a.belief.expand(a.B) if a.belief.batch != a.B else a.belief
        b.landing = RecurrentState.empty(a.B, (a.H, a.W), dev)      # where those rollouts leave their final state: nobody reads it
    return b


@contextlib.contextmanager
def _rollouts_from(model, start, landing):
    """Inside: calling what this yields in front of a training rollout makes that rollout start from `start` -- handed over, not copied -- and leave
    its final state in `landing`, so `start` is never written (a state_backward model writes the final state into its spare buffer, the sweep reads
    the start again).  Behind it, an exception included: the model's carried state and its spare are the objects they were, untouched.  The model
    keeps `start` alive for the sweep of the last rollout.  start None: what is yielded does nothing and the model is not touched."""
    if start is None:
        yield lambda: None
        return
    kept = model._state, model._spare_state

    def put_back():
        model._adopt_state(start)
        model._spare_state = landing
    try:
        yield put_back
    finally:
        model._state, model._spare_state = kept
        model._swept_start = start


def _refine_iterate(model, a, b, cost_fn=None, adam=_adam_launch):
    """The loop of `refine_actions` on its device buffers: rollout, cost, sweep, Adam -- stream-ordered work only (tests/test_gpu_input_grad.py runs it
    under torch's sync debug mode).  b.belief (when `_refine_upload` made one): the state every rollout starts from, a constant of every sweep.
    b.moments / b.costs (when the caller made them, as `MPC.reset` does): Adam's moments and the cost table, instead of fresh ones."""
    T1, t0 = a.steps_T, a.n_past
    p = b.actions[:T1]                    # the optimised buffer: a contiguous prefix
    if getattr(b, 'moments', None) is not None:
        m, v = b.moments
        m.zero_()
        v.zero_()
        costs = b.costs
    else:
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        costs = torch.empty((a.iters + 1, a.B), dtype=torch.float32, device=p.device)
    nf = T1 + 1 - a.ctx

    def rollout_cost(want_grad):
        k = model.scheduled_sampling_k
        model.scheduled_sampling_k = -1
        put_start_back()
        try:
            with using_config('train', True):
                model([b.images, b.actions, b.states])
        finally:
            model.scheduled_sampling_k = k
        gen = model._gen[a.ctx - 1:]
        spec = b.goal_cost
        if cost_fn is None and spec is not None:      # a GoalImageCost: value and d sum(cost) / d gen from ONE op call (include/pivp_goal_cost.h)
            c = torch.empty((a.B,), dtype=torch.float32, device=gen.device)
            per_step = torch.empty((nf, a.B), dtype=torch.float32, device=gen.device)
            grad = torch.empty_like(gen) if want_grad else None
            _goal_launch(spec, gen.data_ptr(), nf, a.B, a.H, a.W, c.data_ptr(), per_step.data_ptr(), grad.data_ptr() if want_grad else None, 0,
                         torch.cuda.current_stream(gen.device).cuda_stream)
            return c, grad
        if cost_fn is None:      # mean over steps and pixels of the squared error, per sample; its gradient in closed form
            diff = gen - b.goal
            return (diff * diff).mean(dim=(0, 2, 3, 4)), (diff * (2.0 / (nf * 3 * a.H * a.W)) if want_grad else None)
        if not want_grad:
            with torch.no_grad():
                return cost_fn(gen), None
        leaf = gen.detach().requires_grad_(True)
        c = cost_fn(leaf)
        if not torch.is_tensor(c) or tuple(c.shape) != (a.B,):
            raise ValueError('cost_fn must return a (%d,) tensor, got %s' % (a.B, tuple(c.shape) if torch.is_tensor(c) else type(c).__name__))
        grad, = torch.autograd.grad(c.sum(), leaf)
        return c.detach(), grad

    with _rollouts_from(model, getattr(b, 'belief', None), getattr(b, 'landing', None)) as put_start_back:
        for it in range(a.iters):
            c, grad = rollout_cost(True)
            costs[it].copy_(c)
            model.backward(frame_grad=grad.to(torch.float32).contiguous(), input_grad=True, params=False, builtin_loss=False)
            g = model.action_grad
            if t0:
                g[:t0].zero_()
            adam(model, p, g, m, v, _adam_lr_t(a.lr, it + 1))
            if b.low is not None:
                free = p[t0:]
                torch.maximum(free, b.low, out=free)
                torch.minimum(free, b.high, out=free)
        costs[a.iters].copy_(rollout_cost(False)[0])
        return p, costs


def cem_refine(model, context_images, state, horizon, goal_image, past_actions=None, refine_steps=10, lr=0.05, belief=None, **cem_arguments):
    """CEM on a goal image, then gradient refinement of its plan on the SAME cost: `cem_plan(goal_image=)` and `refine_actions(goal_image=)` share one
    `GoalImageCost`, so the polish descends the objective that chose the plan.

    model: built with keep_activations=True (the rollouts of CEM run on its inference plan, refinement on its training plan); context_images
    (ctx, 1, 3, H, W), state (1, 5), past_actions (ctx-1, 5) as `cem_plan` takes them; goal_image: a `GoalImageCost` or a bare (3, H, W) array.
    cem_arguments: `cem_plan`'s keywords (iterations, samples, elites, init_mean, init_std, min_std, alpha, action_low, action_high, chunk, seed,
    trace).  The pixel goals and the closed-loop options are not served here.

    belief: a batch-1 `RecurrentState`, the closed-loop case -- CEM runs as `cem_plan(belief=)` does and the refinement as `refine_actions(belief=)`
    does, both from this one belief and on the one cost.  The model must then be built with carry_state=True, keep_activations=True,
    state_backward=True and num_frame_before_prediction=1; context_images is (1, 1, 3, H, W), the newest frame, and past_actions must be None.
    The model's own carried state is what it was afterwards.  None: the path and the bits of a call without the argument.

    After CEM, `refine_actions` runs `refine_steps` Adam steps of size `lr` at batch 2, from CEM's best sequence and from its final mean, the past
    actions held fixed and CEM's action bounds passed as `bounds`.  The cheapest of the three sequences -- CEM's best (0), the refined best (1), the
    refined mean (2) -- is returned, picked by argmin / index_select on the device: nothing synchronises with the host.

    -> an object with `actions` (horizon, 5), `cost`, `source` (0 / 1 / 2, an int64 scalar tensor), `cem` (what `cem_plan` returned) and
    `refine_costs` (refine_steps + 1, 2).  `cost` is never above `cem.cost`.  (The refined costs come from training-plan rollouts, CEM's from
    inference-plan rollouts of the same weights: the two agree to rounding, so does `score_actions(goal_image=)` on the returned actions.)"""
    a = _check_cem_refine_args(model, context_images, state, horizon, goal_image, past_actions, refine_steps, lr, cem_arguments, belief)
    with torch.cuda.device(model.device) if torch.cuda.is_available() else contextlib.nullcontext():
        return _cem_refine_iterate(model, a, _cem_refine_upload(model, a, context_images, state))


def _check_cem_refine_args(model, context_images, state, horizon, goal_image, past_actions, refine_steps, lr, cem_arguments, belief=None):
    """Every complaint of `cem_refine` is a ValueError (an unknown keyword: a TypeError) raised here, before the GPU or the library is needed.
    -> the checked values of its two stages: `cem` (`_check_cem_args`) and `refine` (`_check_refine_args` at batch 2)."""
    if not getattr(model, 'keep_activations', False):
        raise ValueError('cem_refine back-propagates through the rollout: the model needs keep_activations=True')
    for name in ('designated_rc', 'goal_rc', 'step_weights', 'plane_weights', 'miss_cost'):
        if cem_arguments.get(name) is not None:
            raise ValueError('cem_refine plans and refines on the goal image alone: %s is not served' % name)
    if belief is not None:
        if not isinstance(belief, RecurrentState):
            raise ValueError('belief must be a RecurrentState (Model.recurrent_state()), not %r' % (type(belief).__name__,))
        if past_actions is not None:
            raise ValueError('past_actions given with a belief: the belief has consumed the past steps, past_actions must be None')
    for name in ('keep_elites', 'add_mean', 'noise_beta', 'warm', 'designated_planes'):
        v = cem_arguments.get(name)
        if v is not None and not (isinstance(v, (bool, int, float, np.bool_, np.integer, np.floating)) and not v):
            raise ValueError('cem_refine does not serve the closed-loop option %s' % name)
    if goal_image is None:
        raise ValueError('cem_refine needs a goal_image')
    spec = _as_goal_cost(goal_image)      # (one goal per sample is `_check_cem_args`' complaint)
    kw = dict(cem_arguments, designated_rc=None, goal_rc=None, horizon=horizon, past_actions=past_actions, goal_image=spec, belief=belief)
    trace = kw.pop('trace', False)
    cem = _check_cem_args(model, context_images, state, **kw)      # (what was refused above is None or off, as the checker's defaults are)
    shaped = lambda *shape: np.broadcast_to(np.float32(0), shape)      # the refinement's arguments exist on the device only: their shapes are checked
    low, high = kw.get('action_low'), kw.get('action_high')
    refine = _check_refine_args(model, shaped(cem.ctx, 2, 3, cem.H, cem.W), shaped(2, 5), shaped(cem.ctx - 1 + cem.horizon, 2, 5), spec, None, refine_steps,
                                lr, cem.past if cem.ctx > 1 else None, None if low is None and high is None else (low, high), belief)
    return SimpleNamespace(cem=cem, refine=refine, spec=spec, trace=bool(trace))


def _cem_refine_upload(model, a, context_images, state):
    """Everything both stages read or write, uploaded or built ONCE: `_cem_upload`'s buffers and `_refine_upload`'s at batch 2 (the two starting
    sequences are written by the loop; the past rows are set here)."""
    cem = _cem_upload(model, a.cem, context_images, state)
    context2 = model._as_device(context_images, ()).expand(-1, 2, -1, -1, -1)
    state2 = model._as_device(state, (5,)).expand(2, -1)
    starts = torch.zeros((a.refine.steps_T, 2, 5), dtype=torch.float32, device=model.device)
    refine = _refine_upload(model, a.refine, context2, state2, starts, a.spec, cem.past if a.refine.n_past else None)
    return SimpleNamespace(cem=cem, refine=refine)


def _cem_refine_iterate(model, a, b):
    """`cem_refine` on its device buffers: `_cem_iterate`, two device-to-device copies of the starting sequences, `_refine_iterate`, the choice --
    stream-ordered work only."""
    plan = _cem_iterate(model, a.cem, b.cem, a.trace)
    t0, T1 = a.cem.ctx - 1, a.refine.steps_T
    b.refine.actions[t0:T1, 0].copy_(plan.actions)
    b.refine.actions[t0:T1, 1].copy_(plan.mean)
    refined, costs = _refine_iterate(model, a.refine, b.refine)
    three_costs = torch.cat((plan.cost.view(1), costs[-1]))
    three = torch.cat((plan.actions.unsqueeze(0), refined[t0:].transpose(0, 1)))      # (3, horizon, 5)
    source = torch.argmin(three_costs)
    pick = source.view(1)
    return SimpleNamespace(actions=three.index_select(0, pick)[0], cost=three_costs.index_select(0, pick)[0], source=source, cem=plan,
                           refine_costs=costs)


# ---- the closed loop: plan, execute the first action, observe, plan again --------------------------------------------------------------------
class MPC(object):
    """Visual model-predictive control (Finn & Levine 2017; Ebert et al. 2018) around `cem_plan`: per control step ONE planning call from the
    model's belief, warm-started by the previous step's plan moved on by one action.

        ctl = MPC(model, horizon=8, goal_rc=[[40, 24]], samples=32, elites=8)      # model = Model(..., carry_state=True)
        ctl.reset(context_images, state0, past_actions, designated_rc=[[32, 32]])
        while True:
            action = ctl.act()                          # (5,) on the device
            frame, state = robot.step(action)           # the world
            ctl.observe(frame, state)                   # the belief, the designated pixels and the plan move on

    model observes: it carries the recurrent state of the frames seen so far (carry_state=True).  planner (default: model) runs the candidates'
    rollouts from that state and must carry too; a second model with the same weights in another precision serves, the batch-1 observing steps
    being fp32 only.  The goal is goal_rc (P, 2) for the pixels `reset(designated_rc=)` designates, goal_image (a `GoalImageCost` or a bare frame),
    or both.  horizon >= 2.  iterations, samples, elites, init_mean, init_std, min_std, alpha, action_low, action_high, step_weights, plane_weights,
    miss_cost, chunk, keep_elites, add_mean and noise_beta are `cem_plan`'s keywords, with its defaults.  The first `act()` after a `reset()` plans cold with `iterations`;
    later ones start from the shifted plan and run `warm_iterations` (default 1).  tail_mean / tail_std (scalar or (5,); default: the last row of
    init_mean / init_std) fill the step that enters the horizon, std_floor (default: tail_std) is the least std a warm start samples with.
    renormalize: the designated planes are divided by their mass after every observed step (a plane that lost all mass stays zero).  The plan of
    control step i uses seed + i.

    refine_steps > 0 (with goal_image, and without goal_rc: the pixel cost has no backward, and descending one part of the ranked cost could raise the
    total): behind CEM, every `act()` polishes the plan by gradient descent, as `cem_refine(belief=)` does -- the belief is expanded to batch 2 into
    `refiner` (one pivp_state_copy), `refine_steps` Adam steps of size `refine_lr` run from the plan's best sequence and from its mean under the
    controller's action bounds (`refine_actions(belief=)`'s loop), and the cheapest of the three sequences -- CEM's best (0), the refined best (1),
    the refined mean (2) -- is picked on the device.  It becomes the plan's `actions` / `cost`, and, with keep_elites >= 1, kept sequence 0 when it is
    a refined one: the next control step's warm start carries the polish on.  `last_plan` then also holds `source` and `refine_costs`
    (refine_steps + 1, 2).  refiner (default: model) must be built with carry_state=True, keep_activations=True, state_backward=True and
    num_frame_before_prediction=1; a second model serves, as for `planner`, and has to be loaded from the same checkpoint as `model`: the belief
    it starts from was encoded by `model`'s weights.  refine_steps=0, the default: the launches and the bits of a controller without the keyword.

    After `reset()`, `act()` and `observe()` enqueue launches and device-to-device copies only -- given device tensors, they never synchronise
    with the host (`reset()` does the uploads, once)."""

    CEM_ARGUMENTS = ('iterations', 'samples', 'elites', 'init_mean', 'init_std', 'min_std', 'alpha', 'action_low', 'action_high', 'step_weights',
                     'plane_weights', 'miss_cost', 'chunk', 'keep_elites', 'add_mean', 'noise_beta')      # `cem_plan`'s, with its defaults

    def __init__(self, model, horizon, goal_image=None, goal_rc=None, warm_iterations=1, tail_mean=None, tail_std=None, std_floor=None,
                 renormalize=True, seed=0, planner=None, refine_steps=0, refine_lr=0.05, refiner=None, **cem_arguments):
        planner = model if planner is None else planner
        refine_steps, refine_lr = _whole_number(refine_steps, 'refine_steps', 0), _finite_number(refine_lr, 'refine_lr', 0.0)
        if refine_steps:
            if goal_image is None:
                raise ValueError('MPC: refine_steps > 0 descends the goal-image cost: give goal_image')
            if goal_rc is not None:
                raise ValueError('MPC: refine_steps > 0 is not served with goal_rc: the pixel cost has no backward, and descending only the image '
                                 'part of the ranked cost could raise the total')
            refiner = model if refiner is None else refiner
            _check_refine_model(refiner, 'MPC: refiner (refine_steps > 0)')
            if getattr(refiner, '_extra_loss', False):
                raise ValueError('MPC: refiner differentiates the goal-image cost alone: it must not carry an image loss')
        for name, m in (('model', model), ('planner', planner)):
            if not getattr(m, 'carry_state', False):
                raise ValueError('MPC: %s must be a Model built with carry_state=True (the belief is its carried recurrent state)' % name)
        unknown = sorted(set(cem_arguments) - set(self.CEM_ARGUMENTS))
        if unknown:
            raise TypeError('MPC got unexpected keyword arguments %s' % (unknown,))
        horizon, warm_iterations = _whole_number(horizon, 'horizon', 2), _whole_number(warm_iterations, 'warm_iterations', 1)
        if not isinstance(renormalize, (bool, np.bool_)):
            raise ValueError('renormalize must be a bool, not %r' % (renormalize,))
        seed = _whole_number(seed, 'seed', 0, 2 ** 63 - 1)
        if goal_image is None and goal_rc is None:
            raise ValueError('no goal: give goal_rc (where the designated pixels should go), goal_image (a frame to reach), or both')
        init_mean, init_std = cem_arguments.get('init_mean'), cem_arguments.get('init_std')      # (None: `cem_plan`'s 0 and 1, as `_per_step` fills them)
        self.tail_mean = _five(tail_mean, 'tail_mean', 0.0) if tail_mean is not None else _per_step(init_mean, 'init_mean', horizon, 0.0)[-1]
        self.tail_std = _five(tail_std, 'tail_std', 1.0) if tail_std is not None else _per_step(init_std, 'init_std', horizon, 1.0)[-1]
        self.std_floor = _five(std_floor, 'std_floor', 0.0) if std_floor is not None else self.tail_std
        if (self.tail_std < 0).any() or (self.std_floor < 0).any():
            raise ValueError('tail_std and std_floor must be non-negative')
        self.model, self.planner, self.horizon, self.goal_image, self.goal_rc = model, planner, horizon, goal_image, goal_rc
        self.warm_iterations, self.renormalize, self.seed = warm_iterations, bool(renormalize), seed
        self.refine_steps, self.refine_lr, self.refiner = refine_steps, refine_lr, refiner if refine_steps else None
        # what every plan of this controller is checked with, by `cem_plan`'s keywords; `reset` adds the planes, the belief stands for the one to come
        self._plan_arguments = dict(cem_arguments, designated_rc=None, goal_rc=goal_rc, horizon=horizon, goal_image=goal_image, seed=seed,
                                    belief=_BELIEF_TO_COME)
        self._b = None
        self.step, self.last_plan = 0, None

    def _check_reset_args(self, context_images, state, past_actions, designated_rc):
        """Every complaint of `reset` is a ValueError raised here, before the GPU or the library is needed.  -> the checked host-side values."""
        si = Model._host_shape(context_images)
        if len(si) != 5 or si[0] < 1 or si[1] != 1 or si[2] != 3:
            raise ValueError('context_images must be (n, 1, 3, H, W) with n >= 1 observed frames, got shape %s' % (si,))
        n, _, _, H, W = si
        if Model._host_shape(state) != (1, 5):
            raise ValueError('state must be (1, 5): the robot state of the first frame, got shape %s' % (Model._host_shape(state),))
        past = np.zeros((0, 5)) if past_actions is None else _host_array(past_actions, 'past_actions')
        if past.size == 0:
            past = past.reshape(0, 5)
        if past.shape != (n - 1, 5) or not np.isfinite(past).all():
            raise ValueError('past_actions must be finite and (%d, 5): the actions taken between the %d observed frames, got shape %s'
                             % (n - 1, n, past.shape))
        if (designated_rc is None) != (self.goal_rc is None):
            raise ValueError('designated_rc goes with goal_rc: the controller was built %s goal_rc' % ('without' if self.goal_rc is None else 'with'))
        planes = None
        if designated_rc is not None:
            planes = one_hot_planes(_pixel_coords(designated_rc, 'designated_rc', H, W, whole=True)[None], H, W)      # (1, P, H, W), on the host
        frame = np.empty((1, 1, 3, H, W), np.float32)      # (the checks below look at the newest frame's shape alone)
        a = _check_cem_args(self.planner, frame, state, designated_planes=planes[0] if planes is not None else None, **self._plan_arguments)
        refine = None
        if self.refine_steps:      # the polish at batch 2: its arguments exist on the device only, their shapes are checked (as `cem_refine` does)
            shaped = lambda *shape: np.broadcast_to(np.float32(0), shape)
            low, high = self._plan_arguments.get('action_low'), self._plan_arguments.get('action_high')
            refine = _check_refine_args(self.refiner, shaped(1, 2, 3, H, W), shaped(2, 5), shaped(a.horizon, 2, 5), a.image, None, self.refine_steps,
                                        self.refine_lr, None, None if low is None and high is None else (low, high), _BELIEF_TO_COME)
        return SimpleNamespace(n=n, H=H, W=W, past=past, planes=planes, cem=a, refine=refine)


    def reset(self, context_images, state, past_actions=None, designated_rc=None):
        """A new episode.  context_images (n, 1, 3, H, W): the n >= 1 frames observed so far, state (1, 5) the robot state of the FIRST of them,
        past_actions (n-1, 5) the actions taken between them; designated_rc (P, 2): whole (row, col) pixels of the NEWEST frame, one per goal_rc.
        The model's state is reset and all frames but the newest are consumed into it (the newest frame's robot state is then the model's own
        prediction; with n = 1 it is `state`); the designated planes are one-hot; any warm start is forgotten.  Everything the loop needs is
        uploaded and sized here."""
        r = self._check_reset_args(context_images, state, past_actions, designated_rc)
        m, n, H, W = self.model, r.n, r.H, r.W
        with torch.cuda.device(m.device) if torch.cuda.is_available() else contextlib.nullcontext():
            m._require_gpu()
            frames, st = m._as_device(context_images, ()), m._as_device(state, (5,))
            m.reset_state()
            if n > 1:
                m.imagine(frames[:n - 1], m._as_device(r.past, (5,)).view(n - 1, 1, 5), st, observed=n - 1)
                st = m.gen_states[-1].clone()
            else:      # nothing seen yet: the belief is the zero state a reset model starts from
                zero = RecurrentState.empty(1, (H, W), frames.device)
                zero.data.zero_()
                m._adopt_state(zero)
            dev = frames.device
            self._frame, self._state = frames[n - 1:n].contiguous(), st
            self._planes = r.planes.to(dev) if r.planes is not None else None
            a = r.cem
            a.belief = m.recurrent_state()
            b = _cem_upload(self.planner, a, self._frame, self._state)
            self._a = a
            b.per_iter_cold, b.per_iter_warm = b.per_iter, torch.empty((self.warm_iterations,), dtype=torch.float32, device=dev)
            b.init = PlanWarmStart(b.mean.clone(), b.std.clone())      # (what a cold `act()` starts from: the loop writes into b.mean / b.std)
            b.expand_index = torch.zeros((a.chunk,), dtype=torch.int32, device=dev)
            b.tails = torch.from_numpy(np.stack([self.tail_mean, self.tail_std, self.std_floor]).astype(np.float32)).to(dev)
            b.state_config = _state_config(H, W)
            self._b = b
            self._ra = self._rb = None
            if r.refine is not None:      # the polish: `_refine_upload`'s buffers at batch 2, Adam's moments, the cost table and the training plan
                ra, rf = r.refine, self.refiner
                ra.belief = a.belief
                rb = _refine_upload(rf, ra, self._frame.expand(-1, 2, -1, -1, -1), st.expand(2, -1),
                                    torch.zeros((a.horizon, 2, 5), dtype=torch.float32, device=dev), a.image, None)
                rb.moments = (torch.zeros_like(rb.actions[:a.horizon]), torch.zeros_like(rb.actions[:a.horizon]))
                rb.costs = torch.empty((ra.iters + 1, 2), dtype=torch.float32, device=dev)
                rb.expand_index = torch.zeros((2,), dtype=torch.int32, device=dev)
                rf._plan_for(2, a.horizon + 1, H, W)      # sized and bound here, not inside the loop
                self._ra, self._rb = ra, rb
        self._warm, self._action = None, None
        self.step, self.last_plan = 0, None

    def _require_reset(self):
        if self._b is None:
            raise RuntimeError('MPC: call reset() first')

    @property
    def planes(self):
        """The designated pixels as they are believed to lie on the newest frame: (P, H, W) on the device, or None without goal_rc."""
        self._require_reset()
        return self._planes[0] if self._planes is not None else None

    def act(self):
        """Plan from the belief and the newest frame -- `cem_plan(belief=model.recurrent_state(), warm=..., designated_planes=...)` on the buffers
        `reset` made -- and return the plan's first action, (5,) on the device.  `last_plan` holds the whole result until the next call."""
        self._require_reset()
        m, b, a, warm = self.model, self._b, self._a, self._warm
        with torch.cuda.device(self._frame.device):
            b.context.copy_(self._frame.expand_as(b.context))
            b.state.copy_(self._state.expand_as(b.state))
            if self._planes is not None:
                b.planes.copy_(self._planes.expand_as(b.planes))
            _lib.check(_lib.load().pivp_state_copy(ctypes.byref(b.state_config), m._state.data.data_ptr(), 1, b.belief.data.data_ptr(), a.chunk,
                                                   b.expand_index.data_ptr(), m._stream()), 'pivp_state_copy')
            # cold: the initial distribution, `iterations` rounds of the update `cem_plan` would call; warm: the shifted plan and its kept sequences,
            # `warm_iterations` rounds, always of pivp_cem_update_ex
            _cem_arm(b, a, b.init if warm is None else warm)
            b.per_iter = b.per_iter_cold if warm is None else b.per_iter_warm
            how = {} if warm is None else dict(iterations=self.warm_iterations, ex=True)
            self.last_plan = _cem_iterate(self.planner, a, b, seed=self.seed + self.step, **how)
            if self._rb is not None:
                self._polish(self.last_plan)
            self._action = b.best_actions[0].clone()
        return self._action

    def _polish(self, plan):
        """Gradient refinement of `plan` inside `act()`: `cem_refine(belief=)`'s second stage on the buffers `reset` made.  The belief goes to batch 2
        into the refiner's start state, the two starting sequences are copied in, `_refine_iterate` runs, and the cheapest of the three sequences is
        written into the loop's best_actions / best_cost (which `plan.actions` / `plan.cost` are) and, when it is a refined one, into kept sequence
        0 -- stream-ordered work only."""
        m, b, ra, rb = self.model, self._b, self._ra, self._rb
        Hh = ra.steps_T
        rb.images[0].copy_(self._frame[0].expand_as(rb.images[0]))
        rb.states[0].copy_(self._state.expand_as(rb.states[0]))
        _lib.check(_lib.load().pivp_state_copy(ctypes.byref(b.state_config), m._state.data.data_ptr(), 1, rb.belief.data.data_ptr(), 2,
                                               rb.expand_index.data_ptr(), m._stream()), 'pivp_state_copy')
        rb.actions[:Hh, 0].copy_(plan.actions)
        rb.actions[:Hh, 1].copy_(plan.mean)
        refined, costs = _refine_iterate(self.refiner, ra, rb)
        three_costs = torch.cat((plan.cost.view(1), costs[-1]))
        three = torch.cat((plan.actions.unsqueeze(0), refined.transpose(0, 1)))      # (3, horizon, 5): copies, not views of the loop's buffers
        source = torch.argmin(three_costs)
        pick = source.view(1)
        chosen = three.index_select(0, pick)[0]
        if plan.kept is not None:      # CEM's best ever need not be kept sequence 0: only a refined sequence replaces it
            plan.kept[:, 0].copy_(torch.where(source > 0, chosen, plan.kept[:, 0]))
        b.best_actions.copy_(chosen)
        b.best_cost.copy_(three_costs.index_select(0, pick))
        plan.source, plan.refine_costs = source, costs


    def observe(self, frame, state, action=None):
        """The robot has moved.  frame (3, H, W) or (1, 1, 3, H, W): what it sees now, state (5,) or (1, 5): its state now, action (5,): what it
        actually executed (default: what the last `act()` returned).  One `imagine` step on the previous newest frame advances the belief and moves
        the designated planes; the last plan, moved on by one action, becomes the next `act()`'s warm start (an `observe` without an `act()` since
        the last one leaves none: the next plan is cold)."""
        self._require_reset()
        m = self.model
        H, W = self._frame.shape[3:]
        if action is None:
            if self._action is None:
                raise ValueError('observe() without an action: none was given and act() has not been called since the last observe()')
            action = self._action
        if Model._host_shape(frame) not in ((3, H, W), (1, 1, 3, H, W)):
            raise ValueError('frame must be (3, %d, %d) or (1, 1, 3, %d, %d), got shape %s' % (H, W, H, W, Model._host_shape(frame)))
        for name, v in (('state', state), ('action', action)):
            if Model._host_shape(v) not in ((5,), (1, 5)):
                raise ValueError('%s must be (5,) or (1, 5), got shape %s' % (name, Model._host_shape(v)))
        with torch.cuda.device(self._frame.device):
            new_frame = m._as_device(frame, ()).view(1, 1, 3, H, W)
            new_state = m._as_device(state, ()).view(1, 5)
            m.imagine(self._frame, m._as_device(action, ()).view(1, 1, 5), self._state, designated=self._planes, observed=1)
            if self._planes is not None:
                planes = m.pixel_distrib[0]
                if self.renormalize:
                    mass = m.pixel_mass[0]
                    planes = planes / torch.where(mass > 0, mass, torch.ones_like(mass))[..., None, None]
                self._planes = planes
            self._frame, self._state = new_frame, new_state
            self._warm = None
            if self.last_plan is not None and self._action is not None:
                t = self._b.tails
                self._warm = self.last_plan.warm_start(1, t[0], t[1], t[2])
        self._action = None
        self.step += 1
