"""Planning with `Model.imagine` (Finn & Levine 2017, "Deep visual foresight for planning robot motion"): designate pixels of the current frame,
roll the model forward under candidate action sequences, score each candidate by where the model expects the pixels to end up, and optimise the
action sequence.

`cem_plan` is the optimiser: the cross-entropy method over action sequences, on the device from the first sample to the returned plan.  Its loop
body is three stream-ordered calls -- pivp_cem_update (refit + Philox resample, one workgroup), pivp_rollout_predict (the rollout with raw
tracked planes) and pivp_plan_cost (expected distance to the goals, each plane read once) -- with every input uploaded before the loop, no host
synchronisation and no host-to-device copy inside it.  It knows about PAST actions: the steps before the last observed frame are fixed, only the
horizon is optimised (the MPC case).

`refine_actions` is the gradient-based counterpart: Adam on an action sequence, with d cost / d actions from the model's own backward sweep
(`Model.backward(input_grad=True, params=False, builtin_loss=False)`, include/pivp_input_grad.h) and any torch cost of the predicted frames.

`score_actions` scores a given set of candidates with one `imagine` and plain torch (`one_hot_planes`, `expected_position`,
`expected_distance`); it is kept as it was for callers that bring their own optimiser.

Closed-loop control: `cem_plan(..., belief=)` and `score_actions(..., belief=)` start every candidate from ONE recurrent state (`state.RecurrentState`,
what a `Model(carry_state=True)` holds after it has seen the frames so far) and the newest frame, instead of re-encoding the observed frames for every
candidate in every iteration."""
import contextlib
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .model import Model, using_config
from .state import is_recurrent_state


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
    if not is_recurrent_state(belief):
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


def score_actions(model, context_images, state, candidates, designated_rc, goal_rc, belief=None):
    """Cost of K candidate action sequences for moving one designated pixel to a goal.

    belief: a batch-1 `RecurrentState` (carry_state=True models).  context_images is then (1, 1, 3, H, W), the newest frame only; `state` its robot
    state; candidates (K, horizon, 5).  The belief is expanded to K and every candidate runs `horizon` steps from it (`imagine(observed=1,
    advance=False)`); the model's own carried state is what it was afterwards.  None: the path below, with the bits it always had.

    context_images (ctx, 1, 3, H, W), state (1, 5): what the robot sees now; candidates (K, T-1, 5); designated_rc, goal_rc: (row, col) on the
    last context frame.  The context is replicated K times and ONE `imagine` runs at batch K with normalised distributions; the cost of
    candidate k is the sum over the predicted frames of `expected_distance` to the goal.  -> (K,) tensor on the model's device."""
    ctx_shape = Model._host_shape(context_images)
    if len(ctx_shape) != 5 or ctx_shape[1] != 1:
        raise ValueError('context_images must be (ctx, 1, 3, H, W), got shape %s' % (ctx_shape,))
    if belief is not None:
        _check_belief(model, belief, ctx_shape)
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
    with _starting_from(model, belief.expand(K) if belief is not None else None):
        if belief is not None:
            model.imagine(ctx_k, actions, state_k, designated=planes, normalize=True, observed=1, advance=False)
        else:
            model.imagine(ctx_k, actions, state_k, designated=planes, normalize=True)
    return expected_distance(model.pixel_distrib[:, :, 0], goal_rc).sum(dim=0)


MAX_CEM_SAMPLES = 1024


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


def _check_cem_args(model, context_images, state, designated_rc, goal_rc, horizon, past_actions, iterations, samples, elites, init_mean, init_std,
                    min_std, alpha, action_low, action_high, step_weights, plane_weights, miss_cost, chunk, seed, belief=None):
    """Every complaint of `cem_plan` is a ValueError raised here, before the GPU or the library is needed.  -> the checked host-side values."""
    ctx = int(model.num_frame_before_prediction)
    si = Model._host_shape(context_images)
    if len(si) != 5 or si[1] != 1 or si[2] != 3:
        raise ValueError('context_images must be (ctx, 1, 3, H, W), got shape %s' % (si,))
    if belief is not None:      # one observed frame on top of the belief, whatever the model's context length
        _check_belief(model, belief, si, past_actions)
        ctx = 1
    if ctx < 1 or si[0] != ctx:
        raise ValueError('context_images holds %d frames, the model was built with num_frame_before_prediction=%d' % (si[0], ctx))
    H, W = si[3:]
    if H < 2 or W < 2:
        raise ValueError('context_images is empty: shape %s' % (si,))
    if Model._host_shape(state) != (1, 5):
        raise ValueError('state must be (1, 5), got shape %s' % (Model._host_shape(state),))
    for name, v, lo in (('horizon', horizon, 1), ('iterations', iterations, 1), ('samples', samples, 1), ('elites', elites, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError('%s must be an integer >= %d, not %r' % (name, lo, v))
    if samples > MAX_CEM_SAMPLES:
        raise ValueError('samples = %d: the refit runs in one workgroup and serves at most %d' % (samples, MAX_CEM_SAMPLES))
    if elites > samples:
        raise ValueError('elites = %d exceeds samples = %d' % (elites, samples))
    if chunk is None:
        chunk = samples
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1 or chunk > samples or samples % chunk:
        raise ValueError('chunk must divide samples = %d, not %r' % (samples, chunk))
    designated = _pixel_coords(designated_rc, 'designated_rc', H, W, whole=True)
    goals = _pixel_coords(goal_rc, 'goal_rc', H, W, whole=False)
    P = designated.shape[0]
    if goals.shape[0] != P:
        raise ValueError('goal_rc holds %d goals for %d designated pixels' % (goals.shape[0], P))
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
    for name, v in (('min_std', min_std), ('alpha', alpha)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError('%s must be a finite non-negative number, not %r' % (name, v))
    if alpha > 1:
        raise ValueError('alpha must lie in [0, 1], not %r' % (alpha,))
    bounds = []
    for name, v, default in (('action_low', action_low, -np.inf), ('action_high', action_high, np.inf)):
        a = np.full(5, default) if v is None else _host_array(v, name)
        if a.shape not in ((), (5,)) or np.isnan(a).any():
            raise ValueError('%s must be a scalar or (5,) without NaN, got shape %s' % (name, a.shape))
        bounds.append(np.ascontiguousarray(np.broadcast_to(a, (5,))))
    if (bounds[0] > bounds[1]).any():
        raise ValueError('action_low exceeds action_high')
    weights = []
    for name, v, n in (('step_weights', step_weights, horizon), ('plane_weights', plane_weights, P)):
        a = np.ones(n) if v is None else _host_array(v, name)
        if a.shape != (n,) or not np.isfinite(a).all():
            raise ValueError('%s must be finite and (%d,), got shape %s' % (name, n, a.shape))
        weights.append(a)
    if miss_cost is None:
        miss_cost = math.sqrt((H - 1) ** 2 + (W - 1) ** 2)
    if isinstance(miss_cost, bool) or not isinstance(miss_cost, (int, float, np.integer, np.floating)) or not math.isfinite(miss_cost):
        raise ValueError('miss_cost must be a finite number, not %r' % (miss_cost,))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError('seed must be an integer in [0, 2**64), not %r' % (seed,))
    return SimpleNamespace(ctx=ctx, H=H, W=W, P=P, K=int(samples), M=int(elites), chunk=int(chunk), horizon=int(horizon), iterations=int(iterations),
                           designated=designated, goals=goals, past=past, mean=mean, std=std, low=bounds[0], high=bounds[1],
                           step_w=weights[0], plane_w=weights[1], miss_cost=float(miss_cost), min_std=float(min_std), alpha=float(alpha), seed=int(seed),
                           belief=belief)


def cem_plan(model, context_images, state, designated_rc, goal_rc, horizon, past_actions=None, iterations=3, samples=32, elites=8, init_mean=None,
             init_std=1.0, min_std=1e-3, alpha=0.0, action_low=None, action_high=None, step_weights=None, plane_weights=None, miss_cost=None,
             chunk=None, seed=0, trace=False, belief=None):
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

    Side effect: the rollouts run on `model` as `imagine` does, so afterwards `model.gen_images` / `gen_states` hold the LAST rollout (the last
    chunk of the last iteration), `pixel_distrib` / `pixel_mass` are None and `backward()` raises until the model is called again.  With
    chunk < samples every rollout copies its slice of the action buffer and allocates its own frames, on the stream, without a host round trip."""
    a = _check_cem_args(model, context_images, state, designated_rc, goal_rc, horizon, past_actions, iterations, samples, elites, init_mean,
                        init_std, min_std, alpha, action_low, action_high, step_weights, plane_weights, miss_cost, chunk, seed, belief)
    with torch.cuda.device(model.device) if torch.cuda.is_available() else contextlib.nullcontext():
        return _cem_iterate(model, a, _cem_upload(model, a, context_images, state), trace)


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
    b.planes = torch.zeros((C, P, H * W), dtype=torch.float32, device=dev)
    b.planes.scatter_(2, b.pixel.to(torch.int64).view(1, P, 1).expand(C, P, 1), 1.0)      # one-hot planes, built on the device (H * W < 2^24: exact)
    b.planes = b.planes.view(C, P, H, W)
    b.actions = torch.zeros((steps, K, 5), dtype=torch.float32, device=dev)
    if t0:
        b.actions[:t0] = b.past.unsqueeze(1)
    b.best_actions = torch.zeros((Hh, 5), dtype=torch.float32, device=dev)
    b.best_cost = torch.full((1,), float('inf'), dtype=torch.float32, device=dev)
    b.per_iter, b.cost, b.mass, b.edist = new(a.iterations), new(K), new(Hh, K, P), new(Hh, K, P)
    b.part = (new(Hh, C, P), new(Hh, C, P)) if C != K else None      # a chunk's moments: [Hh][C][P] is not a slice of [Hh][K][P]
    b.elite_idx = torch.empty((M,), dtype=torch.int32, device=dev)
    model._ensure_params(H, W)
    b.belief = None
    if getattr(a, 'belief', None) is not None:      # ONE expansion to the chunk size (pivp_state_copy); every rollout of the loop reads it and leaves it untouched
        model._checked_state(a.belief)
        b.belief = a.belief.expand(C)
    model._plan_for(C, steps + 1, H, W, keep_activations=False, observed=1 if b.belief is not None else None)      # sized and bound here, not inside the loop
    return b


def _cem_iterate(model, a, b, trace=False):
    """The loop of `cem_plan` on the buffers of `_cem_upload`: pivp_cem_update, the rollout, pivp_plan_cost -- stream-ordered launches and
    device-to-device copies only (tests/test_gpu_planning.py runs it under torch's sync debug mode)."""
    lib = _lib.load()
    P, K, M, C, Hh = a.P, a.K, a.M, a.chunk, a.horizon
    t0, steps = a.ctx - 1, a.ctx - 1 + Hh
    stream = model._stream()

    def update(have_cost, it):
        _lib.check(lib.pivp_cem_update(b.cost.data_ptr() if have_cost else None, b.actions.data_ptr(), b.mean.data_ptr(), b.std.data_ptr(),
                                       b.best_actions.data_ptr(), b.best_cost.data_ptr(), b.low.data_ptr(), b.high.data_ptr(),
                                       b.elite_idx.data_ptr(), K, steps, t0, M, a.alpha, a.min_std, ctypes.c_ulonglong(a.seed), it, stream),
                   'pivp_cem_update')

    belief = getattr(b, 'belief', None)
    from_belief = dict(observed=1, advance=False) if belief is not None else {}
    records = []
    with _starting_from(model, belief):      # (the expanded belief, read by every rollout and written by none; None: every rollout from zeros)
        for it in range(a.iterations):
            update(it > 0, it)
            if it > 0:
                b.per_iter[it - 1:it].copy_(b.best_cost)
                if trace:
                    records[-1]['elites'] = b.elite_idx.clone()
            for k0 in range(0, K, C):
                _, track = model._rollout_predict(b.context, b.actions if C == K else b.actions[:, k0:k0 + C].contiguous(), b.state, b.planes, t0,
                                                  **from_belief)
                m_out, e_out = (b.mass, b.edist) if C == K else b.part
                _lib.check(lib.pivp_plan_cost(track.data_ptr(), b.goals.data_ptr(), b.step_w.data_ptr(), b.plane_w.data_ptr(), a.miss_cost,
                                              b.cost.data_ptr() + 4 * k0, m_out.data_ptr(), e_out.data_ptr(), Hh, C, P, a.H, a.W, stream),
                           'pivp_plan_cost')
                if C != K and trace:
                    b.mass[:, k0:k0 + C].copy_(m_out)
                    b.edist[:, k0:k0 + C].copy_(e_out)
            if trace:
                records.append(dict(actions=b.actions.clone(), cost=b.cost.clone(), mass=b.mass.clone(), edist=b.edist.clone()))
        update(True, a.iterations)      # the last candidates count too: best_*, mean and std reflect them (the resampled rows are not used)
        b.per_iter[a.iterations - 1:].copy_(b.best_cost)
        if trace:
            records[-1]['elites'] = b.elite_idx.clone()
    return SimpleNamespace(actions=b.best_actions, cost=b.best_cost[0], mean=b.mean, std=b.std, best_cost_per_iteration=b.per_iter,
                           trace=records if trace else None)


# ---- gradient-based refinement of an action sequence ---------------------------------------------------------------------------------------
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8      # refine_actions' Adam: the optimizer's defaults (optimizer.Adam)


def _adam_lr_t(lr, t, beta1=ADAM_BETA1, beta2=ADAM_BETA2):
    """The bias-corrected step size of Adam's update t = 1, 2, ... (optimizer.Adam.lr), formed on the host in double."""
    return lr * math.sqrt(1.0 - math.pow(beta2, t)) / (1.0 - math.pow(beta1, t))


def _adam_launch(model, p, g, m, v, lr_t):
    """ONE pivp_adam_step on the flat buffers p, g, m, v (same numel), on the model's stream."""
    _lib.check(_lib.load().pivp_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr_t, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                                          1.0, model._stream()), 'pivp_adam_step')


def _check_refine_args(model, context_images, state, actions, goal_image, cost_fn, steps, lr, past_actions, bounds):
    """Every complaint of `refine_actions` is a ValueError raised here, before the GPU or the library is needed.  -> the checked host-side values."""
    ctx = int(model.num_frame_before_prediction)
    si = Model._host_shape(context_images)
    if len(si) != 5 or si[2] != 3 or si[1] < 1:
        raise ValueError('context_images must be (ctx, B, 3, H, W), got shape %s' % (si,))
    if ctx < 1 or si[0] != ctx:
        raise ValueError('context_images holds %d frames, the model was built with num_frame_before_prediction=%d' % (si[0], ctx))
    B, H, W = si[1], si[3], si[4]
    if H < 2 or W < 2:
        raise ValueError('context_images is empty: shape %s' % (si,))
    if Model._host_shape(state) != (B, 5):
        raise ValueError('state must be (%d, 5), got shape %s' % (B, Model._host_shape(state)))
    sa = Model._host_shape(actions)
    if len(sa) != 3 or sa[1] != B or sa[2] != 5 or sa[0] < ctx:
        raise ValueError('actions must be (T-1, %d, 5) with T-1 >= %d (one action per rollout step, the steps between the context frames included), '
                         'got shape %s' % (B, ctx, sa))
    if not getattr(model, 'keep_activations', False):
        raise ValueError('refine_actions back-propagates through the rollout: the model needs keep_activations=True')
    if getattr(model, '_extra_loss', False):
        raise ValueError('refine_actions differentiates its own cost alone: the model must not carry an image loss')
    if (goal_image is None) == (cost_fn is None):
        raise ValueError('exactly one of goal_image and cost_fn must be given')
    if cost_fn is not None and not callable(cost_fn):
        raise ValueError('cost_fn must be callable: cost_fn(gen (T-ctx, B, 3, H, W)) -> (B,)')
    if goal_image is not None:
        sg = Model._host_shape(goal_image)
        if sg not in ((3, H, W), (B, 3, H, W)):
            raise ValueError('goal_image must be (3, %d, %d) or (%d, 3, %d, %d), got shape %s' % (H, W, B, H, W, sg))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError('steps must be an integer >= 1, not %r' % (steps,))
    if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not math.isfinite(lr) or lr < 0:
        raise ValueError('lr must be a finite non-negative number, not %r' % (lr,))
    n_past = 0
    if past_actions is not None:
        sp = Model._host_shape(past_actions)
        if ctx < 2 or sp not in ((ctx - 1, 5), (ctx - 1, B, 5)):
            raise ValueError('past_actions must be (%d, 5) or (%d, %d, 5): the actions taken between the %d observed frames, got shape %s'
                             % (ctx - 1, ctx - 1, B, ctx, sp))
        n_past = ctx - 1
    low = high = None
    if bounds is not None:
        if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
            raise ValueError('bounds must be a pair (low, high)')
        pair = []
        for name, v, default in (('bounds[0]', bounds[0], -np.inf), ('bounds[1]', bounds[1], np.inf)):
            a = np.full(5, default) if v is None else _host_array(v, name)
            if a.shape not in ((), (5,)) or np.isnan(a).any():
                raise ValueError('%s must be a scalar or (5,) without NaN, got shape %s' % (name, a.shape))
            pair.append(np.ascontiguousarray(np.broadcast_to(a, (5,))))
        if (pair[0] > pair[1]).any():
            raise ValueError('bounds: low exceeds high')
        low, high = pair
    return SimpleNamespace(ctx=ctx, B=B, H=H, W=W, steps_T=sa[0], n_past=n_past, iters=int(steps), lr=float(lr), low=low, high=high)


def refine_actions(model, context_images, state, actions, goal_image=None, cost_fn=None, steps=10, lr=0.05, past_actions=None, bounds=None):
    """Gradient descent (Adam) on an action sequence, with the gradient from the model's own backward sweep.

    context_images (ctx, B, 3, H, W), state (B, 5): what each of B robots sees now; actions (T-1, B, 5): the sequence to start from, one action per
    rollout step (rows t < ctx-1 are the steps between the context frames).  past_actions (ctx-1, 5) or (ctx-1, B, 5): when given, those first rows
    are set to it and held fixed (the MPC case: they have been executed); None: every row is free (explaining an observed video).

    Per iteration: ONE feed-self training-mode rollout (`model(...)` under config.train with scheduled sampling off, whatever the model's
    scheduled_sampling_k is; the frames after the context are zeros and play no part), the cost of the predictions gen = gen_images[ctx-1:]
    (T-ctx, B, 3, H, W) in torch -- cost_fn(gen) -> (B,), differentiated by autograd, or, with goal_image (3, H, W) / (B, 3, H, W), the squared error
    to it averaged over steps and pixels --, `backward(frame_grad=d sum(cost) / d gen, input_grad=True, params=False, builtin_loss=False)`, the past
    rows of the gradient zeroed, ONE pivp_adam_step on the flat action buffer (beta1 0.9, beta2 0.999, eps 1e-8, its own moments, the bias-corrected
    step size formed on the host) and the clamp to bounds = (low, high), each a scalar, (5,) or None.  Stream-ordered launches only: nothing
    synchronises with the host.  A last rollout scores the returned sequence.

    -> (actions (T-1, B, 5), costs (steps + 1, B)): the refined sequence and the cost of every sample in front of each update and behind the last;
    device tensors.  lr = 0 returns the input's bits.

    It knows nothing of `cem_plan`; refining CEM's plan is the caller's three lines:

        plan = cem_plan(model, context, state, designated_rc, goal_rc, horizon, past_actions=past)
        seq = torch.cat((torch.as_tensor(past, dtype=torch.float32, device=plan.actions.device).view(-1, 5), plan.actions)).unsqueeze(1)
        refined, costs = refine_actions(train_model, context, state, seq, goal_image=goal, past_actions=past)

    (`train_model`: the same weights with keep_activations=True.)  Side effect: the model holds the last rollout; its parameter gradients are
    unspecified afterwards (`cleargrads()` before training on)."""
    a = _check_refine_args(model, context_images, state, actions, goal_image, cost_fn, steps, lr, past_actions, bounds)
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
    b.states = torch.zeros((T, a.B, 5), dtype=torch.float32, device=dev)
    b.states[0] = model._as_device(state, (5,))
    b.actions = torch.zeros((T, a.B, 5), dtype=torch.float32, device=dev)      # (the rollout's action tensor is (T, B, 5); row T-1 is never read)
    b.actions[:T - 1] = model._as_device(actions, (5,))
    if a.n_past:
        past = model._as_device(past_actions, (5,))
        b.actions[:a.n_past] = past if past.dim() == 3 else past.unsqueeze(1)
    b.goal = None if goal_image is None else model._as_device(goal_image, ())
    to_dev = lambda v: None if v is None else torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev)
    b.low, b.high = to_dev(a.low), to_dev(a.high)
    return b


def _refine_iterate(model, a, b, cost_fn=None, adam=_adam_launch):
    """The loop of `refine_actions` on its device buffers: rollout, cost, sweep, Adam -- stream-ordered work only (tests/test_gpu_input_grad.py runs it
    under torch's sync debug mode)."""
    T1, t0 = a.steps_T, a.n_past
    p = b.actions[:T1]                    # the optimised buffer: a contiguous prefix
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    costs = torch.empty((a.iters + 1, a.B), dtype=torch.float32, device=p.device)
    nf = T1 + 1 - a.ctx

    def rollout_cost(want_grad):
        k = model.scheduled_sampling_k
        model.scheduled_sampling_k = -1
        try:
            with using_config('train', True):
                model([b.images, b.actions, b.states])
        finally:
            model.scheduled_sampling_k = k
        gen = model._gen[a.ctx - 1:]
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
