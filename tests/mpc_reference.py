"""Float64 NumPy restatement of the two closed-loop planning ops, written from the text of include/pivp_mpc.h alone (pivp_cem_update_ex,
pivp_cem_shift), on top of tests/plan_reference.py (Philox, ranks, pivp_cem_update), and the planning loops around them.  Nothing here imports
the package."""
import numpy as np

import plan_reference as PR


def color_matrix(n, beta):
    """Q (n, n): column 0 constant, then cos / -sin pairs of frequency j = 1, 2, ..., for even n a last column cos(pi i); s_j = max(j, 1)^(-beta/2);
    all divided by sigma.  The angle is reduced exactly, (j i) mod n."""
    i = np.arange(n)
    s = np.maximum(np.arange(n // 2 + 1), 1).astype(np.float64) ** (-0.5 * float(beta))
    Q = np.zeros((n, n))
    Q[:, 0] = s[0]
    s2 = s[0] ** 2
    for j in range(1, n // 2 + 1):
        if 2 * j == n:
            Q[:, n - 1] = s[j] * np.where(i % 2 == 0, 1.0, -1.0)
            s2 += s[j] ** 2
            break
        ang = 2.0 * np.pi * ((j * i) % n) / n
        Q[:, 2 * j - 1] = np.sqrt(2.0) * s[j] * np.cos(ang)
        Q[:, 2 * j] = -np.sqrt(2.0) * s[j] * np.sin(ang)
        s2 += 2.0 * s[j] ** 2
    return Q / np.sqrt(s2)


def cem_update_ex(cost, actions, mean, std, best_actions, best_cost, low, high, t0, elites, alpha, min_std, seed, iteration, keep=0, kept_in=0,
                  add_mean=0, beta=0.0):
    """One pivp_cem_update_ex: arguments and result as plan_reference.cem_update, which it equals exactly with the four options at their defaults."""
    before = np.array(actions, dtype=np.float64)
    steps, K, _ = before.shape
    n = steps - t0
    assert 0 <= keep <= elites and keep + int(bool(add_mean)) <= K and (beta == 0 or n <= 64)
    out = PR.cem_update(cost, actions, mean, std, best_actions, best_cost, low, high, t0, elites, alpha, min_std, seed, iteration)
    lo, hi = np.broadcast_to(np.asarray(low, np.float64), (5,)), np.broadcast_to(np.asarray(high, np.float64), (5,))
    if beta > 0:
        z = PR.normals(K, range(t0, steps), iteration, seed)                       # (n, K, 5): the white normals of pivp_cem_update
        y = np.einsum('ic,ckd->ikd', color_matrix(n, np.float32(beta)), z)
        y = y.astype(np.float32).astype(np.float64)                                # the op rounds y once
        out['actions'][t0:] = np.clip(out['mean'][:, None] + out['std'][:, None] * y, lo, hi)
    if cost is not None:
        for j in range(keep):
            out['actions'][t0:, j] = before[t0:, out['elites'][j]]
    elif kept_in:
        out['actions'][t0:, :keep] = before[t0:, :keep]
    if add_mean:
        out['actions'][t0:, keep] = np.clip(out['mean'], lo, hi)
    return out


def cem_shift(mean, std, actions, best_actions, low, high, tail_mean, tail_std, std_floor, t0, keep, shift):
    """One pivp_cem_shift -> dict(mean, std, actions, best_actions, best_cost); actions / best_actions may be None."""
    mean, std = np.array(mean, dtype=np.float64), np.array(std, dtype=np.float64)
    n = mean.shape[0]
    assert 1 <= shift < n
    tm, ts, fl = (np.broadcast_to(np.asarray(v, np.float64), (5,)) for v in (tail_mean, tail_std, std_floor))
    clamped = None
    if actions is not None or best_actions is not None:
        clamped = np.clip(tm, np.broadcast_to(np.asarray(low, np.float64), (5,)), np.broadcast_to(np.asarray(high, np.float64), (5,)))

    def up(a, tail):                                                               # rows move up along axis 0, the tail behind
        a = np.array(a, dtype=np.float64)
        a[:n - shift] = a[shift:].copy()
        a[n - shift:] = tail
        return a
    out = dict(mean=up(mean, tm), std=np.maximum(up(std, ts), fl), actions=None, best_actions=None, best_cost=np.inf)
    if actions is not None:
        out['actions'] = np.array(actions, dtype=np.float64)
        out['actions'][t0:, :keep] = up(out['actions'][t0:, :keep], clamped)
    if best_actions is not None:
        out['best_actions'] = up(best_actions, clamped)
    return out


def cem_loop_ex(cost_fn, horizon, samples, elites, iterations, seed=0, init_mean=0.0, init_std=1.0, alpha=0.0, min_std=1e-3, low=-np.inf,
                high=np.inf, keep=0, add_mean=0, beta=0.0, warm=None):
    """The loop of `planning.cem_plan` with the options: as plan_reference.cem_loop (no past actions).  warm: dict(mean, std, kept (horizon, keep, 5) or
    None) replaces init_mean / init_std and fills slots 0 .. keep-1 before the first sampling.  -> cem_loop's dict plus `kept` (horizon, keep, 5)."""
    st = dict(actions=np.zeros((horizon, samples, 5)), mean=np.broadcast_to(np.asarray(init_mean, np.float64), (horizon, 5)).copy(),
              std=np.broadcast_to(np.asarray(init_std, np.float64), (horizon, 5)).copy(), best_actions=np.zeros((horizon, 5)), best_cost=np.inf)
    kept_in = 0
    if warm is not None:
        st['mean'], st['std'] = np.array(warm['mean'], np.float64), np.array(warm['std'], np.float64)
        if keep and warm.get('kept') is not None:
            st['actions'][:, :keep] = warm['kept']
            kept_in = 1
    lo, hi = np.broadcast_to(np.asarray(low, np.float64), (5,)), np.broadcast_to(np.asarray(high, np.float64), (5,))
    cost, per_iter, trace = None, [], []
    for it in range(iterations + 1):
        st = cem_update_ex(cost, st['actions'], st['mean'], st['std'], st['best_actions'], st['best_cost'], lo, hi, 0, elites, alpha, min_std, seed, it,
                           keep=keep, kept_in=kept_in, add_mean=add_mean, beta=beta)
        if it > 0:
            per_iter.append(st['best_cost'])
            trace[-1]['elites'] = st['elites']
        if it == iterations:
            break
        cost = np.asarray(cost_fn(st['actions']), dtype=np.float64)
        trace.append(dict(actions=st['actions'].copy(), cost=cost.copy()))
    return dict(actions=st['best_actions'], cost=st['best_cost'], mean=st['mean'], std=st['std'], best_cost_per_iteration=np.array(per_iter),
                trace=trace, kept=st['actions'][:, :keep].copy())


def colored_noise_statistics(y, beta):
    """y (N, n): N independent draws of one colored sequence (mean 0, unit variance by construction) -> the largest deviation, in standard errors, of
    the per-row second moment from 1 and of the lag-1 product moment from (Q Q^T)[t, t+1].  For a Gaussian pair with correlation r the product has
    variance 1 + r^2, so the standard errors are sqrt(2 / N) and sqrt((1 + r^2) / N)."""
    y = np.asarray(y, dtype=np.float64)
    N, n = y.shape
    Q = color_matrix(n, beta)
    C = Q @ Q.T
    dev = np.abs((y ** 2).mean(axis=0) - 1.0) / np.sqrt(2.0 / N)
    r = np.array([C[t, t + 1] for t in range(n - 1)])
    lag = np.abs((y[:, :-1] * y[:, 1:]).mean(axis=0) - r) / np.sqrt((1.0 + r ** 2) / N)
    return float(max(dev.max(), lag.max() if n > 1 else 0.0)), r


def colored_draws(update, beta=1.0, K=1024, n=9, iterations=8, seed=5):
    """The samples of `iterations` sample-only updates from N(0, 1) without bounds -> (iterations * K * 5, n): one colored sequence per row."""
    ys = []
    for it in range(iterations):
        out = update(None, np.zeros((n, K, 5)), np.zeros((n, 5)), np.ones((n, 5)), np.zeros((n, 5)), np.inf, -np.inf, np.inf, t0=0, elites=1, alpha=0.0,
                     min_std=0.0, seed=seed, iteration=it, beta=beta)
        ys.append(np.asarray(out['actions'], np.float64).transpose(1, 2, 0).reshape(-1, n))
    return np.concatenate(ys)


def point_mass_episode(target, warm, horizon=12, samples=32, elites=8, steps=10, seed=0):
    """The closed loop on a point mass in R^5 whose actions are position increments: per control step ONE CEM iteration (cem_loop_ex) on the mean
    squared distance of the predicted positions to `target`, the best sequence's first action is executed.  warm: the next plan starts from this
    one's mean moved on by one step (cem_shift: tail mean 0, every std back to 1); otherwise every step plans from N(0, 1).
    -> the mean over the control steps of the squared distance to the target after the step."""
    pos = np.zeros(5)
    start, total = None, 0.0
    for step in range(steps):
        cost_fn = lambda actions: ((pos + np.cumsum(actions, axis=0) - target) ** 2).mean(axis=(0, 2))
        res = cem_loop_ex(cost_fn, horizon, samples, elites, 1, seed=seed + step, warm=start)
        pos = pos + res['actions'][0]
        total += float(((pos - target) ** 2).mean())
        if warm:
            sh = cem_shift(res['mean'], res['std'], None, None, None, None, 0.0, 1.0, 1.0, 0, 0, 1)
            start = dict(mean=sh['mean'], std=sh['std'], kept=None)
    return total / steps
