"""Float64 NumPy restatement of the two planning ops, written from the text of include/pivp_hip.h alone (pivp_plan_cost, pivp_cem_update):
Philox4x32-10, the uniform, Box-Muller, rank by counting, the refit, the expected-distance cost with its miss_cost rule, and a CEM loop around
a cost callback.  Nothing here imports the package."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of 32-bit words -> (..., 4) uint32 (Salmon et al. 2011: ten rounds, the key bumped between rounds)."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(x):
    """A 32-bit word -> u = ((x >> 8) + 0.5) * 2^-24, strictly inside (0, 1)."""
    return ((np.asarray(x).astype(np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def box_muller(xa, xb):
    r = np.sqrt(-2.0 * np.log(uniform(xa)))
    ang = 2.0 * np.pi * uniform(xb)
    return r * np.cos(ang), r * np.sin(ang)


def normals(K, rows, iteration, seed):
    """Standard normals of candidates 0..K-1 on the action rows `rows` -> (len(rows), K, 5)."""
    rows = np.asarray(list(rows), dtype=np.uint64)
    t, k = np.meshgrid(rows, np.arange(K, dtype=np.uint64), indexing='ij')
    key = np.stack([np.full(t.shape, seed & 0xFFFFFFFF, np.uint64), np.full(t.shape, seed >> 32, np.uint64)], axis=-1)
    it = np.full(t.shape, iteration, np.uint64)
    x = philox4x32_10(np.stack([k, t, it, np.zeros_like(t)], axis=-1), key)
    y = philox4x32_10(np.stack([k, t, it, np.ones_like(t)], axis=-1), key)
    z0, z1 = box_muller(x[..., 0], x[..., 1])
    z2, z3 = box_muller(x[..., 2], x[..., 3])
    z4, _ = box_muller(y[..., 0], y[..., 1])
    return np.stack([z0, z1, z2, z3, z4], axis=-1)


def ranks(cost):
    """rank_k = #{j : c_j < c_k or (c_j == c_k and j < k)}, a NaN cost counting as +inf."""
    c = np.asarray(cost, dtype=np.float64).copy()
    c[np.isnan(c)] = np.inf
    j = np.arange(len(c))
    less = (c[None, :] < c[:, None]) | ((c[None, :] == c[:, None]) & (j[None, :] < j[:, None]))
    return less.sum(axis=1), c


def elite_indices(cost, M):
    r, _ = ranks(cost)
    out = np.empty(M, np.int64)
    for k, rk in enumerate(r):
        if rk < M:
            out[rk] = k
    return out


def cem_update(cost, actions, mean, std, best_actions, best_cost, low, high, t0, elites, alpha, min_std, seed, iteration):
    """One pivp_cem_update.  actions (steps, K, 5); mean, std, best_actions (Hh, 5); best_cost scalar; cost (K,) or None.
    -> dict(actions, mean, std, best_actions, best_cost, elites); the fp32 buffers of the op are rounded to float32 where the op stores them."""
    actions = np.array(actions, dtype=np.float64)
    mean, std = np.array(mean, dtype=np.float64), np.array(std, dtype=np.float64)
    best_actions, best_cost = np.array(best_actions, dtype=np.float64), float(best_cost)
    steps, K, _ = actions.shape
    alpha, min_std = float(np.float32(alpha)), float(np.float32(min_std))
    el = None
    if cost is not None:
        el = elite_indices(cost, elites)
        _, c = ranks(cost)
        cand = actions[t0:, el]                                   # (Hh, M, 5), rank order
        em = cand.mean(axis=1)
        es = np.sqrt(((cand - em[:, None]) ** 2).mean(axis=1))
        mean = (alpha * mean + (1 - alpha) * em).astype(np.float32).astype(np.float64)
        std = np.maximum((alpha * std + (1 - alpha) * es).astype(np.float32).astype(np.float64), min_std)
        if c[el[0]] < best_cost:
            best_actions, best_cost = actions[t0:, el[0]].copy(), float(c[el[0]])
    z = normals(K, range(t0, steps), iteration, seed)
    actions[t0:] = np.clip(mean[:, None] + std[:, None] * z, np.asarray(low, np.float64), np.asarray(high, np.float64))
    return dict(actions=actions, mean=mean, std=std, best_actions=best_actions, best_cost=best_cost, elites=el)


def plan_cost(track, goals, step_w, plane_w, miss_cost):
    """track (S, K, P, H, W) -> (cost (K,), mass (S, K, P), edist (S, K, P))."""
    track = np.asarray(track, dtype=np.float64)
    S, K, P, H, W = track.shape
    goals = np.asarray(goals, dtype=np.float64).reshape(P, 2)
    rows, cols = np.mgrid[0:H, 0:W]
    dist = np.sqrt((rows[None] - goals[:, 0, None, None]) ** 2 + (cols[None] - goals[:, 1, None, None]) ** 2)      # (P, H, W)
    with np.errstate(invalid='ignore', divide='ignore'):
        mass = track.sum(axis=(3, 4))
        mom = (track * dist[None, None]).sum(axis=(3, 4))
        ok = np.isfinite(mass) & (mass > 0)
        edist = np.where(ok, mom / np.where(ok, mass, 1.0), float(miss_cost))
    cost = np.zeros(K)
    for s in range(S):
        cs = np.zeros(K)
        for p in range(P):
            cs += float(plane_w[p]) * edist[s, :, p]
        cost += float(step_w[s]) * cs
    return cost, mass, edist


def cem_loop(cost_fn, horizon, samples, elites, iterations, seed=0, init_mean=0.0, init_std=1.0, alpha=0.0, min_std=1e-3, low=-np.inf, high=np.inf,
             past=None):
    """The loop of `planning.cem_plan` around cost_fn(actions (steps, K, 5)) -> (K,): sample, score, refit; a last update after the last scoring.
    -> dict(actions, cost, mean, std, best_cost_per_iteration, trace)."""
    past = np.zeros((0, 5)) if past is None else np.asarray(past, dtype=np.float64).reshape(-1, 5)
    t0, steps = len(past), len(past) + horizon
    st = dict(actions=np.zeros((steps, samples, 5)), mean=np.broadcast_to(np.asarray(init_mean, np.float64), (horizon, 5)).copy(),
              std=np.broadcast_to(np.asarray(init_std, np.float64), (horizon, 5)).copy(), best_actions=np.zeros((horizon, 5)), best_cost=np.inf)
    st['actions'][:t0] = past[:, None]
    lo, hi = np.broadcast_to(np.asarray(low, np.float64), (5,)), np.broadcast_to(np.asarray(high, np.float64), (5,))
    cost, per_iter, trace = None, [], []
    for it in range(iterations + 1):
        st = cem_update(cost, st['actions'], st['mean'], st['std'], st['best_actions'], st['best_cost'], lo, hi, t0, elites, alpha, min_std, seed, it)
        if it > 0:
            per_iter.append(st['best_cost'])
            trace[-1]['elites'] = st['elites']
        if it == iterations:
            break
        cost = np.asarray(cost_fn(st['actions']), dtype=np.float64)
        trace.append(dict(actions=st['actions'].copy(), cost=cost.copy()))
    return dict(actions=st['best_actions'], cost=st['best_cost'], mean=st['mean'], std=st['std'], best_cost_per_iteration=np.array(per_iter), trace=trace)
