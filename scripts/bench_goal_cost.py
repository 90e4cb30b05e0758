"""Cost of planning on a goal image (include/pivp_goal_cost.h; profiles/r17/NOTES.md), by the method of scripts/bench_plan.py: legs interleaved round
by round on one device, each 2 warm-up steps and then `--steps` steps between two HIP events; every figure the median of the rounds, with its range.

    op            pivp_goal_image_cost alone at S = 9, K = 32 and K = 128, 64 x 64, with and without the gradient (microseconds per call: two launches),
                  against the same cost composed in torch on the same frames: broadcast difference, square and abs, weighted mean, and -- for the
                  gradient -- the closed form written out as `refine_actions` does for its bare goal image
    cem           per CEM iteration, at K = 32: the rollouts alone (`_rollout_predict` without planes) against `cem_plan(goal_image=)`'s loop on buffers
                  uploaded once; the difference is what the cost, the refit and the resampling add
    refine        one `refine_actions` iteration (rollout, cost, sweep, Adam) at B = 2, T - 1 = 10: a `GoalImageCost` against the bare array
Prints one JSON line.

    python scripts/bench_goal_cost.py [--rounds 7] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX, HORIZON, ITERS, ELITES, SIZE = 2, 9, 3, 8, 64


def stats(v, digits=4):
    return {'median': round(float(np.median(v)), digits), 'min': round(float(np.min(v)), digits), 'max': round(float(np.max(v)), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--samples', type=int, nargs='+', default=[32, 128])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    S = SIZE

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def interleaved(legs, n):
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                series[name].append(timed(step, n))
        return series

    rs = np.random.RandomState(0)
    goal_np = rs.rand(3, S, S).astype(np.float32)
    roi = np.zeros((S, S), np.float32)
    roi[16:48, 16:48] = 1.0
    spec = planning.GoalImageCost(goal_np, mse=1.0, l1=0.25, pixel_weight=roi)
    out = {'shape': 'S=%d %dx%d, mse + 0.25 l1, 32x32 region of interest' % (HORIZON, S, S), 'rounds': args.rounds, 'steps': args.steps, 'op': {}}

    # ---- the op alone -----------------------------------------------------------------------------------------------------------------------------
    stream = torch.cuda.current_stream().cuda_stream
    for K in args.samples:
        frames = torch.rand((HORIZON, K, 3, S, S), device=dev)
        d = planning._goal_upload(spec, HORIZON, dev)
        cost, per_step, grad = torch.empty(K, device=dev), torch.empty((HORIZON, K), device=dev), torch.empty_like(frames)
        goal_d, w_d, sw_d = d.goal, d.pixel_w, d.step_w
        inv = float(spec.inv_norm())

        def hip(want_grad):
            planning._goal_launch(d, frames.data_ptr(), HORIZON, K, S, S, cost.data_ptr(), per_step.data_ptr(), grad.data_ptr() if want_grad else None, 0,
                                  stream)

        def composed(want_grad):
            diff = frames - goal_d
            ps = (w_d * (spec.mse * diff * diff + spec.l1 * diff.abs())).sum(dim=(2, 3, 4)) * inv
            c = spec.weight * (sw_d[:, None] * ps).sum(dim=0)
            g = None
            if want_grad:
                g = (spec.weight * inv) * sw_d[:, None, None, None, None] * w_d * (2.0 * spec.mse * diff + spec.l1 * torch.sign(diff))
            return c, ps, g

        legs = [('hip', lambda: hip(False)), ('hip_grad', lambda: hip(True)), ('torch', lambda: composed(False)), ('torch_grad', lambda: composed(True))]
        series = interleaved(legs, 10 * args.steps)
        rec = {'us_per_call': {n: stats(np.array(v) * 1e3, 2) for n, v in series.items()}, 'bytes_read': HORIZON * K * 3 * S * S * 4}
        c_t, ps_t, g_t = composed(True)
        hip(True)
        torch.cuda.synchronize()
        rec['agrees'] = bool(torch.allclose(c_t, cost, rtol=1e-4) and torch.allclose(g_t, grad, rtol=1e-4, atol=1e-9))
        rec['GB_per_s'] = {n: round(rec['bytes_read'] * (2 if n.endswith('grad') else 1) / (rec['us_per_call'][n]['median'] * 1e-6) / 1e9, 1)
                           for n in ('hip', 'hip_grad')}
        out['op']['K%d' % K] = rec
        del frames, grad

    # ---- per CEM iteration, over the bare rollouts ------------------------------------------------------------------------------------------------
    K = args.samples[0]
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(1, CTX + 1, S, S))
    ctx_np, state_np, past_np = imgs[:CTX], stas[0], acts[:CTX - 1, 0]
    m = pivp_amd.Model(10, prefix='bench', keep_activations=False)
    steps_n = CTX - 1 + HORIZON
    ctx_k = torch.from_numpy(ctx_np).to(dev).expand(-1, K, -1, -1, -1).contiguous()
    state_k = torch.from_numpy(state_np).to(dev).expand(K, -1).contiguous()
    fixed = torch.randn((steps_n, K, 5), device=dev) * 0.3
    m.imagine(ctx_k, fixed, state_k)
    a = planning._check_cem_args(m, ctx_np, state_np, designated_rc=None, goal_rc=None, horizon=HORIZON, past_actions=past_np, iterations=ITERS,
                                 samples=K, elites=ELITES, action_low=-2.0, action_high=2.0, seed=1, goal_image=spec)
    bufs = planning._cem_upload(m, a, ctx_np, state_np)

    def rollouts_only():
        for _ in range(ITERS):
            m._rollout_predict(ctx_k, fixed, state_k, None, CTX - 1)

    series = interleaved([('rollouts_only', rollouts_only), ('cem_goal_image_loop', lambda: planning._cem_iterate(m, a, bufs))], args.steps)
    added = (np.array(series['cem_goal_image_loop']) - np.array(series['rollouts_only'])) / ITERS
    out['cem_K%d' % K] = {'ms_per_plan': {n: stats(v) for n, v in series.items()}, 'added_ms_per_iteration': stats(added)}
    del m, bufs
    torch.cuda.empty_cache()

    # ---- one refine_actions iteration -------------------------------------------------------------------------------------------------------------
    B = 2
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(B, CTX + 1, S, S))
    tm = pivp_amd.Model(10, prefix='bench', keep_activations=True)
    start = (rs.randn(steps_n, B, 5) * 0.3).astype(np.float32)
    ctx_d, state_d, start_d = (torch.from_numpy(x).to(dev) for x in (imgs[:CTX], stas[0], start))
    plain = planning.GoalImageCost(goal_np)
    legs = []
    for name, g in (('bare_array', torch.from_numpy(goal_np).to(dev)), ('goal_image_cost', plain)):
        ra = planning._check_refine_args(tm, ctx_d, state_d, start_d, g, None, 1, 0.0, None, None)
        rb = planning._refine_upload(tm, ra, ctx_d, state_d, start_d, g, None)
        legs.append((name, lambda ra=ra, rb=rb: planning._refine_iterate(tm, ra, rb)))
    series = interleaved(legs, args.steps)
    # (one `_refine_iterate` of one step is two rollouts, two costs, one sweep and one Adam step: the scoring rollout behind the update is included)
    out['refine_B%d' % B] = {'ms_per_iteration_and_final_score': {n: stats(v) for n, v in series.items()},
                             'difference_ms': stats(np.array(series['goal_image_cost']) - np.array(series['bare_array']))}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
