"""Cost of on-device CEM planning around the rollout (CDNA, 64 x 64, ctx 2, horizon 9, one designated pixel, 3 iterations; profiles/r09/NOTES.md).

Settings: samples K = 32 and, if the inference workspace at batch 128 fits, K = 128; precision fp32 and bf16.  Legs, interleaved round by round on
one device (each: 2 warm-up plans, then `--steps` plans between two HIP events; one plan = 3 iterations):
    imagine_only  the rollouts a plan runs -- Model.imagine with the designated plane -- and nothing else
    cem_torch     the loop composed from the public API as it was before `cem_plan`, inputs resident on the device:
                  imagine(normalize=True) -> planning.expected_distance -> torch.topk / mean / std -> torch.randn / clamp
    cem_hip       planning.cem_plan (uploads included); cem_hip_loop: its loop alone on buffers uploaded once (planning._cem_iterate)
and the two ops on their own (microseconds per launch, back-to-back launches).  Reported per setting: milliseconds per plan and the
per-iteration overhead over imagine_only, per round; `accept` = the largest cem_hip overhead lies below the smallest cem_torch overhead.
Prints one JSON line.

    python scripts/bench_plan.py [--rounds 7] [--steps 10]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX, HORIZON, ITERS, ELITES, SIZE = 2, 9, 3, 8, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--samples', type=int, nargs='+', default=[32, 128])
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import _lib, planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    S = SIZE
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(1, CTX + 1, S, S))
    ctx_np, state_np, past_np = imgs[:CTX], stas[0], acts[:CTX - 1, 0]
    designated, goal = (32, 32), (40, 24)
    t0, steps = CTX - 1, CTX - 1 + HORIZON

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

    out = {'shape': 'CDNA ctx=%d horizon=%d P=1 iterations=%d elites=%d %dx%d' % (CTX, HORIZON, ITERS, ELITES, S, S), 'rounds': args.rounds,
           'steps': args.steps, 'settings': {}, 'skipped': []}
    for precision in args.precisions:
        for K in args.samples:
            tag = '%s_K%d' % (precision, K)
            m = pivp_amd.Model(10, prefix='bench', keep_activations=False, precision=precision)
            ctx_k = torch.from_numpy(ctx_np).to(dev).expand(-1, K, -1, -1, -1).contiguous()
            state_k = torch.from_numpy(state_np).to(dev).expand(K, -1).contiguous()
            planes = planning.one_hot_planes(np.tile(np.array([[designated]]), (K, 1, 1)), S, S, device=dev)
            goal_d = torch.tensor(goal, dtype=torch.float32, device=dev)
            past_d = torch.from_numpy(past_np).to(dev)
            low, high = torch.full((5,), -2.0, device=dev), torch.full((5,), 2.0, device=dev)
            fixed = torch.randn((steps, K, 5), device=dev) * 0.3
            try:
                m.imagine(ctx_k, fixed, state_k, designated=planes)
                torch.cuda.synchronize()
            except (RuntimeError, _lib.PivpError) as e:      # the workspace at this batch does not fit
                out['skipped'].append({'setting': tag, 'reason': str(e)[:200]})
                continue

            def imagine_only():
                for _ in range(ITERS):
                    m.imagine(ctx_k, fixed, state_k, designated=planes)

            def cem_torch():
                actions = torch.zeros((steps, K, 5), device=dev)
                actions[:t0] = past_d.unsqueeze(1)
                mean, std = torch.zeros((HORIZON, 5), device=dev), torch.ones((HORIZON, 5), device=dev)
                best_cost, best_actions = torch.full((), float('inf'), device=dev), torch.zeros((HORIZON, 5), device=dev)
                cost = None
                for it in range(ITERS + 1):
                    if cost is not None:
                        idx = torch.topk(cost, ELITES, largest=False).indices
                        elite = actions[t0:, idx]
                        mean, std = elite.mean(dim=1), elite.std(dim=1, unbiased=False).clamp_min(1e-3)
                        better = cost[idx[0]] < best_cost
                        best_actions = torch.where(better, actions[t0:, idx[0]], best_actions)
                        best_cost = torch.where(better, cost[idx[0]], best_cost)
                    if it == ITERS:
                        break
                    z = torch.randn((HORIZON, K, 5), device=dev)
                    actions[t0:] = torch.minimum(torch.maximum(mean[:, None] + std[:, None] * z, low), high)
                    m.imagine(ctx_k, actions, state_k, designated=planes, normalize=True)
                    cost = planning.expected_distance(m.pixel_distrib[:, :, 0], goal_d).sum(dim=0)
                return best_actions, best_cost

            kw = dict(designated_rc=[designated], goal_rc=[goal], horizon=HORIZON, past_actions=past_np, iterations=ITERS, samples=K, elites=ELITES,
                      action_low=-2.0, action_high=2.0, seed=1)

            def cem_hip():
                return planning.cem_plan(m, ctx_k[:, :1], state_k[:1], **kw)

            a = planning._check_cem_args(m, ctx_np, state_np, **kw)
            bufs = planning._cem_upload(m, a, ctx_np, state_np)

            def cem_hip_loop():
                return planning._cem_iterate(m, a, bufs)

            legs = [('imagine_only', imagine_only), ('cem_torch', cem_torch), ('cem_hip', cem_hip), ('cem_hip_loop', cem_hip_loop)]
            series = {name: [] for name, _ in legs}
            for _ in range(args.rounds):
                for name, step in legs:
                    series[name].append(timed(step, args.steps))
            rec = {'ms_per_plan': {n: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)} for n, v in series.items()},
                   'overhead_ms_per_iteration': {}}
            base = np.array(series['imagine_only'])
            for n in ('cem_torch', 'cem_hip', 'cem_hip_loop'):
                ov = (np.array(series[n]) - base) / ITERS
                rec['overhead_ms_per_iteration'][n] = {'median': round(float(np.median(ov)), 4), 'min': round(float(ov.min()), 4),
                                                        'max': round(float(ov.max()), 4), 'rounds': [round(float(x), 4) for x in ov]}
            o = rec['overhead_ms_per_iteration']
            rec['accept'] = bool(o['cem_hip']['max'] < o['cem_torch']['min'])
            # the two ops alone
            lib = _lib.load()
            stream = torch.cuda.current_stream().cuda_stream
            track = torch.rand((HORIZON, K, 1, S, S), device=dev)

            def cost_launch():
                _lib.check(lib.pivp_plan_cost(track.data_ptr(), bufs.goals.data_ptr(), bufs.step_w.data_ptr(), bufs.plane_w.data_ptr(), 89.0,
                                              bufs.cost.data_ptr(), bufs.mass.data_ptr(), bufs.edist.data_ptr(), HORIZON, K, 1, S, S, stream), 'pivp_plan_cost')

            def update_launch():
                _lib.check(lib.pivp_cem_update(bufs.cost.data_ptr(), bufs.actions.data_ptr(), bufs.mean.data_ptr(), bufs.std.data_ptr(),
                                               bufs.best_actions.data_ptr(), bufs.best_cost.data_ptr(), bufs.low.data_ptr(), bufs.high.data_ptr(),
                                               bufs.elite_idx.data_ptr(), K, steps, t0, ELITES, 0.0, 1e-3, ctypes.c_ulonglong(1), 1, stream), 'pivp_cem_update')
            rec['us_per_launch'] = {'pivp_plan_cost': round(min(timed(cost_launch, 200) for _ in range(3)) * 1e3, 2),
                                    'pivp_cem_update': round(min(timed(update_launch, 200) for _ in range(3)) * 1e3, 2)}
            rec['plan_cost_bytes'] = HORIZON * K * S * S * 4
            out['settings'][tag] = rec
            del m, bufs
            torch.cuda.empty_cache()
    out['accept_all'] = all(r['accept'] for r in out['settings'].values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
