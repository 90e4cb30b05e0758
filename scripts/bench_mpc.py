"""Cost of closed-loop planning (include/pivp_mpc.h, `planning.MPC`; profiles/r18/NOTES.md), by the method of scripts/bench_plan.py: legs interleaved
round by round on one device, each 2 warm-up steps and then `--steps` steps between two HIP events; every figure the median of the rounds, with its
range.

    ops           microseconds per call, K = 32: pivp_cem_update against pivp_cem_update_ex with the options off (same run), with keep = 3 and the
                  mean, with beta = 1 at n = 9 and at n = 64; pivp_cem_shift alone (n = 9, three kept sequences)
    control step  `MPC.act()` at K = 32, horizon 9, one designated pixel, fp32 and bf16 rollouts (the observer is fp32 in both): warm (the shifted plan,
                  1 iteration) against cold (3 iterations); and `MPC.observe()`: the belief's step, the planes and the shift
Prints one JSON line and writes it and NOTES.md into --out.

    python scripts/bench_mpc.py [--rounds 7] [--steps 20] [--out profiles/r18]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HORIZON, K, ELITES, KEEP, SIZE = 9, 32, 8, 3, 64


def stats(v, digits=4):
    return {'median': round(float(np.median(v)), digits), 'min': round(float(np.min(v)), digits), 'max': round(float(np.max(v)), digits)}


def notes(out):
    row = lambda d: '%.2f (%.2f .. %.2f)' % (d['median'], d['min'], d['max'])
    lines = ['# Round 18: closed-loop visual MPC (`planning.MPC`, `pivp_cem_update_ex`, `pivp_cem_shift`)', '',
             'Written by `scripts/bench_mpc.py` (%d interleaved rounds, %d steps each; median and range).  MI355X, one device.' % (out['rounds'], out['steps']),
             '', '## The ops alone, K = %d (microseconds per call, back-to-back launches)' % K, '', '| op | us |', '|---|---|']
    lines += ['| %s | %s |' % (name, row(d)) for name, d in out['ops_us'].items()]
    lines += ['', '`pivp_cem_update_ex` with the options off runs the statements of `pivp_cem_update` and returns its bits; both are one workgroup and',
              'bounded by the launch, and the difference between the first two rows is what the larger argument block and the option tests cost.',
              'Colored noise adds Q (n x n, fp64: pow and sincospi per entry) in LDS and, per sample, a chain of n dependent fp64 multiply-adds in the',
              'order the header fixes; n = 64 is the largest horizon served and far from the horizons planning uses (a rollout of 64 steps at K = 32',
              'takes tens of milliseconds).', '',
              '## One control step, K = %d, horizon %d, 64 x 64 (milliseconds)' % (K, HORIZON), '',
              '| rollouts | act(), cold: 3 iterations | act(), warm: 1 iteration | observe() |', '|---|---|---|---|']
    for prec, d in out['control_step_ms'].items():
        lines.append('| %s | %s | %s | %s |' % (prec, row(d['act_cold_3_iterations']), row(d['act_warm_1_iteration']), row(d['observe'])))
    lines += ['', 'A refit iteration is a batch of rollouts, so a control step that starts from the shifted plan and runs one iteration costs about a',
              'third of one that plans from scratch with three.  Whether one warm iteration plans as well as three cold ones depends on the task',
              '(tests/test_mpc_host.py: on the point mass the shift wins on every target).', '']
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18'))
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import _lib, planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    lib = _lib.load()

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

    out = {'rounds': args.rounds, 'steps': args.steps}
    stream = torch.cuda.current_stream().cuda_stream

    # ---- the ops alone ----------------------------------------------------------------------------------------------------------------------------
    def buffers(n):
        b = dict(cost=torch.rand(K, device=dev), actions=torch.randn((n, K, 5), device=dev), mean=torch.zeros((n, 5), device=dev),
                 std=torch.ones((n, 5), device=dev), best_actions=torch.zeros((n, 5), device=dev), best_cost=torch.full((1,), float('inf'), device=dev),
                 low=torch.full((5,), -2.0, device=dev), high=torch.full((5,), 2.0, device=dev), elite=torch.empty(ELITES, dtype=torch.int32, device=dev),
                 tail=torch.tensor([[0.0] * 5, [1.0] * 5, [0.5] * 5], device=dev))
        return {k: v.data_ptr() for k, v in b.items()}, b

    p9, keep9 = buffers(9)
    p64, keep64 = buffers(64)

    def update(p, n):
        _lib.check(lib.pivp_cem_update(p['cost'], p['actions'], p['mean'], p['std'], p['best_actions'], p['best_cost'], p['low'], p['high'], p['elite'], K, n,
                                       0, ELITES, 0.0, 1e-3, ctypes.c_ulonglong(1), 1, stream), 'pivp_cem_update')

    def update_ex(p, n, keep=0, add_mean=0, beta=0.0):
        _lib.check(lib.pivp_cem_update_ex(p['cost'], p['actions'], p['mean'], p['std'], p['best_actions'], p['best_cost'], p['low'], p['high'], p['elite'], K,
                                          n, 0, ELITES, 0.0, 1e-3, ctypes.c_ulonglong(1), 1, keep, 0, add_mean, beta, stream), 'pivp_cem_update_ex')

    def shift(p, n):
        _lib.check(lib.pivp_cem_shift(p['mean'], p['std'], p['actions'], p['best_actions'], p['best_cost'], p['low'], p['high'], p['tail'], p['tail'] + 20,
                                      p['tail'] + 40, K, n, 0, KEEP, 1, stream), 'pivp_cem_shift')

    legs = [('pivp_cem_update n=9', lambda: update(p9, 9)), ('pivp_cem_update_ex n=9, options off', lambda: update_ex(p9, 9)),
            ('pivp_cem_update_ex n=9, keep 3 + mean', lambda: update_ex(p9, 9, KEEP, 1)), ('pivp_cem_update_ex n=9, beta 1', lambda: update_ex(p9, 9, beta=1.0)),
            ('pivp_cem_update n=64', lambda: update(p64, 64)), ('pivp_cem_update_ex n=64, beta 1', lambda: update_ex(p64, 64, beta=1.0)),
            ('pivp_cem_shift n=9, keep 3', lambda: shift(p9, 9))]
    series = interleaved(legs, 10 * args.steps)
    out['ops_us'] = {name: stats(np.array(v) * 1e3, 2) for name, v in series.items()}

    # ---- one control step -------------------------------------------------------------------------------------------------------------------------
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(1, 4, SIZE, SIZE))
    out['control_step_ms'] = {}
    for prec in ('fp32', 'bf16'):
        observer = pivp_amd.Model(10, prefix='bench', carry_state=True)
        planner = observer if prec == 'fp32' else pivp_amd.Model(10, prefix='bench', carry_state=True, precision=prec)
        ctl = planning.MPC(observer, HORIZON, goal_rc=[[40, 24]], iterations=3, samples=K, elites=ELITES, keep_elites=KEEP, action_low=-2.0, action_high=2.0,
                           warm_iterations=1, planner=planner)
        ctl.reset(imgs[:2], stas[0], acts[:1, 0], designated_rc=[[32, 32]])
        frame, state = torch.from_numpy(imgs[2:3]).to(dev), torch.from_numpy(stas[2]).to(dev)
        first = ctl.act().clone()
        belief = observer.recurrent_state()
        ctl.observe(frame, state)
        warm = ctl._warm

        def act(start):
            ctl._warm = start
            ctl.act()

        def observe():      # the same step every time: from the belief and with the action of the first one, the last plan moved on by one
            observer.set_recurrent_state(belief)
            ctl._action = first
            ctl.observe(frame, state)

        ctl._warm = warm
        ctl.act()
        series = interleaved([('act_cold_3_iterations', lambda: act(None)), ('act_warm_1_iteration', lambda: act(warm)), ('observe', observe)], args.steps)
        out['control_step_ms'][prec] = {name: stats(v) for name, v in series.items()}
        del ctl, observer, planner
        torch.cuda.empty_cache()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_mpc.json'), 'w') as f:
        f.write(json.dumps(out) + '\n')
    with open(os.path.join(args.out, 'NOTES.md'), 'w') as f:
        f.write(notes(out))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
