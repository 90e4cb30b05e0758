"""Cost of gradient refinement from a belief (`planning.refine_actions(belief=)`, `planning.MPC(refine_steps=)`), by the method of scripts/bench_mpc.py:
legs interleaved round by round on one device (every other round in reverse order), each 2 warm-up steps and then `--steps` steps between two HIP
events; every figure the median of the rounds, with its range.  64 x 64, horizon 9.

    iteration     one `refine_actions` iteration (rollout, goal-image cost, sweep, Adam) at B = 2: from a belief and the newest frame on a ctx = 1
                  carrying model, against from two context frames on a ctx = 2 model.  A call of n iterations is n of them and the rollout that scores
                  the result, so the iteration is (call of 5 - call of 1) / 4, formed round by round.
    control step  one warm `MPC.act()` at K = 32 on a goal image with refine_steps 0, 2 and 5: fp32 throughout, and with a bf16 planner beside the fp32
                  observer / refiner.  --parent-planning FILE: a copy of another commit's planning.py, loaded beside this tree's; its `MPC.act()`
                  joins the rounds as a leg of its own (the refine_steps = 0 leg must overlap it).
Prints one JSON line and writes it and belief_refine.md into --out.

    python scripts/bench_belief_refine.py [--rounds 7] [--steps 20] [--out profiles/r20] [--parent-planning FILE]"""
import argparse
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HORIZON, K, ELITES, KEEP, SIZE = 9, 32, 8, 3, 64
REFINE_STEPS = (0, 2, 5)


def stats(v, digits=4):
    return {'median': round(float(np.median(v)), digits), 'min': round(float(np.min(v)), digits), 'max': round(float(np.max(v)), digits)}


def notes(out):
    row = lambda d: '%.3f (%.3f .. %.3f)' % (d['median'], d['min'], d['max'])
    it = out['refine_iteration_ms']
    ratio = it['from a belief']['median'] / it['from two context frames']['median']
    lines = ['## Gradient refinement from a belief (`refine_actions(belief=)`, `cem_refine(belief=)`, `MPC(refine_steps=)`)', '',
             'Written by `scripts/bench_belief_refine.py` (%d interleaved rounds, %d steps each; median and range).  MI355X, one device, 64 x 64,'
             % (out['rounds'], out['steps']), 'horizon %d.' % HORIZON, '',
             '### One `refine_actions` iteration at B = 2 (milliseconds)', '', '| route | one iteration | a call of 1 iteration | a call of 5 |', '|---|---|---|---|']
    for name in ('from a belief', 'from two context frames'):
        lines.append('| %s | %s | %s | %s |' % (name, row(it[name]), row(out['refine_call_ms'][name + ', 1 iteration']),
                                                 row(out['refine_call_ms'][name + ', 5 iterations'])))
    lines += ['', 'The belief route costs %.3f of the frame route; horizon / (horizon + ctx - 1) = %.3f.' % (ratio, HORIZON / (HORIZON + 1.0)), '',
              '### One warm `MPC.act()`, K = %d, goal image (milliseconds)' % K, '',
              '| planner | ' + ' | '.join('refine_steps = %d' % n for n in REFINE_STEPS) + ' | the parent commit\'s act() |', '|---|' + '---|' * (len(REFINE_STEPS) + 1)]
    for prec, d in out['act_warm_ms'].items():
        lines.append('| %s | %s | %s |' % (prec, ' | '.join(row(d['refine_steps=%d' % n]) for n in REFINE_STEPS), row(d['parent']) if 'parent' in d else 'not run'))
    lines += ['', 'The refiner is the fp32 observer in both rows: the polish is one training rollout and one sweep at batch 2 per Adam step and one more',
              'rollout that scores the result, whatever the planner\'s precision.', '']
    return '\n'.join(lines)


def load_parent_planning(path):
    """Another commit's planning.py as a module of this tree's package (its relative imports find this tree's modules)."""
    import pivp_amd
    name = pivp_amd.__name__ + '.planning_parent'
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20'))
    ap.add_argument('--parent-planning', default=None)
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    parent = load_parent_planning(args.parent_planning) if args.parent_planning else None

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

    def interleaved(legs, n):      # every other round runs the legs in reverse: a leg inherits clocks and caches from the one before, so none keeps one neighbour
        series = {name: [] for name, _ in legs}
        for r in range(args.rounds):
            for name, step in (legs if r % 2 == 0 else legs[::-1]):
                series[name].append(timed(step, n))
        return series

    out = {'rounds': args.rounds, 'steps': args.steps}
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(2, HORIZON + 3, SIZE, SIZE))
    spec = planning.GoalImageCost(imgs[HORIZON + 2, 0])
    flags = dict(carry_state=True, keep_activations=True, state_backward=True, num_frame_before_prediction=1)

    # ---- one refine_actions iteration at B = 2 ------------------------------------------------------------------------------------------------------
    one = pivp_amd.Model(10, prefix='bench', **flags)
    two = pivp_amd.Model(10, prefix='bench', keep_activations=True, num_frame_before_prediction=2)
    one.imagine(imgs[:1], acts[:1], stas[0], observed=1)
    belief, state1 = one.recurrent_state(), one.gen_states[-1].clone()
    legs = []
    for iters in (1, 5):
        a1 = planning._check_refine_args(one, imgs[1:2], state1, acts[1:1 + HORIZON], spec, None, iters, 0.01, None, None, belief)
        b1 = planning._refine_upload(one, a1, imgs[1:2], state1, acts[1:1 + HORIZON], spec, None)
        a2 = planning._check_refine_args(two, imgs[:2], stas[0], acts[:1 + HORIZON], spec, None, iters, 0.01, acts[:1], None)
        b2 = planning._refine_upload(two, a2, imgs[:2], stas[0], acts[:1 + HORIZON], spec, acts[:1])
        plural = 'iteration' if iters == 1 else 'iterations'
        legs.append(('from a belief, %d %s' % (iters, plural), lambda a=a1, b=b1: planning._refine_iterate(one, a, b)))
        legs.append(('from two context frames, %d %s' % (iters, plural), lambda a=a2, b=b2: planning._refine_iterate(two, a, b)))
    series = interleaved(legs, args.steps)
    out['refine_call_ms'] = {name: stats(v) for name, v in series.items()}
    out['refine_iteration_ms'] = {route: stats((np.array(series[route + ', 5 iterations']) - np.array(series[route + ', 1 iteration'])) / 4.0)
                                  for route in ('from a belief', 'from two context frames')}
    del one, two, legs
    torch.cuda.empty_cache()

    # ---- one warm control step ------------------------------------------------------------------------------------------------------------------------
    frame, state = torch.from_numpy(imgs[2:3, :1]).to(dev), torch.from_numpy(stas[2, :1]).to(dev)
    out['act_warm_ms'] = {}
    for prec in ('fp32', 'bf16 planner'):
        observer = pivp_amd.Model(10, prefix='bench', **flags)
        planner = observer if prec == 'fp32' else pivp_amd.Model(10, prefix='bench', carry_state=True, precision='bf16')
        kw = dict(goal_image=spec, iterations=3, samples=K, elites=ELITES, keep_elites=KEEP, action_low=-2.0, action_high=2.0, warm_iterations=1, planner=planner)
        made = [('refine_steps=%d' % n, planning.MPC(observer, HORIZON, refine_steps=n, refine_lr=0.01, **kw)) for n in REFINE_STEPS]
        if parent is not None:      # beside the leg it is compared with; its own GoalImageCost: the two modules' classes do not know each other
            made.insert(1, ('parent', parent.MPC(observer, HORIZON, **dict(kw, goal_image=parent.GoalImageCost(imgs[HORIZON + 2, 0])))))
        legs = []
        for name, ctl in made:      # every controller: reset, one cold plan, one observed step; the leg is act() from that warm start
            ctl.reset(imgs[:2, :1], stas[0, :1], acts[:1, 0])
            ctl.act()
            ctl.observe(frame, state)
            ctl.act()

            def act(c=SimpleNamespace(ctl=ctl, warm=ctl._warm)):
                c.ctl._warm = c.warm
                c.ctl.act()
            legs.append((name, act))
        series = interleaved(legs, args.steps)
        out['act_warm_ms'][prec] = {name: stats(v) for name, v in series.items()}
        del made, legs, observer, planner
        torch.cuda.empty_cache()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_belief_refine.json'), 'w') as f:
        f.write(json.dumps(out) + '\n')
    with open(os.path.join(args.out, 'belief_refine.md'), 'w') as f:
        f.write(notes(out))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
