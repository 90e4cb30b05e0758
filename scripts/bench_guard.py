"""Cost of the guarded Adam step around the train step (config 2's model: CDNA, 64 x 64, batch 32, 10 frames; profiles/r12/NOTES.md).

Plans: precision fp32 and bf16.  Legs, interleaved round by round on one device (each: 2 warm-up steps, then `--steps` steps between two HIP events;
one step = reset_state + optimizer.update, inputs resident on the device):
    plain         Adam().update: the one pivp_adam_step launch behind the sweep -- the yardstick
    guarded       Adam(skip_nonfinite=True) + GradientClipping: pivp_grad_stats (three launches) + pivp_adam_step_guarded
    torch_guard   the same guard composed in torch on the flat gradient buffer in front of the plain launch, without a host synchronisation:
                  linalg.vector_norm(dtype=float64), isfinite, clamp(threshold / norm, max=1), mul_, and a where-style skip (p, m, v cloned in
                  front of the step, torch.where(finite, new, old) behind it)
and the launches on their own on the model's flat buffers (microseconds per call, back-to-back calls): pivp_adam_step, pivp_grad_stats,
pivp_adam_step_guarded, and torch_guard's tensor operations without the Adam launch.  Reported per plan: milliseconds per step and the
microseconds each guard adds to `plain`, per round (median, min, max).  Prints one JSON line.

    python scripts/bench_guard.py [--rounds 7] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH, FRAMES, SIZE, THRESHOLD = 32, 10, 64, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import _lib
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    x = [torch.tensor(np.asarray(a, dtype=np.float32), device=dev) for a in R.synthetic_batch(BATCH, FRAMES, SIZE, SIZE)]

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

    def summary(v, digits=4):
        return {'median': round(float(np.median(v)), digits), 'min': round(float(np.min(v)), digits), 'max': round(float(np.max(v)), digits)}

    out = {'shape': 'CDNA B=%d T=%d %dx%d' % (BATCH, FRAMES, SIZE, SIZE), 'rounds': args.rounds, 'steps': args.steps, 'plans': {}}
    for precision in args.precisions:
        def fresh(**kw):
            m = pivp_amd.Model(10, prefix='bench', keep_activations=True, precision=precision)
            return m, pivp_amd.Adam(alpha=0.001, **kw).setup(m)
        (mp, op), (mg, og), (mt, ot) = fresh(), fresh(skip_nonfinite=True), fresh()
        og.add_hook(pivp_amd.GradientClipping(THRESHOLD))

        def plain():
            mp.reset_state()
            return op.update(mp, x, 0)

        def guarded():
            mg.reset_state()
            return og.update(mg, x, 0)

        def torch_guard_ops(m, opt, step):
            g = m._flat_grads
            norm = torch.linalg.vector_norm(g, dtype=torch.float64)
            finite = torch.isfinite(norm)
            g.mul_(torch.clamp(THRESHOLD / norm, max=1.0).to(torch.float32))
            state = (m._flat_params, opt._m, opt._v)
            old = [t.clone() for t in state]
            step()
            for t, o in zip(state, old):
                t.copy_(torch.where(finite, t, o))

        def torch_guard():
            mt.reset_state()
            loss = mt(x, 0)
            mt.cleargrads()
            mt.backward()
            ot._state(mt)
            torch_guard_ops(mt, ot, lambda: ot.step(mt))
            return loss

        legs = [('plain', plain), ('guarded', guarded), ('torch_guard', torch_guard)]
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                series[name].append(timed(step, args.steps))
        base = np.array(series['plain'])
        rec = {'ms_per_step': {n: summary(v) for n, v in series.items()},
               'added_us_per_step': {n: dict(summary((np.array(series[n]) - base) * 1e3, 1), rounds=[round(float(d), 1) for d in (np.array(series[n]) - base) * 1e3])
                                     for n in ('guarded', 'torch_guard')},
               'skipped_steps': og.skipped_steps, 'clip_rate': float(og.clip_rate), 'grad_norm': float(og.grad_norm)}
        a = rec['added_us_per_step']
        rec['guarded_beats_torch'] = bool(a['guarded']['max'] < a['torch_guard']['min'])
        # the launches alone, on the guarded model's buffers
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        gd, n = og._guard, mg._flat_params.numel()
        p, g, m_, v_ = mg._flat_params, mg._flat_grads, og._m, og._v
        g.normal_(std=1e-3)

        def adam_launch():
            _lib.check(lib.pivp_adam_step(p.data_ptr(), g.data_ptr(), m_.data_ptr(), v_.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1.0, stream), 'pivp_adam_step')

        def stats_launch():
            _lib.check(lib.pivp_grad_stats(g.data_ptr(), n, gd['seg_end'].data_ptr(), gd['seg_group'].data_ptr(), gd['nseg'], 6, 1.0, THRESHOLD,
                                           gd['ws'].data_ptr(), gd['stats'].data_ptr(), stream), 'pivp_grad_stats')

        def guarded_launch():
            _lib.check(lib.pivp_adam_step_guarded(p.data_ptr(), g.data_ptr(), m_.data_ptr(), v_.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1.0,
                                                  gd['stats'].data_ptr(), 1, og._skipped.data_ptr(), stream), 'pivp_adam_step_guarded')

        def torch_ops():
            torch_guard_ops(mg, og, lambda: None)
        stats_launch()
        rec['us_per_call'] = {name: round(min(timed(fn, 200) for _ in range(3)) * 1e3, 2)
                              for name, fn in (('pivp_adam_step', adam_launch), ('pivp_grad_stats', stats_launch),
                                               ('pivp_adam_step_guarded', guarded_launch), ('torch_guard_ops_without_adam', torch_ops))}
        rec['grad_bytes'] = n * 4
        rec['segments'] = gd['nseg']
        out['plans'][precision] = rec
        del mp, mg, mt, op, og, ot
        torch.cuda.empty_cache()
    out['guarded_beats_torch_all'] = all(r['guarded_beats_torch'] for r in out['plans'].values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
