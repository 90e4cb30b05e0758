"""Cost of the input gradients and of the sweep's modes (CDNA, 64 x 64, B = 32, T = 10, ctx 2, feed-self; profiles/r14/NOTES.md).

Per precision (fp32, bf16), legs interleaved round by round on one device (each: 2 warm-up calls, then `--steps` calls between two HIP events):
    forward            the training-mode rollout (`model(x)` under config.train)
    sweep              `backward()`: flags 3, the sweep as it was
    sweep_input        `backward(input_grad=True)`: flags 3 plus one pivp_action_grad per timestep and the state copy
    sweep_seed_only    `backward(frame_grad=seed, input_grad=True, params=False, builtin_loss=False)`: flags 0 with a seed
    refine_1, refine_4 `planning._refine_iterate` with 1 and 4 iterations on buffers uploaded once; (refine_4 - refine_1) / 3 is ONE iteration of
                       `refine_actions` (rollout, cost and its gradient in torch, sweep, Adam)
and pivp_action_grad on its own (microseconds per launch, back-to-back launches).  Prints one JSON line.

    python scripts/bench_refine.py [--rounds 7] [--steps 10]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, CTX, SIZE = 32, 10, 2, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import _lib, planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    imgs, acts, stas = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in R.synthetic_batch(B, T, SIZE, SIZE))

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

    out = {'shape': 'CDNA B=%d T=%d ctx=%d %dx%d feed-self' % (B, T, CTX, SIZE, SIZE), 'rounds': args.rounds, 'steps': args.steps, 'settings': {}}
    for precision in args.precisions:
        m = pivp_amd.Model(10, prefix='bench', keep_activations=True, precision=precision)

        def forward():
            with pivp_amd.using_config('train', True):
                m([imgs, acts, stas], 0)

        forward()
        m.cleargrads()
        seed = torch.randn((T - CTX, B, 3, SIZE, SIZE), device=dev) * 1e-5
        goal = m._gen[-1].clone()
        a = {n: planning._check_refine_args(m, imgs[:CTX], stas[0], acts[:T - 1], goal, None, n, 0.01, acts[:CTX - 1], None) for n in (1, 4)}
        bufs = planning._refine_upload(m, a[1], imgs[:CTX], stas[0], acts[:T - 1], goal, acts[:CTX - 1])
        legs = [('forward', forward),
                ('sweep', lambda: m.backward()),
                ('sweep_input', lambda: m.backward(input_grad=True)),
                ('sweep_seed_only', lambda: m.backward(frame_grad=seed, input_grad=True, params=False, builtin_loss=False)),
                ('refine_1', lambda: planning._refine_iterate(m, a[1], bufs)),
                ('refine_4', lambda: planning._refine_iterate(m, a[4], bufs))]
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                if name.startswith('sweep'):
                    forward()      # (the refine legs leave their own rollout behind)
                series[name].append(timed(step, args.steps))
        stat = lambda v: {'median': round(float(np.median(v)), 4), 'min': round(float(np.min(v)), 4), 'max': round(float(np.max(v)), 4)}
        rec = {'ms': {n: stat(v) for n, v in series.items()}}
        s = {n: np.array(v) for n, v in series.items()}
        rec['input_grad_extra_ms'] = stat(s['sweep_input'] - s['sweep'])
        rec['seed_only_over_full'] = stat(s['sweep_seed_only'] / s['sweep'])
        rec['refine_iteration_ms'] = stat((s['refine_4'] - s['refine_1']) / 3.0)
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        e3, de3 = torch.randn((B, 64, 64), device=dev), torch.randn((B, 64, 192), device=dev)
        w3, wcs, ds, da = torch.randn((74, 64), device=dev), torch.randn((5, 10), device=dev), torch.randn((B, 5), device=dev), torch.empty((B, 5), device=dev)

        def launch():
            _lib.check(lib.pivp_action_grad(e3.data_ptr(), de3.data_ptr(), 192, w3.data_ptr(), wcs.data_ptr(), ds.data_ptr(), da.data_ptr(), B, 64, 1,
                                            stream), 'pivp_action_grad')
        rec['us_per_launch'] = {'pivp_action_grad': round(min(timed(launch, 200) for _ in range(3)) * 1e3, 2)}
        out['settings'][precision] = rec
        del m, bufs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
