"""Cost of open-loop prediction and of designated-pixel tracking at config 2's shapes (B = 32, T = 10, 64 x 64; profiles/r08/NOTES.md).

Legs, interleaved round by round on one device (each: 2 warm-up steps, then K steps between two HIP events):
    call        Model.__call__ under using_config('train', False)           the rollout bench.py times
    imagine_p0  Model.imagine without planes                                 the same steps without the two loss launches
    imagine_pN  Model.imagine with N tracked planes (N = 1, 4, 8)             + masks_out at every step + one pixel_track launch per step
and pivp_pixel_track on its own for the three heads (microseconds per launch, back-to-back launches).
Prints one JSON line.

    python scripts/bench_imagine.py [--model CDNA] [--rounds 7] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='CDNA', choices=['CDNA', 'STP', 'DNA'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seq-len', type=int, default=10)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    args = ap.parse_args()
    import torch
    import pivp_amd
    from pivp_amd import _lib, planning
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    B, T, S = args.batch, args.seq_len, args.size
    nm = 1 if args.model == 'DNA' else 10
    imgs, acts, stas = (torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev) for a in R.synthetic_batch(B, T, S, S))
    m = pivp_amd.Model(nm, is_cdna=args.model == 'CDNA', is_stp=args.model == 'STP', is_dna=args.model == 'DNA', prefix='bench', keep_activations=False)
    ctx = imgs[:2].contiguous()
    actions, state0 = acts[:T - 1].contiguous(), stas[0].contiguous()

    def planes(P):
        rs = np.random.RandomState(P)
        return planning.one_hot_planes(np.stack([rs.randint(8, S - 8, (B, P)), rs.randint(8, S - 8, (B, P))], axis=-1), S, S, device=dev)

    def call():
        m.reset_state()
        with pivp_amd.using_config('train', False):
            m([imgs, acts, stas], 0)

    def imagine(D):
        def step():
            m.reset_state()
            m.imagine(ctx, actions, state0, designated=D)
        return step

    legs = [('call', call), ('imagine_p0', imagine(None))] + [('imagine_p%d' % P, imagine(planes(P))) for P in (1, 4, 8)]

    def timed(step, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    series = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, step in legs:
            series[name].append(timed(step, args.steps))
    out = {'shape': '%s B=%d T=%d %dx%d' % (args.model, B, T, S, S), 'rounds': args.rounds, 'steps': args.steps, 'ms_per_rollout': {}}
    for name, v in series.items():
        out['ms_per_rollout'][name] = {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
    med = {k: v['median'] for k, v in out['ms_per_rollout'].items()}
    out['imagine_p0_minus_call_ms'] = round(med['imagine_p0'] - med['call'], 4)
    for P in (1, 4, 8):
        out['p%d_minus_p0_ms' % P] = round(med['imagine_p%d' % P] - med['imagine_p0'], 4)

    # the kernel on its own: the three heads, softmaxed masks of a uniform softmax
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    out['pixel_track_us_per_launch'] = {}
    for mt, code, n in (('CDNA', 0, 10), ('STP', 1, 10), ('DNA', 2, 1)):
        masks = torch.full((B, n + 1, S, S), 1.0 / (n + 1), device=dev)
        if code == 0:
            aux = torch.full((B, n, 25), 1.0 / 25, device=dev)
        elif code == 1:
            aux = torch.tensor([1.0, 0.02, 0.01, -0.02, 1.0, 0.03], device=dev).repeat(B, 1).contiguous()
        else:
            aux = torch.rand((B, 25, S, S), device=dev)
        for P in (1, 4, 8):
            a, b = planes(P), torch.empty((B, P, S, S), device=dev)

            def launch():
                _lib.check(lib.pivp_pixel_track(a.data_ptr(), masks.data_ptr(), aux.data_ptr(), b.data_ptr(), B, P, S, S, n, code, 0, stream), 'pivp_pixel_track')
            out['pixel_track_us_per_launch']['%s_p%d' % (mt, P)] = round(min(timed(launch, 200) for _ in range(3)) * 1e3, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
