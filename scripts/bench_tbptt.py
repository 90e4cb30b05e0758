"""What back-propagating through a carried recurrent state costs (include/pivp_state_grad.h; profiles/r16/NOTES.md), by the method of
scripts/bench_belief.py: config 2 shapes (CDNA, B = 32, T = 10, 64 x 64), precision fp32 and bf16.

Legs, interleaved round by round on one device (each: 2 warm-up runs, then `--steps` runs between two HIP events):
    sweep_zeros         `backward()` behind a call that started from zeros (the sweep as it always was)
    sweep_carried       `backward()` behind a call that started from the state the call before it left (state_backward=True): t = 0 has an h operand
    sweep_carried_isg   ... with initial_state_grad=True: t = 0 also forms the h columns of its data gradients, and the gather launch
    sweep_seeded_isg    ... and final_state_grad: the scatter launch in front of the sweep
    one_sweep_2T        one call and `backward()` over 2 T = 20 frames (the activation slabs of 19 steps)
    chunked_2xT         `chunked_backward` over the same frames as two windows of T (slabs of 9 steps; window 1 runs forward twice)
    truncated_2xT       the two windows, each one call and `backward()`, the state carried: what train.py --tbptt_windows 2 runs per sequence, without Adam
and, on their own (microseconds per launch, back-to-back launches, the best of three series of 200): the gather and the scatter at B = 32.
Expected, unmeasured before: the carried sweep costs the zero-start one plus roughly the h half of t = 0's data and weight gradients; the two
launches sit in the tens of microseconds, as pivp_state_copy does.  Prints one JSON line.

    python scripts/bench_tbptt.py [--rounds 7] [--steps 10]"""
import argparse
import ctypes
import gc
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, SIZE = 32, 10, 64
CX = (32, 32, 32, 64, 64, 128, 96)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import _lib
    from pivp_amd import state as ST
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    P = R.init_params_widened(seed=1, scale=1.0)
    imgs, acts, stas = (torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev) for a in R.synthetic_batch(B, 2 * T, SIZE, SIZE))
    whole = [imgs, acts, stas]
    wins = [[imgs[:T], acts[:T], stas[:T]], [imgs[T:], acts[T:], stas[T:]]]

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

    def model(precision, **kw):
        m = pivp_amd.Model(10, prefix='bench', keep_activations=True, precision=precision, **kw)
        m.load_state_dict_reference(P)
        return m

    def rounds_of(legs):
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                series[name].append(timed(step, args.steps))
        return {n: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
                    'rounds': [round(float(x), 4) for x in v]} for n, v in series.items()}

    out = {'shape': 'CDNA B=%d T=%d %dx%d' % (B, T, SIZE, SIZE), 'rounds': args.rounds, 'steps': args.steps, 'precisions': {}}
    # Two groups of legs, each with TWO training plans alive: every plan that has swept owns a side stream, and a process has four hardware queues by
    # default -- with four plans alive some legs measure up to 2.8 x slower than the same sweep measured alone (profiles/r16/NOTES.md).
    for precision in args.precisions:
        rec = {'ms': {}}
        zeros = model(precision)
        zeros(wins[1], 0)
        zeros.cleargrads()
        carried = model(precision, carry_state=True, state_backward=True)
        carried(wins[0], 0); carried(wins[1], 0)
        carried.cleargrads()
        seed = ST.RecurrentState(torch.randn(B * ST.state_layout(SIZE, SIZE)[1], device=dev) * 1e-6, B, (SIZE, SIZE))
        rec['ms'].update(rounds_of([('sweep_zeros', zeros.backward), ('sweep_carried', carried.backward),
                                    ('sweep_carried_isg', lambda: carried.backward(initial_state_grad=True)),
                                    ('sweep_seeded_isg', lambda: carried.backward(initial_state_grad=True, final_state_grad=seed))]))
        rec['workspace_MB'] = {'T': round(carried._active.workspace.numel() * 4 / 1e6, 1)}
        del zeros, carried
        gc.collect(); torch.cuda.empty_cache()
        long = model(precision)
        long(whole, 0)
        long.cleargrads()
        chunk = model(precision, carry_state=True, state_backward=True)
        chunk(wins[0], 0)
        chunk.cleargrads()

        def one_sweep():
            long.reset_state()
            long(whole, 0)
            long.backward()

        def chunked():
            chunk.reset_state()
            pivp_amd.chunked_backward(chunk, wins, iter_num=0)

        def truncated():
            chunk.reset_state()
            for w in wins:
                chunk(w, 0)
                chunk.backward()
        rec['ms'].update(rounds_of([('one_sweep_2T', one_sweep), ('chunked_2xT', chunked), ('truncated_2xT', truncated)]))
        rec['workspace_MB']['2T'] = round(long._active.workspace.numel() * 4 / 1e6, 1)
        out['precisions'][precision] = rec
        del long, chunk
        gc.collect(); torch.cuda.empty_cache()
    # the two launches alone
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = ST._config(SIZE, SIZE)
    cfg.batch = B
    shapes = [(B, SIZE // lv, SIZE // lv, C) for lv, C in zip(ST.CELL_LEVELS, ST.CELL_CHANNELS)]
    dc = [torch.randn(s, device=dev) for s in shapes]
    din = [torch.randn(s[:3] + (cx + s[3],), device=dev) for s, cx in zip(shapes, CX)]
    dst = ST.RecurrentState.empty(B, (SIZE, SIZE), dev)
    ptrs = lambda ts: (ctypes.c_void_p * 7)(*[t.data_ptr() for t in ts])
    pdc, pdin = ptrs(dc), ptrs(din)

    def gather():
        _lib.check(lib.pivp_state_grad_gather(ctypes.byref(cfg), pdc, pdin, dst.data.data_ptr(), stream), 'pivp_state_grad_gather')

    def scatter():
        _lib.check(lib.pivp_state_grad_scatter(ctypes.byref(cfg), dst.data.data_ptr(), pdc, stream), 'pivp_state_grad_scatter')
    out['us_per_launch'] = {'gather': round(min(timed(gather, 200) for _ in range(3)) * 1e3, 2),
                            'scatter': round(min(timed(scatter, 200) for _ in range(3)) * 1e3, 2)}
    out['state_bytes'] = dst.data.numel() * 4
    print(json.dumps(out))


if __name__ == '__main__':
    main()
