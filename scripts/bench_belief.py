"""What planning from a belief costs and saves (CDNA, 64 x 64, ctx 2, horizon 9, one designated pixel, 3 iterations; profiles/r15/NOTES.md), by the
method of scripts/bench_plan.py.

Settings: samples K = 32 and, if the inference workspace at batch 128 fits, K = 128; precision fp32 and bf16.  Legs, interleaved round by round on one
device (each: 2 warm-up plans, then `--steps` plans between two HIP events; one plan = 3 iterations, so milliseconds per iteration = per plan / 3):
    cem_frames   planning._cem_iterate on buffers uploaded once: every rollout runs ctx-1 + horizon = 10 steps from zeros over both context frames
    cem_belief   the same loop from a belief (`cem_plan(belief=...)`'s): every rollout runs horizon = 9 steps from the expanded state
and, on their own (microseconds per launch, back-to-back launches, the best of three series of 200):
    pack         the launch that leaves a rollout's final state behind its last step (pivp_state_copy over the fourteen segments, identity, batch K)
    expand       `RecurrentState.expand(K)`'s launch: a batch-1 state to K samples (pivp_state_copy with an all-zero index)
with the bytes each moves.  The only expectation there is: 9 steps for 10, a tenth fewer.  Prints one JSON line.

    python scripts/bench_belief.py [--rounds 7] [--steps 10]"""
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
    from pivp_amd import state as ST
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    S = SIZE
    imgs, acts, stas = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in R.synthetic_batch(1, CTX + 1, S, S))
    designated, goal = (32, 32), (40, 24)
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

    out = {'shape': 'CDNA ctx=%d horizon=%d P=1 iterations=%d elites=%d %dx%d' % (CTX, HORIZON, ITERS, ELITES, S, S), 'rounds': args.rounds,
           'steps': args.steps, 'settings': {}, 'skipped': []}
    per_sample = ST.state_layout(S, S)[1]
    for precision in args.precisions:
        for K in args.samples:
            tag = '%s_K%d' % (precision, K)
            m = pivp_amd.Model(10, prefix='bench', keep_activations=False, precision=precision, carry_state=True)
            try:
                # the belief: a model has seen frame 0 and taken action 0; frame 1 is the newest frame, the predicted robot state its state.  The
                # observer is an fp32 model at batch 1 (the state is fp32 in every mode; the bf16 gate kernels do not take batch 1 at this size)
                seer = pivp_amd.Model(10, prefix='bench', keep_activations=False, carry_state=True)
                seer.imagine(imgs[:1], acts[:1], stas[0], observed=1)
                belief, state1 = seer.recurrent_state(), seer.gen_states[-1].clone()
                del seer
                kw = dict(designated_rc=[designated], goal_rc=[goal], horizon=HORIZON, iterations=ITERS, samples=K, elites=ELITES, action_low=-2.0,
                          action_high=2.0, seed=1)
                a_frames = planning._check_cem_args(m, imgs[:CTX], stas[0], past_actions=acts[:CTX - 1, 0], **kw)
                a_belief = planning._check_cem_args(m, imgs[1:2], state1, belief=belief, **kw)
                b_frames = planning._cem_upload(m, a_frames, imgs[:CTX], stas[0])
                b_belief = planning._cem_upload(m, a_belief, imgs[1:2], state1)
                planning._cem_iterate(m, a_frames, b_frames)
                planning._cem_iterate(m, a_belief, b_belief)
                torch.cuda.synchronize()
            except (RuntimeError, _lib.PivpError) as e:      # the workspace at this batch does not fit
                out['skipped'].append({'setting': tag, 'reason': str(e)[:200]})
                continue
            legs = [('cem_frames', lambda: planning._cem_iterate(m, a_frames, b_frames)), ('cem_belief', lambda: planning._cem_iterate(m, a_belief, b_belief))]
            series = {name: [] for name, _ in legs}
            for _ in range(args.rounds):
                for name, step in legs:
                    series[name].append(timed(step, args.steps) / ITERS)
            rec = {'ms_per_iteration': {n: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
                                            'rounds': [round(float(x), 4) for x in v]} for n, v in series.items()}}
            gain = 1.0 - np.array(series['cem_belief']) / np.array(series['cem_frames'])
            rec['gain'] = {'median': round(float(np.median(gain)), 4), 'min': round(float(gain.min()), 4), 'max': round(float(gain.max()), 4)}
            rec['steps_per_rollout'] = {'cem_frames': CTX - 1 + HORIZON, 'cem_belief': HORIZON}
            # the two launches alone
            stream = torch.cuda.current_stream().cuda_stream
            cfg = ST._config(S, S)
            full, copy = b_belief.belief, ST.RecurrentState.empty(K, (S, S), dev)
            zeros = torch.zeros(K, dtype=torch.int32, device=dev)

            def pack():
                _lib.check(lib.pivp_state_copy(ctypes.byref(cfg), full.data.data_ptr(), K, copy.data.data_ptr(), K, None, stream), 'pivp_state_copy')

            def expand():
                _lib.check(lib.pivp_state_copy(ctypes.byref(cfg), belief.data.data_ptr(), 1, copy.data.data_ptr(), K, zeros.data_ptr(), stream), 'pivp_state_copy')
            rec['us_per_launch'] = {'pack': round(min(timed(pack, 200) for _ in range(3)) * 1e3, 2),
                                    'expand': round(min(timed(expand, 200) for _ in range(3)) * 1e3, 2)}
            rec['state_bytes'] = K * per_sample * 4
            rec['expand_api_us'] = round(min(timed(lambda: belief.expand(K), 50) for _ in range(3)) * 1e3, 2)      # with its index upload and allocation
            out['settings'][tag] = rec
            del m, b_frames, b_belief, full, copy
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
