"""Cost of Model(deterministic=True): the train step (optimizer.update = forward + BPTT sweep + Adam) in ms, default against deterministic, at
config 2 (fp32) and with config 3's arithmetic (bf16), B = 32, T = 10, CDNA, feed-self, one GPU.  All four Models live in one process; after a
warm-up their steps are timed in interleaved rounds (default, deterministic, default, ...) so that clock and thermal drift hit both alike, and
the median over the rounds is reported.

    python scripts/bench_deterministic.py [rounds] [steps per round]"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
import pivp_amd
from oracle import restatement as R

P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
x = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in R.synthetic_batch(32, 10)]


def make(prec, det):
    m = pivp_amd.Model(10, prefix='b', keep_activations=True, precision=prec, deterministic=det)
    m.load_state_dict_reference(P)
    opt = pivp_amd.Adam(alpha=1e-4).setup(m)
    return m, opt


def run(m, opt, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        opt.update(m, x, i)
        m.reset_state()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


out = {}
for prec in ('fp32', 'bf16'):
    legs = {det: make(prec, det) for det in (False, True)}
    for det in (False, True):
        run(*legs[det], 5)          # warm-up: plans, packs, allocator, clocks
    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for det in (False, True):
            ms[det].append(run(*legs[det], STEPS))
    d, t = float(np.median(ms[False])), float(np.median(ms[True]))
    out[prec] = {'default_ms': round(d, 3), 'deterministic_ms': round(t, 3), 'ratio': round(t / d, 4),
                 'default_ms_all': [round(v, 3) for v in ms[False]], 'deterministic_ms_all': [round(v, 3) for v in ms[True]]}
    del legs
    torch.cuda.empty_cache()
print(json.dumps({'batch': 32, 'seq_len': 10, 'model': 'CDNA', 'rounds': ROUNDS, 'steps_per_round': STEPS,
                  'device': torch.cuda.get_device_name(0), 'train_step': out}))
