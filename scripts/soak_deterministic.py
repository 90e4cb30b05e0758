"""Soak check of Model(deterministic=True) at config 2's size (B = 32, T = 10, CDNA, feed-self; 'bf16' = config 3's arithmetic): N sweeps in one
Model, one in a fresh Model and one with the side stream off must give the same flat gradient, bit for bit (torch.equal).

    python scripts/soak_deterministic.py N {fp32,bf16}"""
import os, sys
import numpy as np, torch
sys.path.insert(0, '.')
N = int(sys.argv[1]) if len(sys.argv) > 1 else 40
prec = sys.argv[2] if len(sys.argv) > 2 else 'fp32'
import pivp_amd
from oracle import restatement as R
P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
imgs, acts, stas = R.synthetic_batch(32, 10)


def grads(side, n):
    os.environ['PIVP_SIDE_STREAM'] = side      # read when a plan is created
    m = pivp_amd.Model(10, prefix='s', keep_activations=True, precision=prec, deterministic=True)
    m.load_state_dict_reference(P)
    out = []
    for _ in range(n):
        m.reset_state()
        m([imgs, acts, stas], 0)
        m.cleargrads(); m.backward()
        out.append(m._flat_grads.clone())
    torch.cuda.synchronize()
    return out


ref = grads('1', 1)[0]
assert bool(torch.isfinite(ref).all())
runs = [('one Model, sweep %d' % i, g) for i, g in enumerate(grads('1', N))]
runs.append(('fresh Model', grads('1', 1)[0]))
runs.append(('PIVP_SIDE_STREAM=0', grads('0', 1)[0]))
bad = [(what, int((g != ref).sum())) for what, g in runs if not torch.equal(g, ref)]
for what, n in bad:
    print('DIFFERS: %s (%d elements)' % (what, n))
print('%s: %d sweeps + a fresh Model + PIVP_SIDE_STREAM=0 against a first Model: %s' % (prec, N, 'bit-identical' if not bad else '%d differ' % len(bad)))
assert not bad
