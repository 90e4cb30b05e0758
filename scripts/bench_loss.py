"""Cost of the L1 / GDL / DSSIM image loss around the train step (config 2's model: CDNA, 64 x 64, batch 32, 10 frames; profiles/r13/NOTES.md).

Plans: precision fp32 and bf16.  Legs, interleaved round by round on one device (each: 2 warm-up steps, then `--steps` steps between two HIP events;
one step = reset_state + forward + backward + Adam, inputs resident on the device):
    off           Model(image_loss=None): the parent's arithmetic -- the yardstick, to be held against the parent's recorded step (PARENT_MS)
    on            Model(image_loss=ImageLoss(0.5, 0.2, 0.1, 0.3)): one pivp_image_loss call behind the rollout, its gradient through the seed hook
    torch_loss    the same loss composed in torch on the predicted frames (float32 conv2d for the window, autograd for the gradient) and fed through
                  backward(frame_grad=...): what a user could do with the hook alone
and the op on its own on 256 frames of 3 x 64 x 64 (microseconds per call, back-to-back calls): the pointwise terms, DSSIM, all four, each with and
without the gradient, with the bytes they must move (pred and truth read, the gradient written) against the HBM figure of scripts/roofline_table.py.
Reported per plan: milliseconds per step and the microseconds each form adds to `off`, per round (median, min, max).  Prints one JSON line.

    python scripts/bench_loss.py [--rounds 7] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH, FRAMES, SIZE, CTX = 32, 10, 64, 2
WEIGHTS = (0.5, 0.2, 0.1, 0.3)
PEAK_TBS = 8.0                                                # scripts/roofline_table.py
PARENT_MS = {'fp32': (26.866, 26.811, 26.903), 'bf16': (10.412, 10.393, 10.433)}      # the parent's plain step: median (min, max), profiles/r12/NOTES.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import torch.nn.functional as F
    import pivp_amd
    from pivp_amd import losses
    from oracle import restatement as R
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    x = [torch.tensor(np.asarray(a, dtype=np.float32), device=dev) for a in R.synthetic_batch(BATCH, FRAMES, SIZE, SIZE)]
    spec = pivp_amd.ImageLoss(*WEIGHTS)
    w1 = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5.0) ** 2 / (2 * 1.5 ** 2))
    w1 = (w1 / w1.sum()).to(torch.float32).to(dev)
    win2d = (w1[:, None] * w1[None, :]).expand(3, 1, 11, 11).contiguous()

    def torch_total(y, t):
        """the loss beyond the reference's own MSE, float32: (mse - 1) MSE + l1 L1 + gdl GDL + dssim (1 - SSIM), means over the 256 frames"""
        d = y - t
        tot = (WEIGHTS[0] - 1.0) * (d * d).mean() + WEIGHTS[1] * d.abs().mean()
        gv = ((y[:, :, 1:] - y[:, :, :-1]).abs() - (t[:, :, 1:] - t[:, :, :-1]).abs()).abs().mean()
        gh = ((y[..., 1:] - y[..., :-1]).abs() - (t[..., 1:] - t[..., :-1]).abs()).abs().mean()
        tot = tot + WEIGHTS[2] * (gv + gh)
        f = lambda a: F.conv2d(a, win2d, groups=3)
        mx, my = f(t), f(y)
        sx, sy, sxy = f(t * t) - mx * mx, f(y * y) - my * my, f(t * y) - mx * my
        s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
        return tot + WEIGHTS[3] * (1.0 - s.mean())

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

    out = {'shape': 'CDNA B=%d T=%d %dx%d' % (BATCH, FRAMES, SIZE, SIZE), 'weights': WEIGHTS, 'rounds': args.rounds, 'steps': args.steps, 'plans': {}}
    for precision in args.precisions:
        def fresh(**kw):
            m = pivp_amd.Model(10, prefix='bench', keep_activations=True, precision=precision, **kw)
            return m, pivp_amd.Adam(alpha=0.001).setup(m)
        (m0, o0), (m1, o1), (mt, ot) = fresh(), fresh(image_loss=spec), fresh()

        def off():
            m0.reset_state()
            return o0.update(m0, x, 0)

        def on():
            m1.reset_state()
            return o1.update(m1, x, 0)

        def torch_loss():
            mt.reset_state()
            loss = mt(x, 0)
            y = mt._gen[CTX - 1:].reshape(-1, 3, SIZE, SIZE).detach().requires_grad_(True)
            extra = torch_total(y, x[0][CTX:].reshape(-1, 3, SIZE, SIZE))
            g, = torch.autograd.grad(extra, y)
            mt.cleargrads()
            mt.backward(frame_grad=g.view(FRAMES - CTX, BATCH, 3, SIZE, SIZE))
            ot._state(mt)
            ot.step(mt)
            return loss + extra.detach()

        legs = [('off', off), ('on', on), ('torch_loss', torch_loss)]
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                series[name].append(timed(step, args.steps))
        base = np.array(series['off'])
        rec = {'ms_per_step': {n: summary(v) for n, v in series.items()},
               'added_us_per_step': {n: dict(summary((np.array(series[n]) - base) * 1e3, 1), rounds=[round(float(d), 1) for d in (np.array(series[n]) - base) * 1e3])
                                     for n in ('on', 'torch_loss')},
               'parent_ms_per_step': dict(zip(('median', 'min', 'max'), PARENT_MS[precision])) if precision in PARENT_MS else None,
               'loss_on': float(on()), 'loss_torch': float(torch_loss())}
        a = rec['added_us_per_step']
        rec['fused_beats_torch'] = bool(a['on']['max'] < a['torch_loss']['min'])
        out['plans'][precision] = rec
        del m0, m1, mt, o0, o1, ot
        torch.cuda.empty_cache()
    # the op alone, on noise frames of config 2's size
    N = (FRAMES - CTX) * BATCH
    y = torch.rand(N, 3, SIZE, SIZE, device=dev)
    t = torch.rand(N, 3, SIZE, SIZE, device=dev)
    moved = 3 * N * 3 * SIZE * SIZE * 4
    alone = {}
    for name, wts in (('pointwise', (0.5, 0.2, 0.1, 0.0)), ('dssim', (0.0, 0.0, 0.0, 0.3)), ('all', WEIGHTS)):
        s = pivp_amd.ImageLoss(*wts)._struct()
        for want in (True, False):
            us = min(timed(lambda: losses._launch(y, t, N, 3, SIZE, SIZE, s, want, (N,)), 200) for _ in range(3)) * 1e3
            nbytes = moved if want else moved * 2 // 3
            alone['%s%s' % (name, '' if want else '_no_grad')] = {'us_per_call': round(us, 2), 'bytes': nbytes, 'tb_per_s': round(nbytes / us * 1e-6, 3),
                                                                   'of_hbm': round(nbytes / us * 1e-6 / PEAK_TBS, 4)}
    out['op_alone'] = alone
    out['fused_beats_torch_all'] = all(r['fused_beats_torch'] for r in out['plans'].values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
