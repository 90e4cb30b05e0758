"""Cost of on-device evaluation: pivp_frame_metrics (per-sample MSE + SSIM, one launch) against the same metric composed in torch
(profiles/r10/NOTES.md).

Sizes: N = 256 of 3 x 64 x 64 (the scored frames of BASELINE config 2: 8 steps x 32 samples), N = 36 of 3 x 128 x 128 (config 5 at B = 2) and
N = 4096 of 3 x 64 x 64 (a validation set in one call).  Legs, interleaved round by round in one process (each: 3 warm-up calls, then `--steps`
calls between two HIP events), inputs resident on the device:
    hip          one pivp_frame_metrics launch, both outputs
    torch_conv   the usual composition: the separable Gaussian as two grouped conv2d over x, y, x*x, y*y, x*y stacked as channels, then the SSIM
                 map and the means -- in float64, which the flat inputs need to meet the tests' 1e-6
    torch_shift  the same with the two filters written as sums of shifted slices (no convolution library involved), float64
    torch_conv32 the float32 form of torch_conv: reported for scale only, it does NOT meet 1e-6 (tests/test_gpu_metrics.py prints its error)
Each torch leg is first checked against the kernel's output (max difference, printed).  Reported: median and range over the rounds in
microseconds per call; `accept` = the kernel's slowest round lies below the fastest round of every float64 torch leg.  At N = 4096 also the share
of the HBM peak (8 TB/s) that 2 * N * C * H * W * 4 bytes in the kernel's median time come to.  Also: `Model.evaluate` minus `Model.__call__` at
config 2 (CDNA, B = 32, T = 10, 64 x 64).  Prints one JSON line.

    python scripts/bench_metrics.py [--rounds 7] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIN, SIGMA = 11, 1.5
HBM_PEAK = 8.0e12
SIZES = [(256, 3, 64, 64), (36, 3, 128, 128), (4096, 3, 64, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--skip_model', action='store_true')
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import torch.nn.functional as F
    import pivp_amd
    from pivp_amd import _lib
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3          # microseconds

    i = torch.arange(WIN, dtype=torch.float64) - (WIN - 1) / 2.0
    w64 = torch.exp(-(i * i) / (2.0 * SIGMA ** 2))
    w64 = (w64 / w64.sum()).to(dev)
    C1, C2 = 1e-4, 9e-4

    def ssim_from(mom, N, C):
        mx, my, xx, yy, xy = (mom[:, k * C:(k + 1) * C] for k in range(5))
        sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
        S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
        return S.mean(dim=(1, 2, 3))

    def torch_conv(x, y, dtype):
        N, C = x.shape[:2]
        x, y = x.to(dtype), y.to(dtype)
        w = w64.to(dtype)
        st = torch.cat((x, y, x * x, y * y, x * y), dim=1)
        st = F.conv2d(st, w.view(1, 1, 1, WIN).expand(5 * C, 1, 1, WIN), groups=5 * C)
        st = F.conv2d(st, w.view(1, 1, WIN, 1).expand(5 * C, 1, WIN, 1), groups=5 * C)
        d = x - y
        return (d * d).mean(dim=(1, 2, 3)), ssim_from(st, N, C)

    def torch_shift(x, y):
        N, C, H, W = x.shape
        x, y = x.double(), y.double()
        st = torch.cat((x, y, x * x, y * y, x * y), dim=1)
        h = sum(w64[k] * st[..., :, k:k + W - WIN + 1] for k in range(WIN))
        v = sum(w64[k] * h[..., k:k + H - WIN + 1, :] for k in range(WIN))
        d = x - y
        return (d * d).mean(dim=(1, 2, 3)), ssim_from(v, N, C)

    out = {'win': WIN, 'sigma': SIGMA, 'rounds': args.rounds, 'steps': args.steps, 'sizes': {}}
    for (N, C, H, W) in SIZES:
        g = torch.Generator(device='cpu').manual_seed(N)
        x = torch.rand((N, C, H, W), generator=g).to(dev)
        y = (x + 0.05 * torch.randn((N, C, H, W), generator=g).to(dev)).clamp(0, 1)
        mse = torch.empty(N, device=dev)
        ssim = torch.empty(N, device=dev)

        def hip():
            _lib.check(lib.pivp_frame_metrics(x.data_ptr(), y.data_ptr(), N, C, H, W, WIN, SIGMA, 1.0, mse.data_ptr(), ssim.data_ptr(), stream),
                       'pivp_frame_metrics')
        # a timed window of the kernel alone holds ten times the calls of a torch leg: tens of microseconds each need the count
        steps = {True: args.steps, False: max(3, args.steps // 4)}[N < 4096]
        legs = [('hip', hip)]
        rec = {'check_vs_hip': {}, 'skipped': {}}
        hip()
        torch.cuda.synchronize()
        for name, fn in (('torch_conv', lambda: torch_conv(x, y, torch.float64)), ('torch_shift', lambda: torch_shift(x, y)),
                         ('torch_conv32', lambda: torch_conv(x, y, torch.float32))):
            try:
                m_t, s_t = fn()
                torch.cuda.synchronize()
            except RuntimeError as e:                      # a composition this torch build does not serve (or that does not fit) is left out, by name
                rec['skipped'][name] = str(e)[:160]
                continue
            rec['check_vs_hip'][name] = {'ssim': float((s_t.double() - ssim.double()).abs().max()),
                                         'mse_rel': float(((m_t.double() - mse.double()).abs() / mse.double()).max())}
            legs.append((name, fn))
        series = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, fn in legs:
                series[name].append(timed(fn, steps * 10 if name == 'hip' else steps))
        rec['us_per_call'] = {n: {'median': round(float(np.median(v)), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)} for n, v in series.items()}
        f64 = [n for n in ('torch_conv', 'torch_shift') if n in series]
        rec['accept'] = bool(f64) and all(max(series['hip']) < min(series[n]) for n in f64)
        nbytes = 2 * N * C * H * W * 4
        rec['bytes'] = nbytes
        if N == 4096:
            rec['hbm_share'] = round(nbytes / (float(np.median(series['hip'])) * 1e-6) / HBM_PEAK, 4)
        out['sizes']['N%d_%dx%dx%d' % (N, C, H, W)] = rec
        del x, y
        torch.cuda.empty_cache()
    out['accept_all'] = all(r['accept'] for r in out['sizes'].values())

    if not args.skip_model:
        from oracle import restatement as R
        xs = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in R.synthetic_batch(32, 10)]
        m = pivp_amd.Model(10, prefix='bench', device='cuda:0')

        def call():
            with pivp_amd.using_config('train', False):
                m(xs)
            m.reset_state()

        def evaluate():
            m.evaluate(xs)
            m.reset_state()
        series = {'call': [], 'evaluate': []}
        for _ in range(args.rounds):
            series['call'].append(timed(call, 5))
            series['evaluate'].append(timed(evaluate, 5))
        diff = np.array(series['evaluate']) - np.array(series['call'])
        out['model_config2'] = {'call_us': round(float(np.median(series['call'])), 1), 'evaluate_us': round(float(np.median(series['evaluate'])), 1),
                                'evaluate_minus_call_us': {'median': round(float(np.median(diff)), 1), 'min': round(float(diff.min()), 1),
                                                           'max': round(float(diff.max()), 1)}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
