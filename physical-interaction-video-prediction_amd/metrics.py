"""Per-sample quality of predicted frames, as video-prediction work reports it (Finn et al. 2016, fig. 5 and 6): MSE, PSNR and SSIM of every
predicted frame against its ground truth, and their statistics per prediction step over a data set.

`frame_metrics` is one launch of pivp_frame_metrics (include/pivp_hip.h) on frames that are already on the device: SSIM after Wang et al. 2004
with the 11-tap sigma-1.5 Gaussian window over valid positions, as tf.image.ssim and scikit-image (gaussian_weights=True,
use_sample_covariance=False) compute it.  `StepCurves` accumulates the per-step mean / std / min / max over batches on the tensors' device.
`Model.evaluate` and `python -m pivp_amd.evaluate` are built on the two.  There is no CPU fallback for `frame_metrics`; `StepCurves` is plain
torch and runs anywhere.

`psnr_all` of the model is another number: the PSNR of the batch-mean MSE (TM:739-756), which depends on the batch size and is not a mean of
per-sample PSNRs."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MIN_WIN, MAX_WIN = 3, 11
METRICS = ('mse', 'psnr', 'ssim')


def _shape(a):
    return tuple(a.shape) if torch.is_tensor(a) else tuple(np.shape(a))


def _check_metric_args(pred_shape, truth_shape, win, sigma, data_range):
    """-> (lead shape, N, C, H, W, win, sigma, data_range); every complaint is a ValueError raised before the GPU or the library is needed."""
    if pred_shape != truth_shape:
        raise ValueError('pred and truth must have the same shape, got %s and %s' % (pred_shape, truth_shape))
    if len(pred_shape) < 3:
        raise ValueError('frames are (..., C, H, W), got shape %s' % (pred_shape,))
    if isinstance(win, bool) or not isinstance(win, (int, np.integer)):
        raise ValueError('win must be an integer, not %r' % (win,))
    win = int(win)
    if win < MIN_WIN or win > MAX_WIN or win % 2 == 0:
        raise ValueError('win must be odd, %d .. %d, got %d' % (MIN_WIN, MAX_WIN, win))
    try:
        sigma, data_range = float(sigma), float(data_range)
    except (TypeError, ValueError):
        raise ValueError('sigma and data_range must be numbers, got %r and %r' % (sigma, data_range))
    if not math.isfinite(sigma):
        raise ValueError('sigma must be finite (<= 0: the uniform window), got %r' % sigma)
    if not math.isfinite(data_range) or data_range <= 0.0:
        raise ValueError('data_range must be positive and finite, got %r' % data_range)
    C, H, W = pred_shape[-3:]
    lead = pred_shape[:-3]
    N = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if N < 1 or C < 1:
        raise ValueError('no frames: shape %s' % (pred_shape,))
    if H < win or W < win:
        raise ValueError('%d x %d frames are smaller than the %d x %d window' % (H, W, win, win))
    if C * H * W >= 2 ** 31 or N >= 2 ** 31:
        raise ValueError('frames too large: shape %s' % (pred_shape,))
    return lead, N, C, H, W, win, sigma, data_range


def _launch(pred, truth, N, C, H, W, win, sigma, data_range, lead):
    """pivp_frame_metrics on contiguous fp32 tensors of one device (the caller holds the device context) -> namespace of `lead`-shaped tensors."""
    lib = _lib.load()
    mse = torch.empty(N, dtype=torch.float32, device=pred.device)
    ssim = torch.empty(N, dtype=torch.float32, device=pred.device)
    _lib.check(lib.pivp_frame_metrics(pred.data_ptr(), truth.data_ptr(), N, C, H, W, win, sigma, data_range, mse.data_ptr(), ssim.data_ptr(),
                                      torch.cuda.current_stream(pred.device).cuda_stream), 'pivp_frame_metrics')
    # identical frames: mse == 0 -> +inf, as the definition has it
    psnr = 10.0 * torch.log10((data_range * data_range) / mse)
    return SimpleNamespace(mse=mse.view(lead), psnr=psnr.view(lead), ssim=ssim.view(lead))


def frame_metrics(pred, truth, win=11, sigma=1.5, data_range=1.0, device=None):
    """MSE, PSNR and SSIM of every frame of `pred` against `truth`: (..., C, H, W) tensors or arrays of equal shape -> SimpleNamespace(mse, psnr,
    ssim) of (...)-shaped fp32 tensors on the device.  Device input is used where it lies, host input is uploaded (to `device`, default the
    other argument's device or cuda:0).  win: odd window size 3 .. 11; sigma: the Gaussian's, <= 0 for the uniform window; data_range: the
    value range L of the frames.  psnr = 10 log10(L^2 / mse), +inf for identical frames.  One kernel launch, no host synchronisation."""
    lead, N, C, H, W, win, sigma, data_range = _check_metric_args(_shape(pred), _shape(truth), win, sigma, data_range)
    if not torch.cuda.is_available():
        raise RuntimeError('no MI355X visible: this path has no CPU fallback (torch.cuda.is_available() is False)')
    _lib.load()
    if device is None:
        device = next((a.device for a in (pred, truth) if torch.is_tensor(a) and a.is_cuda), torch.device('cuda:0'))
    device = torch.device(device)

    def dev(a):
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
        return a.to(device=device, dtype=torch.float32).contiguous()
    with torch.cuda.device(device):
        return _launch(dev(pred), dev(truth), N, C, H, W, win, sigma, data_range, lead)


class StepCurves(object):
    """Running per-step statistics of mse / psnr / ssim over batches.  `add(m)` takes a namespace of (S, B) tensors (what `Model.evaluate`
    returns; B may differ from batch to batch, S may not); `result()` -> {metric: {mean, std, min, max, count, n_inf}} of length-S float64 arrays
    (std with ddof = 0).  Counts, means, sums of squared deviations and extrema stay on the tensors' device, in float64; only `result()`
    synchronises.  A non-finite value (the +inf PSNR of identical frames) is counted in n_inf and left out of every moment and extremum."""

    def __init__(self):
        self._acc = None
        self.steps = None

    def add(self, m):
        vals = {k: getattr(m, k) for k in METRICS}
        for k, v in vals.items():
            if not torch.is_tensor(v) or v.dim() != 2:
                raise ValueError('%s must be an (S, B) tensor, got %r' % (k, _shape(v) if hasattr(v, 'shape') else type(v)))
        shapes = {tuple(v.shape) for v in vals.values()}
        if len(shapes) != 1:
            raise ValueError('mse, psnr and ssim differ in shape: %s' % sorted(shapes))
        S = vals['mse'].shape[0]
        if self.steps is None:
            self.steps = S
            self._acc = {}
        elif S != self.steps:
            raise ValueError('this accumulator holds %d steps, got %d' % (self.steps, S))
        for k, v in vals.items():
            v = v.detach().to(torch.float64)
            ok = torch.isfinite(v)
            zero, inf = torch.zeros_like(v), torch.full_like(v, math.inf)
            pad = v.new_full((S, 1), math.inf)      # a step with nothing finite (or an empty batch) keeps +inf / -inf as its extrema
            n = ok.sum(dim=1)
            mean = torch.where(ok, v, zero).sum(dim=1) / n.clamp(min=1).to(torch.float64)
            dev = torch.where(ok, v - mean[:, None], zero)
            new = dict(n=n, n_inf=(~ok).sum(dim=1), mean=mean, m2=(dev * dev).sum(dim=1),
                       lo=torch.cat((torch.where(ok, v, inf), pad), dim=1).amin(dim=1),
                       hi=torch.cat((torch.where(ok, v, -inf), -pad), dim=1).amax(dim=1))
            old = self._acc.get(k)
            if old is None:
                self._acc[k] = new
                continue
            new = {f: t.to(old['n'].device) for f, t in new.items()}
            # Chan et al. 1979: merge (count, mean, sum of squared deviations) of two groups without cancellation
            tot = old['n'] + new['n']
            frac = new['n'].to(torch.float64) / tot.clamp(min=1).to(torch.float64)      # (integer / integer would be a float32)
            delta = new['mean'] - old['mean']
            old['m2'] = old['m2'] + new['m2'] + delta * delta * old['n'].to(torch.float64) * frac
            old['mean'] = old['mean'] + delta * frac
            old['n'] = tot
            old['n_inf'] = old['n_inf'] + new['n_inf']
            old['lo'] = torch.minimum(old['lo'], new['lo'])
            old['hi'] = torch.maximum(old['hi'], new['hi'])

    def result(self):
        if self._acc is None:
            raise RuntimeError('nothing was added')
        out = {}
        for k, a in self._acc.items():
            h = {f: t.cpu().numpy() for f, t in a.items()}
            none = h['n'] == 0
            std = np.sqrt(h['m2'] / np.maximum(h['n'], 1))
            out[k] = dict(mean=np.where(none, np.nan, h['mean']), std=np.where(none, np.nan, std), min=np.where(none, np.nan, h['lo']),
                          max=np.where(none, np.nan, h['hi']), count=h['n'].astype(np.int64), n_inf=h['n_inf'].astype(np.int64))
        return out
