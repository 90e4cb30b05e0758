"""NumPy restatement of pivp_frame_metrics (include/pivp_hip.h), written from the definition as explicit shifted sums: Wang et al. 2004 with a
separable window over the valid positions, biased weighted moments.  dtype=float64 is the reference of the GPU tests; dtype=float32 is the
"plain float32" formulation (E[x^2] - mu^2 on raw pixels, everything in fp32) whose error the GPU tests print beside the kernel's and never gate."""
import numpy as np


def window(win, sigma, dtype=np.float64):
    """w_i ~ exp(-(i - (win-1)/2)^2 / (2 sigma^2)), normalised to sum 1 in double; sigma <= 0: uniform."""
    i = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-(i * i) / (2.0 * float(sigma) ** 2)) if sigma > 0 else np.ones(win)
    return (w / w.sum()).astype(dtype)


def _filter(a, w):
    """Valid separable correlation of the last two axes with w: horizontal taps first, then vertical, each an explicit shifted sum."""
    win = len(w)
    H, W = a.shape[-2:]
    h = np.zeros(a.shape[:-1] + (W - win + 1,), a.dtype)
    for k in range(win):
        h = h + w[k] * a[..., :, k:k + W - win + 1]
    v = np.zeros(a.shape[:-2] + (H - win + 1, W - win + 1), a.dtype)
    for k in range(win):
        v = v + w[k] * h[..., k:k + H - win + 1, :]
    return v


def ssim_map(pred, truth, win=11, sigma=1.5, data_range=1.0, dtype=np.float64):
    x, y = np.asarray(pred).astype(dtype), np.asarray(truth).astype(dtype)
    w = window(win, sigma, dtype)
    L = dtype(data_range)
    C1, C2 = (dtype(0.01) * L) ** 2, (dtype(0.03) * L) ** 2
    mx, my = _filter(x, w), _filter(y, w)
    sx = _filter(x * x, w) - mx * mx
    sy = _filter(y * y, w) - my * my
    sxy = _filter(x * y, w) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))


def ssim_mse(pred, truth, win=11, sigma=1.5, data_range=1.0, dtype=np.float64):
    """pred, truth (..., C, H, W) -> (ssim, mse) of shape (...), computed in `dtype` throughout."""
    x, y = np.asarray(pred).astype(dtype), np.asarray(truth).astype(dtype)
    if x.shape != y.shape or x.ndim < 3 or win % 2 == 0 or min(x.shape[-2:]) < win:
        raise ValueError('bad arguments: shapes %s / %s, win %d' % (x.shape, y.shape, win))
    s = ssim_map(x, y, win, sigma, data_range, dtype)
    d = x - y
    return s.mean(axis=(-3, -2, -1), dtype=dtype), (d * d).mean(axis=(-3, -2, -1), dtype=dtype)


def psnr(mse, data_range=1.0):
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(float(data_range) ** 2 / np.asarray(mse, dtype=np.float64))
