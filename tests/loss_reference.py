"""Restatement of pivp_image_loss (include/pivp_loss.h) in torch, written from the definitions: per-image MSE, L1, gradient-difference loss
(Mathieu et al. 2016, alpha = 1) and DSSIM = 1 - SSIM (metrics_reference's SSIM: separable window as explicit shifted sums, valid positions,
biased moments), their means over the images, the weighted total and -- by autograd -- its gradient with respect to the prediction.
dtype=torch.float64 is the reference of the GPU tests; dtype=torch.float32 is the "plain float32 autograd" composition whose error the GPU tests
print beside the kernel's and never gate.  `ssim_grad_closed_form` is the three-map form the kernel uses, in NumPy float64."""
import numpy as np
import torch

import metrics_reference as MR

TERMS = ('mse', 'l1', 'gdl', 'dssim')


def _filter(a, w):
    """Valid separable correlation of the last two axes: horizontal taps first, then vertical (metrics_reference._filter on tensors)."""
    win = len(w)
    H, W = a.shape[-2:]
    h = 0
    for k in range(win):
        h = h + w[k] * a[..., :, k:k + W - win + 1]
    v = 0
    for k in range(win):
        v = v + w[k] * h[..., k:k + H - win + 1, :]
    return v


def ssim_map(y, x, win, sigma, data_range):
    w = torch.tensor(MR.window(win, sigma), dtype=y.dtype)
    L = float(data_range)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = _filter(x, w), _filter(y, w)
    sx = _filter(x * x, w) - mx * mx
    sy = _filter(y * y, w) - my * my
    sxy = _filter(x * y, w) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))


def per_image_terms(y, x, which, win=11, sigma=1.5, data_range=1.0):
    """y = pred, x = truth: (N, C, H, W) tensors -> {name: (N,) tensor} for the names in `which`."""
    N, C, H, W = y.shape
    out = {}
    d = y - x
    if 'mse' in which:
        out['mse'] = (d * d).mean(dim=(1, 2, 3))
    if 'l1' in which:
        out['l1'] = d.abs().mean(dim=(1, 2, 3))
    if 'gdl' in which:
        gv = ((y[:, :, 1:, :] - y[:, :, :-1, :]).abs() - (x[:, :, 1:, :] - x[:, :, :-1, :]).abs()).abs().sum(dim=(1, 2, 3)) / (C * (H - 1) * W)
        gh = ((y[:, :, :, 1:] - y[:, :, :, :-1]).abs() - (x[:, :, :, 1:] - x[:, :, :, :-1]).abs()).abs().sum(dim=(1, 2, 3)) / (C * H * (W - 1))
        out['gdl'] = gv + gh
    if 'dssim' in which:
        out['dssim'] = 1.0 - ssim_map(y, x, win, sigma, data_range).mean(dim=(1, 2, 3))
    return out


def total(y, x, weights, win=11, sigma=1.5, data_range=1.0):
    """-> (weighted total: a scalar tensor, {name: (N,) values}, {name: mean}); a zero weight's term is not computed."""
    which = [k for k, w in zip(TERMS, weights) if w != 0]
    vals = per_image_terms(y, x, which, win, sigma, data_range)
    means = {k: v.mean() for k, v in vals.items()}
    tot = y.new_zeros(())
    for k, w in zip(TERMS, weights):
        if w != 0:
            tot = tot + w * means[k]
    return tot, vals, means


def loss_and_grad(pred, truth, weights, win=11, sigma=1.5, data_range=1.0, dtype=torch.float64):
    """NumPy (N, C, H, W) in -> dict(values (4, N), terms (5,), grad (N, C, H, W)) as float64 NumPy arrays, computed in `dtype`; terms that are
    off read 0, as the op writes them."""
    y = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    x = torch.tensor(np.asarray(truth), dtype=dtype)
    tot, vals, means = total(y, x, weights, win, sigma, data_range)
    N = y.shape[0]
    grad = torch.autograd.grad(tot, y)[0] if tot.requires_grad else torch.zeros_like(y)
    values = np.stack([vals[k].detach().double().numpy() if k in vals else np.zeros(N) for k in TERMS])
    terms = np.array([float(means[k].detach().double()) if k in means else 0.0 for k in TERMS] + [float(tot.detach().double())])
    return dict(values=values, terms=terms, grad=grad.detach().double().numpy())


def _full_correlate_t(m, w):
    """Transposed separable window: (N, C, OH, OW) maps over the valid positions -> (N, C, H, W), out[q] = sum_p w[q - p] m[p], zero outside."""
    win = len(w)
    OH, OW = m.shape[-2:]
    h = np.zeros(m.shape[:-1] + (OW + win - 1,))
    for k in range(win):
        h[..., :, k:k + OW] += w[k] * m
    v = np.zeros(m.shape[:-2] + (OH + win - 1, OW + win - 1))
    for k in range(win):
        v[..., k:k + OH, :] += w[k] * h
    return v


def ssim_grad_closed_form(pred, truth, win=11, sigma=1.5, data_range=1.0):
    """d ssim_n / d pred for every image, float64 NumPy, by the three maps: with the raw window moments at position p and S_p = f(m_y, m_yy, m_xy),
    d S_p / d y_q = w_{q-p} (alpha_p + beta_p y_q + gamma_p x_q)."""
    y, x = np.asarray(pred, np.float64), np.asarray(truth, np.float64)
    w = MR.window(win, sigma)
    L = float(data_range)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = MR._filter(x, w), MR._filter(y, w)
    mxx, myy, mxy = MR._filter(x * x, w), MR._filter(y * y, w), MR._filter(x * y, w)
    A1, A2 = 2 * mx * my + C1, 2 * (mxy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, mxx - mx * mx + myy - my * my + C2
    S = A1 * A2 / (B1 * B2)
    alpha = 2 * mx * (A2 - A1) / (B1 * B2) - 2 * my * S * (1 / B1 - 1 / B2)
    beta = -2 * S / B2
    gamma = 2 * A1 / (B1 * B2)
    g = _full_correlate_t(alpha, w) + y * _full_correlate_t(beta, w) + x * _full_correlate_t(gamma, w)
    return g / (S.shape[-3] * S.shape[-2] * S.shape[-1])
