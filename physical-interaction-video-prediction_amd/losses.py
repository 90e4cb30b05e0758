"""Training objectives beyond the reference's L2: L1, the gradient-difference loss (Mathieu et al. 2016, alpha = 1) and DSSIM = 1 - SSIM of
predicted frames against their ground truth, on the device, with the gradient with respect to the prediction.

`ImageLoss` holds the weights and the SSIM window (the one `metrics.frame_metrics` reports with); `image_loss` is one call of pivp_image_loss
(include/pivp_loss.h) on frames that are already on the device.  `Model(..., image_loss=ImageLoss(...))` adds the terms to the reference's loss
and feeds their gradient into the backward sweep; `Model.backward(frame_grad=...)` takes any other d loss / d gen_images the same way.  There is no
CPU fallback."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import metrics as _metrics

TERMS = ('mse', 'l1', 'gdl', 'dssim')
MAX_FRAME = 11      # the largest window


class ImageLoss(object):
    """Weights of the image terms of the training objective: loss = mse * MSE + l1 * L1 + gdl * GDL + dssim * (1 - SSIM), each term the mean over the
    scored frames of its per-frame value (include/pivp_loss.h).  mse=1 and the rest 0 is the reference's objective.  win / sigma / data_range: the
    SSIM window, as `metrics.frame_metrics` takes them (win odd 3 .. 11, sigma <= 0 for the uniform window)."""

    def __init__(self, mse=1.0, l1=0.0, gdl=0.0, dssim=0.0, win=11, sigma=1.5, data_range=1.0):
        w = []
        for name, v in zip(TERMS, (mse, l1, gdl, dssim)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError('%s must be a number, not %r' % (name, v))
            v = float(v)
            if not math.isfinite(v) or abs(v) > float(np.finfo(np.float32).max):      # (the library takes float32 weights)
                raise ValueError('%s must be finite, got %r' % (name, v))
            w.append(v)
        self.mse, self.l1, self.gdl, self.dssim = w
        # the window's rules are the metrics': check them on the smallest frame the window fits
        big = (1, MAX_FRAME, MAX_FRAME)
        _, _, _, _, _, self.win, self.sigma, self.data_range = _metrics._check_metric_args(big, big, win, sigma, data_range)

    def weights(self):
        return (self.mse, self.l1, self.gdl, self.dssim)

    def is_reference(self):
        """The reference's objective and nothing else: the model then calls nothing new."""
        return self.weights() == (1.0, 0.0, 0.0, 0.0)

    def _struct(self, extra_mse=None):
        return _lib.PivpImageLoss(w_mse=self.mse if extra_mse is None else extra_mse, w_l1=self.l1, w_gdl=self.gdl, w_dssim=self.dssim,
                                  win=self.win, sigma=self.sigma, data_range=self.data_range)

    def check_frames(self, shape):
        """ValueError if frames of `shape` (..., C, H, W) cannot be scored with these weights."""
        H, W = shape[-2:]
        if self.dssim != 0.0 and (H < self.win or W < self.win):
            raise ValueError('%d x %d frames are smaller than the %d x %d window' % (H, W, self.win, self.win))
        if self.gdl != 0.0 and (H < 2 or W < 2):
            raise ValueError('the gradient-difference loss needs frames of at least 2 x 2, got %d x %d' % (H, W))

    def __repr__(self):
        return 'ImageLoss(mse=%g, l1=%g, gdl=%g, dssim=%g, win=%d, sigma=%g, data_range=%g)' % (self.weights() + (self.win, self.sigma, self.data_range))


def _launch(pred, truth, N, C, H, W, spec, want_grad, lead):
    """pivp_image_loss on contiguous fp32 tensors of one device (the caller holds the device context); spec: a PivpImageLoss."""
    lib = _lib.load()
    dev = pred.device
    nbytes = lib.pivp_image_loss_ws_bytes(N, C, H, W, ctypes.byref(spec))
    if nbytes < 0:
        _lib.check(int(nbytes), 'pivp_image_loss_ws_bytes')
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    values = torch.empty((4, N), dtype=torch.float32, device=dev)
    terms = torch.empty(5, dtype=torch.float32, device=dev)
    grad = torch.empty((N, C, H, W), dtype=torch.float32, device=dev) if want_grad else None
    _lib.check(lib.pivp_image_loss(pred.data_ptr(), truth.data_ptr(), N, C, H, W, ctypes.byref(spec), values.data_ptr(), terms.data_ptr(),
                                   grad.data_ptr() if want_grad else None, ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               'pivp_image_loss')
    return SimpleNamespace(values=values.view((4,) + tuple(lead)), terms=terms, total=terms[4],
                           grad=grad.view(tuple(lead) + (C, H, W)) if want_grad else None)


def image_loss(pred, truth, spec, want_grad=False, device=None):
    """The image terms of `pred` against `truth`, (..., C, H, W) tensors or arrays of equal shape, under the `ImageLoss` spec ->
    SimpleNamespace(values (4, ...): mse / l1 / gdl / dssim per frame; terms (5,): their means over the frames and the weighted total; total:
    terms[4]; grad (..., C, H, W): d total / d pred, or None).  Device input is used where it lies, host input is uploaded.  A term whose weight
    is 0 is not computed and reads 0.  No host synchronisation."""
    if not isinstance(spec, ImageLoss):
        raise ValueError('spec must be an ImageLoss, not %r' % (spec,))
    lead, N, C, H, W = _check_frame_shapes(_metrics._shape(pred), _metrics._shape(truth))
    spec.check_frames(_metrics._shape(pred))
    if not torch.cuda.is_available():
        raise RuntimeError('no MI355X visible: this path has no CPU fallback (torch.cuda.is_available() is False)')
    _lib.load()
    if device is None:
        device = next((a.device for a in (pred, truth) if torch.is_tensor(a) and a.is_cuda), torch.device('cuda:0'))
    device = torch.device(device)

    def dev(a):
        if not torch.is_tensor(a):
            a = torch.tensor(np.asarray(a, dtype=np.float32))      # (a copy: the caller's array may be read-only)
        return a.to(device=device, dtype=torch.float32).contiguous()
    with torch.cuda.device(device):
        return _launch(dev(pred), dev(truth), N, C, H, W, spec._struct(), bool(want_grad), lead)


def _check_frame_shapes(pred_shape, truth_shape):
    """-> (lead shape, N, C, H, W): the shape rules of the metrics without the window's (the pointwise terms score frames smaller than any window)."""
    if pred_shape != truth_shape:
        raise ValueError('pred and truth must have the same shape, got %s and %s' % (pred_shape, truth_shape))
    if len(pred_shape) < 3:
        raise ValueError('frames are (..., C, H, W), got shape %s' % (pred_shape,))
    C, H, W = pred_shape[-3:]
    lead = pred_shape[:-3]
    N = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if N < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError('no frames: shape %s' % (pred_shape,))
    if C * H * W >= 2 ** 31 or N >= 2 ** 31:
        raise ValueError('frames too large: shape %s' % (pred_shape,))
    return lead, N, C, H, W
