"""NumPy-in / NumPy-out caller of pivp_image_loss on torch device tensors, for the GPU tests (like optim_ops.py / metrics_ops.py)."""
import ctypes

import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, stream

FILL = -7.0   # what the outputs hold before a call: a call that returns BADARG must leave it there


def _t(a):      # a copy: the tests share write-protected reference inputs
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def spec_of(weights, win=11, sigma=1.5, data_range=1.0):
    return _lib.PivpImageLoss(w_mse=weights[0], w_l1=weights[1], w_gdl=weights[2], w_dssim=weights[3], win=int(win), sigma=float(sigma),
                              data_range=float(data_range))


def image_loss_rc(pred, truth, weights, win=11, sigma=1.5, data_range=1.0, want_grad=True, null=(), same=False, **override):
    """pred, truth (N, C, H, W) -> (return code, dict(values (4, N), terms (5,), grad (N, C, H, W) or None) as they lie in FILL pre-filled buffers).
    null: names among pred / truth / spec / values / terms / ws passed as NULL; same: truth IS pred (one device buffer); override: N / C / H / W."""
    lib = _lib.load()
    N, C, H, W = np.shape(pred)
    sp = spec_of(weights, win, sigma, data_range)
    d = dict(pred=_t(pred))
    d['truth'] = d['pred'] if same else _t(truth)
    d['values'] = torch.full((4, N), FILL, device=DEV)
    d['terms'] = torch.full((5,), FILL, device=DEV)
    d['grad'] = torch.full((N, C, H, W), FILL, device=DEV)
    nbytes = lib.pivp_image_loss_ws_bytes(N, C, H, W, ctypes.byref(sp))
    assert nbytes == 4 * N * 8
    d['ws'] = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    ptr = {k: v.data_ptr() for k, v in d.items()}
    if not want_grad:
        ptr['grad'] = None
    ptr['spec'] = ctypes.byref(sp)
    for k in ([null] if isinstance(null, str) else null):
        ptr[k] = None
    n = dict(N=N, C=C, H=H, W=W)
    n.update(override)
    rc = lib.pivp_image_loss(ptr['pred'], ptr['truth'], n['N'], n['C'], n['H'], n['W'], ptr['spec'], ptr['values'], ptr['terms'], ptr['grad'],
                             ptr['ws'], stream())
    torch.cuda.synchronize()
    return rc, dict(values=d['values'].cpu().numpy(), terms=d['terms'].cpu().numpy(), grad=d['grad'].cpu().numpy())


def image_loss(pred, truth, weights, win=11, sigma=1.5, data_range=1.0, **kw):
    rc, out = image_loss_rc(pred, truth, weights, win, sigma, data_range, **kw)
    _lib.check(rc, 'pivp_image_loss')
    return out
