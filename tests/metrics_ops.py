"""NumPy-in / NumPy-out wrapper around pivp_frame_metrics, for the GPU tests (like plan_ops.py)."""
import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, stream


def _t(a):      # a copy: the tests share write-protected reference inputs
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def frame_metrics_rc(pred, truth, win=11, sigma=1.5, data_range=1.0, null=None, same=False, **override):
    """pred, truth (N, C, H, W) -> (return code, (mse, ssim) as they lie in the -7 pre-filled output buffers).  null: 'pred' / 'truth' / 'mse' /
    'ssim' passed as NULL (a NULL output's buffer comes back untouched); same: truth IS pred (one device buffer); override: N / C / H / W."""
    lib = _lib.load()
    N, C, H, W = np.shape(pred)
    d = dict(pred=_t(pred))
    d['truth'] = d['pred'] if same else _t(truth)
    d['mse'] = torch.full((N,), -7.0, device=DEV)
    d['ssim'] = torch.full((N,), -7.0, device=DEV)
    ptr = {k: v.data_ptr() for k, v in d.items()}
    if null is not None:
        for k in ([null] if isinstance(null, str) else null):
            ptr[k] = None
    n = dict(N=N, C=C, H=H, W=W)
    n.update(override)
    rc = lib.pivp_frame_metrics(ptr['pred'], ptr['truth'], n['N'], n['C'], n['H'], n['W'], int(win), float(sigma), float(data_range),
                                ptr['mse'], ptr['ssim'], stream())
    torch.cuda.synchronize()
    return rc, (d['mse'].cpu().numpy(), d['ssim'].cpu().numpy())


def frame_metrics(pred, truth, win=11, sigma=1.5, data_range=1.0, **kw):
    rc, out = frame_metrics_rc(pred, truth, win, sigma, data_range, **kw)
    _lib.check(rc, 'pivp_frame_metrics')
    return out
