"""NumPy-in / NumPy-out wrapper around pivp_pixel_track, for the GPU tests (the other per-op wrappers live in hip_ops.py)."""
import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, _t, stream


def pixel_track_rc(planes, masks, aux, num_masks, model_type, stp_zero=0, P=None, alias=False, null=None):
    """-> (return code, planes_out or None).  P overrides the plane count passed down; alias: planes_out = planes_in; null: name of a pointer to pass as NULL."""
    lib = _lib.load()
    B, Pn, H, W = planes.shape
    pd, md, ad = _t(planes), _t(masks), _t(aux)
    out = torch.full((B, Pn, H, W), -7.0, dtype=torch.float32, device=DEV)
    ptr = dict(planes=pd.data_ptr(), masks=md.data_ptr(), aux=ad.data_ptr(), out=pd.data_ptr() if alias else out.data_ptr())
    if null is not None:
        ptr[null] = None
    rc = lib.pivp_pixel_track(ptr['planes'], ptr['masks'], ptr['aux'], ptr['out'], B, Pn if P is None else P, H, W, num_masks, model_type,
                              stp_zero, stream())
    torch.cuda.synchronize()
    return rc, (out.cpu().numpy() if rc == 0 else None)


def pixel_track(planes, masks, aux, num_masks, model_type, stp_zero=0):
    rc, out = pixel_track_rc(planes, masks, aux, num_masks, model_type, stp_zero)
    _lib.check(rc, 'pivp_pixel_track')
    return out
