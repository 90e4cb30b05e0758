"""NumPy-in / NumPy-out wrapper around pivp_gather_batch, for the GPU tests (like metrics_ops.py).  Every output buffer carries PAD sentinel floats
behind its last element; the wrapper reports whether they survived."""
import numpy as np
import torch

from pivp_amd import _lib
from hip_ops import DEV, stream

PAD = 4096
SENTINEL = -7.0


def _dev(a, dtype=None):
    if isinstance(a, torch.Tensor):
        return a
    return torch.tensor(np.asarray(a, dtype=dtype), device=DEV)      # a copy: the tests share write-protected reference inputs


def gather_batch_rc(frames, actions, states, index, null=None, **override):
    """frames (N,T,H,W,3) uint8 or float32, actions / states (N,T,5), index (B,): host arrays or device tensors -> (return code,
    [images (T,B,3,H,W), actions (T,B,5), states (T,B,5)] as they lie in the SENTINEL pre-filled buffers, sentinels intact?).
    null: argument name(s) passed as NULL; override: B / N / T / H / W / frames_u8 as the call states them."""
    lib = _lib.load()
    N, T, H, W = (int(v) for v in frames.shape[:4])
    B = int(len(index))
    u8 = (frames.dtype == torch.uint8) if isinstance(frames, torch.Tensor) else (np.asarray(frames).dtype == np.uint8)
    d = dict(frames=_dev(frames, np.uint8 if u8 else np.float32), actions=_dev(actions, np.float32), states=_dev(states, np.float32),
             index=_dev(index, np.int32) if B else torch.zeros(1, dtype=torch.int32, device=DEV))
    shapes = dict(out_images=(T, B, 3, H, W), out_actions=(T, B, 5), out_states=(T, B, 5))
    for k, s in shapes.items():
        d[k] = torch.full((int(np.prod(s)) + PAD,), SENTINEL, device=DEV)
    ptr = {k: v.data_ptr() for k, v in d.items()}
    if null is not None:
        for k in ([null] if isinstance(null, str) else null):
            ptr[k] = None
    n = dict(B=B, N=N, T=T, H=H, W=W, frames_u8=int(u8))
    n.update(override)
    rc = lib.pivp_gather_batch(ptr['frames'], n['frames_u8'], ptr['actions'], ptr['states'], ptr['index'], n['B'], n['N'], n['T'], n['H'], n['W'],
                               ptr['out_images'], ptr['out_actions'], ptr['out_states'], stream())
    torch.cuda.synchronize()
    outs, intact = [], True
    for k, s in shapes.items():
        flat = d[k].cpu().numpy()
        m = int(np.prod(s))
        intact = intact and bool((flat[m:] == SENTINEL).all())
        outs.append(flat[:m].reshape(s))
    return rc, outs, intact


def gather_batch(frames, actions, states, index, **kw):
    rc, outs, intact = gather_batch_rc(frames, actions, states, index, **kw)
    _lib.check(rc, 'pivp_gather_batch')
    assert intact, 'pivp_gather_batch wrote behind an output buffer'
    return outs
