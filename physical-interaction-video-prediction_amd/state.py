"""The recurrent state of the model as a value: the (c, h) pairs of the seven ConvLSTM cells of a batch, in ONE flat float32 device buffer
(include/pivp_state.h: for cell i = 0..6, c_i then h_i, each (B, H_i, W_i, C_i)).

`Model(carry_state=True)` keeps one between calls, as the reference's `Model` does until `reset_state()`; `Model.recurrent_state()` /
`Model.set_recurrent_state()` hand it out and take it back, so a caller can snapshot it, try something and come back, or start K rollouts from one
belief (`RecurrentState.expand`, `planning.cem_plan(belief=...)`)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .dataset import check_indices

CELL_LEVELS = (2, 2, 4, 4, 8, 4, 2)      # cell i lives on the (H, W) / level map ...
CELL_CHANNELS = (32, 32, 64, 64, 128, 64, 32)      # ... with this many channels


def _config(H, W):
    # only the frame size matters to the state's layout
    return _lib.PivpConfig(batch=1, seq_len=2, height=int(H), width=int(W), num_masks=1, model_type=0, use_state=1, context_frames=1,
                           keep_activations=0, ln_eps=1e-6, stp_zero_border=0)


def state_layout(H, W):
    """-> (floats per sample of the fourteen segments c_0, h_0, c_1, ..., their sum), from the library (pivp_state_layout: host arithmetic, no GPU)."""
    seg = (ctypes.c_longlong * _lib.STATE_SEGMENTS)()
    total = ctypes.c_longlong()
    cfg = _config(H, W)
    if _lib.load().pivp_state_layout(ctypes.byref(cfg), seg, ctypes.byref(total)) != _lib.PIVP_OK:
        raise ValueError('no recurrent state for %d x %d frames: height and width must be multiples of 8, at least 16' % (H, W))
    return [int(n) for n in seg], int(total.value)


class RecurrentState(object):
    """`data`: flat float32 tensor of batch * floats_per_sample elements; `batch`; `hw` = (H, W) of the frames."""

    def __init__(self, data, batch, hw):
        H, W = int(hw[0]), int(hw[1])
        if isinstance(batch, bool) or int(batch) != batch or batch < 1:
            raise ValueError('batch must be a positive integer, not %r' % (batch,))
        self._seg, per_sample = state_layout(H, W)
        if not torch.is_tensor(data) or data.dtype != torch.float32 or data.dim() != 1 or data.numel() != int(batch) * per_sample or not data.is_contiguous():
            raise ValueError('a recurrent state of batch %d at %d x %d is a flat contiguous float32 tensor of %d elements' % (batch, H, W, int(batch) * per_sample))
        self.data, self.batch, self.hw = data, int(batch), (H, W)

    @classmethod
    def empty(cls, batch, hw, device):
        return cls(torch.empty(int(batch) * state_layout(*hw)[1], dtype=torch.float32, device=device), batch, hw)

    def clone(self):
        return RecurrentState(self.data.clone(), self.batch, self.hw)

    def cells(self):
        """[(c_i, h_i)] for the seven cells: views (B, H_i, W_i, C_i) of `data`, for inspection."""
        H, W = self.hw
        out, at = [], 0
        for i, (lv, C) in enumerate(zip(CELL_LEVELS, CELL_CHANNELS)):
            pair = []
            for g in (2 * i, 2 * i + 1):
                n = self.batch * self._seg[g]
                pair.append(self.data[at:at + n].view(self.batch, H // lv, W // lv, C))
                at += n
            out.append(tuple(pair))
        return out

    def select(self, index):
        """A new state whose sample b is this one's sample index[b] (selection, permutation, repetition): ONE pivp_state_copy launch on the current
        stream.  The indices are validated here, on the host: integers in [0, batch)."""
        idx = check_indices(index, self.batch)
        if not self.data.is_cuda:
            raise ValueError('a recurrent state is selected on the GPU (there is no CPU path), this one lives on %s' % (self.data.device,))
        out = RecurrentState.empty(len(idx), self.hw, self.data.device)
        with torch.cuda.device(self.data.device):
            dev_idx = torch.from_numpy(idx).to(self.data.device)
            cfg = _config(*self.hw)
            _lib.check(_lib.load().pivp_state_copy(ctypes.byref(cfg), self.data.data_ptr(), self.batch, out.data.data_ptr(), out.batch,
                                                   dev_idx.data_ptr(), torch.cuda.current_stream(self.data.device).cuda_stream), 'pivp_state_copy')
        return out

    def expand(self, K):
        """A batch-1 state repeated K times (the belief every candidate of a planner starts from)."""
        if self.batch != 1:
            raise ValueError('expand() repeats a batch-1 state, this one holds %d samples' % self.batch)
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError('K must be a positive integer, not %r' % (K,))
        return self.select(np.zeros(int(K), np.int64))
