"""Chainer-2 style Adam for the MI355X model (reference: `optimizers.Adam(alpha=learning_rate)`, `optimizer.setup(model)`,
`optimizer.update(model, [imgs, acts, stas], itr)` at train_model.py:860-861 and :950).

update() = forward (loss) -> cleargrads -> backward -> [gradient all-reduce when data-parallel] -> Adam step, the
sequence of chainer.Optimizer.update(lossfun, *args).  The step itself is one HIP launch over the model's flat parameter
buffer with Chainer's epsilon placement (eps added to the UNcorrected sqrt(v)).

The guarded step (include/pivp_optim.h) puts one look at the gradient in front of it, on the device: `pivp_grad_stats` reads the flat gradient
buffer once and leaves the L2 norm of every parameter tensor, of every gradient group and of the whole buffer, Chainer's GradientClipping rate
and a non-finite flag in device memory; `pivp_adam_step_guarded` takes its scale and its go / no-go from there.  It is taken iff a
`GradientClipping` hook is present (`add_hook`, chainer.Optimizer.add_hook) or `skip_nonfinite` / `track_grad_norm` is on; otherwise `step` is
the one `pivp_adam_step` launch."""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib


class GradientClipping(object):
    """chainer.optimizer.GradientClipping(threshold): scale the whole gradient by threshold / ||g||_2 when that is below 1.  Added with
    `Adam.add_hook`; the norm and the rate are formed on the device (pivp_grad_stats) and applied inside the Adam launch, not by this object."""
    name = 'GradientClipping'

    def __init__(self, threshold):
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise TypeError('GradientClipping threshold must be a number, got %r' % (threshold,))
        threshold = float(threshold)
        if not (threshold > 0.0 and math.isfinite(threshold)):
            raise ValueError('GradientClipping threshold must be positive and finite, got %r' % threshold)
        self.threshold = threshold


class Adam(object):
    """skip_nonfinite: a step whose gradient holds a NaN or an inf leaves the parameters, m and v untouched and is counted (`skipped_steps`)
    instead of being written into every parameter.  The decision is taken on the device, so the host's step count `t` advances on a skipped step
    too: the bias correction is then ahead by the number of skipped steps (at beta2 = 0.999 and t in the thousands, a relative 1e-3 per skipped
    step on a factor that tends to 1).
    track_grad_norm: keep the gradient norms of every step readable (`grad_norm`, `group_norms`, `param_norms()`), without clipping.
    Under data parallelism the norms are those of the AVERAGED gradient (gscale = 1 / world size, computed after the all-reduce).  With
    algo='rs_ag' every rank holds the same bytes and takes the same clip and skip decision; with algo='allreduce' identical decisions rest on the
    collective returning identical bytes on every rank."""

    def __init__(self, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8, skip_nonfinite=False, track_grad_norm=False):
        self.alpha, self.beta1, self.beta2, self.eps = alpha, beta1, beta2, eps
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        self.t = 0
        self.target = None
        self._m = None
        self._v = None
        self._dp = None
        self._hooks = None             # name -> hook, from setup() on (chainer.Optimizer._hooks)
        self._guard = None             # device tables, workspace and statistics of the guarded step, per model size
        self._skipped = None           # device int: steps skipped by skip_nonfinite
        # after a guarded step: 0-d device tensors (views of the statistics buffer, overwritten by the next step; reading them never synchronises)
        self.grad_norm = None          # ||gscale * g||_2 over the whole flat buffer
        self.clip_rate = None          # what the step multiplied the gradient by (1 without a clipping hook)
        self.grad_nonfinite = None     # 1.0 if the gradient held a NaN or an inf, else 0.0
        self.group_norms = None        # (6,): the norm of every gradient group (Model.grad_group_ranges)

    def setup(self, model, data_parallel=None):
        """`data_parallel`: an optional parallel.GradAllReduce; its world size rescales the summed gradients."""
        self.target = model
        self._dp = data_parallel
        self._hooks = OrderedDict()    # (chainer.Optimizer.setup starts from an empty hook table)
        return self

    # chainer.Optimizer.add_hook / remove_hook (Chainer 2)
    def add_hook(self, hook, name=None):
        if not isinstance(hook, GradientClipping):
            raise TypeError('only GradientClipping hooks are served (the hook runs inside the Adam launch), got %r' % (hook,))
        if self._hooks is None:
            raise RuntimeError('call `setup` method before `add_hook` method')
        if name is None:
            name = hook.name
        if name in self._hooks:
            raise KeyError('hook %s already exists' % name)
        if self._hooks:
            raise ValueError('one GradientClipping hook at a time: remove %r first' % next(iter(self._hooks)))
        self._hooks[name] = hook

    def remove_hook(self, name):
        if self._hooks is None:
            raise RuntimeError('call `setup` method before `remove_hook` method')
        del self._hooks[name]

    @property
    def lr(self):
        """AdamRule.lr: alpha * sqrt(1 - beta2^t) / (1 - beta1^t)."""
        fix1 = 1.0 - math.pow(self.beta1, self.t)
        fix2 = 1.0 - math.pow(self.beta2, self.t)
        return self.alpha * math.sqrt(fix2) / fix1

    def _state(self, model):
        if self._m is None or self._m.numel() != model._flat_params.numel():
            self._m = torch.zeros_like(model._flat_params)
            self._v = torch.zeros_like(model._flat_params)
        return self._m, self._v

    def _guarded(self):
        return bool(self._hooks) or self.skip_nonfinite or self.track_grad_norm

    def _guard_buffers(self, model, lib):
        """Segment and group tables of the model's flat layout (one segment per parameter tensor, padding included), uploaded once per model size,
        with the workspace and the statistics buffer of pivp_grad_stats."""
        n = model._flat_params.numel()
        gd = self._guard
        if gd is not None and gd['n'] == n and gd['device'] == model._flat_params.device:
            return gd
        keys = list(model._offsets)                     # flat order: group by group, checkpoint order inside a group (Model._upload)
        ends, groups, at = [], [], 0
        for i, key in enumerate(keys):
            o, size = model._offsets[key]
            end = model._offsets[keys[i + 1]][0] if i + 1 < len(keys) else n
            if o != at or end < o + size or (end % 64 and end != n):
                raise RuntimeError('flat parameter layout is not a row of 64-aligned segments at %r' % key)
            grp = int(lib.pivp_param_group_by_name(key.encode()))
            if not 0 <= grp < _lib.GRAD_GROUPS:
                raise RuntimeError('%r has no gradient group' % key)
            ends.append(end); groups.append(grp); at = end
        if len(keys) > _lib.OPTIM_MAX_SEGMENTS:
            raise RuntimeError('%d parameter tensors: pivp_grad_stats takes at most %d segments' % (len(keys), _lib.OPTIM_MAX_SEGMENTS))
        dev = model._flat_params.device
        nbytes = lib.pivp_grad_stats_ws_bytes(n, len(keys))
        if nbytes <= 0:
            raise _lib.PivpError('pivp_grad_stats_ws_bytes(%d, %d) failed' % (n, len(keys)))
        head = 3 + _lib.GRAD_GROUPS
        stats = torch.zeros(head + len(keys), dtype=torch.float32, device=dev)
        gd = dict(n=n, device=dev, keys=keys, nseg=len(keys), stats=stats,
                  seg_end=torch.tensor(ends, dtype=torch.int64, device=dev), seg_group=torch.tensor(groups, dtype=torch.int32, device=dev),
                  ws=torch.empty(nbytes // 8, dtype=torch.float64, device=dev),
                  seg_norm={key: stats[head + i] for i, key in enumerate(keys)})
        if self._skipped is None or self._skipped.device != dev:
            self._skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self._guard = gd
        self.grad_norm, self.clip_rate, self.grad_nonfinite, self.group_norms = stats[0], stats[1], stats[2], stats[3:head]
        return gd

    def param_norms(self):
        """After a guarded step: checkpoint key -> 0-d device tensor, the L2 norm of that tensor's (averaged) gradient.  Views of the statistics
        buffer: no synchronisation here, and the next guarded step overwrites them."""
        if self._guard is None:
            raise RuntimeError('no guarded step has run (add a GradientClipping hook, or Adam(skip_nonfinite=True / track_grad_norm=True))')
        seg = self._guard['seg_norm']
        return OrderedDict((key, seg[key]) for key in self.target._shapes())

    @property
    def skipped_steps(self):
        """Steps skipped by skip_nonfinite so far, as a host int.  Reads the device counter: this SYNCHRONISES with the device."""
        return 0 if self._skipped is None else int(self._skipped.item())

    def step(self, model=None):
        """Apply one Adam step from the gradients currently held by the model."""
        model = model or self.target
        g = model._ensure_grads()
        m, v = self._state(model)
        self.t += 1
        gscale = 1.0
        if self._dp is not None:
            gscale = 1.0 / self._dp.world_size
        lib = _lib.load()
        if self._guarded():
            gd = self._guard_buffers(model, lib)
            threshold = next(iter(self._hooks.values())).threshold if self._hooks else 0.0      # 0: no clipping, rate 1
            with torch.cuda.device(model._flat_params.device):
                _lib.check(lib.pivp_grad_stats(g.data_ptr(), gd['n'], gd['seg_end'].data_ptr(), gd['seg_group'].data_ptr(), gd['nseg'],
                                               _lib.GRAD_GROUPS, gscale, threshold, gd['ws'].data_ptr(), gd['stats'].data_ptr(),
                                               model._stream()), 'pivp_grad_stats')
                _lib.check(lib.pivp_adam_step_guarded(model._flat_params.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), gd['n'],
                                                      self.lr, self.beta1, self.beta2, self.eps, gscale, gd['stats'].data_ptr(),
                                                      1 if self.skip_nonfinite else 0, self._skipped.data_ptr(), model._stream()),
                           'pivp_adam_step_guarded')
            if hasattr(model, 'params_changed'):
                model.params_changed()
            return
        with torch.cuda.device(model._flat_params.device):      # launches need the model's device to be the current one
            _lib.check(lib.pivp_adam_step(model._flat_params.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                          model._flat_params.numel(), self.lr, self.beta1, self.beta2, self.eps, gscale,
                                          model._stream()), 'pivp_adam_step')
        if hasattr(model, 'params_changed'):
            model.params_changed()      # (a raw-pointer write: torch's version counter does not see it)

    def update(self, lossfun, *args):
        """chainer.Optimizer.update(lossfun, *args): loss = lossfun(*args); cleargrads; backward; update."""
        model = self.target
        loss = lossfun(*args)
        model.cleargrads()
        if self._dp is not None:
            self._dp.backward_and_allreduce(model)   # all-reduce of each gradient group overlapped with the rest of the sweep
        else:
            model.backward()
        self.step(model)
        return loss

    # state-<epoch> files of the reference (train_model.py:1037) hold t and per-parameter m, v
    def state_dict_reference(self):
        from . import checkpoint as ckpt
        model = self.target
        out = {'t': np.asarray(self.t)}
        self._state(model)
        if self._m is not None:
            for key, shape in model._shapes().items():
                o, n = model._offsets[key]
                out[key + '/m'] = ckpt.from_internal(key, self._m[o:o + n].cpu().numpy(), shape)
                out[key + '/v'] = ckpt.from_internal(key, self._v[o:o + n].cpu().numpy(), shape)
        return out
