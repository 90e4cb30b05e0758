"""Host-side mirror of the reference's `Model` (src/models/train_model.py:478-764, "TM").

Same constructor, call, `reset_state()` and attribute surface:
    model = Model(num_masks, is_cdna=True, is_dna=False, is_stp=False, use_state=True,
                  scheduled_sampling_k=-1, num_frame_before_prediction=2, prefix=None)
    loss = model([images, actions, states], iter_num)      # time-major, NCHW float32 frames in [0,1]
    model.gen_images, model.psnr_all, model.summaries, model.conv_res, model.loss
    model.reset_state()
All arithmetic runs in the gfx950 HIP library behind include/pivp_hip.h; PyTorch supplies device
memory and the stream only.  There is no CPU fallback: without the built library or without a
GPU the call raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import re
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from . import checkpoint as ckpt
from .state import RecurrentState


class _Config(object):
    """Stand-in for chainer.config: only the `train` flag matters on this path (TM:649)."""
    train = True


config = _Config()


@contextlib.contextmanager
def using_config(name, value):
    """chainer.using_config equivalent (used as `with using_config('train', False)`, predict_model.py:126)."""
    old = getattr(config, name)
    setattr(config, name, value)
    try:
        yield
    finally:
        setattr(config, name, old)


LSTM_SIZES = OrderedDict(lstm1=(32, 32), lstm2=(32, 32), lstm3=(32, 64), lstm4=(64, 64),
                         lstm5=(64, 128), lstm6=(128, 64), lstm7=(96, 32))   # name -> (x channels, C); TM:509-515


MAX_INPUT_DIM = 16      # include/pivp_hip.h, the accepted domain: action_dim, state_dim 1 .. 16


def check_input_dim(name, value):
    """The width of an action or of a robot state: an integer 1 .. 16 (a bool, a float or a string is not one)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= MAX_INPUT_DIM:
        raise ValueError('%s must be an integer 1 .. %d, not %r' % (name, MAX_INPUT_DIM, value))
    return int(value)


def reference_param_shapes(num_masks, model_type, use_state, height, width, action_dim=5, state_dim=5):
    """Key -> shape in the reference's Chainer npz layout (TM:499-542).  action_dim / state_dim: the widths of an action and of a
    robot state (5 / 5 in the reference's data): enc3's input is sized by the data (TM:503), the state predictor is L.Linear(state_dim) (TM:529)."""
    smear = action_dim + state_dim
    h2, w2, h4, w4, h8, w8 = height // 2, width // 2, height // 4, width // 4, height // 8, width // 8
    s = OrderedDict()
    s['enc0/W'] = (32, 3, 5, 5); s['enc0/b'] = (32,)
    s['enc1/W'] = (32, 32, 3, 3); s['enc1/b'] = (32,)
    s['enc2/W'] = (64, 64, 3, 3); s['enc2/b'] = (64,)
    s['enc3/W'] = (64, 64 + (smear if use_state else 0), 1, 1); s['enc3/b'] = (64,)
    s['enc4/W'] = (128, 128, 3, 3); s['enc4/b'] = (128,)
    s['enc5/W'] = (96, 96, 3, 3); s['enc5/b'] = (96,)
    s['enc6/W'] = (64, 64, 3, 3); s['enc6/b'] = (64,)
    for name, (cx, c) in LSTM_SIZES.items():
        s[name + '/conv/W'] = (4 * c, cx + c, 5, 5)
        s[name + '/conv/b'] = (4 * c,)
    ln = OrderedDict(norm_enc0=32 * h2 * w2, hidden1=32 * h2 * w2, hidden2=32 * h2 * w2, hidden3=64 * h4 * w4,
                     hidden4=64 * h4 * w4, hidden5=128 * h8 * w8, hidden6=64 * h4 * w4, hidden7=32 * h2 * w2,
                     norm_enc6=64 * height * width)
    for name, n in ln.items():
        s[name + '/norm/gamma'] = (n,)
        s[name + '/norm/beta'] = (n,)
    s['masks/W'] = (64, num_masks + 1, 1, 1); s['masks/b'] = (num_masks + 1,)
    s['current_state/W'] = (state_dim, smear); s['current_state/b'] = (state_dim,)
    if model_type == 'CDNA':
        s['model/enc7/W'] = (64, 3, 1, 1); s['model/enc7/b'] = (3,)
        s['model/cdna_kerns/W'] = (25 * num_masks, 128 * h8 * w8); s['model/cdna_kerns/b'] = (25 * num_masks,)
    elif model_type == 'STP':
        s['model/enc7/W'] = (64, 3, 1, 1); s['model/enc7/b'] = (3,)
        s['model/stp_input/W'] = (100, 128 * h8 * w8); s['model/stp_input/b'] = (100,)
        s['model/identity_params/W'] = (6, 100); s['model/identity_params/b'] = (6,)
    else:
        s['model/enc7/W'] = (64, 25, 1, 1); s['model/enc7/b'] = (25,)
    return s


def default_init(shapes, rng=None):
    """Chainer 2 defaults: LeCunNormal W (std sqrt(1/fan_in)), zero bias, LN gamma 1 / beta 0."""
    rng = np.random if rng is None else rng
    out = OrderedDict()
    for key, shape in shapes.items():
        if key.endswith('/W'):
            fan_in = shape[1] if len(shape) == 2 else shape[1] * shape[2] * shape[3]
            out[key] = (rng.standard_normal(shape) * math.sqrt(1.0 / fan_in)).astype(np.float32)
        elif key.endswith('/gamma'):
            out[key] = np.ones(shape, np.float32)
        else:
            out[key] = np.zeros(shape, np.float32)
    return out


def scheduled_sampling_masks(batch_size, seq_len, context_frames, k, iter_num, rng=None):
    """Per-step ground-truth selection of the reference's scheduled sampling (TM:654-656, TM:73-122).

    Returns uint8 [T-1][B]; one `shuffle(arange(B))` is drawn from NumPy's global RNG per step that
    the reference would call scheduled_sample for (t >= context_frames), in the same order."""
    rng = np.random if rng is None else rng
    ngt = int(np.int32(np.round(np.float32(batch_size) * (k / (k + np.exp(iter_num / k))))))
    mask = np.zeros((seq_len - 1, batch_size), np.uint8)
    for t in range(seq_len - 1):
        if t > context_frames - 1:
            idx = np.arange(int(batch_size))
            rng.shuffle(idx)
            mask[t, idx[:ngt]] = 1
    return mask


# Plan options (include/pivp_hip.h, pivp_plan_set_option): `plan_options` key -> (PIVP_OPT_* id, the library's default, the environment variable this
# package reads as ITS default -- the library reads none)
PLAN_OPTIONS = OrderedDict(side_stream=(0, 1, 'PIVP_SIDE_STREAM'), finish_rider=(1, 1, 'PIVP_FINISH_RIDER'), fuse_enc3=(2, 1, 'PIVP_FUSE_ENC3'),
                           ln_fold_train=(3, 1, 'PIVP_LN_FOLD_TRAIN'), wgrad_batch=(4, 0, 'PIVP_WGRAD_BATCH'))
WGRAD_BATCH_MAX = 8


def check_plan_options(given):
    unknown = sorted(set(given or ()) - set(PLAN_OPTIONS))
    if unknown:
        raise ValueError('unknown plan option %s (known: %s)' % (', '.join(map(repr, unknown)), ', '.join(PLAN_OPTIONS)))


def resolve_plan_options(given=None, environ=None):
    """key -> value for every plan option: what `given` (Model(plan_options=...)) names, else the option's PIVP_* environment variable as it is now, else
    the library's default.  A switch is off when its variable starts with '0'; PIVP_WGRAD_BATCH is its leading integer (0, unset or no number: the precision
    mode's own choice), brought into 1 .. 8 when outside -- the plan cuts it to the rings' capacity either way, an exported value never raises.  Values
    given by keyword are passed on as they are: the library refuses what is out of range."""
    check_plan_options(given)
    environ = os.environ if environ is None else environ
    out = OrderedDict()
    for key, (_, default, var) in PLAN_OPTIONS.items():
        env = environ.get(var)
        if given is not None and key in given:
            out[key] = int(given[key])
        elif env is None:
            out[key] = default
        elif key == 'wgrad_batch':
            number = re.match(r'\s*[+-]?\d+', env)
            v = int(number.group()) if number else 0
            out[key] = v if v == 0 else min(max(v, 1), WGRAD_BATCH_MAX)
        else:
            out[key] = 0 if env.startswith('0') else 1
    return out


class _Plan(object):
    def __init__(self, lib, cfg):
        self.lib = lib
        self.cfg = cfg
        h = ctypes.c_void_p()
        _lib.check(lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)), 'pivp_plan_create')
        self.h = h
        self.names = [lib.pivp_param_name(h, i).decode() for i in range(lib.pivp_param_count(h))]
        self.numel = [lib.pivp_param_numel(h, i) for i in range(len(self.names))]
        self.workspace = None

    def __del__(self):
        try:
            if self.h:
                self.lib.pivp_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Model(object):
    """MI355X drop-in for the reference's `Model` (TM:478-764).

    deterministic=True: a training step (forward, `backward()`, `Adam.update`) gives the same bits every time for the same inputs, parameters,
    optimizer state, plan shape, precision, the 'wgrad_batch' plan option and GPU model -- whatever the side-stream schedule, the process or the workspace
    address (include/pivp_hip.h, pivp_plan_set_deterministic).  Served with precision 'fp32', 'bf16' and 'bf16x3', for CDNA, STP and DNA;
    other combinations raise ValueError.  Under the switch the ConvLSTM weight gradients are computed in fp32 in every precision mode, so
    deterministic 'bf16' differs from default 'bf16' there (it is the more precise of the two) and its step is slower (README).  A data-parallel
    run is deterministic only if its collective is: `algo='rs_ag'` sums the shards in rank order, the RCCL ring is not guaranteed to
    (DESIGN.md 6).

    plan_options: a dict of the plan's A/B levers (include/pivp_hip.h, pivp_plan_set_option) with keys 'side_stream', 'finish_rider', 'fuse_enc3',
    'ln_fold_train' (0 / 1, default 1) and 'wgrad_batch' (0 .. 8 timesteps per ConvLSTM weight-gradient launch, default 0 = the precision mode's own
    choice).  An option the dict does not name takes its default from PIVP_SIDE_STREAM, PIVP_FINISH_RIDER, PIVP_FUSE_ENC3, PIVP_LN_FOLD_TRAIN or
    PIVP_WGRAD_BATCH, read when a plan is made (`resolve_plan_options`); `effective_plan_options()` reads the current plan's values back.

    carry_state=True: the seven ConvLSTM (c, h) pairs live on between calls, as the reference's do until `reset_state()` (TM:230-232, 254-257): a call
    continues from the state the last one left -- `__call__`, `evaluate` and `imagine` alike, whatever their T -- and `reset_state()` clears it.  The
    model then owns one state buffer for its (B, H, W); a call at another batch or frame size while a state is carried raises ValueError (the
    reference fails in F.concat).  `recurrent_state()` / `set_recurrent_state()` snapshot and restore it (state.RecurrentState).  `backward()` after a
    call that started from a carried state raises unless the model was built with state_backward=True (below).
    With the default False every call starts from zeros and nothing of this runs.

    state_backward=True (needs carry_state=True and keep_activations=True): `backward()` serves a call that started from a carried state, with that
    state as a constant -- truncated back-propagation through time across calls (include/pivp_state_grad.h).  `backward(initial_state_grad=True)`
    also leaves d loss / d (that state) in `model.initial_state_grad`, and `backward(final_state_grad=rs)` seeds the sweep with d (a later loss) /
    d (the state the call left): chained over consecutive windows that is the exact gradient in the memory of one window
    (`pivp_amd.chunked_backward`).  The model then alternates two state buffers instead of advancing one in place -- same frames, same states.

    action_dim, state_dim (integers 1 .. 16, default 5 / 5, the reference's push data): the widths of an action and of a robot state.  The reference
    reads them off its data (enc3's input is sized lazily, TM:503; only L.Linear(5), TM:529, pins the state); here they are explicit: actions are
    (T, B, action_dim), states (T, B, state_dim), enc3/W (64, 64 + action_dim + state_dim, 1, 1), current_state/W (state_dim, action_dim + state_dim),
    and a call with other widths raises ValueError.  `planning.cem_plan` / `cem_refine` / `MPC` and `DeviceDataset` serve 5 / 5 alone."""

    DETERMINISTIC_PRECISIONS = ('fp32', 'bf16', 'bf16x3')

    def __init__(self, num_masks, is_cdna=True, is_dna=False, is_stp=False, use_state=True,
                 scheduled_sampling_k=-1, num_frame_before_prediction=2, prefix=None,
                 device='cuda:0', ln_eps=1e-6, stp_border='clamp', keep_activations=False, precision='fp32', main_priority=None,
                 deterministic=False, image_loss=None, plan_options=None, state_backward=False, action_dim=5, state_dim=5,
                 carry_state=False):
        # the widths of an action and of a robot state (the reference's data: 5 / 5); explicit, not sized by the first batch (TM:503 sizes enc3 lazily)
        self.action_dim = check_input_dim('action_dim', action_dim)
        self.state_dim = check_input_dim('state_dim', state_dim)
        if is_cdna:                      # TM:531-542, precedence cdna > stp > dna
            self.model_type = 'CDNA'
        elif is_stp:
            self.model_type = 'STP'
        elif is_dna:
            self.model_type = 'DNA'
        else:
            raise ValueError("No network specified")
        self.num_masks = num_masks
        self.use_state = use_state
        self.scheduled_sampling_k = scheduled_sampling_k
        # scheduled_sample draws from NumPy's GLOBAL RNG in the reference (TM:94); None keeps that.  Data-parallel training gives
        # every rank its own stream here (train.py: RandomState(seed + 1 + rank)), or all ranks would draw the same shuffle
        # for their shards.
        self.sampling_rng = None
        self.num_frame_before_prediction = num_frame_before_prediction
        self.prefix = prefix
        self.device = torch.device(device)
        self.ln_eps = float(ln_eps)
        if stp_border not in ('clamp', 'zeros'):
            raise ValueError("stp_border must be 'clamp' or 'zeros'")
        self.stp_border = stp_border
        self.keep_activations = bool(keep_activations)
        # 'fp32' is the parity path (per-pixel L2 < 1e-4 vs the reference).  'bf16' (BASELINE.json config 3) rounds the operands of
        # the seven ConvLSTM gate convolutions, of their data / weight gradients and of the enc5 / enc6 transposed convs to bf16 -- fp32 accumulation, gates, state, every
        # other op, the parameters, the gradients and Adam stay fp32 -- and reports, not gates, its error.
        # 'bf16x3' is the split mode: the forward gate convolutions (and the enc5 / enc6 transposed convs) take every fp32 operand as two bf16 pieces and form a product on
        # three bf16 MFMAs (16 bits of product mantissa); the rollout stays inside the 1e-4 gate; backward and everything else fp32.
        # 'bf16x6': three bf16 pieces per operand and the six significant products (fp32-grade results on the bf16 matrix cores) in the forward gate
        # convolutions of every layer whose map is a multiple of 16 wide; everything else, and the whole backward pass, fp32.
        # 'fp16x3': the forward gate convolutions with every operand as two fp16 pieces (weights pre-scaled by a per-tensor power of two), three MFMAs per product: 22-bit operands,
        # still fp32-grade (its truncation is a quarter of fp32's own rounding error); the data gradients of the sweep take the same form with dG staged times a power of two from its largest value (gradients lie below fp16's normal range).
        if precision not in ('fp32', 'bf16', 'bf16x3', 'bf16x6', 'fp16x3'):
            raise ValueError("precision must be 'fp32', 'bf16', 'bf16x3', 'bf16x6' or 'fp16x3'")
        self.precision = precision
        if not isinstance(deterministic, bool):
            raise ValueError('deterministic must be a bool, not %r' % (deterministic,))
        if deterministic and precision not in self.DETERMINISTIC_PRECISIONS:
            raise ValueError("deterministic=True is not served with precision=%r (only %s)"
                             % (precision, ', '.join(map(repr, self.DETERMINISTIC_PRECISIONS))))
        self.deterministic = deterministic
        # image_loss: an `ImageLoss` (losses.py) -- L1 / gradient-difference / DSSIM terms (and another weight on the MSE) beside the reference's
        # objective.  None, or the reference's weights (1, 0, 0, 0): nothing new is called and every output is what it is without the argument.
        if image_loss is not None:
            from .losses import ImageLoss
            if not isinstance(image_loss, ImageLoss):
                raise ValueError('image_loss must be an ImageLoss or None, not %r' % (image_loss,))
        self.image_loss = image_loss
        self._extra_loss = image_loss is not None and not image_loss.is_reference()
        self.loss_terms = None         # with an image loss: device scalars mse / l1 / gdl / dssim (means over the scored frames) and extra (their weighted sum
                                       # beyond the reference's loss) of the last call
        self._loss_grad = None         # ... and d extra / d gen_images[ctx-1:], when the call kept what backward() needs
        self.action_grad = None        # backward(input_grad=True): d loss / d actions[:T-1] (T-1, B, action_dim) and ...
        self.state_grad = None         # ... d loss / d states[0] (B, state_dim), device tensors
        if not isinstance(carry_state, bool):
            raise ValueError('carry_state must be a bool, not %r' % (carry_state,))
        self.carry_state = carry_state
        self._state = None             # carry_state: the RecurrentState the next call starts from (None: zeros, as after reset_state())
        self._carried_start = False    # the last __call__ started from a carried state: backward() needs state_backward=True
        # state_backward: backward() also serves a call that started from a carried state (include/pivp_state_grad.h).  The sweep reads that state
        # again, so the model no longer advances its state in place: it alternates two buffers, and the one a call started from is intact until the next call
        if not isinstance(state_backward, bool):
            raise ValueError('state_backward must be a bool, not %r' % (state_backward,))
        if state_backward and not (carry_state and self.keep_activations):
            raise ValueError('state_backward=True back-propagates through a carried recurrent state: the model needs carry_state=True and keep_activations=True')
        self.state_backward = state_backward
        self._spare_state = None       # state_backward: the other of the two state buffers = the state the last call started from
        self.initial_state_grad = None   # backward(initial_state_grad=True): d loss / d (the state the last call started from), a RecurrentState
        self._spare_state_grad = None    # ... and the buffer it alternates with when the next sweep is seeded with it
        check_plan_options(plan_options)
        self.plan_options = dict(plan_options or {})
        self.main_priority = main_priority     # None / False / True: include/pivp_hip.h, pivp_plan_set_main_priority
        self._ref_pending = None       # reference-layout arrays loaded before the first call
        self._params = None            # name -> view into _flat_params (internal layout)
        self._flat_params = None
        self._flat_grads = None
        self._grads = None
        self._offsets = None
        self._gt_mask = None
        self._hw = None
        self._plans = {}
        self._active = None
        self._results = None
        self._gen = None
        self.gen_states = None
        self.loss = 0.0
        self.psnr_all = 0.0
        self.gen_images = []
        self._imagined = False         # the last rollout was imagine(): taps exist, a loss does not
        self.pixel_distrib = None      # imagine(designated=...): (T-1-f, B, P, H, W) tracked planes on the predicted frames
        self.pixel_mass = None         # ... and their raw sums (T-1-f, B, P)
        self.metrics = None            # evaluate(): per-sample mse / psnr / ssim (T-ctx, B) of the last evaluated rollout

    # ---- parameters ---------------------------------------------------------------------
    def _shapes(self):
        H, W = self._hw
        return reference_param_shapes(self.num_masks, self.model_type, self.use_state, H, W, self.action_dim, self.state_dim)

    def _require_gpu(self):
        if not torch.cuda.is_available():
            raise RuntimeError('no MI355X visible: this path has no CPU fallback (torch.cuda.is_available() is False)')
        return _lib.load()

    def _ensure_params(self, H, W):
        if self._params is not None:
            if self._hw != (H, W):
                # TM:186-208 / quirk 3: lazily sized LN gamma/beta weld a model to one frame size
                raise ValueError('model was sized for %dx%d frames, got %dx%d' % (self._hw + (H, W)))
            return
        self._hw = (H, W)
        shapes = self._shapes()
        ref = self._ref_pending if self._ref_pending is not None else default_init(shapes)
        self._ref_pending = None
        self._upload(ref, shapes)

    def _upload(self, ref, shapes):
        """Parameters live in ONE flat device buffer (internal layouts, 256-B aligned slices): Adam is a single
        launch over it and the data-parallel gradient all-reduce a single collective on its twin `_flat_grads`."""
        host = OrderedDict()
        for key, shape in shapes.items():
            if key not in ref:
                raise KeyError('checkpoint is missing %r' % key)
            a = np.asarray(ref[key])
            if tuple(a.shape) != tuple(shape):
                raise ValueError('%s: expected shape %s, got %s' % (key, shape, a.shape))
            host[key] = ckpt.to_internal(key, a)
        # Flat layout: the parameters (and so their gradients) are laid out in the order in which the backward sweep finishes
        # them at t = 0 (pivp_param_group: 6 groups, heads first, enc0 last), so that each group is ONE contiguous slice the
        # data-parallel all-reduce can send while the sweep is still working on the next group.
        lib = _lib.load()                                       # host-only query: works without a GPU
        group = {key: int(lib.pivp_param_group_by_name(key.encode())) for key in host}
        order = sorted(host, key=lambda k: group[k])            # stable: checkpoint order inside a group
        offsets, off = OrderedDict(), 0
        bounds = []
        for key in order:
            if not bounds or bounds[-1][0] != group[key]:
                bounds.append([group[key], off, off])
            offsets[key] = (off, host[key].size)
            off += (host[key].size + 63) // 64 * 64
            bounds[-1][2] = off
        self._group_ranges = [(a, b) for _, a, b in bounds]     # [(start, end)] floats, one per gradient group in sweep order
        flat = np.zeros(off, np.float32)
        for key, v in host.items():
            o, n = offsets[key]
            flat[o:o + n] = v
        new_flat = torch.from_numpy(flat).to(self.device)
        if self._flat_params is not None and self._flat_params.numel() == new_flat.numel():
            self._flat_params.copy_(new_flat)          # keep addresses stable for plans and optimizers
        else:
            self._flat_params = new_flat
            self._flat_grads = None
        self._offsets = offsets
        self._params = OrderedDict((k, self._flat_params[o:o + n]) for k, (o, n) in offsets.items())
        for plan in self._plans.values():
            self._bind(plan)

    def _ensure_grads(self):
        if self._flat_grads is None:
            self._flat_grads = torch.zeros_like(self._flat_params)
            self._grads = OrderedDict((k, self._flat_grads[o:o + n]) for k, (o, n) in self._offsets.items())
            for plan in self._plans.values():
                self._bind(plan)
        return self._flat_grads

    def load_state_dict_reference(self, ref):
        """Load arrays in the reference's Chainer-npz layout (chainer.serializers.load_npz target)."""
        ref = {k: np.asarray(v) for k, v in ref.items()}
        if self._hw is None:
            self._ref_pending = ref
        else:
            self._require_gpu()
            self._upload(ref, self._shapes())

    def state_dict_reference(self):
        """Parameters in the reference's Chainer-npz layout (what save_npz would write)."""
        if self._params is None:
            if self._ref_pending is not None:
                return OrderedDict(self._ref_pending)
            raise RuntimeError('parameters are lazily sized from the first input (as in the reference); call the model first')
        out = OrderedDict()
        for key, shape in self._shapes().items():
            out[key] = ckpt.from_internal(key, self._params[key].cpu().numpy(), shape)
        return out

    def count_params(self):
        return sum(int(np.prod(s)) for s in self._shapes().values())

    def params_changed(self):
        """Tell the model that its parameters were written behind torch's back: a collective (`dist.broadcast` / `all_reduce` leave
        `Tensor._version` untouched), a ctypes kernel, a raw-pointer copy.  The precision modes keep bf16 / fp16 packs of the weights
        across calls (pivp_plan_set_pack_cache); they are keyed by torch's in-place version counter and this epoch, so every writer
        torch cannot see must call this (include/pivp_hip.h: pivp_plan_params_changed).  `Adam.step` and `broadcast_params` do."""
        self._params_epoch = getattr(self, '_params_epoch', 0) + 1

    def broadcast_params(self, src=0, group=None):
        """Data-parallel replicas start identical: rank `src`'s parameters to every rank, and the weight packs of the
        precision modes invalidated (the collective writes through the raw pointer).  Parameters are lazily sized: call the model once first."""
        import torch.distributed as dist
        if self._flat_params is None:
            raise RuntimeError('call the model first (parameters are lazily sized)')
        dist.broadcast(self._flat_params, src=src, group=group)
        self.params_changed()

    # ---- plans --------------------------------------------------------------------------
    def _bind(self, plan):
        lib = plan.lib
        for i, (name, n) in enumerate(zip(plan.names, plan.numel)):
            t = self._params[name]
            if t.numel() != n:
                raise ValueError('%s: internal size %d != library size %d' % (name, t.numel(), n))
            _lib.check(lib.pivp_plan_set_param(plan.h, i, t.data_ptr()), 'pivp_plan_set_param(%s)' % name)
            if self._grads is not None:
                _lib.check(lib.pivp_plan_set_grad(plan.h, i, self._grads[name].data_ptr()), 'pivp_plan_set_grad(%s)' % name)

    def _plan_for(self, B, T, H, W, keep_activations=None, observed=None):
        keep = self.keep_activations if keep_activations is None else bool(keep_activations)
        # a rollout told how many frames it observes (imagine(observed=...)) may be shorter than the configured context: its plan is then made with
        # the context cut to T-1 -- the registration overrides it anyway -- and kept under a key of its own
        ctx = self.num_frame_before_prediction if observed is None else min(self.num_frame_before_prediction, T - 1)
        key = (B, T, H, W, keep) if ctx == self.num_frame_before_prediction else (B, T, H, W, keep, ctx)
        plan = self._plans.get(key)
        if plan is None:
            lib = self._require_gpu()
            cfg = _lib.PivpConfig(batch=B, seq_len=T, height=H, width=W, num_masks=self.num_masks,
                                  model_type={'CDNA': 0, 'STP': 1, 'DNA': 2}[self.model_type],
                                  use_state=1 if self.use_state else 0,
                                  context_frames=ctx,
                                  keep_activations=1 if keep else 0,
                                  ln_eps=self.ln_eps, stp_zero_border=1 if self.stp_border == 'zeros' else 0,
                                  action_dim=self.action_dim, state_dim=self.state_dim)
            plan = _Plan(lib, cfg)      # the door: a configuration the kernels do not serve is refused here (PIVP_ERR_BADARG), before a parameter is laid out
            self._ensure_params(H, W)
            for name, value in resolve_plan_options(self.plan_options).items():
                opt, default, _ = PLAN_OPTIONS[name]
                if value != default:
                    _lib.check(lib.pivp_plan_set_option(plan.h, opt, value), 'pivp_plan_set_option(%s, %d)' % (name, value))
            _lib.check(lib.pivp_plan_set_pack_cache(plan.h, 1), 'pivp_plan_set_pack_cache')
            if self.main_priority is not None:      # None: the library's rule (wave priority 3 for the sweep's kernels unless a gradient listener is registered)
                _lib.check(lib.pivp_plan_set_main_priority(plan.h, 1 if self.main_priority else 0), 'pivp_plan_set_main_priority')
            if self.precision != 'fp32':
                _lib.check(lib.pivp_plan_set_precision(plan.h, {'bf16': 1, 'bf16x3': 2, 'bf16x6': 3, 'fp16x3': 4}[self.precision]),
                           'pivp_plan_set_precision(%s)' % self.precision)
            if self.deterministic:      # before the workspace is sized: the fixed-order forms add slots to it
                if lib.pivp_plan_set_deterministic(plan.h, 1) != 0:
                    raise ValueError('deterministic=True is not served for precision=%r, model %s at B=%d, %dx%d'
                                     % (self.precision, self.model_type, B, H, W))
            nbytes = lib.pivp_plan_workspace_bytes(plan.h)
            plan.workspace = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            base = plan.workspace.data_ptr()
            aligned = (base + 255) // 256 * 256
            _lib.check(lib.pivp_plan_set_workspace(plan.h, aligned, nbytes), 'pivp_plan_set_workspace')
            self._bind(plan)
            self._plans[key] = plan
            self._reset_plan(plan)
        return plan

    def effective_plan_options(self):
        """The options of the current plan, read back from the library (pivp_plan_get_option): key -> value as in `plan_options`."""
        if self._active is None:
            raise RuntimeError('no plan yet: plans are made by the first call')
        lib, h = self._active.lib, self._active.h
        return OrderedDict((name, int(lib.pivp_plan_get_option(h, opt))) for name, (opt, _, _) in PLAN_OPTIONS.items())

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _reset_plan(self, plan):
        with torch.cuda.device(self.device):
            _lib.check(plan.lib.pivp_reset_state(plan.h, self._stream()), 'pivp_reset_state')

    # ---- the recurrent state across calls (carry_state=True; include/pivp_state.h) -----------------------------------------------------
    def _check_carried_shape(self, B, H, W):
        s = self._state
        if self.carry_state and s is not None and (s.batch, s.hw) != (B, (H, W)):
            raise ValueError('the model carries the recurrent state of batch %d at %dx%d frames, this call has batch %d at %dx%d: reset_state() first'
                             % (s.batch, s.hw[0], s.hw[1], B, H, W))

    @contextlib.contextmanager
    def _carried(self, plan, B, H, W, advance=True, observed=0):
        """Around ONE rollout of `plan`: registers where it reads its initial recurrent state (the carried one, if any) and leaves its final one (the
        model's buffer, unless advance=False), and clears the registration behind it, as backward() does with its seed.  With carry_state=False and
        no `observed` the library's setter is never called.  Yields whether the rollout starts from a carried state."""
        if not self.carry_state and not observed:
            yield False
            return
        cur = self._state if self.carry_state else None
        out = None
        if self.carry_state and advance:
            if self.state_backward:      # the final state goes to the OTHER buffer: a sweep reads the one this rollout starts from again
                spare = self._spare_state      # (a start from zeros reuses it too: what it held belonged to a call this one supersedes)
                fits = spare is not None and spare is not cur and (spare.batch, spare.hw) == (B, (H, W))
                out = spare if fits else RecurrentState.empty(B, (H, W), self.device)
            else:
                out = cur if cur is not None else RecurrentState.empty(B, (H, W), self.device)
        lib = plan.lib
        try:
            _lib.check(lib.pivp_plan_set_rollout_state(plan.h, cur.data.data_ptr() if cur is not None else None,
                                                       out.data.data_ptr() if out is not None else None, int(observed)), 'pivp_plan_set_rollout_state')
            yield cur is not None
            if out is not None:
                if out is not cur and cur is not None:
                    self._spare_state = cur      # (kept alive and unmodified until the next rollout)
                elif self._spare_state is out:
                    self._spare_state = None
                self._state = out      # (only behind a rollout that was enqueued whole)
        finally:
            lib.pivp_plan_set_rollout_state(plan.h, None, None, 0)

    def recurrent_state(self):
        """A snapshot (copy) of the carried recurrent state as a `RecurrentState`, or None when the next call starts from zeros (nothing was called
        since `reset_state()`).  Needs carry_state=True."""
        if not self.carry_state:
            raise RuntimeError('recurrent_state() needs Model(..., carry_state=True): without it no state exists between calls')
        return None if self._state is None else self._state.clone()

    def set_recurrent_state(self, s):
        """The next call starts from `s` (a `RecurrentState` on the model's device; it is copied, so later calls leave `s` itself untouched), or from
        zeros with None.  Loss, PSNR and the other results of the last call stay."""
        if not self.carry_state:
            raise RuntimeError('set_recurrent_state() needs Model(..., carry_state=True)')
        if s is None:
            self._state = None
            return
        self._checked_state(s)
        self._state = s.clone()

    def _checked_state(self, s):
        if not isinstance(s, RecurrentState):
            raise ValueError('a RecurrentState (or None) is expected, not %r' % (type(s).__name__,))
        if self._hw is not None and s.hw != self._hw:
            raise ValueError('the model was sized for %dx%d frames, the state is of %dx%d' % (self._hw + s.hw))
        if s.data.device != self.device and not (s.data.is_cuda and self.device.type == 'cuda' and self.device.index is None):
            raise ValueError('the state lives on %s, the model on %s' % (s.data.device, self.device))
        return True

    def _adopt_state(self, s):
        """set_recurrent_state without the copy: the model takes `s` itself and later calls write into it."""
        self._checked_state(s)
        self._state = s

    # ---- reference surface ----------------------------------------------------------------
    def reset_state(self):
        """TM:604-618: clears loss/PSNR/summaries/conv_res and the seven ConvLSTM (c, h) pairs: with carry_state=True the carried state is dropped and
        the next call starts from zeros; without it every call does, and only the plan's zero buffer is cleared."""
        self._state = None
        self._carried_start = False
        self.loss = 0.0
        self.psnr_all = 0.0
        self._results = None
        self._imagined = False
        self.loss_terms = None
        self._loss_grad = None
        if self._active is not None:
            self._reset_plan(self._active)

    def to_gpu(self, device=None):
        if device is not None:
            self.device = torch.device('cuda:%d' % device if isinstance(device, int) else device)
        return self

    def _as_device(self, a, shape_tail, what=None):
        if isinstance(a, (list, tuple)):
            a = torch.stack([x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, dtype=np.float32)) for x in a])
        elif not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
        a = a.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(a.shape[-len(shape_tail):]) != tuple(shape_tail) and shape_tail:
            raise ValueError('unexpected trailing shape %s%s' % (tuple(a.shape), ': %s' % what if what else ''))
        return a

    def _sync_packs(self, plan):
        """The precision modes' weight packs are kept across calls while the parameters are untouched: torch counts in-place writes to the flat
        buffer and its views (_version), the optimizer's own kernel reports itself (_params_epoch)."""
        pkey = (self._flat_params.data_ptr(), self._flat_params._version, getattr(self, '_params_epoch', 0))
        if getattr(plan, 'packed_key', None) != pkey:
            _lib.check(plan.lib.pivp_plan_params_changed(plan.h), 'pivp_plan_params_changed')
            plan.packed_key = pkey

    def _left_by_rollout(self, inputs, gen, gen_states, results):
        """What either rollout leaves on the model.  results: pivp_rollout_forward's, or None behind pivp_rollout_predict (taps exist, a loss does not)."""
        self._inputs = inputs   # keep alive until the stream has consumed them
        self._gen = gen
        self._gen_states = gen_states
        self._results = results
        self._imagined = results is None
        self.gen_images = [gen[t] for t in range(gen.shape[0])]
        self.gen_states = [gen_states[t] for t in range(gen_states.shape[0])]
        self.loss_terms = None
        self._loss_grad = None

    def __call__(self, x, iter_num=-1.0):
        """TM:620-764.  x = [images (T,B,3,H,W), actions (T,B,action_dim), states (T,B,state_dim)], time-major (5 / 5 unless the model was built otherwise)."""
        if len(x) > 1:
            images, actions, states = x
        else:
            images, actions, states = x[0], None, None
        if actions is None or states is None:
            # the reference dereferences states[0] (TM:646) and fails the same way
            raise TypeError("'NoneType' object is not subscriptable")
        if self._state is not None:      # a carried state of another batch or frame size: refused before any GPU work
            shp = self._host_shape(images)
            if len(shp) == 5:
                self._check_carried_shape(shp[1], shp[3], shp[4])
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            self._require_gpu()
            images = self._as_device(images, ())
            if images.dim() != 5 or images.shape[2] != 3:
                raise ValueError('images must be time-major (T, B, 3, H, W)')
            T, B, _, H, W = images.shape
            actions = self._as_device(actions, (self.action_dim,), 'actions must be (T, B, %d), the model\'s action_dim' % self.action_dim)
            states = self._as_device(states, (self.state_dim,), 'states must be (T, B, %d), the model\'s state_dim' % self.state_dim)
            plan = self._plan_for(B, T, H, W)
            self._active = plan
            ctx = self.num_frame_before_prediction
            # feed-self when not training or k == -1 (TM:649-657)
            gt_ptr = None
            self._gt_mask = None
            if config.train and self.scheduled_sampling_k != -1:
                mask = scheduled_sampling_masks(B, T, ctx, self.scheduled_sampling_k, iter_num, rng=self.sampling_rng)
                self._gt_mask = torch.from_numpy(mask).to(self.device)
                gt_ptr = self._gt_mask.data_ptr()
            gen = torch.empty((T - 1, B, 3, H, W), dtype=torch.float32, device=self.device)
            gen_states = torch.empty((T - 1, B, self.state_dim), dtype=torch.float32, device=self.device)
            nf = T - ctx
            results = torch.empty(2 + 3 * nf, dtype=torch.float32, device=self.device)
            self._sync_packs(plan)
            with self._carried(plan, B, H, W) as carried:
                _lib.check(plan.lib.pivp_rollout_forward(plan.h, images.data_ptr(), actions.data_ptr(), states.data_ptr(),
                                                         gt_ptr, gen.data_ptr(), gen_states.data_ptr(), results.data_ptr(),
                                                         self._stream()), 'pivp_rollout_forward')
            self._carried_start = carried
            self._left_by_rollout((images, actions, states), gen, gen_states, results)
            self._nf = nf
            self.loss = results[0]
            self.psnr_all = results[1]
            if self._extra_loss:
                self._add_image_loss(gen, images, ctx, config.train and self.keep_activations)
        return self.loss

    def _add_image_loss(self, gen, images, ctx, want_grad):
        """ONE pivp_image_loss call on the scored frames gen[ctx-1:] against images[ctx:] (both contiguous: N = (T-ctx) * B images), on the rollout's
        stream and without a synchronisation.  The reference's loss already holds the MSE once, so the op's MSE weight is mse - 1."""
        from .losses import _launch
        spec = self.image_loss
        T, B, C, H, W = images.shape
        spec.check_frames((C, H, W))
        out = _launch(gen[ctx - 1:], images[ctx:], (T - ctx) * B, C, H, W, spec._struct(extra_mse=spec.mse - 1.0), bool(want_grad), (T - ctx, B))
        self.loss = self._results[0] + out.terms[4]
        self.loss_terms = dict(mse=out.terms[0], l1=out.terms[1], gdl=out.terms[2], dssim=out.terms[3], extra=out.terms[4])
        self._loss_grad = out.grad

    # ---- evaluation surface (no counterpart in the reference, whose only quality number is psnr_all: the PSNR of the batch-mean MSE) -------
    def evaluate(self, x, win=11, sigma=1.5, data_range=1.0):
        """Per-sample quality of a feed-self rollout: `__call__(x)` under using_config('train', False) -- ground truth enters through the context
        frames only --, then ONE pivp_frame_metrics launch on the scored frames gen[ctx-1:] against images[ctx:], on the same stream and without
        a host synchronisation in between.  -> SimpleNamespace(mse, psnr, ssim) of (T-ctx, B) device tensors (`metrics.frame_metrics`), also kept
        as `model.metrics`; feed it to `metrics.StepCurves`.  `loss`, `psnr_all`, `summaries`, `gen_images` and `gen_states` are what that
        `__call__` leaves."""
        from . import metrics as M
        images = x[0]
        shp = self._host_shape(images)
        ctx = int(self.num_frame_before_prediction)
        if len(shp) != 5 or shp[2] != 3:
            raise ValueError('images must be time-major (T, B, 3, H, W)')
        if not 1 <= ctx < shp[0]:
            raise ValueError('no scored frames: %d frames with num_frame_before_prediction=%d' % (shp[0], ctx))
        lead, N, C, H, W, win, sigma, data_range = M._check_metric_args((shp[0] - ctx,) + shp[1:], (shp[0] - ctx,) + shp[1:], win, sigma, data_range)
        with using_config('train', False):
            self(x)
        with torch.cuda.device(self.device):
            self.metrics = M._launch(self._gen[ctx - 1:], self._inputs[0][ctx:], N, C, H, W, win, sigma, data_range, lead)
        return self.metrics

    # ---- planning surface (no counterpart in the reference: Finn & Levine 2017 roll this model forward under candidate actions) -------
    MAX_TRACK_PLANES = 8

    @staticmethod
    def _host_shape(a):
        """Shape of an argument as `_as_device` would see it, without touching a device."""
        if torch.is_tensor(a):
            return tuple(a.shape)
        if isinstance(a, (list, tuple)) and len(a) and torch.is_tensor(a[0]):
            return (len(a),) + tuple(a[0].shape)
        return tuple(np.shape(a))

    def _check_imagine_args(self, context_images, actions, state, designated, designated_frame, observed=None, advance=True):
        """-> (ctx, T, B, H, W, P, f); every complaint is a ValueError raised before the GPU or the library is needed.  ctx: the number of observed
        frames -- `observed`, or num_frame_before_prediction with None."""
        ctx = int(self.num_frame_before_prediction)
        if observed is not None:
            if isinstance(observed, bool) or not isinstance(observed, (int, np.integer)) or observed < 1:
                raise ValueError('observed must be a positive integer (the number of frames in context_images) or None, not %r' % (observed,))
            if not self.carry_state:
                raise ValueError('observed is for continuing from a carried recurrent state: the model needs carry_state=True')
            ctx = int(observed)
        if not isinstance(advance, bool):
            raise ValueError('advance must be a bool, not %r' % (advance,))
        if not advance and not self.carry_state:
            raise ValueError('advance=False leaves a carried recurrent state untouched: the model needs carry_state=True')
        si, sa, ss = self._host_shape(context_images), self._host_shape(actions), self._host_shape(state)
        if len(si) != 5 or si[2] != 3:
            raise ValueError('context_images must be time-major (ctx, B, 3, H, W), got shape %s' % (si,))
        if observed is not None and si[0] != ctx:
            raise ValueError('context_images holds %d frames, observed=%d was given' % (si[0], ctx))
        if ctx < 1 or si[0] != ctx:
            raise ValueError('context_images holds %d frames, the model was built with num_frame_before_prediction=%d' % (si[0], ctx))
        _, B, _, H, W = si
        if B < 1 or H < 1 or W < 1:
            raise ValueError('context_images is empty: shape %s' % (si,))
        self._check_carried_shape(B, H, W)
        A, S = self.action_dim, self.state_dim
        if len(sa) != 3 or sa[1] != B or sa[2] != A:
            raise ValueError('actions must be (T-1, %d, %d) for a model with action_dim=%d, got shape %s' % (B, A, A, sa))
        if sa[0] < ctx:
            raise ValueError('actions cover %d steps; at least the %d context steps are needed (T - 1 >= ctx)' % (sa[0], ctx))
        if ss != (B, S):
            raise ValueError('state must be (%d, %d) for a model with state_dim=%d: the robot state of frame 0, got shape %s' % (B, S, S, ss))
        T = sa[0] + 1
        P, f = 0, ctx - 1
        if designated is None:
            if designated_frame is not None:
                raise ValueError('designated_frame given without designated planes')
        else:
            sd = self._host_shape(designated)
            if len(sd) != 4 or sd[0] != B or sd[2:] != (H, W):
                raise ValueError('designated must be (%d, P, %d, %d), got shape %s' % (B, H, W, sd))
            P = sd[1]
            if not 1 <= P <= self.MAX_TRACK_PLANES:
                raise ValueError('designated holds %d planes per sample; 1 to %d are served' % (P, self.MAX_TRACK_PLANES))
            if designated_frame is not None:
                if isinstance(designated_frame, bool) or int(designated_frame) != designated_frame:
                    raise ValueError('designated_frame must be an integer frame index, not %r' % (designated_frame,))
                f = int(designated_frame)
            if not 0 <= f <= ctx - 1:
                raise ValueError('designated_frame %d is not an observed frame (0 .. %d)' % (f, ctx - 1))
        return ctx, T, B, H, W, P, f

    def imagine(self, context_images, actions, state, designated=None, designated_frame=None, normalize=False, observed=None, advance=True):
        """Open-loop prediction for planning: roll the model forward from `context_images` (ctx, B, 3, H, W) -- the observed frames --, the robot
        `state` (B, state_dim) of frame 0 and candidate `actions` (T-1, B, action_dim), feeding its own predictions back after the context.  No ground truth beyond
        the context, no loss: `loss` / `psnr_all` are left alone, `summaries` is [] and `backward()` raises until the model is called again.  Always
        feed-self (ignores config.train and scheduled sampling) and always on an inference plan.  Sets `gen_images` / `gen_states` as `__call__`
        does and returns the frames as one tensor (T-1, B, 3, H, W): bit-identical to a feed-self `__call__` on the same context.

        designated: (B, P, H, W) non-negative planes (1 <= P <= 8; `planning.one_hot_planes`) given on frame `designated_frame` (0 .. ctx-1, default
        the last observed one).  Every step from that frame on moves them exactly as it moves the frame's pixels -- the step's transforms and
        compositing masks are a linear map, applied here to the planes with the synthesised layer set to zero (painted-from-scratch pixels carry
        no mass) -- giving the predicted distribution of the designated pixels: `pixel_distrib` (T-1-f, B, P, H, W), entry i on predicted frame
        f+1+i, and `pixel_mass` (T-1-f, B, P), always the raw plane sums.  normalize=True divides each plane by its sum; the raw mass is
        informative (how much of the pixel the model explains by motion), so this is optional.

        With carry_state=True the rollout starts from the carried recurrent state (zeros after `reset_state()`) and leaves its own behind.
        observed: the number of frames in `context_images` when it is not num_frame_before_prediction (None: that one, as ever): 1 <= observed <= T-1,
        and designated_frame <= observed-1 (default observed-1).  advance=False reads the carried state and leaves it untouched -- K what-ifs from one
        belief.  To CONTINUE an open-loop prediction, pass the last predicted frame as the one observed frame and the last predicted robot state:

            gen = model.imagine(context, actions[:n], state0)                                                  # steps 0 .. n-1
            more = model.imagine(gen[-1:], actions[n:], model.gen_states[-1], observed=1)                      # steps n ..: torch.cat((gen, more)) is
                                                                                                               # the one rollout over all of actions, bit for bit

        (tracked planes continue the same way: designated=model.pixel_distrib[-1] of an un-normalised first call, on frame 0 of the second)."""
        ctx, T, B, H, W, P, f = self._check_imagine_args(context_images, actions, state, designated, designated_frame, observed, advance)
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            self._require_gpu()
            images = self._as_device(context_images, ())
            actions = self._as_device(actions, (self.action_dim,))
            state = self._as_device(state, (self.state_dim,))
            planes = self._as_device(designated, ()) if P else None
            gen, track = self._rollout_predict(images, actions, state, planes, f, observed=observed, advance=advance)
            if P:
                mass = track.sum(dim=(3, 4))
                self.pixel_mass = mass
                self.pixel_distrib = track / mass[..., None, None] if normalize else track
        return gen

    def _rollout_predict(self, images, actions, state, planes, f, observed=None, advance=True):
        """pivp_rollout_predict on checked, contiguous fp32 tensors of this device (the caller holds the device context): -> (frames, raw tracked
        planes or None).  Sets what `imagine` sets, with `pixel_distrib` / `pixel_mass` cleared; no torch pass over the planes.  observed / advance:
        as `imagine`'s (carry_state=True only)."""
        _, B, _, H, W = images.shape
        T = actions.shape[0] + 1
        P = planes.shape[1] if planes is not None else 0
        plan = self._plan_for(B, T, H, W, keep_activations=False, observed=observed)
        self._active = plan
        gen = torch.empty((T - 1, B, 3, H, W), dtype=torch.float32, device=self.device)
        gen_states = torch.empty((T - 1, B, self.state_dim), dtype=torch.float32, device=self.device)
        track = torch.empty((T - 1 - f, B, P, H, W), dtype=torch.float32, device=self.device) if P else None
        self._sync_packs(plan)
        with self._carried(plan, B, H, W, advance=advance, observed=observed or 0):
            _lib.check(plan.lib.pivp_rollout_predict(plan.h, images.data_ptr(), actions.data_ptr(), state.data_ptr(),
                                                     planes.data_ptr() if P else None, P, f, gen.data_ptr(), gen_states.data_ptr(),
                                                     track.data_ptr() if P else None, self._stream()), 'pivp_rollout_predict')
        self._left_by_rollout((images, actions, state, planes), gen, gen_states, None)
        self._gt_mask = None
        self.pixel_mass = None
        self.pixel_distrib = None
        return gen, track

    # ---- training surface (Chainer: model.cleargrads(); loss.backward(); TM:950 via optimizer.update) -------
    def cleargrads(self):
        if self._flat_params is None:
            raise RuntimeError('call the model first (parameters are lazily sized)')
        self._ensure_grads().zero_()

    def grad_group_ranges(self):
        """[(start, end)] slices of `_flat_grads`, in the order the backward sweep completes them (include/pivp_hip.h)."""
        if self._offsets is None:
            raise RuntimeError('call the model first (parameters are lazily sized)')
        return list(self._group_ranges)

    def _state_grad_args(self, initial_state_grad, final_state_grad):
        """The argument checks of backward()'s two state keywords: every complaint is a ValueError raised before the GPU or the library is needed."""
        if not isinstance(initial_state_grad, bool):
            raise ValueError('initial_state_grad must be a bool, not %r' % (initial_state_grad,))
        if (initial_state_grad or final_state_grad is not None) and not self.state_backward:
            raise ValueError('initial_state_grad / final_state_grad need Model(..., carry_state=True, keep_activations=True, state_backward=True)')
        if initial_state_grad and not self._carried_start:
            raise ValueError('initial_state_grad=True: the last call started from zeros (after reset_state()), not from a carried state')
        if final_state_grad is not None:
            if not isinstance(final_state_grad, RecurrentState):
                raise ValueError('final_state_grad must be a RecurrentState (or None), not %r' % (type(final_state_grad).__name__,))
            self._checked_state(final_state_grad)
            swept = self._swept_shape()
            if swept is not None and (final_state_grad.batch, final_state_grad.hw) != swept:
                raise ValueError('final_state_grad is of batch %d at %dx%d frames, the last call ran batch %d at %dx%d'
                                 % ((final_state_grad.batch,) + final_state_grad.hw + (swept[0],) + swept[1]))

    def _swept_shape(self):
        """(batch, (H, W)) of the last training call -- what its plan was made for and the sweep will run at, whatever was done to the carried state
        since -- or None before any call."""
        inputs = getattr(self, '_inputs', None)
        if inputs is None or self._hw is None:
            return None
        return int(inputs[1].shape[1]), tuple(self._hw)

    def _state_grad_buffer(self, seed):
        """Where the sweep leaves d loss / d (initial state), sized for the call that is swept: `initial_state_grad` again when it fits -- or, when that
        very buffer seeds this sweep (chunked_backward hands one window's result to the next sweep), the buffer it alternates with."""
        batch, hw = self._swept_shape()
        fits = lambda g: g is not None and (g.batch, g.hw) == (batch, hw)
        dst = self.initial_state_grad if fits(self.initial_state_grad) else None
        if dst is not None and seed is not None and dst.data.data_ptr() == seed.data.data_ptr():
            dst, self._spare_state_grad = (self._spare_state_grad if fits(self._spare_state_grad) else None), dst
        if dst is None:
            dst = RecurrentState.empty(batch, hw, self.device)
        self.initial_state_grad = dst
        return dst

    def backward(self, on_group=None, frame_grad=None, input_grad=False, params=True, builtin_loss=True, initial_state_grad=False, final_state_grad=None):
        """Back-propagate the loss of the LAST call through time (needs keep_activations=True).  Gradients
        accumulate into `model._flat_grads` (internal layouts); `grads_reference()` returns them in checkpoint layout.

        frame_grad: an additional d loss / d gen_images[ctx-1:], a (T-ctx, B, 3, H, W) float32 tensor on the model's device -- the gradient of any
        loss of the predicted frames the caller computed (in torch, say).  It joins the sweep's seed beside the reference loss's own gradient and
        the model's image loss's, if it has one (pivp_plan_set_frame_grad, include/pivp_loss.h).

        on_group(i): optional host callback, invoked from inside the sweep as soon as every kernel that contributes to
        gradient group i (slice grad_group_ranges()[i]) has been enqueued on the model's stream -- the hook the
        data-parallel all-reduce uses to overlap communication with the rest of the sweep.

        input_grad=True: the sweep also leaves d loss / d actions[:T-1] in `model.action_grad` (T-1, B, action_dim) and d loss / d states[0] in
        `model.state_grad` (B, state_dim), float32 tensors on the model's device (pivp_plan_set_input_grad, include/pivp_input_grad.h).  They are overwritten, not
        accumulated; the buffers are reused by the next such call of the same shape, and nothing synchronises.
        params=False: the sweep skips every launch that only forms parameter gradients (pivp_plan_set_sweep_mode) -- for callers who want the input
        gradients alone.  `_flat_grads` then holds unspecified values: `cleargrads()` before the next full sweep.  `on_group` must be None.
        builtin_loss=False: the sweep differentiates `frame_grad` (and the model's image loss, if it has one) alone, without the reference's frame and
        state MSE; without either there is nothing to differentiate and the call raises ValueError.
        Both switches hold for this call only.

        On a model built with state_backward=True (otherwise a call that started from a carried state is refused: truncated BPTT needs the flag):
        the state the last call started from is a constant of the sweep.  initial_state_grad=True: the sweep also leaves d loss / d (that state) in
        `model.initial_state_grad`, a `RecurrentState`; it is overwritten by each such call and reused by the next one of the same shape.
        final_state_grad: a `RecurrentState` of the model's batch and frame size, d (some later loss) / d (the state the last call left); it joins the
        sweep at its first visited timestep and alone counts as something to differentiate under builtin_loss=False.  Both hold for this call only."""
        if not params and on_group is not None:
            raise ValueError('backward(params=False) announces no gradient group: on_group must be None')
        self._state_grad_args(initial_state_grad, final_state_grad)
        if not builtin_loss and frame_grad is None and self._loss_grad is None and final_state_grad is None:
            raise ValueError('backward(builtin_loss=False) needs frame_grad (or a model with an image loss): there is nothing to differentiate')
        plan = self._active
        if plan is None or self._results is None:
            raise RuntimeError('call the model first')
        if not self.keep_activations:
            raise RuntimeError('backward() needs Model(..., keep_activations=True)')
        if self._carried_start and not self.state_backward:
            raise RuntimeError('the last call started from a carried recurrent state: truncated BPTT across calls needs Model(..., state_backward=True) '
                               '(or reset_state() in front of every call that is back-propagated)')
        self._ensure_grads()
        images, actions, states = self._inputs
        gt_ptr = self._gt_mask.data_ptr() if self._gt_mask is not None else None
        seed = self._loss_grad
        if self._extra_loss and seed is None:
            raise RuntimeError('the last call kept no gradient of the image loss (it ran under using_config(\'train\', False)): call the model in training mode')
        if frame_grad is not None:
            want = (images.shape[0] - self.num_frame_before_prediction,) + tuple(images.shape[1:])
            if not torch.is_tensor(frame_grad) or tuple(frame_grad.shape) != want or frame_grad.dtype != torch.float32 or frame_grad.device != images.device:
                raise ValueError('frame_grad must be a float32 tensor of shape %s on %s' % (want, images.device))
            frame_grad = frame_grad.contiguous()
            seed = frame_grad if seed is None else seed + frame_grad
        cb = None
        if on_group is not None:
            import ctypes
            errors = []

            def _trampoline(_user, g):
                try:
                    on_group(int(g))
                except BaseException as e:      # never unwind through the C frames
                    errors.append(e)
            cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)(_trampoline)
            _lib.check(plan.lib.pivp_plan_set_grad_callback(plan.h, ctypes.cast(cb, ctypes.c_void_p), None), 'pivp_plan_set_grad_callback')
        mode = (_lib.SWEEP_PARAMS if params else 0) | (_lib.SWEEP_BUILTIN_LOSS if builtin_loss else 0)
        if input_grad:
            shape = (images.shape[0] - 1, images.shape[1], self.action_dim)
            if self.action_grad is None or tuple(self.action_grad.shape) != shape or self.action_grad.device != images.device:
                self.action_grad = torch.empty(shape, dtype=torch.float32, device=images.device)
                self.state_grad = torch.empty((shape[1], self.state_dim), dtype=torch.float32, device=images.device)
        state_dst = self._state_grad_buffer(final_state_grad) if initial_state_grad else None
        try:
            # the model's device must be the CURRENT one for the launches (and for the plan's own side stream, created on first use)
            with torch.cuda.device(self.device):
                if self.state_backward:      # the sweep may start at a carried state; the seed on the final state and where d / d (initial state) goes
                    _lib.check(plan.lib.pivp_plan_set_state_grad(plan.h, 1, final_state_grad.data.data_ptr() if final_state_grad is not None else None,
                                                                 state_dst.data.data_ptr() if state_dst is not None else None), 'pivp_plan_set_state_grad')
                if input_grad:
                    _lib.check(plan.lib.pivp_plan_set_input_grad(plan.h, self.action_grad.data_ptr(), self.state_grad.data_ptr()), 'pivp_plan_set_input_grad')
                if mode != 3:
                    _lib.check(plan.lib.pivp_plan_set_sweep_mode(plan.h, mode), 'pivp_plan_set_sweep_mode')
                if seed is not None:      # (torch keeps the tensor's memory for the stream that is current here, the sweep's)
                    _lib.check(plan.lib.pivp_plan_set_frame_grad(plan.h, seed.data_ptr()), 'pivp_plan_set_frame_grad')
                _lib.check(plan.lib.pivp_rollout_backward(plan.h, images.data_ptr(), actions.data_ptr(), states.data_ptr(), gt_ptr,
                                                          self._gen.data_ptr(), self._gen_states.data_ptr(), self._stream()),
                           'pivp_rollout_backward')
        finally:
            if self.state_backward:
                plan.lib.pivp_plan_set_state_grad(plan.h, 0, None, None)
            if input_grad:
                plan.lib.pivp_plan_set_input_grad(plan.h, None, None)
            if mode != 3:
                plan.lib.pivp_plan_set_sweep_mode(plan.h, 3)
            if seed is not None:
                plan.lib.pivp_plan_set_frame_grad(plan.h, None)
            if cb is not None:
                plan.lib.pivp_plan_set_grad_callback(plan.h, None, None)
        if cb is not None and errors:
            raise errors[0]

    def set_group_join(self, join):
        """join=False: a gradient group's announcement no longer makes the model's stream wait for the group's weight gradients on the
        plan's side stream; the listener must then call wait_group(g, its_stream) (include/pivp_hip.h: pivp_plan_set_group_join)."""
        plan = self._active
        if plan is None:
            raise RuntimeError('call the model first')
        _lib.check(plan.lib.pivp_plan_set_group_join(plan.h, 1 if join else 0), 'pivp_plan_set_group_join')

    def wait_group(self, g, stream):
        """Make `stream` (a torch.cuda.Stream) wait for the side-stream work of gradient group g."""
        plan = self._active
        with torch.cuda.device(self.device):
            _lib.check(plan.lib.pivp_plan_group_wait(plan.h, int(g), stream.cuda_stream), 'pivp_plan_group_wait')

    def grads_reference(self):
        """Gradients in the reference's Chainer-npz layout (same permutations as the parameters)."""
        if self._grads is None:
            raise RuntimeError('no gradients: call cleargrads()/backward() first')
        out = OrderedDict()
        for key, shape in self._shapes().items():
            out[key] = ckpt.from_internal(key, self._grads[key].cpu().numpy(), shape)
        return out

    @property
    def summaries(self):
        """TM:744-759: strings '<prefix>_recon_cost<i>: v', '_psnr<i>', '_state_cost<i>', '_psnr_all', '_loss'."""
        if self._results is None:
            return []
        r = self._results.cpu().numpy()
        nf = self._nf
        p = str(self.prefix)
        out = []
        for i in range(nf):
            out.append(p + '_recon_cost' + str(i) + ': ' + str(r[2 + i]))
            out.append(p + '_psnr' + str(i) + ': ' + str(r[2 + nf + i]))
        for i in range(nf):
            out.append(p + '_state_cost' + str(i) + ': ' + str(r[2 + 2 * nf + i]))
        out.append(p + '_psnr_all: ' + str(r[1]))
        out.append(p + '_loss: ' + str(r[0]))
        return out

    def tap(self, name, step=None):
        """Activation of a timestep, planar NCHW like the reference's encs/hiddens (TM:703-708)."""
        plan = self._active
        if plan is None or (self._results is None and not self._imagined):
            raise RuntimeError('call the model first')
        cfg = plan.cfg
        T1 = cfg.seq_len - 1
        step = T1 - 1 if step is None else step
        H, W, B = cfg.height, cfg.width, cfg.batch
        lv = {'enc0': (32, 2), 'enc1': (32, 4), 'enc2': (64, 8), 'enc3': (64, 8), 'enc4': (128, 4), 'enc5': (96, 2),
              'enc6': (64, 1), 'hidden1': (32, 2), 'hidden2': (32, 2), 'hidden3': (64, 4), 'hidden4': (64, 4),
              'hidden5': (128, 8), 'hidden6': (64, 4), 'hidden7': (32, 2)}
        for i, (nm, (_, c)) in enumerate(LSTM_SIZES.items()):
            d = [2, 2, 4, 4, 8, 4, 2][i]
            lv[nm + '_h'] = (c, d); lv[nm + '_c'] = (c, d)
        if name in lv:
            C, d = lv[name]
            shape = (B, C, H // d, W // d)
        elif name == 'enc7':
            shape = (B, 25 if self.model_type == 'DNA' else 3, H, W)
        elif name == 'masks':
            shape = (B, self.num_masks + 1, H, W)
        elif name == 'cdna_kerns':
            shape = (B, self.num_masks, 5, 5)
        elif name == 'stp_theta':
            shape = (B, 2, 3)
        else:
            raise KeyError(name)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            n = plan.lib.pivp_get_tap(plan.h, name.encode(), step, out.data_ptr(), self._stream())
        if n < 0:
            _lib.check(int(n), 'pivp_get_tap(%s, %d)' % (name, step))
        assert n == out.numel()
        return out

    @property
    def conv_res(self):
        """TM:715, TM:734: [enc0..enc6, enc7] of the LAST timestep."""
        if self._results is None and not self._imagined:
            return []
        return [self.tap(n) for n in ('enc0', 'enc1', 'enc2', 'enc3', 'enc4', 'enc5', 'enc6', 'enc7')]
