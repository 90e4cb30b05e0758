"""CPU-side tests of the recurrent state across calls: the C-ABI surface of include/pivp_state.h against `_lib.STATE_SIGNATURES` and the built
library, pivp_state_layout against a table written out here, the plan's registration and its refusals, the argument checks of
`imagine(observed=...)`, `cem_plan(belief=...)` / `score_actions(belief=...)` and `RecurrentState.select`, and that a model without carry_state
never calls the setter (a recording stand-in for the library).  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import RecurrentState, _lib, planning
from pivp_amd.state import state_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'pivp_state_layout', 'pivp_plan_set_rollout_state', 'pivp_plan_get_rollout_state', 'pivp_state_copy'}
# floats per sample of c_0, h_0, c_1, h_1, ...: cell i lives on the (H, W) / level_i map with C_i channels, levels 2 2 4 4 8 4 2, channels
# 32 32 64 64 128 64 32 (TM:509-515) -- written out, not computed
LAYOUT = {
    (64, 64): ([32768, 32768, 32768, 32768, 16384, 16384, 16384, 16384, 8192, 8192, 16384, 16384, 32768, 32768], 311296),
    (16, 16): ([2048, 2048, 2048, 2048, 1024, 1024, 1024, 1024, 512, 512, 1024, 1024, 2048, 2048], 19456),
    (128, 64): ([65536, 65536, 65536, 65536, 32768, 32768, 32768, 32768, 16384, 16384, 32768, 32768, 65536, 65536], 622592),
}


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def _cfg(H=64, W=64, B=2, T=4, keep=0):
    return _lib.PivpConfig(batch=B, seq_len=T, height=H, width=W, num_masks=10, model_type=0, use_state=1, context_frames=2, keep_activations=keep,
                           ln_eps=1e-6, stp_zero_border=0)


def test_state_header_library_and_ctypes_table_agree():
    """The new entry points have a header and a table of their own; the model's ABI, its version and the other headers stay as they were."""
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_state.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.STATE_SIGNATURES) == NAMES and declared <= exported
    for header, other in _lib.HEADER_SIGNATURES.items():
        assert header == 'pivp_state.h' or not declared & set(other)
    assert len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)      # (as before)
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17
    i, vp, ll, ptr = _lib._i, _lib._vp, _lib._ll, ctypes.POINTER
    assert _lib.STATE_SIGNATURES['pivp_state_layout'] == (i, [ptr(_lib.PivpConfig), ptr(ll), ptr(ll)])
    assert _lib.STATE_SIGNATURES['pivp_plan_set_rollout_state'] == (i, [vp, vp, vp, i])
    assert _lib.STATE_SIGNATURES['pivp_plan_get_rollout_state'] == (i, [vp, ptr(vp), ptr(vp), ptr(i)])
    assert _lib.STATE_SIGNATURES['pivp_state_copy'] == (i, [ptr(_lib.PivpConfig), vp, i, vp, i, vp, vp])
    for name, (res, args) in _lib.STATE_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    # the rollouts keep their signatures
    assert _lib.SIGNATURES['pivp_rollout_forward'] == (i, [vp] * 9) and _lib.SIGNATURES['pivp_rollout_predict'] == (i, [vp] * 5 + [i, i] + [vp] * 4)
    assert 'state.hip' in build.SOURCES and 'pivp_state.h' in [os.path.basename(f) for f in _digest.source_files()]
    header = open(os.path.join(ROOT, 'include', 'pivp_state.h')).read()
    assert int(re.search(r'#define PIVP_STATE_SEGMENTS (\d+)', header).group(1)) == _lib.STATE_SEGMENTS == 14
    assert 'truncated back-propagation' in header and 'PIVP_ERR_STATE' in header      # the follow-up left out is named where the ABI is declared


@pytest.mark.parametrize('hw', sorted(LAYOUT))
def test_state_layout_against_the_table(hw):
    lib = _lib.load()
    seg = (ctypes.c_longlong * 14)()
    total = ctypes.c_longlong()
    cfg = _cfg(*hw)
    assert lib.pivp_state_layout(ctypes.byref(cfg), seg, ctypes.byref(total)) == 0
    assert (list(seg), total.value) == LAYOUT[hw] == state_layout(*hw)
    assert sum(LAYOUT[hw][0]) == LAYOUT[hw][1] and all(n % 4 == 0 for n in LAYOUT[hw][0])      # whole 16-byte pieces per sample
    assert lib.pivp_state_layout(ctypes.byref(cfg), None, ctypes.byref(total)) == 0 and lib.pivp_state_layout(ctypes.byref(cfg), seg, None) == 0


def test_layout_and_copy_refusals_need_no_gpu():
    lib = _lib.load()
    seg = (ctypes.c_longlong * 14)()
    assert lib.pivp_state_layout(None, seg, None) == -1
    for H, W in ((8, 64), (64, 60), (20, 64)):
        cfg = _cfg(H, W)
        assert lib.pivp_state_layout(ctypes.byref(cfg), seg, None) == -1
        assert lib.pivp_state_copy(ctypes.byref(cfg), 4096, 1, 8192, 1, None, None) == -1
    cfg = _cfg(16, 16)
    c = ctypes.byref(cfg)
    # (refused before anything is launched or read: the pointers are never followed)
    assert lib.pivp_state_copy(None, 4096, 1, 8192, 1, None, None) == -1
    assert lib.pivp_state_copy(c, None, 1, 8192, 1, None, None) == -1 and lib.pivp_state_copy(c, 4096, 1, None, 1, None, None) == -1
    assert lib.pivp_state_copy(c, 4096, 0, 8192, 1, 4096, None) == -1 and lib.pivp_state_copy(c, 4096, 1, 8192, 0, 4096, None) == -1
    assert lib.pivp_state_copy(c, 4096, 2, 8192, 3, None, None) == -1      # no index: the identity needs equal batches
    assert lib.pivp_state_copy(c, 4097, 1, 8192, 1, None, None) == -1 and lib.pivp_state_copy(c, 4096, 1, 8194, 1, None, None) == -1
    with pytest.raises(ValueError, match='multiples of 8'):
        state_layout(60, 64)


def test_plan_registration_needs_no_gpu():
    lib = _lib.load()
    cfg = _cfg(T=5)
    h = _lib._vp()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    a, b, o = _lib._vp(1), _lib._vp(1), ctypes.c_int(-7)
    try:
        assert lib.pivp_plan_get_rollout_state(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o)) == 0
        assert (a.value, b.value, o.value) == (None, None, 0)                      # the default: nothing registered
        assert lib.pivp_plan_set_rollout_state(h, 4096, 8192, 1) == 0
        assert lib.pivp_plan_get_rollout_state(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o)) == 0
        assert (a.value, b.value, o.value) == (4096, 8192, 1)
        assert lib.pivp_plan_set_rollout_state(h, 4096, 4096, 4) == 0               # in == out is allowed; observed up to T-1
        assert lib.pivp_plan_get_rollout_state(h, None, None, ctypes.byref(o)) == 0 and o.value == 4
        for bad in ((4100, None, 0), (None, 4104, 0), (None, None, -1), (None, None, 5)):      # off 16 bytes; observed outside 0 .. T-1
            assert lib.pivp_plan_set_rollout_state(h, *bad) == -1
        assert lib.pivp_plan_get_rollout_state(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o)) == 0
        assert (a.value, b.value, o.value) == (4096, 4096, 4)                      # a refused call changes nothing
        assert lib.pivp_plan_set_rollout_state(h, None, None, 0) == 0
        assert lib.pivp_plan_get_rollout_state(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o)) == 0
        assert (a.value, b.value, o.value) == (None, None, 0)
    finally:
        lib.pivp_plan_destroy(h)
    assert lib.pivp_plan_set_rollout_state(None, None, None, 0) == -1 and lib.pivp_plan_get_rollout_state(None, None, None, None) == -1


def _host_state(batch=1, hw=(16, 16), fill=None):
    n = batch * LAYOUT[hw][1] if hw in LAYOUT else batch * state_layout(*hw)[1]
    data = torch.arange(n, dtype=torch.float32) if fill is None else torch.full((n,), float(fill))
    return RecurrentState(data, batch, hw)


def test_recurrent_state_value_and_select_checks():
    s = _host_state(3)
    assert (s.batch, s.hw, s.data.numel()) == (3, (16, 16), 3 * 19456)
    cells = s.cells()
    assert len(cells) == 7 and [tuple(c.shape) for c, _ in cells] == [(3, 8, 8, 32), (3, 8, 8, 32), (3, 4, 4, 64), (3, 4, 4, 64), (3, 2, 2, 128),
                                                                      (3, 4, 4, 64), (3, 8, 8, 32)]
    assert all(c.shape == h.shape for c, h in cells)
    # views of the one buffer, c before h, cell after cell
    at = 0
    for c, h in cells:
        for t in (c, h):
            assert t.data_ptr() == s.data.data_ptr() + 4 * at and float(t.reshape(-1)[0]) == at
            at += t.numel()
    assert at == s.data.numel()
    k = s.clone()
    assert k.data.data_ptr() != s.data.data_ptr() and torch.equal(k.data, s.data) and (k.batch, k.hw) == (3, (16, 16))
    for bad in ([], [[0]], [3], [-1], [0.0], [True], 'x'):
        with pytest.raises(ValueError):
            s.select(bad)
    with pytest.raises(ValueError, match='there is no CPU path'):      # validated first, then refused: nothing is copied on the host
        s.select([2, 0])
    with pytest.raises(ValueError, match='batch-1'):
        s.expand(4)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            _host_state(1).expand(bad)
    for data, batch in ((torch.zeros(19455), 1), (torch.zeros(19456, dtype=torch.float64), 1), (torch.zeros(1, 19456), 1), (torch.zeros(19456), 2),
                        (torch.zeros(19456), 0), (np.zeros(19456, np.float32), 1)):
        with pytest.raises(ValueError):
            RecurrentState(data, batch, (16, 16))
    assert pivp_amd.RecurrentState.__name__ == 'RecurrentState' and pivp_amd.state.state_layout(16, 16) == LAYOUT[(16, 16)]


def test_model_keywords_and_state_accessors():
    sig = inspect.signature(pivp_amd.Model.__init__).parameters
    assert sig['carry_state'].default is False and list(sig)[-1] == 'carry_state'      # appended: positional callers are undisturbed
    sig = inspect.signature(pivp_amd.Model.imagine).parameters
    assert (sig['observed'].default, sig['advance'].default) == (None, True)
    with pytest.raises(ValueError, match='carry_state must be a bool'):
        pivp_amd.Model(10, carry_state=1)
    off, on = pivp_amd.Model(10), pivp_amd.Model(10, carry_state=True)
    assert off.carry_state is False and on.carry_state is True and on._state is None
    for call in (off.recurrent_state, lambda: off.set_recurrent_state(None)):
        with pytest.raises(RuntimeError, match='carry_state=True'):
            call()
    assert on.recurrent_state() is None
    with pytest.raises(ValueError, match='RecurrentState'):
        on.set_recurrent_state(torch.zeros(4))
    on._state = _host_state(2, (64, 64), fill=0)       # (a host tensor stands in: the checks below never reach a device)
    with pytest.raises(ValueError, match='carries the recurrent state of batch 2 at 64x64'):
        on([np.zeros((4, 3, 3, 64, 64), np.float32), np.zeros((4, 3, 5), np.float32), np.zeros((4, 3, 5), np.float32)])
    with pytest.raises(ValueError, match='carries the recurrent state'):
        on([np.zeros((4, 2, 3, 32, 32), np.float32), np.zeros((4, 2, 5), np.float32), np.zeros((4, 2, 5), np.float32)])
    on.reset_state()
    assert on._state is None and on.recurrent_state() is None
    assert 'truncated BPTT' in inspect.getsource(pivp_amd.Model.backward)
    # the registration is per call: cleared in a `finally`, as the seed hook is
    src = inspect.getsource(pivp_amd.Model._carried)
    assert 'pivp_plan_set_rollout_state(plan.h, None, None, 0)' in src[src.index('finally:'):]
    assert 'observed=1' in pivp_amd.Model.imagine.__doc__ and 'gen_states[-1]' in pivp_amd.Model.imagine.__doc__      # the continuation recipe


def test_imagine_observed_argument_errors_need_no_gpu():
    z = np.zeros
    on, off = pivp_amd.Model(10, carry_state=True), pivp_amd.Model(10)
    good = dict(context_images=z((1, 2, 3, 64, 64)), actions=z((5, 2, 5)), state=z((2, 5)), designated=None, designated_frame=None)
    assert on._check_imagine_args(**good, observed=1) == (1, 6, 2, 64, 64, 0, 0)
    assert on._check_imagine_args(**dict(good, context_images=z((5, 2, 3, 64, 64))), observed=5)[0] == 5            # observed = T-1
    assert on._check_imagine_args(**dict(good, actions=z((1, 2, 5))), observed=1)[:2] == (1, 2)                      # one step from one frame
    assert on._check_imagine_args(**dict(good, context_images=z((2, 2, 3, 64, 64))))[0] == 2                         # None: today's check
    planes = z((2, 3, 64, 64))
    assert on._check_imagine_args(**dict(good, designated=planes), observed=1)[5:] == (3, 0)                         # default frame: observed-1
    assert on._check_imagine_args(**dict(good, context_images=z((3, 2, 3, 64, 64)), designated=planes, designated_frame=2), observed=3)[6] == 2
    bad = [dict(observed=0), dict(observed=-1), dict(observed=1.0), dict(observed=True), dict(observed='1'),
           dict(observed=2),                                                          # context_images holds one frame
           dict(observed=6, context_images=z((6, 2, 3, 64, 64))),                     # observed > T-1
           dict(observed=1, designated=planes, designated_frame=1),                   # designated_frame > observed-1
           dict(observed=1, advance=0), dict(observed=1, advance=None)]
    for over in bad:
        with pytest.raises(ValueError):
            on._check_imagine_args(**dict(good, **over))
    with pytest.raises(ValueError, match='num_frame_before_prediction=2'):            # None keeps the model's own count
        on._check_imagine_args(**good)
    with pytest.raises(ValueError, match='carry_state=True'):
        off._check_imagine_args(**good, observed=1)
    with pytest.raises(ValueError, match='carry_state=True'):
        off._check_imagine_args(**dict(good, context_images=z((2, 2, 3, 64, 64))), advance=False)
    # through the public call, before the GPU or the library is needed
    with pytest.raises(ValueError, match='observed=2'):
        on.imagine(z((1, 2, 3, 64, 64)), z((5, 2, 5)), z((2, 5)), observed=2)
    on._state = _host_state(2, (64, 64), fill=0)
    with pytest.raises(ValueError, match='carries the recurrent state'):
        on.imagine(z((1, 3, 3, 64, 64)), z((5, 3, 5)), z((3, 5)), observed=1)


def _cem_kwargs(model, belief, **over):
    kw = dict(model=model, context_images=np.zeros((1, 1, 3, 64, 64), np.float32), state=np.zeros((1, 5), np.float32), designated_rc=[[32, 32]],
              goal_rc=[[40, 24]], horizon=3, past_actions=None, iterations=2, samples=8, elites=2, init_mean=None, init_std=1.0, min_std=1e-3,
              alpha=0.0, action_low=None, action_high=None, step_weights=None, plane_weights=None, miss_cost=None, chunk=None, seed=0, belief=belief)
    kw.update(over)
    return kw


def test_belief_argument_errors_need_no_gpu():
    on, off = pivp_amd.Model(10, carry_state=True), pivp_amd.Model(10)
    belief = _host_state(1, (64, 64), fill=0)
    a = planning._check_cem_args(**_cem_kwargs(on, belief))
    assert (a.ctx, a.horizon, a.K, a.past.shape) == (1, 3, 8, (0, 5)) and a.belief is belief      # one observed frame whatever the model's context is
    assert planning._check_cem_args(**_cem_kwargs(on, belief, past_actions=np.zeros((0, 5)))).ctx == 1
    none = planning._check_cem_args(**_cem_kwargs(on, None, context_images=np.zeros((2, 1, 3, 64, 64)), past_actions=np.zeros((1, 5))))
    assert none.ctx == 2 and none.belief is None                                                   # without a belief: today's checks
    assert inspect.signature(planning.cem_plan).parameters['belief'].default is None
    assert inspect.signature(planning.score_actions).parameters['belief'].default is None
    bad = [dict(belief=torch.zeros(311296)), dict(belief=_host_state(2, (64, 64), fill=0)), dict(belief=_host_state(1, (16, 16))),
           dict(context_images=np.zeros((2, 1, 3, 64, 64), np.float32)),                          # the newest frame only
           dict(past_actions=np.zeros((1, 5))),                                                   # the belief has consumed the past
           dict(model=off)]
    for over in bad:
        with pytest.raises(ValueError):
            planning._check_cem_args(**dict(_cem_kwargs(on, belief), **over))
    # through the public calls, before the GPU or the library is needed
    with pytest.raises(ValueError, match='past_actions'):
        planning.cem_plan(on, np.zeros((1, 1, 3, 64, 64)), np.zeros((1, 5)), [[32, 32]], [[40, 24]], 3, past_actions=np.zeros((1, 5)), belief=belief)
    with pytest.raises(ValueError, match='carry_state=True'):
        planning.score_actions(off, np.zeros((1, 1, 3, 64, 64)), np.zeros((1, 5)), np.zeros((4, 3, 5)), (32, 32), (40, 24), belief=belief)
    with pytest.raises(ValueError, match='newest frame only'):
        planning.score_actions(on, np.zeros((2, 1, 3, 64, 64)), np.zeros((1, 5)), np.zeros((4, 3, 5)), (32, 32), (40, 24), belief=belief)
    with pytest.raises(ValueError, match='batch-1'):
        planning.score_actions(on, np.zeros((1, 1, 3, 64, 64)), np.zeros((1, 5)), np.zeros((4, 3, 5)), (32, 32), (40, 24),
                               belief=_host_state(2, (64, 64), fill=0))


class _RecordingLib(object):
    """Stands in for the loaded library behind a plan: every call is recorded by name and answered with PIVP_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Tensor(object):
    """What the model needs of a tensor it only takes addresses of."""

    def __init__(self, ptr):
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr


class _Stub(object):
    def __init__(self, ptr):
        self.data, self.batch, self.hw = _Tensor(ptr), 2, (64, 64)


def test_without_carry_state_the_setter_is_never_called(monkeypatch):
    from types import SimpleNamespace
    rec = _RecordingLib()
    plan = SimpleNamespace(lib=rec, h=7)
    off = pivp_amd.Model(10)
    with off._carried(plan, 2, 64, 64) as carried:
        assert carried is False
    with off._carried(plan, 2, 64, 64, advance=False) as carried:
        assert carried is False
    assert rec.calls == [] and off._state is None
    # with the flag: one registration in front of the rollout, one clearing behind it -- also when the rollout raises
    made = []
    monkeypatch.setattr(RecurrentState, 'empty', classmethod(lambda cls, B, hw, device: made.append((B, hw)) or _Stub(4096)))
    on = pivp_amd.Model(10, carry_state=True)
    with on._carried(plan, 2, 64, 64) as carried:
        assert carried is False and rec.calls == [('pivp_plan_set_rollout_state', (7, None, 4096, 0))]      # a first call: zeros in, the new buffer out
        assert on._state is None
    assert made == [(2, (64, 64))] and on._state.data.data_ptr() == 4096
    assert rec.calls[1:] == [('pivp_plan_set_rollout_state', (7, None, None, 0))]
    del rec.calls[:]
    with on._carried(plan, 2, 64, 64) as carried:                                                          # a second call: the buffer in and out
        assert carried is True and rec.calls == [('pivp_plan_set_rollout_state', (7, 4096, 4096, 0))]
    del rec.calls[:]
    with on._carried(plan, 2, 64, 64, advance=False, observed=1) as carried:                              # read, do not advance
        assert carried is True and rec.calls == [('pivp_plan_set_rollout_state', (7, 4096, None, 1))]
    del rec.calls[:]
    with pytest.raises(KeyError):
        with on._carried(plan, 2, 64, 64):
            raise KeyError('the rollout failed')
    assert rec.calls == [('pivp_plan_set_rollout_state', (7, 4096, 4096, 0)), ('pivp_plan_set_rollout_state', (7, None, None, 0))]
    assert len(made) == 1
    # the calls themselves go through _carried
    for fn in (pivp_amd.Model.__call__, pivp_amd.Model._rollout_predict):
        assert 'with self._carried(' in inspect.getsource(fn)


def test_planning_without_a_belief_starts_from_zeros_on_a_carrying_model_too():
    on = pivp_amd.Model(10, carry_state=True, device='cpu')      # (host tensors stand in for the states: nothing here reaches a device)
    on._state = _host_state(1, (64, 64), fill=0)
    with planning._starting_from(on, None):
        assert on.carry_state is False           # no registration is made inside, no shape is held against the carried state
        on._check_carried_shape(16, 64, 64)
    assert on.carry_state is True and on._state is not None
    with pytest.raises(KeyError):
        with planning._starting_from(on, None):
            raise KeyError('a rollout failed')
    assert on.carry_state is True
    # with a belief: the model carries the given state inside and its own one behind
    mine, other = on._state, _host_state(4, (64, 64), fill=1)
    with planning._starting_from(on, other):
        assert on._state is other and on.carry_state is True
    assert on._state is mine
