"""CPU-side tests of the gradients through a carried recurrent state: the C-ABI surface of include/pivp_state_grad.h against
`_lib.STATE_GRAD_SIGNATURES` and the built library, the setter's refusals, that a model built without state_backward never calls the setter and one
built with it clears it in a `finally` (a recording stand-in for the library), the argument errors of the new keywords, the call order of
`chunked_backward`, `train.py --tbptt_windows`, and the reference module's packing helpers.  No GPU."""
import contextlib
import ctypes
import inspect
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import RecurrentState, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_grad_reference as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'pivp_plan_set_state_grad', 'pivp_plan_get_state_grad', 'pivp_state_grad_gather', 'pivp_state_grad_scatter'}
STATE_NAMES = {'pivp_state_layout', 'pivp_plan_set_rollout_state', 'pivp_plan_get_rollout_state', 'pivp_state_copy'}


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def _cfg(H=64, W=64, B=2, T=4, keep=1):
    return _lib.PivpConfig(batch=B, seq_len=T, height=H, width=W, num_masks=10, model_type=0, use_state=1, context_frames=2, keep_activations=keep,
                           ln_eps=1e-6, stp_zero_border=0)


def test_state_grad_header_library_and_ctypes_table_agree():
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_state_grad.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.STATE_GRAD_SIGNATURES) == NAMES and declared <= exported
    for header, other in _lib.HEADER_SIGNATURES.items():
        assert header == 'pivp_state_grad.h' or not declared & set(other)
    # the model's ABI, its version and the state header stay what they were
    assert len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)
    assert _declared('pivp_state.h') == set(_lib.STATE_SIGNATURES) == STATE_NAMES
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17
    i, vp, ptr, cells = _lib._i, _lib._vp, ctypes.POINTER, _lib._vp * 7
    assert _lib.STATE_GRAD_SIGNATURES['pivp_plan_set_state_grad'] == (i, [vp, i, vp, vp])
    assert _lib.STATE_GRAD_SIGNATURES['pivp_plan_get_state_grad'] == (i, [vp, ptr(i), ptr(vp), ptr(vp)])
    assert _lib.STATE_GRAD_SIGNATURES['pivp_state_grad_gather'] == (i, [ptr(_lib.PivpConfig), cells, cells, vp, vp])
    assert _lib.STATE_GRAD_SIGNATURES['pivp_state_grad_scatter'] == (i, [ptr(_lib.PivpConfig), vp, cells, vp])
    for name, (res, args) in _lib.STATE_GRAD_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert _lib.SIGNATURES['pivp_rollout_backward'] == (i, [vp] * 8)      # the sweep keeps its signature
    assert 'state_grad.hip' in build.SOURCES and 'pivp_state_grad.h' in [os.path.basename(f) for f in _digest.source_files()]
    header = open(os.path.join(ROOT, 'include', 'pivp_state.h')).read()
    assert 'truncated back-propagation' in header and 'PIVP_ERR_STATE' in header and 'pivp_state_grad.h' in header
    header = open(os.path.join(ROOT, 'include', 'pivp_state_grad.h')).read()
    assert 'UNMODIFIED' in header and 'state_in == state_out' in header      # what the caller owes an enabled sweep is said where the ABI is declared


def test_setter_registration_and_refusals_need_no_gpu():
    lib = _lib.load()
    cfg = _cfg()
    h = _lib._vp()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    nbytes = 4 * 2 * 311296                                   # the state of batch 2 at 64 x 64 (tests/test_state_host.py's table)
    en, so, si = ctypes.c_int(-7), _lib._vp(1), _lib._vp(1)
    read = lambda: (lib.pivp_plan_get_state_grad(h, ctypes.byref(en), ctypes.byref(so), ctypes.byref(si)), en.value, so.value, si.value)
    try:
        assert read() == (0, 0, None, None)                   # the default: nothing registered
        a, b = 1 << 20, (1 << 20) + nbytes
        assert lib.pivp_plan_set_state_grad(h, 1, a, b) == 0 and read() == (0, 1, a, b)      # adjacent buffers do not overlap
        assert lib.pivp_plan_set_state_grad(h, 0, a, None) == 0 and read() == (0, 0, a, None)      # a seed needs no enable
        assert lib.pivp_plan_set_state_grad(h, 1, None, b) == 0
        for bad in ((2, None, None), (-1, None, None), (1, a + 4, None), (1, None, b + 8), (0, None, b),      # range; off 16 bytes; d_state_in without enable
                    (1, a, a), (1, a, a + nbytes - 16), (1, a + nbytes - 16, a)):                              # overlap
            assert lib.pivp_plan_set_state_grad(h, *bad) == -1, bad
        assert read() == (0, 1, None, b)                      # a refused call changes nothing
        assert lib.pivp_plan_get_state_grad(h, None, None, None) == 0
        assert lib.pivp_plan_set_state_grad(h, 0, None, None) == 0 and read() == (0, 0, None, None)
        # the sweep itself is refused without a workspace, whatever is registered (nothing was run)
        assert lib.pivp_plan_set_state_grad(h, 1, None, None) == 0
        assert lib.pivp_rollout_backward(h, 4096, 4096, 4096, None, 4096, 4096, None) == -3
    finally:
        lib.pivp_plan_destroy(h)
    assert lib.pivp_plan_set_state_grad(None, 0, None, None) == -1 and lib.pivp_plan_get_state_grad(None, None, None, None) == -1
    cells = (_lib._vp * 7)(*([4096] * 7))
    for H, W, B in ((8, 64, 1), (64, 60, 1), (64, 64, 0)):      # refused before anything is launched: the pointers are never followed
        c = _cfg(H, W, B)
        assert lib.pivp_state_grad_gather(ctypes.byref(c), cells, cells, 8192, None) == -1
        assert lib.pivp_state_grad_scatter(ctypes.byref(c), 8192, cells, None) == -1
    c = ctypes.byref(_cfg(16, 16, 1))
    assert lib.pivp_state_grad_gather(c, cells, cells, None, None) == -1 and lib.pivp_state_grad_gather(c, cells, cells, 8194, None) == -1
    assert lib.pivp_state_grad_scatter(c, None, cells, None) == -1 and lib.pivp_state_grad_scatter(c, 8194, cells, None) == -1
    holed = (_lib._vp * 7)(*([4096] * 6 + [None]))
    assert lib.pivp_state_grad_gather(c, holed, cells, 8192, None) == -1 and lib.pivp_state_grad_gather(c, cells, holed, 8192, None) == -1
    assert lib.pivp_state_grad_scatter(c, 8192, holed, None) == -1


# ---- the model: a recording stand-in for the library ---------------------------------------------------------------------------------------------
class _RecordingLib(object):
    """Stands in for the loaded library behind a plan: every call is recorded by name and answered with PIVP_OK (or what `answers` says)."""

    def __init__(self, **answers):
        self.calls, self.answers = [], answers

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return self.answers.get(name, 0)
        return call

    def names(self):
        return [n for n, _ in self.calls]


class _Tensor(object):
    """What backward() needs of a tensor it only takes the address and shape of."""

    def __init__(self, ptr, shape=()):
        self._ptr, self.shape, self.device = ptr, shape, 'stub'

    def data_ptr(self):
        return self._ptr


class _State(RecurrentState):
    def __init__(self, ptr, batch=2, hw=(64, 64)):      # (not the parent's: no buffer is sized or checked)
        self.data, self.batch, self.hw = _Tensor(ptr), batch, hw
        self.data.device = torch.device('cpu')


def _after_a_call(m, rec, carried):
    """the model as a training call leaves it, without a GPU"""
    m._active = SimpleNamespace(lib=rec, h=7)
    m._results = object()
    m._inputs = (_Tensor(100, (4, 2, 3, 64, 64)), _Tensor(200, (4, 2, 5)), _Tensor(300, (4, 2, 5)))
    m._gen, m._gen_states = _Tensor(400), _Tensor(500)
    m._carried_start = carried
    m._hw = (64, 64)
    m._ensure_grads = lambda: None
    m._stream = lambda: 9
    return m


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'device', lambda d: contextlib.nullcontext())


def test_without_the_flag_the_setter_is_never_called(no_device):
    for kw, carried in ((dict(), False), (dict(carry_state=True), False)):
        rec = _RecordingLib()
        m = _after_a_call(pivp_amd.Model(10, keep_activations=True, device='cpu', **kw), rec, carried)
        m.backward()
        m.backward(params=False, builtin_loss=True)
        assert 'pivp_rollout_backward' in rec.names() and 'pivp_plan_set_state_grad' not in rec.names()
    # ... and after a carried start such a model refuses as it always did, in front of the library
    rec = _RecordingLib()
    m = _after_a_call(pivp_amd.Model(10, keep_activations=True, carry_state=True, device='cpu'), rec, True)
    with pytest.raises(RuntimeError, match='truncated BPTT'):
        m.backward()
    assert rec.calls == []


def test_with_the_flag_the_setter_brackets_the_sweep_and_is_cleared_in_a_finally(no_device, monkeypatch):
    made = []
    monkeypatch.setattr(RecurrentState, 'empty', classmethod(lambda cls, B, hw, device: made.append((B, hw)) or _State(4096 + 1024 * len(made), B, hw)))
    rec = _RecordingLib()
    m = _after_a_call(pivp_amd.Model(10, keep_activations=True, carry_state=True, state_backward=True, device='cpu'), rec, True)
    m._state = _State(64)
    m.backward()
    assert rec.names() == ['pivp_plan_set_state_grad', 'pivp_rollout_backward', 'pivp_plan_set_state_grad']
    assert rec.calls[0][1] == (7, 1, None, None) and rec.calls[-1][1] == (7, 0, None, None)
    del rec.calls[:]
    seed = _State(8192)
    m.backward(final_state_grad=seed, initial_state_grad=True)
    assert rec.calls[0] == ('pivp_plan_set_state_grad', (7, 1, 8192, 4096 + 1024)) and rec.calls[-1] == ('pivp_plan_set_state_grad', (7, 0, None, None))
    assert m.initial_state_grad.data.data_ptr() == 4096 + 1024 and made == [(2, (64, 64))]
    del rec.calls[:]
    m.backward(initial_state_grad=True)                      # reused by the next call of the same shape
    assert rec.calls[0][1] == (7, 1, None, 4096 + 1024) and len(made) == 1
    del rec.calls[:]
    m.backward(final_state_grad=m.initial_state_grad, initial_state_grad=True)      # seeded with the last result: written to the other buffer
    assert rec.calls[0][1] == (7, 1, 4096 + 1024, 4096 + 2048) and len(made) == 2
    del rec.calls[:]
    m.backward(final_state_grad=m.initial_state_grad, initial_state_grad=True)      # ... and back
    assert rec.calls[0][1] == (7, 1, 4096 + 2048, 4096 + 1024) and len(made) == 2
    # a sweep the library refuses: the registration is cleared all the same
    bad = _RecordingLib(pivp_rollout_backward=-3)
    m._active = SimpleNamespace(lib=bad, h=7)
    with pytest.raises(_lib.PivpError, match='PIVP_ERR_STATE'):
        m.backward(initial_state_grad=True, input_grad=False)
    assert bad.calls[-1] == ('pivp_plan_set_state_grad', (7, 0, None, None))
    src = inspect.getsource(pivp_amd.Model.backward)
    assert 'pivp_plan_set_state_grad(plan.h, 0, None, None)' in src[src.index('finally:'):] and 'truncated BPTT' in src
    # the rollout alternates two buffers: the one it started from is not its destination
    src = inspect.getsource(pivp_amd.Model._carried)
    assert 'pivp_plan_set_rollout_state(plan.h, None, None, 0)' in src[src.index('finally:'):]
    plan = SimpleNamespace(lib=_RecordingLib(), h=7)
    m2 = pivp_amd.Model(10, keep_activations=True, carry_state=True, state_backward=True, device='cpu')
    ptrs = []
    for _ in range(4):
        with m2._carried(plan, 2, 64, 64):
            ptrs.append(plan.lib.calls[-1][1][1:3])
    assert ptrs[0][0] is None and all(a != b for a, b in ptrs)
    assert ptrs[1][0] == ptrs[0][1] and ptrs[2] == (ptrs[1][1], ptrs[1][0]) and ptrs[3] == ptrs[1]      # A -> B, B -> A, A -> B
    m2.reset_state()                                         # a start from zeros writes into the spare buffer: no third one is made
    with m2._carried(plan, 2, 64, 64):
        assert plan.lib.calls[-1][1][1:3] == (None, ptrs[3][0])
    assert m2._state.data.data_ptr() == ptrs[3][0] and m2._spare_state is None


def test_keyword_argument_errors_need_no_gpu(no_device):
    sig = inspect.signature(pivp_amd.Model.__init__).parameters
    assert sig['state_backward'].default is False
    sig = inspect.signature(pivp_amd.Model.backward).parameters
    assert (sig['initial_state_grad'].default, sig['final_state_grad'].default) == (False, None)
    for kw in (dict(state_backward=1), dict(state_backward=True), dict(state_backward=True, carry_state=True),
               dict(state_backward=True, keep_activations=True)):
        with pytest.raises(ValueError, match='state_backward'):
            pivp_amd.Model(10, **kw)
    on = _after_a_call(pivp_amd.Model(10, keep_activations=True, carry_state=True, state_backward=True, device='cpu'), _RecordingLib(), True)
    on._state = _State(64)
    off = _after_a_call(pivp_amd.Model(10, keep_activations=True, carry_state=True, device='cpu'), _RecordingLib(), False)
    for call in (lambda: off.backward(initial_state_grad=True), lambda: off.backward(final_state_grad=_State(8192))):
        with pytest.raises(ValueError, match='state_backward=True'):
            call()
    for bad in (1, None, 'yes'):
        with pytest.raises(ValueError, match='initial_state_grad must be a bool'):
            on.backward(initial_state_grad=bad)
    for bad in (torch.zeros(4), 3, 'x'):
        with pytest.raises(ValueError, match='final_state_grad must be a RecurrentState'):
            on.backward(final_state_grad=bad)
    with pytest.raises(ValueError, match='of batch 3'):
        on.backward(final_state_grad=_State(8192, batch=3))
    with pytest.raises(ValueError, match='sized for 64x64'):
        on.backward(final_state_grad=_State(8192, hw=(32, 32)))
    # the buffers are sized and checked by the call that is swept, whatever was done to the carried state since
    made = []
    on._state = None                                         # (set_recurrent_state(None) between the call and backward())
    RS = RecurrentState
    keep = RS.__dict__['empty']
    RS.empty = classmethod(lambda cls, B, hw, device: made.append((B, hw)) or _State(4096, B, hw))
    try:
        on.backward(initial_state_grad=True)
        on._state = _State(64, batch=5)                      # (a state of another batch adopted since)
        on.backward(initial_state_grad=True, final_state_grad=_State(8192))
        with pytest.raises(ValueError, match='the last call ran batch 2'):
            on.backward(final_state_grad=_State(8192, batch=5))
    finally:
        RS.empty = keep
    assert made == [(2, (64, 64))] and (on.initial_state_grad.batch, on.initial_state_grad.hw) == (2, (64, 64))
    del on._active.lib.calls[:]
    on._state = _State(64)
    on._carried_start = False
    with pytest.raises(ValueError, match='started from zeros'):
        on.backward(initial_state_grad=True)
    with pytest.raises(ValueError, match='nothing to differentiate'):
        on.backward(builtin_loss=False)
    assert on._active.lib.calls == [] and off._active.lib.calls == []      # every complaint came before the library
    on.backward(builtin_loss=False, final_state_grad=_State(8192))         # the seed alone is something to differentiate
    assert 'pivp_rollout_backward' in on._active.lib.names()


# ---- chunked_backward ----------------------------------------------------------------------------------------------------------------------------
class _FakeModel(object):
    state_backward, sampling_rng = True, None

    def __init__(self):
        self.log, self._s, self.initial_state_grad, self._n = [], None, None, 0

    def recurrent_state(self):
        self.log.append(('snapshot', self._s))
        return None if self._s is None else _State(self._s)

    def set_recurrent_state(self, s):
        self._s = None if s is None else s.data.data_ptr()
        self.log.append(('set', self._s))

    def _adopt_state(self, s):
        self._s = s.data.data_ptr()
        self.log.append(('adopt', self._s))

    def __call__(self, w, iter_num):
        self.log.append(('call', w[0], self._s, iter_num, np.random.get_state()[1][:2].tolist()))
        np.random.random_sample()                              # (a call draws from the host RNG, as scheduled sampling does)
        self._s = (self._s or 0) + 10
        return float(w[0])

    def backward(self, **kw):
        seed = kw['final_state_grad']
        self.log.append(('backward', None if seed is None else seed.data.data_ptr(), kw['initial_state_grad']))
        if kw['initial_state_grad']:
            self._n += 1
            self.initial_state_grad = _State(1000 + self._n)


def test_chunked_backward_call_order():
    from pivp_amd import tbptt
    m = _FakeModel()
    np.random.seed(4)
    total = tbptt.chunked_backward(m, [[1, 'a', 's'], [2, 'a', 's'], [3, 'a', 's']], iter_num=5)
    assert total == 6.0
    kinds = [e[0] for e in m.log]
    assert kinds == ['snapshot', 'call', 'snapshot', 'call', 'snapshot', 'call', 'snapshot',      # forward: a snapshot in front of each window, one behind
                     'backward',                                                                 # window 3 still holds its activations
                     'set', 'call', 'backward', 'set', 'call', 'backward', 'adopt']
    calls = [e for e in m.log if e[0] == 'call']
    assert [c[1] for c in calls] == [1, 2, 3, 2, 1] and all(c[3] == 5 for c in calls)
    assert [c[2] for c in calls] == [None, 10, 20, 10, None]                      # each repeat starts from its window's snapshot
    assert calls[3][4] == calls[1][4] and calls[4][4] == calls[0][4]              # ... and draws what the first pass drew
    backs = [e for e in m.log if e[0] == 'backward']
    assert backs == [('backward', None, True), ('backward', 1001, True), ('backward', 1002, False)]      # each seeded with the next window's result
    assert m.log[-1] == ('adopt', 30)                                             # the state the last window left
    # one window: a plain call and backward()
    m = _FakeModel()
    assert tbptt.chunked_backward(m, [[1, 'a', 's']]) == 1.0
    assert [e[0] for e in m.log] == ['snapshot', 'call', 'snapshot', 'backward', 'adopt'] and m.log[3] == ('backward', None, False)
    for bad_model, bad_windows in ((pivp_amd.Model(10), [[1, 2, 3]]), (_FakeModel(), []), (_FakeModel(), [[1, 2]]), (_FakeModel(), 'x')):
        with pytest.raises(ValueError):
            tbptt.chunked_backward(bad_model, bad_windows)
    assert pivp_amd.chunked_backward is tbptt.chunked_backward
    # the host RNG whose state is put back: NumPy's global stream, a RandomState or a Generator; anything else is refused before a window runs
    for rng in (np.random, np.random.RandomState(3), np.random.default_rng(3)):
        st = tbptt._rng_state(rng)
        first = rng.random_sample() if hasattr(rng, 'random_sample') else rng.random()
        tbptt._rng_restore(rng, st)
        assert (rng.random_sample() if hasattr(rng, 'random_sample') else rng.random()) == first
    m = _FakeModel()
    m.sampling_rng = np.random.default_rng(5)
    assert tbptt.chunked_backward(m, [[1, 'a', 's'], [2, 'a', 's']]) == 3.0
    m = _FakeModel()
    m.sampling_rng = SimpleNamespace(shuffle=lambda idx: None)
    with pytest.raises(ValueError, match='sampling_rng'):
        tbptt.chunked_backward(m, [[1, 'a', 's']])
    assert m.log == []
    src = inspect.getsource(tbptt.chunked_backward)
    assert 'synchronize' not in src.split('"""')[2] and '.item()' not in src and 'float(' not in src      # nothing in the loop reads the device


def test_train_py_tbptt_windows():
    from pivp_amd import train, tbptt
    args = train.build_parser().parse_args([])
    assert args.tbptt_windows == 1 and train.model_state_flags(args) == {}          # the model is built exactly as before
    args = train.build_parser().parse_args(['--tbptt_windows', '2'])
    assert train.model_state_flags(args) == dict(carry_state=True, state_backward=True)
    with pytest.raises(SystemExit):
        train.model_state_flags(train.build_parser().parse_args(['--tbptt_windows', '0']))

    class Opt(object):
        def __init__(self):
            self.seen = []

        def update(self, model, x, itr):
            self.seen.append((x, itr))
            model.loss, model.psnr_all = len(self.seen), -len(self.seen)

    x = [np.arange(10)[:, None], np.arange(10)[:, None] * 2, np.arange(10)[:, None] * 3]
    opt, model = Opt(), SimpleNamespace()
    assert train.train_step(opt, model, x, 3) == [(1, -1)] and opt.seen[0][0] is x and opt.seen[0][1] == 3      # 1: the old path, the batch itself
    opt = Opt()
    assert train.train_step(opt, model, x, 4, windows=2) == [(1, -1), (2, -2)]
    assert [w[0][:, 0].tolist() for w, _ in opt.seen] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]] and opt.seen[1][0][2][0, 0] == 15
    for n in (0, 3, 10, True, 2.0):
        with pytest.raises(ValueError):
            tbptt.split_windows(x, n)
    assert 'optimizer.update(model, x, itr)' in inspect.getsource(train.train_step)


# ---- the reference module's helpers -----------------------------------------------------------------------------------------------------------
def test_reference_packing_matches_the_state_layout():
    B, H, W = 2, 16, 16
    n = SR.state_numel(B, H, W)
    assert n == 2 * 19456                                                      # tests/test_state_host.py's table
    flat = np.arange(n, dtype=np.float64)
    pairs = SR.unpack_state(flat, B, H, W, torch.float64)
    assert [tuple(c.shape) for c, _ in pairs] == [(2, 32, 8, 8), (2, 32, 8, 8), (2, 64, 4, 4), (2, 64, 4, 4), (2, 128, 2, 2), (2, 64, 4, 4), (2, 32, 8, 8)]
    assert np.array_equal(SR.pack_state(pairs), flat)
    segs = SR.segments(flat, B, H, W)
    assert len(segs) == 14 and segs[1][0] == 2 * 2048 and sum(len(s) for s in segs) == n
    s = RecurrentState(torch.arange(n, dtype=torch.float32), B, (H, W))
    c0, h0 = s.cells()[0]
    assert torch.equal(pairs[0][1].permute(0, 2, 3, 1).float(), h0)           # NCHW in the restatement, [B][H][W][C] in the buffer
    assert set(SR.SEEDS_OUTSIDE) <= set(SR.CASES) and all(SR.CASES[k][5] not in v for k, v in SR.SEEDS_OUTSIDE.items())
