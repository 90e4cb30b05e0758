"""Plan options through the C ABI (include/pivp_hip.h: pivp_plan_set_option / pivp_plan_get_option) and the one place that still honours the
PIVP_* variables, the Python package's `resolve_plan_options`.  Host only: plans are created and laid out, nothing is launched."""
import ctypes

import pytest

from pivp_amd import _lib
from pivp_amd import model as M

OK, BADARG, STATE = 0, -1, -3
SIDE_STREAM, FINISH_RIDER, FUSE_ENC3, LN_FOLD_TRAIN, WGRAD_BATCH, OPT_COUNT = range(6)     # PIVP_OPT_*
SWITCHES = (SIDE_STREAM, FINISH_RIDER, FUSE_ENC3, LN_FOLD_TRAIN)
DEFAULTS = [1, 1, 1, 1, 0]
VARIABLES = ('PIVP_SIDE_STREAM', 'PIVP_FINISH_RIDER', 'PIVP_FUSE_ENC3', 'PIVP_LN_FOLD_TRAIN', 'PIVP_WGRAD_BATCH')


@pytest.fixture
def lib():
    return _lib.load()


@pytest.fixture
def make_plan(lib):
    """make_plan(keep_activations=1) -> a 64 x 64, B = 2, T = 10 plan's handle; every plan is destroyed behind the test"""
    made = []

    def make(keep_activations=1):
        cfg = _lib.PivpConfig(batch=2, seq_len=10, height=64, width=64, num_masks=10, model_type=0, use_state=1,
                              context_frames=2, keep_activations=keep_activations, ln_eps=1e-6, stp_zero_border=0)
        h = ctypes.c_void_p()
        assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == OK
        made.append(h)
        return h
    yield make
    for h in made:
        lib.pivp_plan_destroy(h)


def _options(lib, h):
    return [lib.pivp_plan_get_option(h, o) for o in range(OPT_COUNT)]


def _bytes_with(lib, h, batch):
    assert lib.pivp_plan_set_option(h, WGRAD_BATCH, batch) == OK
    return lib.pivp_plan_workspace_bytes(h)


def test_defaults_round_trips_and_refusals(lib, make_plan):
    h = make_plan()
    assert _options(lib, h) == DEFAULTS
    for o in SWITCHES:
        for v in (0, 1):
            assert lib.pivp_plan_set_option(h, o, v) == OK and lib.pivp_plan_get_option(h, o) == v
    for v in list(range(9)) + [0]:
        assert lib.pivp_plan_set_option(h, WGRAD_BATCH, v) == OK and lib.pivp_plan_get_option(h, WGRAD_BATCH) == v
    assert _options(lib, h) == DEFAULTS
    # a refused call leaves what was there: set every option away from its default first
    want = [0, 0, 0, 0, 3]
    for o, v in enumerate(want):
        assert lib.pivp_plan_set_option(h, o, v) == OK
    nbytes = lib.pivp_plan_workspace_bytes(h)
    for o in (-1, OPT_COUNT):
        assert lib.pivp_plan_set_option(h, o, 1) == BADARG and lib.pivp_plan_get_option(h, o) == BADARG
    for o in SWITCHES:
        for v in (2, -1):
            assert lib.pivp_plan_set_option(h, o, v) == BADARG
    for v in (-1, 9):
        assert lib.pivp_plan_set_option(h, WGRAD_BATCH, v) == BADARG
    assert lib.pivp_plan_set_option(None, SIDE_STREAM, 0) == BADARG and lib.pivp_plan_get_option(None, SIDE_STREAM) == BADARG
    assert _options(lib, h) == want and lib.pivp_plan_workspace_bytes(h) == nbytes


def test_fp32_workspace_follows_the_weight_gradient_batch(lib, make_plan):
    h = make_plan()
    b0 = lib.pivp_plan_workspace_bytes(h)
    b1, b4, b8 = (_bytes_with(lib, h, v) for v in (1, 4, 8))
    assert b0 == b1 < b4 < b8           # fp32's own choice is one timestep per launch: one slot per dG ring
    assert _bytes_with(lib, h, 0) == b0


def test_bf16_workspace_is_independent_of_the_order_of_the_setters(lib, make_plan):
    sizes = {}
    for batch in (0, 1, 8):
        first, second = make_plan(), make_plan()
        assert lib.pivp_plan_set_precision(first, 1) == OK
        sizes[batch] = _bytes_with(lib, first, batch)
        assert lib.pivp_plan_set_option(second, WGRAD_BATCH, batch) == OK and lib.pivp_plan_set_precision(second, 1) == OK
        assert lib.pivp_plan_workspace_bytes(second) == sizes[batch], batch
        assert lib.pivp_plan_get_option(second, WGRAD_BATCH) == batch and lib.pivp_plan_get_precision(second) == 1
    assert sizes[0] == sizes[8] > sizes[1]      # the bf16 mode's own choice: as many timesteps as the rings hold (T - 2 = 8)


def test_inference_plan_accepts_the_batch_and_keeps_its_size(lib, make_plan):
    h = make_plan(keep_activations=0)
    b0 = lib.pivp_plan_workspace_bytes(h)
    for v in (1, 4, 8, 0):
        assert _bytes_with(lib, h, v) == b0 and lib.pivp_plan_get_option(h, WGRAD_BATCH) == v


def test_options_are_fixed_once_a_workspace_is_bound(lib, make_plan):
    h = make_plan()
    want = [0, 1, 0, 1, 4]
    for o, v in enumerate(want):
        assert lib.pivp_plan_set_option(h, o, v) == OK
    nbytes = lib.pivp_plan_workspace_bytes(h)
    assert lib.pivp_plan_set_workspace(h, 1 << 20, nbytes) == OK      # any aligned non-null address: nothing is launched
    for o in range(OPT_COUNT):
        for v in (0, 1):
            assert lib.pivp_plan_set_option(h, o, v) == STATE
    assert _options(lib, h) == want and lib.pivp_plan_workspace_bytes(h) == nbytes


def test_the_library_ignores_the_environment(lib, make_plan, monkeypatch):
    for var in VARIABLES:
        monkeypatch.delenv(var, raising=False)
    unset = lib.pivp_plan_workspace_bytes(make_plan())
    monkeypatch.setenv('PIVP_WGRAD_BATCH', '4')
    monkeypatch.setenv('PIVP_SIDE_STREAM', '0')
    h = make_plan()
    assert _options(lib, h) == DEFAULTS
    assert lib.pivp_plan_workspace_bytes(h) == unset


def test_the_package_reads_the_environment_and_the_keyword_overrides_it(monkeypatch):
    keys = ('side_stream', 'finish_rider', 'fuse_enc3', 'ln_fold_train', 'wgrad_batch')
    assert tuple(M.PLAN_OPTIONS) == keys
    assert [M.PLAN_OPTIONS[k][:2] for k in keys] == list(enumerate(DEFAULTS)) and tuple(M.PLAN_OPTIONS[k][2] for k in keys) == VARIABLES
    for var in VARIABLES:
        monkeypatch.delenv(var, raising=False)
    assert list(M.resolve_plan_options().values()) == DEFAULTS and tuple(M.resolve_plan_options()) == keys
    for key, var in zip(keys[:4], VARIABLES[:4]):
        for text, value in (('0', 0), ('1', 1), ('00', 0), ('on', 1), ('', 1)):      # off = starts with '0', as the library parsed it
            monkeypatch.setenv(var, text)
            got = M.resolve_plan_options()
            assert got.pop(key) == value and list(got.values()) == [d for k, d in zip(keys, DEFAULTS) if k != key]
        monkeypatch.setenv(var, '0')
        assert M.resolve_plan_options({key: 1})[key] == 1      # the keyword wins
        monkeypatch.delenv(var)
    # the batch: its integer; 0, unset or no number = the mode's own choice; outside 1 .. 8 clamped as the plan clamped it, never an error
    for text, value in (('0', 0), ('1', 1), ('3', 3), ('8', 8), ('9', 8), ('100', 8), ('-1', 1), ('', 0), ('x', 0)):
        monkeypatch.setenv('PIVP_WGRAD_BATCH', text)
        assert M.resolve_plan_options()['wgrad_batch'] == value, text
    assert M.resolve_plan_options({'wgrad_batch': 0})['wgrad_batch'] == 0
    assert M.resolve_plan_options({'wgrad_batch': 5, 'side_stream': 0}) == dict(zip(keys, [0, 1, 1, 1, 5]))
    # read when asked, not once per process
    monkeypatch.setenv('PIVP_WGRAD_BATCH', '2')
    assert M.resolve_plan_options()['wgrad_batch'] == 2
    monkeypatch.delenv('PIVP_WGRAD_BATCH')
    assert M.resolve_plan_options()['wgrad_batch'] == 0
    assert M.resolve_plan_options(environ={'PIVP_FUSE_ENC3': '0'})['fuse_enc3'] == 0
    # unknown keys: from the helper and from the constructor, before anything touches a device
    with pytest.raises(ValueError, match='no_such_option'):
        M.resolve_plan_options({'no_such_option': 1})
    with pytest.raises(ValueError, match='wgrad_batches'):
        M.Model(10, plan_options={'wgrad_batches': 2})
    assert M.Model(10, plan_options={'wgrad_batch': 2}).plan_options == {'wgrad_batch': 2} and M.Model(10).plan_options == {}
