"""CPU-side checks of the deterministic-training switch: the C ABI entry points, the workspace they size and the Python / CLI surface
(no compute calls, no GPU)."""
import ctypes

import pytest

import pivp_amd
from pivp_amd import _lib

BADARG, STATE = -1, -3


def _plan(lib, model_type=0, num_masks=10, B=2, H=64, train=1):
    cfg = _lib.PivpConfig(batch=B, seq_len=5, height=H, width=H, num_masks=num_masks, model_type=model_type, use_state=1,
                          context_frames=2, keep_activations=train, ln_eps=1e-6, stp_zero_border=0)
    h = ctypes.c_void_p()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def test_setter_getter_and_refusals():
    lib = _lib.load()
    assert lib.pivp_plan_set_deterministic(None, 1) == BADARG
    assert lib.pivp_plan_get_deterministic(None) == BADARG
    h = _plan(lib)
    try:
        assert lib.pivp_plan_get_deterministic(h) == 0
        off = lib.pivp_plan_workspace_bytes(h)
        assert lib.pivp_plan_set_deterministic(h, 1) == 0 and lib.pivp_plan_get_deterministic(h) == 1
        on = lib.pivp_plan_workspace_bytes(h)
        assert on >= off
        # precision modes whose weight gradients have no fixed-order form are refused while the switch is on, and nothing changes
        for prec in (3, 4):      # PIVP_PRECISION_BF16X6, _FP16X3
            assert lib.pivp_plan_set_precision(h, prec) == BADARG
            assert lib.pivp_plan_get_precision(h) == 0
        for prec in (1, 2, 0):   # BF16, BF16X3, F32
            assert lib.pivp_plan_set_precision(h, prec) == 0
        assert lib.pivp_plan_set_deterministic(h, 0) == 0 and lib.pivp_plan_workspace_bytes(h) == off
    finally:
        lib.pivp_plan_destroy(h)
    h = _plan(lib)
    try:      # ... and in the other order: the switch refuses an unsupported precision, the plan stays as it was
        assert lib.pivp_plan_set_precision(h, 3) == 0
        assert lib.pivp_plan_set_deterministic(h, 1) == BADARG and lib.pivp_plan_get_deterministic(h) == 0
    finally:
        lib.pivp_plan_destroy(h)
    for mt, nm in ((1, 10), (2, 1)):      # STP and DNA are served too, and their workspace grows as CDNA's does
        h = _plan(lib, model_type=mt, num_masks=nm)
        try:
            off = lib.pivp_plan_workspace_bytes(h)
            assert lib.pivp_plan_set_deterministic(h, 1) == 0 and lib.pivp_plan_workspace_bytes(h) > off
        finally:
            lib.pivp_plan_destroy(h)
    h = _plan(lib, H=48)     # ConvLSTM maps 24 / 12 / 6 wide: not served by the fixed-order weight gradient
    try:
        assert lib.pivp_plan_set_deterministic(h, 1) == BADARG and lib.pivp_plan_get_deterministic(h) == 0
    finally:
        lib.pivp_plan_destroy(h)


def test_switching_on_over_a_bound_workspace_that_lacks_the_slots_is_a_state_error():
    lib = _lib.load()
    h = _plan(lib)
    try:
        n = lib.pivp_plan_workspace_bytes(h)
        assert lib.pivp_plan_set_workspace(h, 256, n) == 0      # never dereferenced here: no rollout runs
        assert lib.pivp_plan_set_deterministic(h, 1) == STATE and lib.pivp_plan_get_deterministic(h) == 0
    finally:
        lib.pivp_plan_destroy(h)


def test_model_validates_the_keyword():
    with pytest.raises(ValueError, match='bool'):
        pivp_amd.Model(10, deterministic='yes')
    with pytest.raises(ValueError, match='bool'):
        pivp_amd.Model(10, deterministic=1)
    with pytest.raises(ValueError, match='bf16x6'):
        pivp_amd.Model(10, precision='bf16x6', deterministic=True)
    assert pivp_amd.Model(10, is_cdna=False, is_stp=True, deterministic=True).deterministic is True
    assert pivp_amd.Model(10).deterministic is False
    assert pivp_amd.Model(10, precision='bf16', deterministic=True).deterministic is True


def test_train_parser_accepts_the_flag():
    from pivp_amd import train
    assert train.build_parser().parse_args([]).deterministic == 0
    assert train.build_parser().parse_args(['--deterministic', '1']).deterministic == 1
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(['--deterministic', '2'])
