"""CPU-side checks of pivp_plan_set_precision over a bound workspace: a mode whose ConvLSTM dG rings must be deeper than the workspace was
laid out for is refused with PIVP_ERR_STATE and leaves the plan exactly as it was (no compute calls, no GPU)."""
import ctypes

from pivp_amd import _lib

STATE = -3
F32, BF16, BF16X3, BF16X6, FP16X3 = 0, 1, 2, 3, 4


def _bound_training_plan(lib, seq_len):
    cfg = _lib.PivpConfig(batch=2, seq_len=seq_len, height=64, width=64, num_masks=10, model_type=0, use_state=1,
                          context_frames=2, keep_activations=1, ln_eps=1e-6, stp_zero_border=0)
    h = ctypes.c_void_p()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    n = lib.pivp_plan_workspace_bytes(h)
    assert lib.pivp_plan_set_workspace(h, 256, n) == 0      # never dereferenced here: no rollout runs
    return h, n


def test_modes_that_need_deeper_rings_are_refused_and_roll_back():
    # seq_len = 4 is the smallest length where the ring depth differs between modes: min(T - 2, 8) = 2 slots per ring for BF16 (eight timesteps
    # per weight-gradient launch) and for BF16X6 / FP16X3 (two), against the 1 slot an fp32 layout holds
    lib = _lib.load()
    h, n = _bound_training_plan(lib, seq_len=4)
    try:
        assert lib.pivp_plan_get_precision(h) == F32
        for prec in (BF16, BF16X6, FP16X3):
            assert lib.pivp_plan_set_precision(h, prec) == STATE
            assert lib.pivp_plan_get_precision(h) == F32
            assert lib.pivp_plan_workspace_bytes(h) == n
        # BF16X3 keeps the fp32 weight gradients (one timestep per launch): the bound layout serves it
        assert lib.pivp_plan_set_precision(h, BF16X3) == 0 and lib.pivp_plan_get_precision(h) == BF16X3
        assert lib.pivp_plan_set_precision(h, BF16) == STATE and lib.pivp_plan_get_precision(h) == BF16X3      # ... and a refusal rolls back to IT
        assert lib.pivp_plan_set_precision(h, F32) == 0 and lib.pivp_plan_get_precision(h) == F32
        assert lib.pivp_plan_workspace_bytes(h) == n
    finally:
        lib.pivp_plan_destroy(h)
    # seq_len = 3: one slot per ring whatever the mode, so every mode fits the bound layout
    for prec in (F32, BF16, BF16X3, BF16X6, FP16X3):
        h, n = _bound_training_plan(lib, seq_len=3)
        try:
            assert lib.pivp_plan_set_precision(h, prec) == 0
            assert lib.pivp_plan_get_precision(h) == prec
            assert lib.pivp_plan_workspace_bytes(h) == n
        finally:
            lib.pivp_plan_destroy(h)
