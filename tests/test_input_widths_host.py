"""Action and robot-state vectors of any width 1 .. 16 (pivp_config_t::action_dim / state_dim, Model(action_dim=, state_dim=)): the struct, the plan's
parameter table and workspace, the Python door and the refusals of what stays five wide (the on-device CEM, the device-resident data set).
Host only: plans are created and laid out, nothing is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib, dataset, planning
from pivp_amd import evaluate as evaluate_cli
from pivp_amd import predict as predict_cli
from pivp_amd import train as train_cli
from pivp_amd.model import reference_param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG = 0, -1
# pivp_plan_workspace_bytes of the 64 x 64, B = 2, T = 10, ten-mask CDNA plan of tests/test_plan_options_host.py in front of this change, by keep_activations
WORKSPACE_BEFORE = {1: 364120320, 0: 58487296}


@pytest.fixture
def lib():
    return _lib.load()


@pytest.fixture
def make_plan(lib):
    """make_plan(keep_activations, **widths) -> (return code, handle) of the plan tests/test_plan_options_host.py makes, with the widths as given"""
    made = []

    def make(keep_activations=1, **widths):
        cfg = _lib.PivpConfig(batch=2, seq_len=10, height=64, width=64, num_masks=10, model_type=0, use_state=1,
                              context_frames=2, keep_activations=keep_activations, ln_eps=1e-6, stp_zero_border=0, **widths)
        h = ctypes.c_void_p()
        rc = lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == OK:
            made.append(h)
        return rc, h
    yield make
    for h in made:
        lib.pivp_plan_destroy(h)


def _params(lib, h):
    return {lib.pivp_param_name(h, i).decode(): lib.pivp_param_numel(h, i) for i in range(lib.pivp_param_count(h))}


def test_the_struct_ends_in_the_two_widths_in_the_header_s_order():
    text = open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()
    body = re.search(r'typedef struct pivp_config \{(.*?)\} pivp_config_t;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r'\b(int|float)\s+([a-z_0-9, ]+);', body):
        fields += [(n.strip(), ctypes.c_int if ctype == 'int' else ctypes.c_float) for n in names.split(',')]
    assert _lib.PivpConfig._fields_ == fields
    assert _lib.PivpConfig._fields_[-2:] == [('action_dim', ctypes.c_int), ('state_dim', ctypes.c_int)]
    assert ctypes.sizeof(_lib.PivpConfig) == 4 * len(fields) == 52
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', text)) - {'pivp_config', 'pivp_plan'}
    assert len(declared) == 118 and declared == set(_lib.SIGNATURES)      # no new symbol: the widths travel in the struct
    assert _lib.load().pivp_abi_version() == 17


@pytest.mark.parametrize('keep', [1, 0])
def test_the_reference_s_widths_lay_out_the_plan_that_was(lib, make_plan, keep):
    rc, unnamed = make_plan(keep)
    assert rc == OK
    before = _params(lib, unnamed)
    assert before['enc3/W'] == 74 * 64 and before['current_state/W'] == 50 and before['current_state/b'] == 5
    for widths in (dict(action_dim=0, state_dim=0), dict(action_dim=5, state_dim=5), dict(action_dim=5), dict(state_dim=5)):
        rc, h = make_plan(keep, **widths)
        assert rc == OK
        assert lib.pivp_plan_workspace_bytes(h) == lib.pivp_plan_workspace_bytes(unnamed) == WORKSPACE_BEFORE[keep], widths
        assert _params(lib, h) == before and list(_params(lib, h)) == list(before)


@pytest.mark.parametrize('A,S', [(4, 3), (7, 5), (1, 1), (16, 16)])
def test_other_widths_move_three_parameters_and_nothing_else(lib, make_plan, A, S):
    ref = _params(lib, make_plan(1)[1])
    rc, h = make_plan(1, action_dim=A, state_dim=S)
    assert rc == OK
    got = _params(lib, h)
    assert list(got) == list(ref)
    assert got['enc3/W'] == (64 + A + S) * 64 and got['current_state/W'] == S * (A + S) and got['current_state/b'] == S
    assert {k for k in ref if got[k] != ref[k]} == {'enc3/W', 'current_state/W', 'current_state/b'} - ({'current_state/b'} if S == 5 else set())
    assert sum(got.values()) - sum(ref.values()) == ((A + S) - 10) * 64 + S * (A + S) + S - 55
    # the training workspace holds d state [T][B][S]: it follows S, within the carve's alignment
    assert abs(lib.pivp_plan_workspace_bytes(h) - WORKSPACE_BEFORE[1]) <= 10 * 2 * 16 * 4 + 4096


def test_without_the_smear_enc3_keeps_its_64_inputs(lib):
    cfg = _lib.PivpConfig(batch=2, seq_len=4, height=16, width=16, num_masks=3, model_type=0, use_state=0, context_frames=2, keep_activations=1,
                          ln_eps=1e-6, stp_zero_border=0, action_dim=4, state_dim=3)
    h = ctypes.c_void_p()
    assert lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(h)) == OK
    try:
        got = _params(lib, h)
        assert got['enc3/W'] == 64 * 64 and got['current_state/W'] == 3 * 7 and got['current_state/b'] == 3
    finally:
        lib.pivp_plan_destroy(h)


@pytest.mark.parametrize('widths', [dict(action_dim=-1), dict(state_dim=-1), dict(action_dim=17), dict(state_dim=17), dict(action_dim=16, state_dim=17),
                                    dict(action_dim=17, state_dim=16), dict(action_dim=1 << 20, state_dim=1 << 20)])
def test_widths_outside_the_domain_are_refused_at_the_door(make_plan, widths):
    for keep in (1, 0):
        rc, h = make_plan(keep, **widths)
        assert rc == BADARG and not h.value


@pytest.mark.parametrize('bad', [0, 17, -1, 2.5, '4', None, True])
def test_the_model_takes_whole_widths_from_1_to_16(bad):
    with pytest.raises(ValueError, match='action_dim'):
        pivp_amd.Model(10, action_dim=bad)
    with pytest.raises(ValueError, match='state_dim'):
        pivp_amd.Model(10, state_dim=bad)


def test_the_model_s_widths_and_shapes():
    m = pivp_amd.Model(10)
    assert (m.action_dim, m.state_dim) == (5, 5)
    m = pivp_amd.Model(10, action_dim=np.int64(16), state_dim=1)
    assert (m.action_dim, m.state_dim) == (16, 1) and type(m.action_dim) is int
    default = reference_param_shapes(10, 'CDNA', True, 64, 64)
    assert default == reference_param_shapes(10, 'CDNA', True, 64, 64, action_dim=5, state_dim=5)
    assert default['enc3/W'] == (64, 74, 1, 1) and default['current_state/W'] == (5, 10) and default['current_state/b'] == (5,)
    got = reference_param_shapes(10, 'CDNA', True, 64, 64, action_dim=4, state_dim=3)
    assert got['enc3/W'] == (64, 64 + 4 + 3, 1, 1) and got['current_state/W'] == (3, 4 + 3) and got['current_state/b'] == (3,)
    assert {k for k in default if got[k] != default[k]} == {'enc3/W', 'current_state/W', 'current_state/b'} and list(got) == list(default)
    assert reference_param_shapes(10, 'CDNA', False, 64, 64, action_dim=4, state_dim=3)['enc3/W'] == (64, 64, 1, 1)
    m = pivp_amd.Model(10, action_dim=4, state_dim=3)
    m._hw = (64, 64)
    assert m._shapes() == got


def _args(A, S, ctx=2, B=2, steps=5, H=64, W=64):
    return np.zeros((ctx, B, 3, H, W), np.float32), np.zeros((steps, B, A), np.float32), np.zeros((B, S), np.float32)


def test_a_4_3_model_takes_its_own_widths_and_refuses_the_reference_s():
    m = pivp_amd.Model(10, action_dim=4, state_dim=3)
    ci, ac5, st5 = _args(5, 5)
    _, ac, st = _args(4, 3)
    with pytest.raises(ValueError, match=r'actions must be \(T-1, 2, 4\).*action_dim=4'):
        m.imagine(ci, ac5, st)
    with pytest.raises(ValueError, match=r'state must be \(2, 3\).*state_dim=3'):
        m.imagine(ci, ac, st5)
    with pytest.raises(ValueError):
        m.imagine(ci, ac5, st5)
    with pytest.raises(ValueError, match='candidates'):
        planning.score_actions(m, ci[:, :1], st[:1], np.zeros((4, 5, 5), np.float32), (3, 3), (4, 4))
    with pytest.raises(ValueError, match=r'state must be \(1, 3\)'):
        planning.score_actions(m, ci[:, :1], st5[:1], np.zeros((4, 5, 4), np.float32), (3, 3), (4, 4))
    train = pivp_amd.Model(10, action_dim=4, state_dim=3, keep_activations=True)
    with pytest.raises(ValueError, match=r'actions must be \(T-1, 2, 4\)'):
        planning.refine_actions(train, ci, st, ac5, goal_image=np.zeros((3, 64, 64), np.float32))
    with pytest.raises(ValueError, match=r'bounds\[0\] must be a scalar or \(4,\)'):
        planning.refine_actions(train, ci, st, ac, goal_image=np.zeros((3, 64, 64), np.float32), bounds=(np.zeros(5), None))
    if not torch.cuda.is_available():      # good arguments get as far as the GPU requirement: there is no CPU fallback
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.imagine(ci, ac, st)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            planning.score_actions(m, ci[:, :1], st[:1], np.zeros((4, 5, 4), np.float32), (3, 3), (4, 4))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            planning.refine_actions(train, ci, st, ac, goal_image=np.zeros((3, 64, 64), np.float32), bounds=(np.zeros(4), None))


def test_the_default_model_refuses_what_it_always_refused():
    m = pivp_amd.Model(10)
    ci, ac, st = _args(5, 5)
    _, ac4, st3 = _args(4, 3)
    for kw in (dict(actions=ac4), dict(state=st3), dict(actions=ac[:, :, :4]), dict(state=np.zeros((5, 2, 5), np.float32))):
        with pytest.raises(ValueError):
            m.imagine(**dict(dict(context_images=ci, actions=ac, state=st), **kw))
    with pytest.raises(ValueError, match=r'candidates must be \(K, T-1, 5\)'):
        planning.score_actions(m, ci[:, :1], st[:1], np.zeros((4, 5, 4), np.float32), (3, 3), (4, 4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.imagine(ci, ac, st)


def test_the_on_device_cem_serves_five_column_actions_alone():
    frame, robot = np.zeros((1, 1, 3, 64, 64), np.float32), np.zeros((1, 5), np.float32)
    m = pivp_amd.Model(10, action_dim=4, state_dim=5, num_frame_before_prediction=1)
    with pytest.raises(ValueError, match='action_dim=4'):
        planning.cem_plan(m, frame, robot, [[32, 32]], [[40, 24]], 3)
    train = pivp_amd.Model(10, action_dim=4, state_dim=5, num_frame_before_prediction=1, keep_activations=True)
    with pytest.raises(ValueError, match='action_dim=4'):
        planning.cem_refine(train, frame, robot, 3, np.zeros((3, 64, 64), np.float32))
    carried = pivp_amd.Model(10, action_dim=4, state_dim=5, carry_state=True)
    ctl = planning.MPC(carried, 3, goal_rc=[[40, 24]])
    with pytest.raises(ValueError, match='action_dim=4'):
        ctl.reset(frame, robot, designated_rc=[[32, 32]])


def test_the_device_data_set_holds_five_column_rows_alone():
    images = np.zeros((3, 4, 16, 16, 3), np.float32)
    with pytest.raises(ValueError, match='action_dim=4'):
        dataset.DeviceDataset(images, np.zeros((3, 4, 4), np.float32), np.zeros((3, 4, 5), np.float32))
    with pytest.raises(ValueError, match='state_dim=3'):
        dataset.DeviceDataset(images, np.zeros((3, 4, 5), np.float32), np.zeros((3, 4, 3), np.float32))
    with pytest.raises(ValueError, match='action_dim=4'):
        dataset.check_device_widths(4, 5)
    dataset.check_device_widths(5, 5)
    # the host feed lays out any width
    from pivp_amd.data import concat_examples
    img, act, sta = concat_examples([[images[i], np.full((4, 4), i, np.float32), np.full((4, 3), -i, np.float32)] for i in range(3)])
    assert img.shape == (4, 3, 3, 16, 16) and act.shape == (4, 3, 4) and sta.shape == (4, 3, 3) and act[2, 1, 3] == 1 and sta[0, 2, 0] == -2


@pytest.mark.parametrize('cli,positional', [(train_cli, []), (predict_cli, ['dir', 'name', '0']), (evaluate_cli, ['dir', 'name'])])
def test_the_command_lines_know_the_widths(cli, positional):
    args = cli.build_parser().parse_args(positional)
    assert (args.action_dim, args.state_dim) == (5, 5)
    args = cli.build_parser().parse_args(positional + ['--action_dim', '4', '--state_dim', '3'])
    assert (args.action_dim, args.state_dim) == (4, 3)
