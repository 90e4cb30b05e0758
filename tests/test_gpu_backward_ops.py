"""GPU parity tests of the backward kernels, per op: HIP (through the C ABI) vs PyTorch autograd in float64 on the CPU,
on the same seeded inputs.  Gradients are O(1)-scaled test cotangents; tolerances are relative to the gradient scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def env():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    from pivp_amd import _lib
    return pivp_amd, _lib, _lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def _nhwc(a):
    return _t(np.asarray(a).transpose(0, 2, 3, 1))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / (np.abs(b).max() + 1e-30)


@pytest.mark.parametrize('B,cx,C,H,first', [(2, 32, 32, 64, False), (2, 32, 32, 32, False), (2, 32, 64, 16, False), (3, 64, 128, 8, False),
                                            (2, 96, 32, 32, False), (2, 128, 64, 16, True)])
def test_convlstm_backward(env, B, cx, C, H, first):
    cases.convlstm_backward(env, B, cx, C, H, H, first)


@pytest.mark.parametrize('mode,B,cin,cout,H', [(0, 2, 32, 32, 32), (0, 3, 64, 64, 16), (1, 2, 128, 128, 8), (1, 2, 96, 96, 16), (1, 2, 64, 64, 32), (1, 2, 64, 64, 64),
                                               (0, 2, 32, 32, 64)])
def test_conv_deconv_backward(env, mode, B, cin, cout, H):
    cases.conv_deconv_backward(env, mode, B, cin, cout, H, H)


@pytest.mark.parametrize('B,C,H,relu', [(2, 32, 32, True), (3, 64, 16, False), (2, 128, 8, False), (2, 64, 64, True), (2, 64, 128, True),
                                       (2, 32, 64, False)])
def test_layernorm_backward(env, B, C, H, relu):
    cases.layernorm_backward(env, B, C, H, H, relu)


def test_adam_step_matches_chainer_rule(env):
    pivp, _lib, lib = env
    from oracle.torch_restatement import chainer_adam_step
    rs = np.random.RandomState(0)
    n = 100003
    p = rs.randn(n); g = rs.randn(n) * 0.01
    P = {'w': p.copy()}; G = {'w': g.copy()}; M = {'w': np.zeros(n)}; V = {'w': np.zeros(n)}
    pd, gd = _t(p), _t(g); md = torch.zeros_like(pd); vd = torch.zeros_like(pd)
    import math
    for t in (1, 2, 3):
        chainer_adam_step(P, G, M, V, t)
        lr_t = 0.001 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        _lib.check(lib.pivp_adam_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr_t, 0.9, 0.999, 1e-8, 1.0, _st()), 'adam')
    torch.cuda.synchronize()
    assert np.abs(pd.cpu().numpy() - P['w']).max() < 2e-6
    assert _rel(md.cpu().numpy(), M['w']) < 1e-5 and _rel(vd.cpu().numpy(), V['w']) < 1e-5


def test_adam_epsilon_placement_kat(env):
    """Chainer 2's AdamRule adds eps to the UNcorrected sqrt(v): p -= alpha * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps).
    PyTorch / the paper divide the corrected moments: p -= alpha * mhat / (sqrt(vhat) + eps).  They differ where sqrt(v) ~ eps, i.e. for
    |g| ~ eps / sqrt(1 - b2) = 3e-7 at t = 1: there Chainer's first step is alpha / 2, the other placement's 0.97 alpha.  Gradients that
    small pin the placement; the 0.01-sized gradients of test_adam_step_matches_chainer_rule cannot."""
    pivp, _lib, lib = env
    import math
    g = np.array([1e-9, 1e-8, 1e-7, 3.1623e-7, 1e-6, 1e-5, 1e-3, -3.1623e-7, -1e-8, 0.0], dtype=np.float64)
    alpha, b1, b2, eps = 0.001, 0.9, 0.999, 1e-8
    m = (1 - b1) * g; v = (1 - b2) * g * g
    lr_t = alpha * math.sqrt(1 - b2) / (1 - b1)
    chainer = -lr_t * m / (np.sqrt(v) + eps)                       # AdamRule.update_core at t = 1 from zero moments
    paper = -alpha * g / (np.abs(g) + eps)                         # mhat = g, vhat = g^2
    assert abs(chainer[3] / -alpha - 0.5) < 1e-3 and abs(paper[3] / -alpha - 0.97) < 1e-2   # the two rules really differ here
    pd = _t(np.zeros_like(g)); gd = _t(g); md = torch.zeros_like(pd); vd = torch.zeros_like(pd)
    _lib.check(lib.pivp_adam_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), g.size, lr_t, b1, b2, eps, 1.0, _st()), 'adam')
    torch.cuda.synchronize()
    got = pd.cpu().numpy().astype(np.float64)
    assert np.abs(got - chainer).max() < 2e-9, (got, chainer)
    assert np.abs(got - paper).max() > 4e-4                        # and is NOT the other placement


@pytest.mark.parametrize('mode,B,cin,cout,H,repeats', [(0, 3, 32, 32, 32, 2), (0, 5, 64, 64, 16, 3), (1, 3, 128, 128, 8, 2), (1, 5, 96, 96, 16, 3),
                                                       (1, 1, 64, 64, 32, 1), (0, 1, 32, 32, 64, 2), (1, 7, 64, 64, 8, 2)])
def test_conv_weight_gradient_through_partial_planes(env, mode, B, cin, cout, H, repeats):
    """The enc convs' weight gradients as the BPTT sweep runs them (round 2): per-block partial planes accumulated over `repeats` launches
    with plain loads and stores, ONE reduction into dW, bias gradient summed by the tap blocks that see every dY element once (conv:
    tap 0; transposed conv: taps (1,1), (1,2), (2,1), (2,2)).  Odd batch sizes put tile tails into the pixel splits; exact to fp32."""
    pivp, _lib, lib = env
    rs = np.random.RandomState(cin + mode + B)
    x = rs.randn(B, cin, H, H)
    Ho = 2 * H if mode else H // 2
    dy = rs.randn(B, cout, Ho, Ho)
    if mode:
        W = rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin); key = 'enc4/W'
    else:
        W = rs.randn(cout, cin, 3, 3) / np.sqrt(9 * cin); key = 'enc1/W'
    tx = torch.tensor(x, dtype=torch.float64); tW = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(tx, tW, tb, stride=2, padding=1, output_padding=1) if mode else F.conv2d(tx, tW, tb, stride=2, padding=1)
    (y * torch.tensor(dy)).sum().backward()
    xd, dyd = _nhwc(x), _nhwc(dy)
    n = lib.pivp_conv_backward_part_floats(mode, cin, cout, B, H, H)
    assert n > 0
    part = torch.zeros(n, dtype=torch.float32, device=DEV)
    prior = rs.randn(W.size).astype(np.float32) * 0.01                      # dW is accumulated into, not overwritten
    dW = _t(prior); db = torch.zeros(cout, dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_conv_wgrad_partial(mode, xd.data_ptr(), cin, cin, dyd.data_ptr(), cout, cout, part.data_ptr(), dW.data_ptr(),
                                           db.data_ptr(), B, H, H, repeats, _st()), 'conv_wgrad_partial')
    torch.cuda.synchronize()
    got = pivp.from_internal(key, dW.cpu().numpy() - prior, W.shape)
    assert _rel(got, repeats * tW.grad.numpy()) < 2e-5
    assert _rel(db.cpu().numpy(), repeats * tb.grad.numpy()) < 2e-5


@pytest.mark.parametrize('mode,B,cin,cout,H,T', [(0, 3, 32, 32, 32, 3), (0, 5, 64, 64, 16, 4), (1, 3, 128, 128, 8, 3), (1, 5, 96, 96, 16, 2), (1, 2, 64, 64, 32, 3),
                                                 (0, 1, 32, 32, 64, 2), (1, 7, 64, 64, 8, 5), (1, 2, 64, 64, 64, 2), (1, 2, 32, 32, 16, 2), (0, 2, 32, 32, 24, 2)])
def test_conv_weight_gradient_batched_over_timesteps(env, mode, B, cin, cout, H, T):
    """The sweep's form since round 5: ONE launch takes a batch of timesteps (x walked backwards through the forward slabs: a negative step; dY forwards
    through its ring), the first launch of a sweep stores into the partial planes (no zeroing: they start as garbage here), a second launch adds, one
    reduction.  The model's shapes run all nine taps from one staging (wgrad3x3s2.hip); 32 -> 32 transposed and the 12 x 12 anchor map fall to the
    per-tap kernel.  dW = sum over timesteps, against float64 autograd."""
    cases.conv_weight_gradient_batched_over_timesteps(env, mode, B, cin, cout, H, H, T)


@pytest.mark.parametrize('B,cx,C,H', [(3, 32, 32, 32), (5, 32, 64, 16), (3, 64, 128, 8), (1, 96, 32, 32), (2, 128, 64, 16)])
def test_convlstm_backward_last_timestep_computes_dx_only(env, B, cx, C, H):
    """t = 0 of the sweep: the data gradient runs on the first cx columns of the transposed weight pack (IgemmDesc::wN); d x, d c, dW, db
    are those of the full backward and the d h_{-1} columns of d_in are NOT computed (they keep their content, or are zero where the gate
    kernel cleared d_in for a K-split data gradient).  Odd batches: M tails of the column-limited tiles."""
    cases.convlstm_backward_dx_only(env, B, cx, C, H, H)


@pytest.mark.parametrize('B,C,H,lddy,recurrent', [(32, 32, 32, 64, True), (8, 64, 16, 96, True), (32, 128, 8, 128, True), (5, 32, 32, 32, False),
                                                  (2, 64, 16, 64, True)])
def test_layernorm_plus_gate_backward_pair(env, B, C, H, lddy, recurrent):
    """hidden<k>'s LayerNorm backward + lstm<k>'s gate backward as the sweep runs the pair (TM:203-208, TM:269-272: sums and parameter
    planes, then the gate kernel forming the norm's dx from the partials) against float64 autograd."""
    cases.layernorm_plus_gate_backward_pair(env, B, C, H, H, lddy, recurrent)


# (B, cx, C, H, timesteps per launch): every map width of the model (8 ... 64) and 128 (config 5), odd batches, cx != C, partitions with one and several
# pixel parts, segments that cross tile boundaries, a batch of timesteps per launch and several launches into the same slots
@pytest.mark.parametrize('B,cx,C,H,Ts', [(2, 32, 32, 32, (1,)), (3, 32, 32, 32, (2, 1)), (2, 32, 64, 16, (1, 1, 1)), (5, 64, 64, 16, (3,)), (3, 64, 128, 8, (1, 2)),
                                         (1, 96, 32, 32, (1,)), (2, 128, 64, 16, (2,)), (2, 32, 32, 64, (1,)), (1, 32, 32, 128, (1,)), (32, 64, 128, 8, (1,)),
                                         (8, 96, 32, 32, (1,))])
@pytest.mark.parametrize('form', [1, 2])      # 32 / 64 gate columns per wave
def test_convlstm_weight_gradient_in_partial_slots(env, B, cx, C, H, Ts, form):
    """Round 6's fp32 ConvLSTM weight gradient (csrc/wgrad5x5p.hip): launches add into NaN-initialised partial slots (the first one stores), one reduction
    forms dW and db.  Against float64 sums; against the round-2 kernel; and bit-identical when repeated."""
    cases.convlstm_weight_gradient_in_partial_slots(B, cx, C, H, H, Ts, form)
