"""bf16-operand ConvLSTM (BASELINE.json config 3) against the float64 oracle.

The kernel rounds x, h and the weights to bf16 (nearest even) and accumulates in fp32.  Two kinds of check:
  * operands that ARE bf16 numbers: every product is exact in fp32, so the result must agree with the oracle to fp32
    summation-order accuracy -- this pins every index of the patch / weight-ring scheme as tightly as the fp32 tests do;
  * arbitrary fp32 operands: the difference to the oracle is the bf16 rounding of the operands, reported and bounded.
"""
import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu
TOL = 2e-5

SHAPES = [(2, 32, 32, 32), (2, 32, 64, 16), (4, 64, 128, 8), (2, 128, 64, 16), (1, 96, 32, 32), (3, 64, 64, 16), (2, 16, 16, 8),
          (1, 32, 32, 64)]


@pytest.fixture(scope='module')
def ops():
    import hip_ops
    return hip_ops


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


def _lstm_ref(x, h, c, W, b):
    g = R.conv2d(np.concatenate([x, h], 1), W, b, 1, 2)
    j, i, f, o = np.split(g, 4, axis=1)
    cn = c * R.sigmoid(f + 1.0) + R.sigmoid(i) * np.tanh(j)
    return np.tanh(cn) * R.sigmoid(o), cn, (np.tanh(j), R.sigmoid(i), R.sigmoid(f + 1.0), R.sigmoid(o))


def _case(B, cx, C, H, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, cx, H, H); h = rs.randn(B, C, H, H) * 0.5; c = rs.randn(B, C, H, H)
    W = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
    return x, h, c, W, b


@pytest.mark.parametrize('nch', [0, 16, 32])
@pytest.mark.parametrize('B,cx,C,H', SHAPES)
def test_convlstm_bf16_exact_on_bf16_operands(ops, B, cx, C, H, nch):
    if nch == 32 and C % 32:
        pytest.skip('32-channel blocks need C % 32 == 0')
    x, h, c, W, b = _case(B, cx, C, H, B * 100 + C + H)
    x, h, W = _bf16(x), _bf16(h), _bf16(W)
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    hg, cg = ops.convlstm_bf16(x, h, c, W, b, nch)
    assert np.abs(hg - hr).max() < TOL and np.abs(cg - cr).max() < TOL


@pytest.mark.parametrize('B,cx,C,H', SHAPES[:5])
def test_convlstm_bf16_rounding_error(ops, B, cx, C, H):
    # fp32 operands: the result is the oracle's on bf16-rounded operands; against the unrounded oracle the error is the
    # operand rounding (2^-9 relative per operand, K = 25 (cx + C) random-sign terms) -- well under 1e-2 on O(1) gates
    x, h, c, W, b = _case(B, cx, C, H, 7 + H)
    hq, cq, _ = _lstm_ref(_bf16(x), _bf16(h), c, _bf16(W), b)
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    hg, cg = ops.convlstm_bf16(x, h, c, W, b)
    assert np.abs(hg - hq).max() < TOL and np.abs(cg - cq).max() < TOL
    err = max(np.abs(hg - hr).max(), np.abs(cg - cr).max())
    print('bf16 ConvLSTM B=%d cx=%d C=%d H=%d: max |err| vs fp64 oracle %.2e' % (B, cx, C, H, err))
    assert 1e-5 < err < 1e-2


def test_convlstm_bf16_first_step_zero_h(ops):
    x, h, c, W, b = _case(2, 64, 128, 8, 5)
    x, W = _bf16(x), _bf16(W)
    h = np.zeros_like(h); c = np.zeros_like(c)
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    hg, cg = ops.convlstm_bf16(x, h, c, W, b, h_is_zero=True)
    hz, cz = ops.convlstm_bf16(x, h, c, W, b, h_is_zero=False)
    assert np.abs(hg - hr).max() < TOL and np.abs(cg - cr).max() < TOL
    assert np.abs(hg - hz).max() < 2e-6 and np.abs(cg - cz).max() < 2e-6


@pytest.mark.parametrize('B,cx,C,H', [(2, 32, 32, 32), (2, 64, 128, 8), (2, 32, 64, 16)])
def test_convlstm_bf16_gates_and_layernorm_partials(ops, B, cx, C, H):
    x, h, c, W, b = _case(B, cx, C, H, 11 + C)
    x, h, W = _bf16(x), _bf16(h), _bf16(W)
    hr, cr, gr = _lstm_ref(x, h, c, W, b)
    hg, cg, gates, (part, n) = ops.convlstm_bf16(x, h, c, W, b, want_gates=True, want_ln=True)
    assert np.abs(hg - hr).max() < TOL
    gn = gates.reshape(B, H, H, 4, C).transpose(3, 0, 4, 1, 2)      # [gate][B][C][H][W]
    for k in range(4):
        assert np.abs(gn[k] - gr[k]).max() < TOL
    assert n > 0
    for s in range(B):                                              # Chan merge of the (count, mean, M2) partials
        cnt = part[s, :, 0].astype(np.float64); mean = part[s, :, 1].astype(np.float64); m2 = part[s, :, 2].astype(np.float64)
        assert cnt.sum() == C * H * H
        tot_mean = (cnt * mean).sum() / cnt.sum()
        tot_m2 = m2.sum() + (cnt * (mean - tot_mean) ** 2).sum()
        assert abs(tot_mean - hr[s].mean()) < 1e-5
        assert abs(tot_m2 / cnt.sum() - hr[s].var()) < 1e-5


def test_convlstm_bf16_rejects_bad_shapes(ops):
    x, h, c, W, b = _case(1, 32, 32, 8, 1)                          # 8-wide map with odd batch
    with pytest.raises(RuntimeError):
        ops.convlstm_bf16(x, h, c, W, b)
    x, h, c, W, b = _case(2, 32, 32, 12, 1)                         # H % 8 != 0
    with pytest.raises(RuntimeError):
        ops.convlstm_bf16(x, h, c, W, b)


# ---- whole rollout in the bf16 precision mode (BASELINE.json config 3) ---------------------------------------------------
GOLD = __import__('os').path.join(__import__('os').path.dirname(__file__), 'golden')


def _rollout(precision, mt='CDNA', nm=10, B=2, T=10, train=False, keep=False, smooth=False):
    import pivp_amd
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=nm, model_type=mt)
    imgs, acts, stas = R.synthetic_batch(B, T)
    if smooth:                          # video-like frames (11x11 box blur of the noise), as tests/test_gpu_model.py's STP case
        from numpy.lib.stride_tricks import sliding_window_view
        pad = np.pad(imgs, ((0, 0), (0, 0), (0, 0), (5, 5), (5, 5)), mode='reflect')
        imgs = np.ascontiguousarray(sliding_window_view(pad, (11, 11), axis=(3, 4)).mean(axis=(-1, -2))).astype(np.float32)
    m = pivp_amd.Model(nm, is_cdna=mt == 'CDNA', is_stp=mt == 'STP', is_dna=mt == 'DNA', prefix='test', precision=precision,
                       keep_activations=keep)
    m.load_state_dict_reference(P)
    with pivp_amd.using_config('train', train):
        loss = m([imgs, acts, stas], 0)
    return m, float(loss), torch.stack(m.gen_images).cpu().numpy()


def test_rollout_bf16_reports_error_against_the_golden_fixture():
    # config 1's golden rollout (float64 oracle): the bf16 mode is not held to the 1e-4 gate ("bf16 config
    # reports its error"); the bound below only guards against a broken kernel, the printed numbers are the report
    g = np.load(__import__('os').path.join(GOLD, 'cdna_b2_t10.npz'))
    m32, loss32, gen32 = _rollout('fp32')
    m16, loss16, gen16 = _rollout('bf16')
    l2_32 = R.per_pixel_l2(gen32, g['gen_images']); l2_16 = R.per_pixel_l2(gen16, g['gen_images'])
    print('per-pixel L2 vs float64 oracle: fp32 max %.2e rms %.2e | bf16 max %.2e rms %.2e | loss %.6f / %.6f / %.6f'
          % (l2_32.max(), np.sqrt((l2_32 ** 2).mean()), l2_16.max(), np.sqrt((l2_16 ** 2).mean()), float(g['loss']), loss32, loss16))
    assert l2_32.max() < 1e-4
    assert 1e-6 < l2_16.max() < 5e-2            # bf16 really ran, and is a rounding-level perturbation
    assert abs(loss16 - float(g['loss'])) < 1e-3
    assert m16._active.lib.pivp_plan_get_precision(m16._active.h) == 1
    assert m32._active.lib.pivp_plan_get_precision(m32._active.h) == 0


@pytest.mark.parametrize('mt,nm', [('STP', 10), ('DNA', 1)])
def test_rollout_bf16_other_heads(mt, nm):
    # STP warps the previous frame bilinearly: on white-noise frames a 1e-3 change of the affine parameters moves O(1) pixel
    # values (tests/test_gpu_model.py has the fp32 analysis), so the STP comparison uses smooth frames
    _, l32, g32 = _rollout('fp32', mt, nm, T=4, smooth=mt == 'STP')
    _, l16, g16 = _rollout('bf16', mt, nm, T=4, smooth=mt == 'STP')
    l2 = R.per_pixel_l2(g16, g32)
    rms = float(np.sqrt((l2 ** 2).mean()))
    print('%s bf16 vs fp32 rollout: per-pixel L2 max %.2e rms %.2e' % (mt, l2.max(), rms))
    # (measured: DNA max 2.5e-2; STP max 1.5e-1 at a few pixels where the warp crosses an edge, rms an order below)
    assert 1e-7 < l2.max() < (5e-1 if mt == 'STP' else 5e-2) and rms < 2e-2 and abs(l16 - l32) < 1e-3


def test_train_step_in_bf16_mode_tracks_fp32():
    # forward gate convolutions in bf16, backward in fp32 on the fp32 parameters: gradients stay close to the fp32 path's
    import pivp_amd
    outs = {}
    for prec in ('fp32', 'bf16'):
        m, loss, _ = _rollout(prec, T=4, train=True, keep=True)
        with pivp_amd.using_config('train', True):
            m.backward()
        outs[prec] = (loss, m._flat_grads.clone())
    g32, g16 = outs['fp32'][1], outs['bf16'][1]
    rel = float((g16 - g32).norm() / g32.norm())
    print('bf16-forward train step: loss %.6f vs %.6f, relative gradient difference %.2e' % (outs['bf16'][0], outs['fp32'][0], rel))
    assert abs(outs['bf16'][0] - outs['fp32'][0]) < 1e-3
    assert 1e-6 < rel < 5e-2


def test_bf16_precision_refused_for_unsupported_geometry():
    import pivp_amd
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=10, model_type='CDNA')
    imgs, acts, stas = R.synthetic_batch(1, 3)                      # 8-wide lstm5 map with an odd batch
    m = pivp_amd.Model(10, precision='bf16', prefix='t')
    m.load_state_dict_reference(P)
    with pytest.raises(RuntimeError):
        m([imgs, acts, stas], 0)
    with pytest.raises(ValueError):
        pivp_amd.Model(10, precision='fp16')


# ---- plain 5x5 convolution of the same kernel (the ConvLSTM data gradient of the bf16 mode) -----------------------------
def _conv5x5_bf16_exact(ops, B, cin, cout, H, Wd):
    # shapes of the seven data gradients (cin = 4C gate channels, cout = Cx + C); cout = 96 exercises the padded column block,
    # the 8x8 / B = 4 case the K-split over channel groups with atomic adds, B = 32 the unsplit 8x8 grid
    rs = np.random.RandomState(cin + cout + H)
    x = _bf16(rs.randn(B, cin, H, Wd)); W = _bf16(rs.randn(cout, cin, 5, 5) / np.sqrt(25 * cin))
    ref = R.conv2d(x, W, np.zeros(cout), 1, 2)
    got = ops.conv5x5_bf16(x, W)
    assert np.abs(got - ref).max() < TOL


@pytest.mark.parametrize('B,cin,cout,H', [(2, 128, 64, 32), (2, 256, 96, 16), (4, 512, 192, 8), (2, 256, 128, 16), (1, 128, 128, 32),
                                          (32, 512, 192, 8), (1, 128, 64, 64)])
def test_conv5x5_bf16_exact_on_bf16_operands(ops, B, cin, cout, H):
    _conv5x5_bf16_exact(ops, B, cin, cout, H, H)


def test_conv5x5_bf16_accumulates(ops):
    rs = np.random.RandomState(3)
    x = _bf16(rs.randn(2, 128, 16, 16)); W = _bf16(rs.randn(64, 128, 5, 5) / np.sqrt(3200)); base = rs.randn(2, 64, 16, 16)
    ref = base + R.conv2d(x, W, np.zeros(64), 1, 2)
    assert np.abs(ops.conv5x5_bf16(x, W, accum_into=base) - ref).max() < TOL


# ---- ConvLSTM weight gradient with bf16 operands (transposing LDS reads) ----------------------------------------------------
def _wgrad_ref(x, h, dG):
    """dW[n, ci, ky, kx] = sum_{b,y,x} concat(x,h)[b, ci, y+ky-2, x+kx-2] * dG[b, n, y, x] (zero outside the image), float64."""
    xin = np.concatenate([x, h], 1)
    B, cin, H, W = xin.shape
    pad = np.pad(xin, ((0, 0), (0, 0), (2, 2), (2, 2)))
    dW = np.zeros((dG.shape[1], cin, 5, 5))
    for ky in range(5):
        for kx in range(5):
            dW[:, :, ky, kx] = np.einsum('bnyx,bcyx->nc', dG, pad[:, :, ky:ky + H, kx:kx + W])
    return dW


@pytest.mark.parametrize('B,cx,C,H', [(2, 32, 32, 32), (2, 32, 64, 16), (4, 64, 128, 8), (2, 128, 64, 16), (1, 96, 32, 32), (3, 64, 64, 16),
                                      (1, 32, 32, 64)])
def test_wgrad5x5_bf16_exact_on_bf16_operands(ops, B, cx, C, H):
    rs = np.random.RandomState(B + cx + C + H)
    x = _bf16(rs.randn(B, cx, H, H)); h = _bf16(rs.randn(B, C, H, H) * 0.5); dG = _bf16(rs.randn(B, 4 * C, H, H) * 0.1)
    ref = _wgrad_ref(x, h, dG)
    got, db = ops.wgrad5x5_bf16(x, h, dG)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, scale)      # fp32 accumulation over B*H*W products per element
    assert np.abs(db - dG.sum(axis=(0, 2, 3))).max() < 2e-4      # bias gradient: fp32 column sums of dG taken on the side


def test_wgrad5x5_bf16_first_step_leaves_h_rows_alone(ops):
    rs = np.random.RandomState(9)
    B, cx, C, H = 2, 64, 128, 8
    x = _bf16(rs.randn(B, cx, H, H)); h = np.zeros((B, C, H, H)); dG = _bf16(rs.randn(B, 4 * C, H, H) * 0.1)
    ref = _wgrad_ref(x, h, dG)
    got, _ = ops.wgrad5x5_bf16(x, h, dG, h_is_zero=True)
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    assert np.all(got[:, cx:] == 0)


def _wgrad5x5_bf16_batch(ops, B, cx, C, H, Wd, T, form):
    # one launch for T timesteps (operands at signed byte strides) = the sum of the per-timestep gradients
    rs = np.random.RandomState(B + cx + C + H + T)
    xs = [_bf16(rs.randn(B, cx, H, Wd)) for _ in range(T)]; hs = [_bf16(rs.randn(B, C, H, Wd) * 0.5) for _ in range(T)]
    dGs = [_bf16(rs.randn(B, 4 * C, H, Wd) * 0.1) for _ in range(T)]
    ref = sum(_wgrad_ref(x, h, g) for x, h, g in zip(xs, hs, dGs))
    got, db = ops.wgrad5x5_bf16_batch(xs, hs, dGs, form=form)
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(db - sum(g.sum(axis=(0, 2, 3)) for g in dGs)).max() < 4e-4


@pytest.mark.parametrize('form', [0, 1, 2])      # 1: four-wave blocks (co-resident with the sweep's small kernels; what 0 picks at these sizes), 2: eight-wave blocks
@pytest.mark.parametrize('B,cx,C,H,T', [(2, 32, 32, 32, 3), (2, 32, 64, 16, 4), (4, 64, 128, 8, 3), (1, 96, 32, 32, 2)])
def test_wgrad5x5_bf16_batch_of_timesteps(ops, B, cx, C, H, T, form):
    _wgrad5x5_bf16_batch(ops, B, cx, C, H, H, T, form)


def _wgrad5x5_split_batch(ops, B, cx, C, H, Wd, T, gscale, mode):
    # the fp16x3 mode's weight gradient: two fp16 pieces per operand, dG scaled by a power of two from the batch's largest value.  fp32-representable
    # operands against the float64 sums and against the fp32 kernel; dG of gradient size (1e-7) and timesteps / gates whose sizes differ by 1e4
    rs = np.random.RandomState(B + cx + C + H + T + 5)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    xs = [f32(rs.randn(B, cx, H, Wd)) for _ in range(T)]; hs = [f32(rs.randn(B, C, H, Wd) * 0.5) for _ in range(T)]
    if gscale == 'ragged':
        dGs = [f32(rs.randn(B, 4 * C, H, Wd) * 10.0 ** rs.uniform(-7, -3, size=(1, 4 * C, 1, 1)) * 10.0 ** (-t)) for t in range(T)]
    else:
        dGs = [f32(rs.randn(B, 4 * C, H, Wd) * gscale) for _ in range(T)]
    ref = sum(_wgrad_ref(x, h, g) for x, h, g in zip(xs, hs, dGs))
    kw = {'fp16x3': True} if mode == 'fp16x3' else {'bf16x6': True}     # (three bf16 pieces: the bf16x6 mode's form, no scale)
    got, db = ops.wgrad5x5_bf16_batch(xs, hs, dGs, **kw)
    unit = np.sqrt((ref ** 2).mean())
    e3 = (got - ref) / unit
    ef = (sum(ops.convlstm_wgrad(x, h, g)[0] for x, h, g in zip(xs, hs, dGs)) - ref) / unit if hasattr(ops, 'convlstm_wgrad') else None
    print('wgrad %d+%d @%d x %d steps, dG %s: %s max |err| %.2e rms %.2e of the gradient rms' % (cx, C, H, T, gscale, mode, np.abs(e3).max(), np.sqrt((e3 ** 2).mean()))
          + ('' if ef is None else '; fp32 kernel max %.2e rms %.2e' % (np.abs(ef).max(), np.sqrt((ef ** 2).mean()))))
    assert np.abs(e3).max() < 2e-5 and np.sqrt((e3 ** 2).mean()) < 2e-6
    if ef is not None:
        assert np.sqrt((e3 ** 2).mean()) < 1.5 * np.sqrt((ef ** 2).mean())
    dbr = sum(g.sum(axis=(0, 2, 3)) for g in dGs)
    assert np.abs(db - dbr).max() < 1e-4 * np.abs(dbr).max() + 1e-12
    if T == 1:       # the sweep's t = 0: no h operand, only the x rows are touched
        got0, _ = ops.wgrad5x5_bf16_batch(xs, hs, dGs, h_is_zero=True, **kw)
        assert np.abs(got0[:, :cx] - ref[:, :cx]).max() < 2e-5 * unit and np.all(got0[:, cx:] == 0)


@pytest.mark.parametrize('mode', ['fp16x3', 'bf16x6'])
@pytest.mark.parametrize('gscale', [0.1, 1e-7, 'ragged'])
@pytest.mark.parametrize('B,cx,C,H,T', [(2, 32, 32, 32, 3), (2, 32, 64, 16, 4), (4, 64, 128, 8, 3), (1, 96, 32, 32, 1)])
def test_wgrad5x5_fp16x3_batch_of_timesteps(ops, B, cx, C, H, T, gscale, mode):
    _wgrad5x5_split_batch(ops, B, cx, C, H, H, T, gscale, mode)


def test_bf16_mode_batched_weight_gradients_match_per_step():
    # the bf16 mode's plan batches the ConvLSTM weight gradients of up to 8 timesteps per launch (default) -- same products as one launch
    # per timestep, other summation order.  The batch is the plan option 'wgrad_batch' (None: not named, the mode's own choice); each Model must
    # report the batch asked for, and its dG rings -- so its workspace -- the depth that goes with it (T - 2 = 5 slots hold the default's batches)
    import torch
    import pivp_amd
    from oracle import restatement as R
    assert torch.cuda.is_available()
    P = R.init_params_widened(seed=1, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(2, 7)
    outs, ws_bytes = {}, {}
    for batch in ('1', '3', None):
        m = pivp_amd.Model(10, prefix='t', keep_activations=True, precision='bf16',
                           plan_options={'wgrad_batch': 0 if batch is None else int(batch)})
        m.load_state_dict_reference(P)
        m([imgs, acts, stas], 0)
        m.cleargrads(); m.backward()
        assert m.effective_plan_options()['wgrad_batch'] == (0 if batch is None else int(batch))
        ws_bytes[batch] = m._active.lib.pivp_plan_workspace_bytes(m._active.h)
        outs[batch] = m._flat_grads.clone()
    assert ws_bytes['1'] < ws_bytes['3'] < ws_bytes[None], ws_bytes      # ring depths 1, 3, 5
    for key, g in outs.items():
        rel = float((g - outs['1']).norm() / outs['1'].norm())
        # Two bf16 sweeps of the SAME configuration already differ by 1.5e-4 .. 6e-4 (the K-split data gradients' atomics reorder fp32 sums
        # whose results are then rounded to bf16 operands downstream: scripts/soak_bf16_sweeps.py); a batching bug (a timestep dropped,
        # a wrong stride) is O(0.1 - 1).  The exact statement about the batched kernel is test_wgrad5x5_bf16_batch_of_timesteps.
        assert rel < 3e-3, (key, rel)


# ---- transposed 3x3 stride-2 conv with bf16 operands (enc5 / enc6 in the bf16 mode) ---------------------------------------------------
@pytest.mark.parametrize('B,cin,cout,H,relu', [(2, 64, 64, 32, False), (4, 96, 96, 16, True), (2, 128, 128, 16, True)])
def test_deconv3x3s2_bf16_exact_on_bf16_operands(ops, B, cin, cout, H, relu):
    rs = np.random.RandomState(cin + H)
    x = _bf16(rs.randn(B, cin, H, H)); W = _bf16(rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin)); b = rs.randn(cout) * 0.1
    ref = R.deconv2d(x, W, b, 2, 1, (2 * H, 2 * H))
    if relu:
        ref = R.relu(ref)
    got = ops.deconv3x3s2(x, W, b, relu, bf16=True)
    assert np.abs(got - ref).max() < TOL
    # and the unrounded operands differ from the fp32 op by the operand rounding only
    x2 = rs.randn(B, cin, H, H); W2 = rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin)
    d = np.abs(ops.deconv3x3s2(x2, W2, b, relu, bf16=True) - ops.deconv3x3s2(x2, W2, b, relu)).max()
    assert 1e-5 < d < 2e-2


# ---- split mode: two bf16 pieces per fp32 operand, three MFMAs per product -------------------------------------------------------
@pytest.mark.parametrize('nch', [16, 32])
@pytest.mark.parametrize('B,cx,C,H', SHAPES[:6])
def test_convlstm_bf16x3_on_fp32_operands(ops, B, cx, C, H, nch):
    # arbitrary fp32 operands: what is lost is the lo*lo product and the third piece of each operand, ~2^-16 relative per product
    x, h, c, W, b = _case(B, cx, C, H, 31 + C + H)
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    hg, cg = ops.convlstm_bf16x3(x, h, c, W, b, nch=nch)   # 16: four ring slots, mid-tap barrier; 32: two slots, end-of-tap barrier
    h1, c1 = ops.convlstm_bf16(x, h, c, W, b)
    e3 = max(np.abs(hg - hr).max(), np.abs(cg - cr).max()); e1 = max(np.abs(h1 - hr).max(), np.abs(c1 - cr).max())
    print('B=%d cx=%d C=%d H=%d: max |err| split %.2e, plain bf16 %.2e' % (B, cx, C, H, e3, e1))
    assert e3 < 5e-5 and e3 < e1 / 50


def test_convlstm_bf16x3_exact_when_operands_fit_two_pieces(ops):
    # operands with 16 significant bits (hi + lo exactly): every kept product is exact, the dropped lo*lo terms are ~2^-16 of the result
    x, h, c, W, b = _case(2, 32, 64, 16, 77)
    def two(a):
        hi = _bf16(a); return hi + _bf16(a - hi)
    x, h, W = two(x), two(h), two(W)
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    for nch in (16, 32):
        hg, cg = ops.convlstm_bf16x3(x, h, c, W, b, nch=nch)
        assert np.abs(hg - hr).max() < TOL and np.abs(cg - cr).max() < TOL


# ---- three pieces per operand, six MFMAs per product: fp32-grade results on the bf16 matrix cores ----------------------
X6_SHAPES = [(2, 32, 32, 32), (2, 32, 64, 16), (2, 128, 64, 16), (1, 96, 32, 32), (3, 64, 64, 16), (1, 32, 32, 64), (2, 64, 128, 16)]


@pytest.mark.parametrize('nch', [16, 32])    # channels per block of the eight-wave kernel (weights from L2 into the operand registers)
@pytest.mark.parametrize('B,cx,C,H', X6_SHAPES)
def test_convlstm_bf16x6_is_fp32_grade(ops, B, cx, C, H, nch):
    # fp32-representable operands, so that neither kernel is charged for the rounding of its inputs: hi + mid + lo is every operand exactly,
    # the dropped products are < 2^-24 of a product, and the main accumulator rounds once per 16 products (the fp32 kernel: once per product)
    x, h, c, W, b = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(B, cx, C, H, 131 + C + H)]
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    h6, c6 = ops.convlstm_bf16x6(x, h, c, W, b, nch=nch)
    hf, cf = ops.convlstm(x, h, c, W, b)
    e6 = max(np.abs(h6 - hr).max(), np.abs(c6 - cr).max()); ef = max(np.abs(hf - hr).max(), np.abs(cf - cr).max())
    r6 = np.sqrt(((c6 - cr) ** 2).mean()); rf = np.sqrt(((cf - cr) ** 2).mean())
    print('B=%d cx=%d C=%d H=%d: max |err| three-piece %.2e, fp32 kernel %.2e; rms of c %.2e vs %.2e' % (B, cx, C, H, e6, ef, r6, rf))
    assert e6 < 2e-6 and e6 < 2.0 * ef and r6 < 1.2 * rf       # (the maximum over 1e5 values scatters; the rms is the robust figure: 0.8-0.95 of the fp32 kernel's)


def test_convlstm_bf16x6_first_step_and_narrow_maps(ops):
    # t = 0 (no h operand: its K range is skipped) on a 16-wide map; 8-wide maps: tiles of two images (an even batch), an odd batch is refused
    x, h, c, W, b = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(2, 32, 32, 16, 5)]
    hr, cr, _ = _lstm_ref(x, h * 0, c, W, b)
    for nch in (16, 32):
        h6, c6 = ops.convlstm_bf16x6(x, h, c, W, b, h_is_zero=True, nch=nch)
        assert np.abs(h6 - hr).max() < 2e-6 and np.abs(c6 - cr).max() < 2e-6
    # both forms against each other, and the LayerNorm partial statistics of their epilogues
    xa, ha, ca, Wa, ba = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(2, 96, 32, 32, 9)]
    h16, c16, (p16, n16) = ops.convlstm_bf16x6(xa, ha, ca, Wa, ba, nch=16, want_ln=True)
    h32, c32, (p32, n32) = ops.convlstm_bf16x6(xa, ha, ca, Wa, ba, nch=32, want_ln=True)
    assert np.abs(h16 - h32).max() < 2e-6 and np.abs(c16 - c32).max() < 2e-6      # (same terms; the blocks walk the taps in different rotations)
    h16b, c16b = ops.convlstm_bf16x6(xa, ha, ca, Wa, ba, nch=16)
    assert np.array_equal(h16, h16b) and np.array_equal(c16, c16b)                  # same blocks, same rotations, same order: identical bits
    assert n16 == 2 * n32 and n32 == 8
    for pp, hh in ((p16, h16), (p32, h32)):
        cnt = pp[:, :, 0].sum(axis=1)
        mean = (pp[:, :, 0] * pp[:, :, 1]).sum(axis=1) / cnt
        assert np.allclose(cnt, 32 * 32 * 32) and np.allclose(mean, hh.reshape(2, -1).mean(axis=1), atol=1e-6)
    lib = __import__('pivp_amd')._lib.load()
    import torch
    z = torch.zeros(1 << 20, device='cuda')
    rc = lib.pivp_convlstm_bf16x6(z.data_ptr(), 64, 64, z.data_ptr(), 128, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                  None, None, 0, None, 3, 8, 8, 0, None)
    assert rc == -1            # PIVP_ERR_BADARG (8-wide map, odd batch): the per-op entry has no fp32 weights to fall back on (the plan does)
    # 8-wide maps (lstm5 at 64 x 64 frames: 64 + 128 -> 128), both block widths, t = 0 too, and the LayerNorm partials of the two images of a tile
    x8, h8, c8, W8, b8 = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(4, 64, 128, 8, 11)]
    hr8, cr8, _ = _lstm_ref(x8, h8, c8, W8, b8)
    hf8, cf8 = ops.convlstm(x8, h8, c8, W8, b8)
    ef8 = max(np.abs(hf8 - hr8).max(), np.abs(cf8 - cr8).max())
    for nch in (16, 32):
        h6, c6, (p6, n6) = ops.convlstm_bf16x6(x8, h8, c8, W8, b8, nch=nch, want_ln=True)
        e6 = max(np.abs(h6 - hr8).max(), np.abs(c6 - cr8).max())
        print('8-wide map, %d-channel blocks: max |err| three-piece %.2e, fp32 kernel %.2e' % (nch, e6, ef8))
        assert e6 < 2e-6 and e6 < 2.0 * ef8
        assert n6 == 128 // nch
        cnt = p6[:, :, 0].sum(axis=1)
        mean = (p6[:, :, 0] * p6[:, :, 1]).sum(axis=1) / cnt
        var = (p6[:, :, 2] + p6[:, :, 0] * (p6[:, :, 1] - mean[:, None]) ** 2).sum(axis=1) / cnt
        assert np.allclose(cnt, 128 * 64) and np.allclose(mean, h6.reshape(4, -1).mean(axis=1), atol=1e-6) and np.allclose(var, h6.reshape(4, -1).var(axis=1), rtol=1e-4)
    hr0, cr0, _ = _lstm_ref(x8, h8 * 0, c8, W8, b8)
    h0, c0 = ops.convlstm_bf16x6(x8, h8, c8, W8, b8, h_is_zero=True)
    assert np.abs(h0 - hr0).max() < 2e-6 and np.abs(c0 - cr0).max() < 2e-6


def _conv5x5_bf16x6(ops, B, cin, cout, H, Wd, accumulate=True):
    # the data gradients of the three-piece mode: 64-column blocks on the k-step ring, padded columns (96), K split over the channel groups (B = 32
    # on a 16 x 16 map: 64 tiles x 3 column blocks), against the float64 convolution and the fp32 kernel
    rs = np.random.RandomState(cin + cout + H + 6)
    x = rs.randn(B, cin, H, Wd).astype(np.float32).astype(np.float64); W = (rs.randn(cout, cin, 5, 5) / np.sqrt(25 * cin)).astype(np.float32).astype(np.float64)
    ref = R.conv2d(x, W, np.zeros(cout), 1, 2)
    e6 = ops.conv5x5_bf16(x, W, pieces=3) - ref
    ef = ops.conv_s1(x, W, 5) - ref if hasattr(ops, 'conv_s1') else None
    print('conv5x5 %d->%d @%d: three-piece max |err| %.2e rms %.2e' % (cin, cout, H, np.abs(e6).max(), np.sqrt((e6 ** 2).mean()))
          + ('' if ef is None else '; fp32 kernel max %.2e rms %.2e' % (np.abs(ef).max(), np.sqrt((ef ** 2).mean()))))
    # (one accumulation chain per output over K = 25 cin: 2.1e-7 rms at K = 3200-6400 with the channel groups split over blocks, 4.4e-7 for the unsplit 6400)
    assert np.abs(e6).max() < 2e-5 and np.sqrt((e6 ** 2).mean()) < 7e-7      # (observed up to 6.7e-6 / 5.2e-7; the K-split sums meet by atomic adds in any order)
    if ef is not None:
        assert np.sqrt((e6 ** 2).mean()) < 1.2 * np.sqrt((ef ** 2).mean())
    acc = rs.randn(B, cout, H, Wd).astype(np.float32)
    if B < 32 and accumulate:                        # accumulate form
        out = ops.conv5x5_bf16(x, W, accum_into=acc.astype(np.float64), pieces=3)
        assert np.abs(out - (ref + acc)).max() < 6e-6       # (+ the rounding of the final add at |values| up to 5)


@pytest.mark.parametrize('B,cin,cout,H', [(2, 128, 64, 32), (2, 256, 96, 16), (2, 256, 128, 16), (32, 256, 192, 16), (1, 128, 128, 32), (4, 512, 192, 8), (32, 512, 192, 8)])    # 8-wide maps: tiles of two images (lstm5's data gradient)
def test_conv5x5_bf16x6(ops, B, cin, cout, H):
    _conv5x5_bf16x6(ops, B, cin, cout, H, H)


def _conv5x5_fp16x3(ops, B, cin, cout, H, Wd, scale, accumulate=True):
    # the data gradients of the fp16x3 mode: two fp16 pieces per operand, x staged times a power of two from its largest |value|.  Unit-scale x, x of
    # gradient size (1e-6: every fp16 piece would be subnormal or zero without the scale), and channels whose sizes differ by 1e6 (the small ones lose
    # second-piece bits: their ABSOLUTE error stays below the rounding of the large ones)
    rs = np.random.RandomState(cin + cout + H + 16)
    x = rs.randn(B, cin, H, Wd)
    if scale == 'ragged':
        x = x * (10.0 ** rs.uniform(-9, -3, size=(1, cin, 1, 1)))
    else:
        x = x * scale
    x = x.astype(np.float32).astype(np.float64); W = (rs.randn(cout, cin, 5, 5) / np.sqrt(25 * cin)).astype(np.float32).astype(np.float64)
    ref = R.conv2d(x, W, np.zeros(cout), 1, 2)
    unit = np.sqrt((ref ** 2).mean())
    e3 = (ops.conv5x5_bf16(x, W, pieces='fp16x3') - ref) / unit
    ef = (ops.conv5x5_bf16(x, W, pieces=3) - ref) / unit        # the three-bf16-piece form it replaces in the fp16x3 mode's sweep
    print('conv5x5 %d->%d @%d, x scale %s: two fp16 pieces max |err| %.2e rms %.2e of the output rms; three bf16 pieces max %.2e rms %.2e'
          % (cin, cout, H, scale, np.abs(e3).max(), np.sqrt((e3 ** 2).mean()), np.abs(ef).max(), np.sqrt((ef ** 2).mean())))
    assert np.abs(e3).max() < 2e-5 and np.sqrt((e3 ** 2).mean()) < 7e-7      # (observed up to 7.8e-6 / 5.3e-7; the K-split sums meet by atomic adds in any order)
    assert np.sqrt((e3 ** 2).mean()) < 1.5 * np.sqrt((ef ** 2).mean())
    if B < 32 and scale == 1.0 and accumulate:       # accumulate form
        acc = rs.randn(B, cout, H, Wd).astype(np.float32)
        out = ops.conv5x5_bf16(x, W, accum_into=acc.astype(np.float64), pieces='fp16x3')
        assert np.abs(out - (ref + acc)).max() < 6e-6
    if scale == 1.0 and B == 2 and cin == 128:       # an all-zero x: scale 1, zeros out
        assert np.abs(ops.conv5x5_bf16(x * 0, W, pieces='fp16x3')).max() == 0


@pytest.mark.parametrize('scale', [1.0, 1e-6, 'ragged'])
@pytest.mark.parametrize('B,cin,cout,H', [(2, 128, 64, 32), (2, 256, 96, 16), (32, 256, 192, 16), (1, 128, 128, 32), (4, 512, 192, 8), (32, 512, 192, 8)])    # 8-wide maps: the ring kernel's fp16 form (lstm5's data gradient)
def test_conv5x5_fp16x3(ops, B, cin, cout, H, scale):
    _conv5x5_fp16x3(ops, B, cin, cout, H, H, scale)


# ---- two fp16 pieces per operand, three MFMAs per product (weights packed times 2^8): 22-bit operands, forward only ---------------------------
@pytest.mark.parametrize('nch', [16, 32])
@pytest.mark.parametrize('B,cx,C,H', X6_SHAPES + [(4, 64, 128, 8), (2, 32, 32, 8), (32, 64, 128, 8)])       # 8-wide maps: the ring kernel's fp16 form
def test_convlstm_fp16x3_is_fp32_grade(ops, B, cx, C, H, nch):
    x, h, c, W, b = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(B, cx, C, H, 231 + C + H)]
    hr, cr, _ = _lstm_ref(x, h, c, W, b)
    if nch == 32 and C % 32:
        pytest.skip('32-channel blocks need C % 32 == 0')
    h3, c3 = ops.convlstm_fp16x3(x, h, c, W, b, nch=nch)
    hf, cf = ops.convlstm(x, h, c, W, b)
    e3 = max(np.abs(h3 - hr).max(), np.abs(c3 - cr).max()); ef = max(np.abs(hf - hr).max(), np.abs(cf - cr).max())
    r3 = np.sqrt(((c3 - cr) ** 2).mean()); rf = np.sqrt(((cf - cr) ** 2).mean())
    print('B=%d cx=%d C=%d H=%d nch=%d: max |err| two fp16 pieces %.2e, fp32 kernel %.2e; rms of c %.2e vs %.2e' % (B, cx, C, H, nch, e3, ef, r3, rf))
    assert e3 < 3e-6 and e3 < 2.5 * ef and r3 < 1.5 * rf


def test_convlstm_fp16x3_ranges(ops):
    # the weights' scale is chosen per tensor (largest weight into [2^14, 2^15)): tiny and huge weights alike keep 22 bits; activations of 1e3 do not overflow
    x, h, c, W, b = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(2, 32, 32, 16, 77)]
    for xs, ws in ((1e3, 1e-3), (0.25, 4.0), (1e-2, 1e2), (1e-4, 1e4)):      # the last two: pre-activations up to +-150 / +-15,000 (saturated gates)
        xx = np.asarray(x * xs, dtype=np.float32).astype(np.float64); WW = np.asarray(W * ws, dtype=np.float32).astype(np.float64)
        with np.errstate(over='ignore'):
            hr, cr, _ = _lstm_ref(xx, h, c, WW, b)
        h3, c3 = ops.convlstm_fp16x3(xx, h, c, WW, b)
        h6, c6 = ops.convlstm_bf16x6(xx, h, c, WW, b)
        hf, cf = ops.convlstm(xx, h, c, WW, b)
        # (the fp32 kernel wrote NaN cells here until round 4: its sigmoid's Newton step met exp = inf below -88)
        assert np.isfinite(h3).all() and np.isfinite(h6).all() and np.isfinite(hf).all() and np.isfinite(cf).all()
        ef = max(np.abs(cf - cr).max(), 1e-6)
        assert np.abs(c3 - cr).max() < 3 * ef and np.abs(c6 - cr).max() < 3 * ef
    h3, c3 = ops.convlstm_fp16x3(x, h, c, W, b, h_is_zero=True)
    hr, cr, _ = _lstm_ref(x, h * 0, c, W, b)
    assert np.abs(h3 - hr).max() < 3e-6 and np.abs(c3 - cr).max() < 3e-6


def test_convlstm_fp16x3_tile_forms_agree(ops):
    # 16- and 32-channel blocks: the same terms in another tap rotation; the LayerNorm partials of each epilogue; t = 0 (no h operand)
    xa, ha, ca, Wa, ba = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in _case(2, 96, 32, 32, 9)]
    h16, c16, (p16, n16) = ops.convlstm_fp16x3(xa, ha, ca, Wa, ba, nch=16, want_ln=True)
    h32, c32, (p32, n32) = ops.convlstm_fp16x3(xa, ha, ca, Wa, ba, nch=32, want_ln=True)
    assert np.abs(h16 - h32).max() < 2e-6 and np.abs(c16 - c32).max() < 2e-6
    assert n16 == 16 and n32 == 8       # tiles per image x channel blocks: 8 x 2, 8 x 1
    for pp, hh in ((p16, h16), (p32, h32)):
        cnt = pp[:, :, 0].sum(axis=1)
        mean = (pp[:, :, 0] * pp[:, :, 1]).sum(axis=1) / cnt
        var = (pp[:, :, 2] + pp[:, :, 0] * (pp[:, :, 1] - mean[:, None]) ** 2).sum(axis=1) / cnt
        assert np.allclose(cnt, 32 * 32 * 32) and np.allclose(mean, hh.reshape(2, -1).mean(axis=1), atol=1e-6)
        assert np.allclose(var, hh.reshape(2, -1).var(axis=1), rtol=1e-4)
    hr, cr, _ = _lstm_ref(xa, ha * 0, ca, Wa, ba)
    h0, c0 = ops.convlstm_fp16x3(xa, ha, ca, Wa, ba, h_is_zero=True, nch=32)
    assert np.abs(h0 - hr).max() < 3e-6 and np.abs(c0 - cr).max() < 3e-6


def test_rollout_fp16x3_is_as_close_to_float64_as_the_fp32_path():
    g = np.load(__import__('os').path.join(GOLD, 'cdna_b2_t10.npz'))
    m3, loss3, gen3 = _rollout('fp16x3')
    mf, lossf, genf = _rollout('fp32')
    l3 = R.per_pixel_l2(gen3, g['gen_images']); lf = R.per_pixel_l2(genf, g['gen_images'])
    print('fp16x3 rollout: per-pixel L2 vs float64 oracle max %.2e rms %.2e (fp32 path: max %.2e rms %.2e); loss %.8f vs %.8f'
          % (l3.max(), np.sqrt((l3 ** 2).mean()), lf.max(), np.sqrt((lf ** 2).mean()), loss3, float(g['loss'])))
    per3 = l3.reshape(l3.shape[0], -1).max(axis=1); perf = lf.reshape(lf.shape[0], -1).max(axis=1)
    assert (per3 < 2.0 * np.maximum(perf, 1e-6)).all() and abs(loss3 - float(g['loss'])) < 1e-6
    assert m3._active.lib.pivp_plan_get_precision(m3._active.h) == 4


@pytest.mark.parametrize('B', [1, 3])
def test_split_modes_with_odd_batches(B):
    """An odd batch: the 8 x 8 map of lstm5 cannot be paired into the ring kernel's two-image tiles and takes the fp32 kernel inside the plan; every other
    layer stays on the split kernels (any batch).  Both modes against the fp32 path on the same input."""
    import pivp_amd
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(B, 4)
    gens = {}
    for prec in ('fp32', 'bf16x6', 'fp16x3'):
        m = pivp_amd.Model(10, prefix='t', precision=prec)
        m.load_state_dict_reference(P)
        with pivp_amd.using_config('train', False):
            m([imgs, acts, stas], 0)
        gens[prec] = torch.stack(m.gen_images).cpu().numpy()
    for prec in ('bf16x6', 'fp16x3'):
        l2 = R.per_pixel_l2(gens[prec], gens['fp32'])
        print('B = %d, %s against the fp32 kernels: max per-pixel L2 %.2e' % (B, prec, l2.max()))
        assert np.isfinite(gens[prec]).all() and l2.max() < 2e-5


@pytest.mark.parametrize('B', [2, 32])      # 32: the 32 x 32 layers take the 32-channel blocks (a block per CU), lstm2 with the norm folded in
def test_split_modes_apply_hidden1_and_hidden3_inside_lstm2_and_lstm4(B):
    """Inference rollouts of the split modes have no ln_apply launch for hidden1 / hidden3 (the norm is applied while lstm2 / lstm4 stage their patch);
    Model.tap rebuilds the tensors on request, and they agree with the fp32 kernels' taps (whose plan keeps the separate launches)."""
    import pivp_amd
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(B, 4)
    taps = {}
    for prec in ('fp32', 'bf16x6', 'fp16x3'):
        m = pivp_amd.Model(10, prefix='t', precision=prec)
        m.load_state_dict_reference(P)
        with pivp_amd.using_config('train', False):
            m([imgs, acts, stas], 0)
        taps[prec] = {k: m.tap(k).cpu().numpy() for k in ('hidden1', 'hidden2', 'hidden3', 'hidden4', 'hidden5')}
    for prec in ('bf16x6', 'fp16x3'):
        for k, v in taps[prec].items():
            d = np.abs(v - taps['fp32'][k]).max()
            assert d < 2e-5, (prec, k, d)


def test_split_entry_points_refuse_what_they_cannot_serve():
    """The new C entry points return PIVP_ERR_BADARG (-1) for shapes their kernels do not take, before any launch."""
    lib = __import__('pivp_amd')._lib.load()
    z = torch.zeros(1 << 22, device='cuda')
    p = z.data_ptr()
    # three bf16 pieces: 8-wide map (no fp32 weights to fall back on in the per-op call), channels not a multiple of 16, bad block code
    assert lib.pivp_convlstm_bf16x6(p, 64, 64, p, 128, p, p, p, p, p, None, None, 0, None, 3, 8, 8, 0, None) == -1
    assert lib.pivp_convlstm_bf16x6(p, 32, 32, p, 24, p, p, p, p, p, None, None, 0, None, 2, 16, 16, 0, None) == -1
    assert lib.pivp_convlstm_bf16x6(p, 32, 32, p, 32, p, p, p, p, p, None, None, 0, None, 2, 16, 16, 7, None) == -1
    # two fp16 pieces: odd batch on an 8-wide map, map height not a multiple of 8, missing buffers
    assert lib.pivp_convlstm_fp16x3(p, 64, 64, p, 128, p, p, p, p, p, None, None, 0, None, 3, 8, 8, 0, None) == -1
    assert lib.pivp_convlstm_fp16x3(p, 32, 32, p, 32, p, p, p, p, p, None, None, 0, None, 2, 12, 16, 0, None) == -1
    assert lib.pivp_convlstm_fp16x3(p, 32, 32, p, 32, None, p, p, p, p, None, None, 0, None, 2, 16, 16, 0, None) == -1
    assert lib.pivp_pack_lstm_fp16x3(p, p, 64, 32, 0, None) == -1
    assert lib.pivp_conv5x5_bf16x6(p, 128, 128, p, p, p, 64, 64, 0, 3, 8, 8, None) == -1            # 8-wide map and an odd batch
    assert lib.pivp_conv5x5_fp16x3(p, 128, 128, p, p, p, 64, 64, 0, 3, 8, 8, p, None) == -1         # 8-wide map and an odd batch
    assert lib.pivp_conv5x5_fp16x3(p, 128, 256, p, p, p, 64, 64, 0, 2, 16, 16, p, None) == -1       # x not contiguous: its maximum is taken over one span
    assert lib.pivp_conv5x5_fp16x3(p, 128, 128, p, p, p, 64, 64, 0, 2, 16, 16, None, None) == -1    # no scratch for x's maxima
    assert lib.pivp_deconv3x3s2_fp16x3(p, 64, 64, p, p, p, 64, 64, 1, 2, 32, 32, None, None) == -1   # no scratch for the weights' scale
    torch.cuda.synchronize()


def test_weight_packs_are_rebuilt_when_the_parameters_change():
    """The precision modes keep their weight packs across calls (pivp_plan_set_pack_cache) while the parameters are untouched; an in-place write through
    torch (its version counter) and the optimizer's own kernel (Model._params_epoch) must both invalidate them."""
    import pivp_amd
    imgs, acts, stas = R.synthetic_batch(2, 4)
    for prec in ('fp16x3', 'bf16x6', 'bf16'):
        P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
        m = pivp_amd.Model(10, prefix='t', precision=prec, keep_activations=True)
        m.load_state_dict_reference(P)
        with pivp_amd.using_config('train', False):
            l0 = float(m([imgs, acts, stas], 0)); l0b = float(m([imgs, acts, stas], 0))
            assert l0 == l0b                                              # (second call: cached packs)
            m._params['lstm1/conv/W'].mul_(1.5)                           # an in-place write through a view of the flat buffer
            l1 = float(m([imgs, acts, stas], 0))
        assert abs(l1 - l0) > 1e-7, (prec, l0, l1)
        opt = pivp_amd.Adam(alpha=0.01).setup(m)
        opt.update(m, [imgs, acts, stas], 0)                              # the optimizer's kernel writes through raw pointers
        with pivp_amd.using_config('train', False):
            l2 = float(m([imgs, acts, stas], 0))
        fresh = pivp_amd.Model(10, prefix='t', precision=prec)
        with pivp_amd.using_config('train', False):
            fresh([imgs, acts, stas], 0)
            fresh._flat_params.copy_(m._flat_params)
            l2f = float(fresh([imgs, acts, stas], 0))
        assert l2 == l2f and abs(l2 - l1) > 1e-7, (prec, l1, l2, l2f)
        # a writer torch cannot see (dist.broadcast / all_reduce leave Tensor._version alone; here a ctypes kernel through raw pointers):
        # the caller owes Model.params_changed() (Model.broadcast_params does it), and then the next forward equals a fresh model's on those weights
        lib = m._active.lib
        v0 = m._flat_params._version
        src = (m._flat_params * 0.75).to(torch.bfloat16)
        assert lib.pivp_grad_unpack_bf16(src.data_ptr(), m._flat_params.data_ptr(), src.numel(), None) == 0
        assert m._flat_params._version == v0
        m.params_changed()
        with pivp_amd.using_config('train', False):
            l3 = float(m([imgs, acts, stas], 0))
            fresh._flat_params.copy_(m._flat_params)
            l3f = float(fresh([imgs, acts, stas], 0))
        assert l3 == l3f and abs(l3 - l2) > 1e-7, (prec, l2, l3, l3f)


def _relu_mismatches(ma, mb, steps):
    """post-ReLU activations of two models' rollouts that are zero in one and positive in the other (all ReLU layers, the first `steps` timesteps)"""
    n = 0
    for name in ('enc0', 'enc1', 'enc2', 'enc3', 'enc4', 'enc5', 'enc6'):
        for st in range(steps):
            a, b = ma.tap(name, st), mb.tap(name, st)
            a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
            b = b.cpu().numpy() if hasattr(b, 'cpu') else np.asarray(b)
            n += int(((a > 0) != (b > 0)).sum())
    return n


@pytest.mark.parametrize('B', [2, 3])       # 3: lstm5's 8-wide map cannot be paired into two-image tiles: its three kernels of the sweep are the fp32 ones
def test_train_step_in_fp16x3_mode_matches_the_fp32_gradients(B):
    import pivp_amd
    outs = {}
    for prec in ('fp32', 'fp16x3'):
        m, loss, _ = _rollout(prec, T=4, train=True, keep=True, B=B)
        with pivp_amd.using_config('train', True):
            m.backward()
        outs[prec] = (loss, m._flat_grads.clone(), m)
    rel = float((outs['fp16x3'][1] - outs['fp32'][1]).norm() / outs['fp32'][1].norm())
    flips = _relu_mismatches(outs['fp32'][2], outs['fp16x3'][2], 3)
    print('fp16x3 train step: loss %.8f vs %.8f, relative gradient difference %.2e, ReLU units on different sides of zero: %d' % (
        outs['fp16x3'][0], outs['fp32'][0], rel, flips))
    # A unit whose pre-activation is ~1e-8 sits on either side of zero from one summation order to the next, and ONE such unit of enc5 moves the whole
    # gradient by ~1e-3 (profiles/r06/NOTES.md 3: the same fp32 model against itself with two LayerNorm merge orders): the 1e-4 gate holds when the two
    # modes' ReLU patterns agree, a run in which they do not is gated at what one unit can do.
    assert abs(outs['fp16x3'][0] - outs['fp32'][0]) < 1e-6 and rel < (1e-4 if flips == 0 else 2e-3)


def test_rollout_bf16x6_is_as_close_to_float64_as_the_fp32_path():
    g = np.load(__import__('os').path.join(GOLD, 'cdna_b2_t10.npz'))
    m6, loss6, gen6 = _rollout('bf16x6')
    mf, lossf, genf = _rollout('fp32')
    l6 = R.per_pixel_l2(gen6, g['gen_images']); lf = R.per_pixel_l2(genf, g['gen_images'])
    print('bf16x6 rollout: per-pixel L2 vs float64 oracle max %.2e rms %.2e (fp32 path: max %.2e rms %.2e); loss %.8f vs %.8f'
          % (l6.max(), np.sqrt((l6 ** 2).mean()), lf.max(), np.sqrt((lf ** 2).mean()), loss6, float(g['loss'])))
    per6 = l6.reshape(l6.shape[0], -1).max(axis=1); perf = lf.reshape(lf.shape[0], -1).max(axis=1)
    assert (per6 < 2.0 * np.maximum(perf, 1e-6)).all() and abs(loss6 - float(g['loss'])) < 1e-6
    assert m6._active.lib.pivp_plan_get_precision(m6._active.h) == 3


def test_train_step_in_bf16x6_mode_matches_the_fp32_gradients():
    import pivp_amd
    outs = {}
    for prec in ('fp32', 'bf16x6'):
        m, loss, _ = _rollout(prec, T=4, train=True, keep=True)
        with pivp_amd.using_config('train', True):
            m.backward()
        outs[prec] = (loss, m._flat_grads.clone())
    rel = float((outs['bf16x6'][1] - outs['fp32'][1]).norm() / outs['fp32'][1].norm())
    print('bf16x6 train step: loss %.8f vs %.8f, relative gradient difference %.2e' % (outs['bf16x6'][0], outs['fp32'][0], rel))
    assert abs(outs['bf16x6'][0] - outs['fp32'][0]) < 1e-6 and rel < 1e-4


def test_rollout_bf16x3_stays_inside_the_gate():
    # the split mode on the config 1 golden rollout: the CPU study (scripts/split_bf16_study.py) predicts 3.2e-5 max per-pixel L2
    g = np.load(__import__('os').path.join(GOLD, 'cdna_b2_t10.npz'))
    m, loss, gen = _rollout('bf16x3')
    l2 = R.per_pixel_l2(gen, g['gen_images'])
    print('bf16x3 rollout: per-pixel L2 vs float64 oracle max %.2e rms %.2e; loss %.8f vs %.8f'
          % (l2.max(), np.sqrt((l2 ** 2).mean()), loss, float(g['loss'])))
    assert l2.max() < 1e-4 and abs(loss - float(g['loss'])) < 1e-5
    assert m._active.lib.pivp_plan_get_precision(m._active.h) == 2


def test_train_step_in_bf16x3_mode_matches_fp32_gradients():
    # split forward; in the backward the ConvLSTM data gradients run in the split form too (Modes::dgrad, csrc/plan.h), the weight gradients and everything
    # else in fp32: gradients agree with the fp32 path to the 1e-5-level differences of the split products
    import pivp_amd
    outs = {}
    for prec in ('fp32', 'bf16x3'):
        m, loss, _ = _rollout(prec, T=4, train=True, keep=True)
        with pivp_amd.using_config('train', True):
            m.backward()
        outs[prec] = (loss, m._flat_grads.clone())
    rel = float((outs['bf16x3'][1] - outs['fp32'][1]).norm() / outs['fp32'][1].norm())
    print('bf16x3 train step: loss %.8f vs %.8f, relative gradient difference %.2e' % (outs['bf16x3'][0], outs['fp32'][0], rel))
    assert abs(outs['bf16x3'][0] - outs['fp32'][0]) < 1e-5 and rel < 1e-3


@pytest.mark.parametrize('wscale', [1.0, 1e-3, 300.0])
@pytest.mark.parametrize('B,cin,cout,H', [(2, 64, 64, 32), (4, 96, 96, 16), (1, 32, 32, 64)])
def test_deconv3x3s2_fp16x3_is_fp32_grade(ops, B, cin, cout, H, wscale):
    # enc5 / enc6 in the fp16x3 mode: two fp16 pieces per operand, the weights' scale from their absolute maximum (tiny and large weights alike)
    rs = np.random.RandomState(cin + H + 3)
    x = rs.randn(B, cin, H, H).astype(np.float32).astype(np.float64)
    W = (wscale * rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin)).astype(np.float32).astype(np.float64); b = (rs.randn(cout) * 0.1).astype(np.float32).astype(np.float64)
    ref = R.relu(R.deconv2d(x, W, b, 2, 1, (2 * H, 2 * H)))
    e3 = ops.deconv3x3s2(x, W, b, True, bf16='fp16x3') - ref; ef = ops.deconv3x3s2(x, W, b, True) - ref
    print('deconv %d->%d @%d (weights x %g): two fp16 pieces max |err| %.2e rms %.2e; fp32 kernel %.2e / %.2e'
          % (cin, cout, H, wscale, np.abs(e3).max(), np.sqrt((e3 ** 2).mean()), np.abs(ef).max(), np.sqrt((ef ** 2).mean())))
    assert np.sqrt((e3 ** 2).mean()) < 1.5 * np.sqrt((ef ** 2).mean()) and np.abs(e3).max() < 2.5 * np.abs(ef).max()


@pytest.mark.parametrize('B,cin,cout,H', [(2, 64, 64, 32), (4, 96, 96, 16)])
def test_deconv3x3s2_bf16x3(ops, B, cin, cout, H):
    rs = np.random.RandomState(cin + H + 1)
    x = rs.randn(B, cin, H, H); W = rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin); b = rs.randn(cout) * 0.1
    ref = R.relu(R.deconv2d(x, W, b, 2, 1, (2 * H, 2 * H)))
    e3 = np.abs(ops.deconv3x3s2(x, W, b, True, bf16=3) - ref).max(); e1 = np.abs(ops.deconv3x3s2(x, W, b, True, bf16=True) - ref).max()
    print('deconv %d->%d @%d: max |err| split %.2e, plain bf16 %.2e' % (cin, cout, H, e3, e1))
    assert e3 < 3e-5 and e3 < e1 / 50


def _conv5x5_bf16x3(ops, B, cin, cout, H, Wd):
    # the data gradients of the split mode: 64-column blocks (four ring slots), 128-column blocks (two slots), padded columns, K split
    rs = np.random.RandomState(cin + cout + H + 5)
    x = rs.randn(B, cin, H, Wd); W = rs.randn(cout, cin, 5, 5) / np.sqrt(25 * cin)
    ref = R.conv2d(x, W, np.zeros(cout), 1, 2)
    e3 = np.abs(ops.conv5x5_bf16(x, W, split=True) - ref).max(); e1 = np.abs(ops.conv5x5_bf16(x, W) - ref).max()
    print('conv5x5 %d->%d @%d: max |err| split %.2e, plain bf16 %.2e' % (cin, cout, H, e3, e1))
    assert e3 < 5e-5 and e3 < e1 / 50


@pytest.mark.parametrize('B,cin,cout,H', [(2, 128, 64, 32), (2, 256, 96, 16), (4, 512, 192, 8), (2, 256, 128, 16), (32, 512, 192, 8)])
def test_conv5x5_bf16x3(ops, B, cin, cout, H):
    _conv5x5_bf16x3(ops, B, cin, cout, H, H)
