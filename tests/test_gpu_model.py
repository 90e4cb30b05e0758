"""GPU parity tests of the whole rollout through the reference's Model surface, against the
committed golden fixtures (float64 oracle) and against the oracle run live on small cases.
Gate: max per-pixel L2 over the colour axis < 1e-4 in fp32."""
import os

import numpy as np
import pytest

from oracle import restatement as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
GATE = 1e-4
# STP and the 1e-4 gate.  The bilinear warp multiplies an error in theta by ~63 pixels x the image gradient, and theta hangs on
# hidden5 through Linear(8192 -> 100): an rms error of 6e-7 in hidden5 (the floor of ANY float32 evaluation of this trunk: every
# ConvLSTM + LayerNorm stage adds ~3e-7, scripts/gate_math_study.py) is ~8e-7 in theta and 5e-5..1e-4 in a white-noise frame
# (scripts/debug_stp_theta.py).  The reference's own arithmetic shows it: the float32 NumPy oracle is 1.1e-4 (max over 32 samples)
# from the float64 oracle on the FIRST step of tests/golden/stp_b32_t10.npz and 2.3e-3 after nine fed-back steps.  So for STP:
#  * the 1e-4 gate applies where plain float32 meets it with margin: frames with the smoothness of video while they are ground truth
#    (test_stp_smooth_frames, test_config4_stp_batch32[smooth] steps 0-1), and the ground-truth-fed steps of the white-noise fixture;
#  * everywhere else the HIP path is held to "no less accurate than plain float32 on the same pixels" over 32 samples x 9 steps
#    (test_config4_stp_batch32), which is a statement about the kernels rather than about one draw of a theta error.
STP_VS_FP32_PER_STEP = 1.35     # rms over 32 samples of one step: HIP <= 1.35 x float32 oracle (32 draws: ~ +-15 % noise)
STP_VS_FP32_OVERALL = 1.10      # geometric mean of the nine per-step ratios
STP_VS_FP32_MAX = 3.0           # per step, the largest error over the sampled pixels: HIP <= 3 x the float32 oracle's largest on the same
                                # pixels.  An rms over 32 samples barely sees a localised kernel error (a tile tail, an edge tap: a few
                                # pixels at 1e-3); the maximum does.  3x: the step's maximum is ONE sample's draw of a theta error.


@pytest.fixture(scope='module')
def pivp():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def _run(pivp, mt, nm, imgs, acts, stas, P, train=False, k=-1, it=0, **kw):
    import torch
    m = pivp.Model(nm, is_cdna=mt == 'CDNA', is_stp=mt == 'STP', is_dna=mt == 'DNA', prefix='test',
                   scheduled_sampling_k=k, **kw)
    m.load_state_dict_reference(P)
    with pivp.using_config('train', train):
        loss = m([imgs, acts, stas], it)
    return m, float(loss), torch.stack(m.gen_images).cpu().numpy()


@pytest.mark.parametrize('precision', ['fp32', 'bf16x6', 'fp16x3'])      # the two split modes are held to the SAME gates as the fp32 kernels
@pytest.mark.parametrize('name,mt,nm', [('cdna_b2_t10', 'CDNA', 10), ('stp_b2_t4', 'STP', 10), ('dna_b2_t4', 'DNA', 1)])
def test_rollout_matches_golden(pivp, name, mt, nm, precision):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    B, T = int(g['batch']), int(g['seq_len'])
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=nm, model_type=mt)
    imgs, acts, stas = R.synthetic_batch(B, T)
    m, loss, gen = _run(pivp, mt, nm, imgs, acts, stas, P, precision=precision)
    l2 = R.per_pixel_l2(gen, g['gen_images'])
    print('%s (%s): max per-pixel L2 %.3e, rms %.3e, loss %.8f vs %.8f' % (name, precision, l2.max(), np.sqrt((l2 ** 2).mean()), loss, float(g['loss'])))
    ctx = 2                                                     # frames 0, 1 are ground truth; later ones are fed back
    assert l2[:ctx].max() < GATE
    if mt != 'STP':                                             # STP fed-back steps: see the note at the top and test_config4_stp_batch32
        assert l2.max() < GATE
    else:
        # White-noise frames put plain float32 itself within a factor of two of the gate (note at the top), so the absolute gate alone would let a
        # summation-order change pass or fail by a few per cent.  The statement that fails loudly: on these frames the HIP path is no less accurate than
        # the float32 evaluation of the reference's arithmetic (the NumPy oracle in float32), ground-truth-fed steps and all steps, printed side by side.
        ref32 = R.Model(nm, is_cdna=False, is_stp=True, params=P, dtype=np.float32, prefix='x'); ref32.train = False
        ref32([imgs, acts, stas], 0)
        l32 = R.per_pixel_l2(np.stack(ref32.gen_images), g['gen_images'])
        print('%s (%s): max per-pixel L2, ground-truth-fed steps %.3e (float32 oracle %.3e), all steps %.3e (float32 oracle %.3e)'
              % (name, precision, l2[:ctx].max(), l32[:ctx].max(), l2.max(), l32.max()))
        assert l2[:ctx].max() < max(5e-5, 1.5 * l32[:ctx].max()) and l2.max() < max(5e-5, 2.0 * l32.max())
    assert np.sqrt((l2 ** 2).mean()) < 2e-5
    assert abs(loss - float(g['loss'])) < 1e-5
    assert abs(float(m.psnr_all) - float(g['psnr_all'])) < 1e-2
    import torch
    gs = torch.stack(m.gen_states).cpu().numpy()
    assert np.abs(gs - g['gen_states']).max() < 1e-5
    # last-step taps (T-2) against the fixture's strided samples
    last = T - 2
    for tap in ('enc0', 'enc1', 'enc2', 'enc3', 'enc4', 'enc5', 'enc6', 'enc7', 'hidden5', 'masks'):
        key = 'tap%d_%s' % (last, tap)
        if key in g.files:
            got = m.tap(tap).cpu().numpy().ravel()[::97]
            assert np.abs(got - g[key]).max() < 5e-4, tap
    res = m.conv_res
    assert len(res) == 8 and tuple(res[6].shape) == (B, 64, 64, 64)
    summ = m.summaries
    assert len(summ) == 3 * (T - 2) + 2 and summ[0].startswith('test_recon_cost0: ') and summ[-1].startswith('test_loss: ')


def test_stp_smooth_frames(pivp):
    # frames with video-like smoothness (box-blurred noise): the 1e-4 gate holds for STP
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, model_type='STP')
    imgs, acts, stas = R.synthetic_batch(2, 4)
    from numpy.lib.stride_tricks import sliding_window_view
    pad = np.pad(imgs, ((0, 0), (0, 0), (0, 0), (5, 5), (5, 5)), mode='reflect')
    imgs = np.ascontiguousarray(sliding_window_view(pad, (11, 11), axis=(3, 4)).mean(axis=(-1, -2))).astype(np.float32)
    assert imgs.shape[-2:] == (64, 64)
    ref = R.Model(10, is_cdna=False, is_stp=True, params=P, dtype=np.float64, prefix='x'); ref.train = False
    ref([imgs, acts, stas], 0)
    m, loss, gen = _run(pivp, 'STP', 10, imgs, acts, stas, P)
    l2 = R.per_pixel_l2(gen, np.stack(ref.gen_images))
    print('stp smooth: max per-pixel L2 %.3e' % l2.max())
    assert l2.max() < GATE


def test_default_init_runs_and_reset_state(pivp):
    import torch
    imgs, acts, stas = R.synthetic_batch(2, 4)
    np.random.seed(3)
    m = pivp.Model(10, prefix='x')
    with pivp.using_config('train', False):
        l1 = float(m([imgs, acts, stas], 0))
        g1 = torch.stack(m.gen_images).clone()
        m.reset_state()
        assert m.loss == 0.0 and m.psnr_all == 0.0 and m.summaries == [] and m.conv_res == []
        l2 = float(m([imgs, acts, stas], 0))
        g2 = torch.stack(m.gen_images)
    assert l1 == l2 and torch.equal(g1, g2)                  # deterministic, state fully reset
    assert m.count_params() == 9212159
    assert np.isfinite(l1)


def test_checkpoint_roundtrip_reference_layout(pivp, tmp_path):
    import torch
    P = R.init_params(seed=5, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(2, 3)
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)
    path = str(tmp_path / 'training-0')                      # the reference writes files without extension (TM:1035)
    pivp.save_npz(path, m)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(P.keys())
        for k in P:
            assert z[k].shape == P[k].shape and np.array_equal(z[k], P[k]), k
    m2 = pivp.Model(10, prefix='test')
    pivp.load_npz(path, m2)                                  # before the first call: lazily bound like chainer
    with pivp.using_config('train', False):
        loss2 = float(m2([imgs, acts, stas], 0))
    assert loss2 == loss and np.array_equal(torch.stack(m2.gen_images).cpu().numpy(), gen)


def test_scheduled_sampling_matches_oracle(pivp):
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(4, 5)
    ref = R.Model(10, params=P, dtype=np.float64, prefix='x', scheduled_sampling_k=2.0)
    np.random.seed(21)
    ref([imgs, acts, stas], 1.0)
    np.random.seed(21)
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, train=True, k=2.0, it=1.0)
    assert R.per_pixel_l2(gen, np.stack(ref.gen_images)).max() < GATE
    assert abs(loss - float(ref.loss)) < 1e-5
    # eval mode ignores the schedule (TM:649)
    _, loss_eval, gen_eval = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, train=False, k=2.0, it=1.0)
    ref2 = R.Model(10, params=P, dtype=np.float64, prefix='x', scheduled_sampling_k=2.0); ref2.train = False
    ref2([imgs, acts, stas], 1.0)
    assert R.per_pixel_l2(gen_eval, np.stack(ref2.gen_images)).max() < GATE


def test_use_state_false_and_keep_activations(pivp):
    P = R.init_params(seed=2, dtype=np.float32, scale=1.0, use_state=False)
    imgs, acts, stas = R.synthetic_batch(2, 4)
    ref = R.Model(10, params=P, dtype=np.float64, prefix='x', use_state=False); ref.train = False
    ref([imgs, acts, stas], 0, tap_steps=(0, 1, 2))
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, use_state=False, keep_activations=True)
    assert R.per_pixel_l2(gen, np.stack(ref.gen_images)).max() < GATE
    for step in (0, 1, 2):                                   # every timestep's activations are retained
        for tap in ('enc0', 'enc3', 'hidden5', 'enc5', 'enc6', 'hidden7'):
            got = m.tap(tap, step).cpu().numpy()
            assert np.abs(got - ref.taps[step][tap]).max() < 5e-4, (step, tap)


def test_inference_taps_of_norms_applied_inside_their_consumers(pivp):
    # an inference plan applies norm(hidden2) / norm(hidden4) while enc1 / enc2 stage their input and norm(hidden6) / norm(hidden7) while
    # enc5 / enc6 stage theirs (run_conv3x3s2_ln, run_deconv3x3s2_ln: no ln_apply launch, the normalised tensor is never written); the
    # consumers must equal the oracle's, and tap() rebuilds the four hidden tensors on request.  B = 4: enough tiles for enc5's tile kernel.
    P = R.init_params(seed=3, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(4, 4)
    ref = R.Model(10, params=P, dtype=np.float64, prefix='x'); ref.train = False
    ref([imgs, acts, stas], 0, tap_steps=(2,))
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)              # keep_activations = False
    assert R.per_pixel_l2(gen, np.stack(ref.gen_images)).max() < GATE
    for tap in ('enc1', 'enc2', 'enc5', 'enc6', 'hidden2', 'hidden4', 'hidden5', 'hidden6', 'hidden7'):
        got = m.tap(tap).cpu().numpy()
        assert np.abs(got - ref.taps[2][tap]).max() < 5e-4, tap


@pytest.mark.parametrize('H,W', [(16, 16), (24, 40)])
def test_inference_taps_where_the_norms_are_not_folded(pivp, H, W):
    """Frame sizes on which an inference plan applies none of the norms of hidden2 / hidden4 inside enc1 / enc2 (StepForm rules the fold out from the
    geometry): tap() then returns the tensor the step wrote and the model used, not a rebuild.  Every tap is held to the float64 oracle at the gate of the
    test above; hidden2 / hidden4 are bit-equal to those of a training plan without 'ln_fold_train', whose ln_apply launches are the same ones."""
    B, T = 3, 4
    P = R.init_params(seed=3, dtype=np.float32, scale=1.0, height=H, width=W)
    imgs, acts, stas = R.synthetic_batch(B, T, height=H, width=W)
    ref = R.Model(10, params=P, dtype=np.float64, prefix='x'); ref.train = False
    ref([imgs, acts, stas], 0, tap_steps=(T - 2,))
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)              # keep_activations = False
    assert R.per_pixel_l2(gen, np.stack(ref.gen_images)).max() < GATE
    got = {}
    for tap in ['hidden%d' % j for j in range(1, 8)] + ['enc1', 'enc2', 'enc5', 'enc6']:
        got[tap] = m.tap(tap).cpu().numpy()
        err = np.abs(got[tap] - ref.taps[T - 2][tap]).max()
        print('%dx%d %s: max abs difference from the float64 oracle %.3e' % (H, W, tap, err))
        assert err < 5e-4, tap
    mt, _, _ = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, keep_activations=True, plan_options={'ln_fold_train': 0})
    for tap in ('hidden2', 'hidden4'):
        assert np.array_equal(mt.tap(tap, T - 2).cpu().numpy(), got[tap]), tap


def test_profile_record_of_a_rollout(pivp):
    """pivp_plan_set_profiling: a rollout of T - 1 = 3 steps leaves three timed launches per ConvLSTM cell -- one without the h half of K, two full ones, in
    executed flops -- and reading the record empties it."""
    import ctypes
    B, T, H, W = 2, 4, 16, 16
    P = R.init_params(seed=3, dtype=np.float32, scale=1.0, height=H, width=W)
    imgs, acts, stas = R.synthetic_batch(B, T, height=H, width=W)
    m, _, _ = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)
    plan = m._active
    ms, n, fl = (ctypes.c_double * 7)(), (ctypes.c_int * 7)(), (ctypes.c_double * 7)()
    assert plan.lib.pivp_plan_set_profiling(plan.h, 1) == 0
    try:
        with pivp.using_config('train', False):
            m([imgs, acts, stas], 0)
        import torch
        torch.cuda.synchronize()
        assert plan.lib.pivp_plan_profile_read(plan.h, ms, n, fl) == 0
        cells = [(32, 32, 2), (32, 32, 2), (32, 64, 4), (64, 64, 4), (64, 128, 8), (128, 64, 4), (96, 32, 2)]      # (cx, C, pyramid level) of lstm1..lstm7
        for i, (cx, C, lv) in enumerate(cells):
            M = B * (H // lv) * (W // lv)
            first, full = 2.0 * M * 4 * C * 25 * cx, 2.0 * M * 4 * C * 25 * (cx + C)
            assert n[i] == 3 and ms[i] > 0.0 and fl[i] == first + 2 * full, (i, n[i], ms[i], fl[i])
        assert plan.lib.pivp_plan_profile_read(plan.h, ms, n, fl) == 0
        assert list(n) == [0] * 7 and list(ms) == [0.0] * 7 and list(fl) == [0.0] * 7
    finally:
        assert plan.lib.pivp_plan_set_profiling(plan.h, 0) == 0


def test_batch32_properties(pivp):
    """Full-size batch (config 2: B=32, T=10): size-independent properties instead of the slow oracle.
    (a) samples are independent: rows of a B=32 run equal the same sequences run as B=2;
    (b) a sample duplicated inside the batch yields bit-identical frames;
    (c) outputs are finite and the loss equals the mean of per-frame costs recomputed on the host."""
    import torch
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(32, 10)
    imgs[:, 7] = imgs[:, 3]; acts[:, 7] = acts[:, 3]; stas[:, 7] = stas[:, 3]
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)
    assert np.isfinite(gen).all()
    assert np.array_equal(gen[:, 7], gen[:, 3])
    _, _, gen2 = _run(pivp, 'CDNA', 10, imgs[:, 2:4], acts[:, 2:4], stas[:, 2:4], P)
    assert R.per_pixel_l2(gen[:, 2:4], gen2).max() < 2e-5
    gs = torch.stack(m.gen_states).cpu().numpy()
    fr = [np.mean((imgs[t + 2].astype(np.float64) - gen[t + 1]) ** 2) for t in range(8)]
    st = [np.mean((stas[t + 2].astype(np.float64) - gs[t + 1]) ** 2) * 1e-4 for t in range(8)]
    assert abs(loss - (sum(fr) + sum(st)) / 8.0) < 1e-6


def _sampled_pixels(gen, stride):
    """(T-1, B, 3, H, W) -> every stride-th pixel of the flat (t, b, y, x) order, colours last (tests/golden/make_golden.py)."""
    return np.ascontiguousarray(gen.transpose(0, 1, 3, 4, 2)).reshape(-1, 3)[::stride]


@pytest.mark.parametrize('precision', ['fp32', 'bf16x6', 'fp16x3'])
def test_config2_batch32_matches_golden(pivp, precision):
    """BASELINE.json config 2 at full size (B = 32, T = 10, CDNA) against the float64 oracle's committed fixture: the fp32 kernels, and the two split
    modes (fp32 operands as three bf16 / two fp16 pieces on the matrix cores) at the same 1e-4 gate."""
    import torch
    g = np.load(os.path.join(GOLD, 'cdna_b32_t10.npz'))
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(32, 10)
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, precision=precision)
    pix = _sampled_pixels(gen, int(g['pixel_stride']))
    l2 = np.sqrt(((pix.astype(np.float64) - g['gen_pixels']) ** 2).sum(axis=1))
    print('config 2 (B=32, %s): max per-pixel L2 %.3e over %d sampled pixels, loss %.8f vs %.8f' % (precision, l2.max(), l2.size, loss, float(g['loss'])))
    assert l2.max() < GATE
    assert abs(loss - float(g['loss'])) < 1e-5
    assert abs(float(m.psnr_all) - float(g['psnr_all'])) < 1e-2
    assert np.abs(torch.stack(m.gen_states).cpu().numpy() - g['gen_states']).max() < 1e-5
    assert np.abs(gen.mean(axis=(2, 3, 4), dtype=np.float64) - g['frame_mean']).max() < 1e-6   # every (step, sample), all pixels


@pytest.mark.parametrize('name', ['stp_b32_t10', 'stp_b32_t10_smooth'])
def test_config4_stp_batch32(pivp, name):
    """BASELINE.json config 4 (STP, B = 32, T = 10) against the float64 oracle's fixture, which also holds the float32 oracle's
    error on the same pixels: see the note on STP at the top of this file."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    smooth = bool(int(g['smooth']))
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, model_type='STP')
    imgs, acts, stas = (R.smooth_batch if smooth else R.synthetic_batch)(32, 10)
    m, loss, gen = _run(pivp, 'STP', 10, imgs, acts, stas, P)
    pix = _sampled_pixels(gen, int(g['pixel_stride']))
    l2 = np.sqrt(((pix.astype(np.float64) - g['gen_pixels']) ** 2).sum(axis=1))
    ref32 = g['fp32_oracle_pixels_l2'].astype(np.float64)
    n = (l2.size // 9) * 9                                       # flat order is step-major: nine equal slabs (up to the stride's remainder)
    rms = lambda v: np.sqrt((v[:n].reshape(9, -1) ** 2).mean(axis=1))
    mx = lambda v: v[:n].reshape(9, -1).max(axis=1)
    r_hip, r_32 = rms(l2), rms(ref32)
    ratio = r_hip / r_32
    print(name, 'per-step rms HIP', ['%.1e' % v for v in r_hip], 'fp32 oracle', ['%.1e' % v for v in r_32])
    print(name, 'per-step max HIP', ['%.1e' % v for v in mx(l2)], 'fp32 oracle', ['%.1e' % v for v in mx(ref32)])
    print(name, 'rms ratio HIP / fp32 oracle per step', ['%.2f' % v for v in ratio], 'geometric mean %.3f' % np.exp(np.log(ratio).mean()))
    assert np.isfinite(gen).all()
    assert (ratio < STP_VS_FP32_PER_STEP).all()
    assert np.exp(np.log(ratio).mean()) < STP_VS_FP32_OVERALL
    assert (mx(l2) < STP_VS_FP32_MAX * mx(ref32)).all()
    print(name, 'max over all steps: HIP %.3e, float32 oracle %.3e' % (mx(l2).max(), mx(ref32).max()))
    if smooth:
        assert mx(l2)[:2].max() < 5e-5                           # ground-truth-fed steps of video-like frames: 2.8e-6 measured, half the 1e-4 gate asked
    assert abs(loss - float(g['loss'])) < 1e-5


def test_frame_size_128_generalisation(pivp):
    # BASELINE.json config 5 needs outsize = 2*in (the reference hard-codes 16/32/64, TM:505-507)
    P = R.init_params(seed=1, dtype=np.float32, scale=1.0, height=128, width=128)
    imgs, acts, stas = R.synthetic_batch(1, 3, 128, 128)
    ref = R.Model(10, params=P, dtype=np.float64, prefix='x'); ref.train = False
    ref([imgs, acts, stas], 0)
    m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P)
    assert R.per_pixel_l2(gen, np.stack(ref.gen_images)).max() < GATE
    assert m.count_params() == 18059519


@pytest.mark.parametrize('mt,nm', [('CDNA', 4), ('CDNA', 2), ('STP', 3)])
def test_other_mask_counts(pivp, mt, nm):
    # num_masks is a constructor argument of the reference (TM:484); the flat softmax groups are then nm+1 wide
    P = R.init_params(seed=3, dtype=np.float32, scale=1.0, num_masks=nm, model_type=mt)
    imgs, acts, stas = R.synthetic_batch(3, 4)
    ref = R.Model(nm, params=P, dtype=np.float64, prefix='x', is_cdna=mt == 'CDNA', is_stp=mt == 'STP'); ref.train = False
    ref([imgs, acts, stas], 0)
    m, loss, gen = _run(pivp, mt, nm, imgs, acts, stas, P)
    l2 = R.per_pixel_l2(gen, np.stack(ref.gen_images))
    assert l2[:2].max() < GATE                                 # ground-truth-fed steps
    if mt == 'STP':                                            # fed-back step of white-noise frames: not worse than plain float32 (note at the top)
        r32 = R.Model(nm, params=P, dtype=np.float32, prefix='x', is_cdna=False, is_stp=True); r32.train = False
        r32([imgs, acts, stas], 0)
        l32 = R.per_pixel_l2(np.stack(r32.gen_images), np.stack(ref.gen_images))
        print('STP-%d: HIP max %.2e rms %.2e | fp32 oracle max %.2e rms %.2e' % (nm, l2.max(), np.sqrt((l2 ** 2).mean()), l32.max(), np.sqrt((l32 ** 2).mean())))
        assert np.sqrt((l2 ** 2).mean()) < 1.5 * np.sqrt((l32 ** 2).mean())
    else:
        assert l2.max() < GATE
    assert abs(loss - float(ref.loss)) < 1e-5


@pytest.mark.parametrize('mt,nm', [('CDNA', 10), ('CDNA', 3), ('STP', 10)])
@pytest.mark.parametrize('train', [False, True])
def test_motion_finisher_behind_enc5_is_bit_identical(pivp, mt, nm, train):
    """Round 6: the motion head's finisher (sum of the Linear's K-slice partials, bias, activation, normalisation: TM:326-329 / 458-468) runs as B "rider"
    blocks behind enc5's tiles instead of inside each of frame_head's 16 bands per sample (plan option 'finish_rider').
    Same arithmetic in the same order: frames and loss are bit-identical with the switch off; in training mode the gradients agree to the
    last bits the sweep's atomics leave undetermined."""
    B, T = 3, 4
    P = R.init_params(seed=5, dtype=np.float32, scale=1.0, num_masks=nm, model_type=mt)
    imgs, acts, stas = R.synthetic_batch(B, T)
    out = {}
    for rider in ('1', '0'):
        m, loss, gen = _run(pivp, mt, nm, imgs, acts, stas, P, train=train, keep_activations=train, plan_options={'finish_rider': int(rider)})
        assert m.effective_plan_options()['finish_rider'] == int(rider)
        grads = None
        if train:
            m.cleargrads(); m.backward()
            grads = m.grads_reference()
        out[rider] = (loss, gen, grads)
    assert out['1'][0] == out['0'][0] and np.array_equal(out['1'][1], out['0'][1])
    if train:
        for k in out['1'][2]:
            a, b = np.asarray(out['1'][2][k]), np.asarray(out['0'][2][k])
            assert np.abs(a - b).max() <= 2e-5 * max(1e-30, np.abs(a).max()), k


@pytest.mark.parametrize('mt,nm,use_state', [('CDNA', 10, True), ('CDNA', 10, False), ('STP', 10, True), ('DNA', 1, True)])
def test_group3_in_enc2s_epilogue_is_bit_identical(pivp, mt, nm, use_state):
    """Round 6: in inference plans the smear + 1x1 conv + ReLU of group 3 (TM:598) and the state predictor (TM:730) run in the
    epilogue of enc2's launch (plan option 'fuse_enc3') -- the same fmaf chain on the matrix cores: frames, predicted states and
    loss are bit-identical to the two-launch form."""
    import torch
    B, T = 3, 4
    P = R.init_params(seed=7, dtype=np.float32, scale=1.0, num_masks=nm, model_type=mt, use_state=use_state)
    imgs, acts, stas = R.synthetic_batch(B, T)
    out = {}
    for fuse in ('1', '0'):
        m, loss, gen = _run(pivp, mt, nm, imgs, acts, stas, P, use_state=use_state, plan_options={'fuse_enc3': int(fuse)})
        assert m.effective_plan_options()['fuse_enc3'] == int(fuse)
        out[fuse] = (loss, gen, torch.stack(m.gen_states).cpu().numpy())
    assert out['1'][0] == out['0'][0] and np.array_equal(out['1'][1], out['0'][1]) and np.array_equal(out['1'][2], out['0'][2])


def test_training_plans_apply_the_norms_of_hidden2_and_hidden4_inside_enc1_and_enc2(pivp):
    """Round 6: in training plans too enc1 / enc2's launches apply the LayerNorm of their input while staging it -- and WRITE the normalised tensor and the
    samples' (mean, rstd) that the backward sweep reads (plan option 'ln_fold_train' 0: the two ln_apply launches per timestep, as before).  The expression is
    ln_apply's: frames and loss bit-identical, gradients equal to the last bits the sweep's atomics leave undetermined."""
    B, T = 3, 4
    P = R.init_params(seed=11, dtype=np.float32, scale=1.0)
    imgs, acts, stas = R.synthetic_batch(B, T)
    out = {}
    for fold in ('1', '0'):
        m, loss, gen = _run(pivp, 'CDNA', 10, imgs, acts, stas, P, train=True, keep_activations=True, plan_options={'ln_fold_train': int(fold)})
        assert m.effective_plan_options()['ln_fold_train'] == int(fold)
        m.cleargrads(); m.backward()
        out[fold] = (loss, gen, m.grads_reference())
    assert out['1'][0] == out['0'][0] and np.array_equal(out['1'][1], out['0'][1])
    for k in out['1'][2]:
        a, b = np.asarray(out['1'][2][k]), np.asarray(out['0'][2][k])
        assert np.abs(a - b).max() <= 2e-5 * max(1e-30, np.abs(a).max()), k
