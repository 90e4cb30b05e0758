"""GPU tests of open-loop prediction with designated-pixel tracking: `Model.imagine` / pivp_rollout_predict / pivp_pixel_track.

Bounds.  Frames are compared bit for bit with `__call__` (the same run_step sequence).  The tracking kernel is compared (a) per op with
pivp_composite(prev = planes, layer0 = 0), the validated kernel that computes the same linear map with the same functions, bit for bit, and (b) over
rollouts with the float64 restatement tests/track_reference.py at ten times max(float32-oracle error, 1e-6) per step -- the form of
tests/test_gpu_trained.py:70.  tests/test_imagine_host.py checks on the oracle alone that the float32 oracle is within 1e-6 there and which
cases keep a plane maximum of 1e-3 on every step (the six-frame STP case does not: see there; it is gated all the same)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
CODE = {'CDNA': 0, 'STP': 1, 'DNA': 2}


def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return torch, pivp_amd


def _model(pivp_amd, model_type, nm, P, **kw):
    m = pivp_amd.Model(nm, is_cdna=model_type == 'CDNA', is_stp=model_type == 'STP', is_dna=model_type == 'DNA', prefix='t', **kw)
    m.load_state_dict_reference(P)
    return m


def _random_params(model_type, size=64, seed=4):
    nm = 1 if model_type == 'DNA' else 10
    return R.init_params_widened(seed=seed, scale=1.0, num_masks=nm, model_type=model_type, height=size, width=size), nm


SAME_FRAMES = [('CDNA', 'random', 64, 'fp32'), ('STP', 'random', 64, 'fp32'), ('DNA', 'random', 64, 'fp32'),
               ('CDNA', 'trained', 64, 'fp32'), ('STP', 'trained', 64, 'fp32'), ('DNA', 'trained', 64, 'fp32'),
               ('CDNA', 'random', 128, 'fp32'),         # frames wider than 64 take the separate heads + composite launches
               ('CDNA', 'random', 64, 'bf16x3')]        # a precision mode: the forward is its own, the tracking kernel fp32


@pytest.mark.parametrize('model_type,weights,size,precision', SAME_FRAMES, ids=['-'.join(map(str, c)) for c in SAME_FRAMES])
def test_imagine_gives_the_frames_of_a_feed_self_call(model_type, weights, size, precision):
    torch, pivp_amd = _gpu()
    P, nm = TR.load_trained(model_type) if weights == 'trained' else _random_params(model_type, size)
    T = 6 if size == 64 else 4
    imgs, acts, stas = R.moving_batch(2, T, size, size, seed=31)
    # scheduled sampling configured and config.train left on: imagine ignores both
    m = _model(pivp_amd, model_type, nm, P, keep_activations=False, precision=precision, scheduled_sampling_k=900.0)
    with pivp_amd.using_config('train', False):
        m([imgs, acts, stas], 0)
    gen0, st0 = torch.stack(m.gen_images).clone(), torch.stack(m.gen_states).clone()
    loss0 = float(m.loss)
    assert torch.isfinite(gen0).all()
    ctx_imgs, actions, state0 = np.asarray(imgs)[:2], np.asarray(acts)[:T - 1], np.asarray(stas)[0]
    m.reset_state()
    gen = m.imagine(ctx_imgs, actions, state0)
    assert gen.shape == (T - 1, 2, 3, size, size) and m.pixel_distrib is None and m.pixel_mass is None
    assert torch.equal(gen, gen0) and torch.equal(torch.stack(m.gen_images), gen0) and torch.equal(torch.stack(m.gen_states), st0)
    assert m.summaries == [] and float(m.loss) == 0.0                   # reset_state cleared them, imagine left them alone
    planes = np.random.RandomState(1).rand(2, 3, size, size).astype(np.float32)
    for f in (None, 0):
        m.reset_state()
        gen = m.imagine(ctx_imgs, actions, state0, designated=planes, designated_frame=f)
        assert torch.equal(gen, gen0) and torch.equal(torch.stack(m.gen_states), st0)      # tracking does not disturb the frames
        assert m.pixel_distrib.shape == (T - 1 - (1 if f is None else 0), 2, 3, size, size) and torch.isfinite(m.pixel_distrib).all()
    # device tensors are taken as they are
    m.reset_state()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(m.device)
    assert torch.equal(m.imagine(dev(ctx_imgs), dev(actions), dev(state0)), gen0)
    with pivp_amd.using_config('train', False):
        assert float(m([imgs, acts, stas], 0)) == loss0


def _softmax_inputs(rs, B, NM, H, W):
    return (rs.randn(B, NM + 1, H, W) * 1.5).clip(0, None).astype(np.float32)     # mask logits are post-ReLU (TM:719)


def _aux(rs, model_type, B, NM, H, W):
    if model_type == 'CDNA':
        k = rs.rand(B, NM, 5, 5) ** 3 + 1e-12
        return (k / k.sum(axis=(2, 3), keepdims=True)).astype(np.float32)
    if model_type == 'STP':
        th = np.tile(np.array([[1.0, 0, 0, 0, 1.0, 0]]), (B, 1)) + rs.randn(B, 6) * 0.05
        th[-1] += np.array([0.1, 0.2, 0.6, -0.2, 0.1, -0.5])             # one sample samples far outside the frame: the border rule
        return th.astype(np.float32)
    return (rs.randn(B, 25, H, W)).clip(0, None).astype(np.float32)


PER_OP = [(mt, nm, H, W, z) for mt in ('CDNA', 'STP') for nm in (1, 5, 10) for (H, W) in ((64, 64), (32, 128), (30, 72))
          for z in ((0, 1) if mt == 'STP' else (0,))] + [('DNA', 1, H, W, 0) for (H, W) in ((64, 64), (32, 128), (30, 72))]


@pytest.mark.parametrize('model_type,NM,H,W,stp_zero', PER_OP, ids=['%s-nm%d-%dx%d-z%d' % c for c in PER_OP])
def test_pixel_track_against_composite(model_type, NM, H, W, stp_zero):
    """pivp_pixel_track(D, masks_out of pivp_composite, aux) against pivp_composite(prev = D, logits, layer0 = 0, aux): independent of the new host
    code.  Eight planes against the three-channel kernel in three chunks; (30, 72): a last band of two rows and a width that is no power of two."""
    _gpu()
    import hip_ops as ops
    import track_ops
    rs = np.random.RandomState(NM * 1000 + H + W + stp_zero)
    B = 3
    D = rs.rand(B, 8, H, W).astype(np.float32)
    D[:, 1] = 0; D[:, 1, H // 2, W // 2] = 1.0                        # a one-hot among them
    logits, aux = _softmax_inputs(rs, B, NM, H, W), _aux(rs, model_type, B, NM, H, W)
    code = CODE[model_type]
    zeros = np.zeros((B, 3, H, W), np.float32) if model_type != 'DNA' else None
    got = None
    worst, same = 0.0, True
    for c0 in (0, 3, 5):
        want, masks = ops.composite(D[:, c0:c0 + 3], logits, zeros, aux, NM, code, stp_zero)
        if got is None:
            got = track_ops.pixel_track(D, masks, aux, NM, code, stp_zero)
            again = track_ops.pixel_track(D, masks, aux, NM, code, stp_zero)
            assert np.array_equal(got, again)                          # no atomics: the same bits every launch
            one = track_ops.pixel_track(D[:, 4:5], masks, aux, NM, code, stp_zero)
            assert np.array_equal(one[:, 0], got[:, 4])                # a plane's arithmetic does not depend on P
        worst = max(worst, float(np.abs(got[:, c0:c0 + 3].astype(np.float64) - want).max()))
        same = same and np.array_equal(got[:, c0:c0 + 3], want)
    print(model_type, NM, H, W, stp_zero, 'max |pixel_track - composite| = %.2e, plane max %.2f' % (worst, got.max()))
    assert np.isfinite(got).all() and got.min() >= 0
    assert same, worst      # equal bits: the two kernels call the same functions (csrc/frame_transform.h) and layer0 = 0 adds an exact zero


def test_pixel_track_refuses_what_it_does_not_serve():
    _gpu()
    import track_ops
    rs = np.random.RandomState(0)
    B, NM, H, W = 2, 10, 64, 64
    D = rs.rand(B, 8, H, W).astype(np.float32)
    masks = np.full((B, NM + 1, H, W), 1.0 / (NM + 1), np.float32)
    aux = _aux(rs, 'CDNA', B, NM, H, W)
    assert track_ops.pixel_track_rc(D, masks, aux, NM, 0)[0] == 0
    for kw in (dict(P=0), dict(P=9), dict(P=-1), dict(alias=True), dict(null='planes'), dict(null='masks'), dict(null='aux'), dict(null='out')):
        assert track_ops.pixel_track_rc(D, masks, aux, NM, 0, **kw)[0] == -1, kw
    assert track_ops.pixel_track_rc(D, masks, aux, 12, 0)[0] == -1                      # more masks than pivp_composite takes
    assert track_ops.pixel_track_rc(D, masks, aux, NM, 3)[0] == -1                      # no such head
    assert track_ops.pixel_track_rc(D, masks, aux, NM, 2)[0] == -1                      # DNA has one mask (TM:389-390)
    wide = np.zeros((1, 1, 8, 256), np.float32)
    assert track_ops.pixel_track_rc(wide, np.zeros((1, 2, 8, 256), np.float32), np.zeros((1, 6), np.float32), 1, 1)[0] == -1   # W + 4 > 256


@pytest.mark.parametrize('model_type,T,planes,keeps_signal', TR.ROLLOUT_CASES, ids=['%s-T%d' % (c[0], c[1]) for c in TR.ROLLOUT_CASES])
def test_rollout_tracking_against_float64(model_type, T, planes, keeps_signal):
    torch, pivp_amd = _gpu()
    P, nm = TR.load_trained(model_type)
    batch = R.moving_batch(2, T, 64, 64, seed=123)
    imgs, acts, stas = (np.asarray(a) for a in batch)
    rs = np.random.RandomState(8)
    D8 = np.concatenate([planes(2), rs.rand(2, 5, 64, 64) * (rs.rand(2, 5, 64, 64) < 0.02)], axis=1)     # P = 8: the three planes + sparse random ones
    m64 = TR.run_oracle(P, model_type, nm, batch, np.float64)
    m32 = TR.run_oracle(P, model_type, nm, batch, np.float32)
    m = _model(pivp_amd, model_type, nm, P)
    for f in (0, 1):
        want = TR.advect_rollout(m64, D8, f)
        f32 = np.abs(TR.advect_rollout(m32, D8, f).astype(np.float64) - want).max(axis=(1, 2, 3, 4))
        m.reset_state()
        m.imagine(imgs[:2], acts[:T - 1], stas[0], designated=D8.astype(np.float32), designated_frame=f)
        raw = m.pixel_distrib
        assert raw.shape == (T - 1 - f, 2, 8, 64, 64) and m.pixel_mass.shape == (T - 1 - f, 2, 8)
        got = raw.cpu().numpy().astype(np.float64)
        err = np.abs(got - want).max(axis=(1, 2, 3, 4))
        pmax = want.max(axis=(3, 4)).min(axis=(1, 2))
        for t in range(len(err)):
            print('%s T=%d f=%d step %d: |HIP - float64| %.2e  float32 oracle %.2e  bound %.1e  smallest plane maximum %.2e  error / that %.1e'
                  % (model_type, T, f, f + t, err[t], f32[t], 10 * max(f32[t], 1e-6), pmax[t], err[t] / pmax[t]))
        assert np.isfinite(got).all()
        for t in range(len(err)):
            assert err[t] < 10 * max(f32[t], 1e-6)                       # every step, sample and plane
        # the raw sums, and the optional normalisation exactly as torch computes it
        sums = got.sum(axis=(3, 4))
        assert np.abs(m.pixel_mass.cpu().numpy() - sums).max() <= 1e-6 * sums.max()
        assert (np.abs(m.pixel_mass.cpu().numpy() - sums) <= 1e-6 * sums + 1e-30).all()
        mass = m.pixel_mass.clone()
        m.reset_state()
        m.imagine(imgs[:2], acts[:T - 1], stas[0], designated=D8.astype(np.float32), designated_frame=f, normalize=True)
        assert torch.equal(m.pixel_mass, mass)
        assert torch.equal(m.pixel_distrib, raw / raw.sum(dim=(3, 4), keepdim=True))
        # P = 1: the same bits as that plane among eight
        m.reset_state()
        m.imagine(imgs[:2], acts[:T - 1], stas[0], designated=D8[:, 2:3].astype(np.float32), designated_frame=f)
        assert m.pixel_distrib.shape == (T - 1 - f, 2, 1, 64, 64) and torch.equal(m.pixel_distrib[:, :, 0], raw[:, :, 2])


def test_imagine_is_reproducible():
    torch, pivp_amd = _gpu()
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, 6, 64, 64, seed=123))
    D = TR.standard_planes(2).astype(np.float32)
    m = _model(pivp_amd, 'CDNA', nm, P)
    runs = []
    for _ in range(2):
        m.reset_state()
        gen = m.imagine(imgs[:2], acts[:5], stas[0], designated=D)
        runs.append((gen.clone(), m.pixel_distrib.clone(), torch.stack(m.gen_states).clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # ... and from a second model object (another workspace address)
    m2 = _model(pivp_amd, 'CDNA', nm, P)
    m2.imagine(imgs[:2], acts[:5], stas[0], designated=D)
    assert torch.equal(m2.pixel_distrib, runs[0][1]) and torch.equal(torch.stack(m2.gen_images), runs[0][0])


def test_state_machine_around_imagine():
    torch, pivp_amd = _gpu()
    from pivp_amd import _lib
    P, nm = _random_params('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(2, 5, 64, 64, seed=3))
    D = TR.standard_planes(2).astype(np.float32)
    m = _model(pivp_amd, 'CDNA', nm, P, keep_activations=True, deterministic=True)   # a training model (bit-reproducible sweeps): imagine still runs an inference plan
    loss0 = m([imgs, acts, stas], 0).clone()
    gen0 = torch.stack(m.gen_images).clone()
    train_plan = m._active
    m.cleargrads(); m.backward()
    g0 = m._flat_grads.clone()
    m.reset_state()
    m.imagine(imgs[:2], acts[:4], stas[0], designated=D)
    assert m._active is not train_plan and m._active.cfg.keep_activations == 0
    with pytest.raises(RuntimeError, match='call the model first'):
        m.backward()
    assert m.summaries == []
    # taps after imagine: the last step's masks sum to one over the flat groups, enc7 is there, conv_res has its eight entries
    masks = m.tap('masks')
    assert masks.shape == (2, nm + 1, 64, 64) and abs(float(masks.sum()) - 2 * 64 * 64) < 1e-2
    assert m.tap('enc7').shape == (2, 3, 64, 64) and len(m.conv_res) == 8
    with pivp_amd.using_config('train', False):
        ref = _model(pivp_amd, 'CDNA', nm, P)
        ref([imgs, acts, stas], 0)
    assert torch.equal(ref.tap('masks'), masks)                          # writing the masks at every step leaves the last step's as they were
    # the library's own answer on the predict plan
    lib, plan = _lib.load(), m._active
    ci, ac, st = (torch.from_numpy(np.ascontiguousarray(a)).to(m.device) for a in (imgs[:2], acts[:4], stas[0]))
    gen = torch.empty((4, 2, 3, 64, 64), device=m.device); gs = torch.empty((4, 2, 5), device=m.device)
    tin = torch.from_numpy(np.ascontiguousarray(np.repeat(D, 3, axis=1)[:, :9])).to(m.device); tout = torch.empty((4, 2, 9, 64, 64), device=m.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda tin_p, P_, f_, gen_p=gen.data_ptr(), tout_p=tout.data_ptr(): lib.pivp_rollout_predict(
        plan.h, ci.data_ptr(), ac.data_ptr(), st.data_ptr(), tin_p, P_, f_, gen_p, gs.data_ptr(), tout_p, s)
    assert call(tin.data_ptr(), 9, 1) == -1 and call(tin.data_ptr(), 0, 1) == -1 and call(tin.data_ptr(), -1, 1) == -1      # bad P
    assert call(tin.data_ptr(), 3, 2) == -1 and call(tin.data_ptr(), 3, -1) == -1                                        # bad f
    assert call(None, 3, 1) == -1 and call(tin.data_ptr(), 3, 1, tout_p=None) == -1 and call(None, 0, 0, gen_p=None) == -1   # null pointers
    assert call(None, 0, 0) == 0 and call(tin.data_ptr(), 8, 0) == 0
    torch.cuda.synchronize()
    assert lib.pivp_rollout_backward(plan.h, ci.data_ptr(), ac.data_ptr(), st.data_ptr(), None, gen.data_ptr(), gs.data_ptr(), s) == -3
    # __call__ after imagine: the same loss, frames and gradients as without it
    m.reset_state()
    loss1 = m([imgs, acts, stas], 0)
    assert torch.equal(loss1, loss0) and torch.equal(torch.stack(m.gen_images), gen0)
    m.cleargrads(); m.backward()
    assert torch.equal(m._flat_grads, g0)


def test_score_actions_is_one_imagine_at_batch_k():
    torch, pivp_amd = _gpu()
    from pivp_amd import planning
    P, nm = TR.load_trained('CDNA')
    imgs, acts, stas = (np.asarray(a) for a in R.moving_batch(1, 6, 64, 64, seed=123))
    K, steps = 8, 5
    rs = np.random.RandomState(2)
    cand = (acts[:steps, 0][None] + rs.randn(K, steps, 5) * 0.5).astype(np.float32)
    cand[0] = acts[:steps, 0]
    m = _model(pivp_amd, 'CDNA', nm, P)
    cost = planning.score_actions(m, imgs[:2], stas[0], cand, (32, 32), (40, 24))
    assert cost.shape == (K,) and torch.isfinite(cost).all() and float(cost.min()) > 0
    frames = torch.stack(m.gen_images)
    assert frames.shape == (steps, K, 3, 64, 64)
    for k in range(1, K):
        assert not torch.equal(frames[-1, k], frames[-1, 0])            # the actions reach the rollout
    assert not torch.equal(cost[1:], cost[:1].expand(K - 1))
    # by hand: the same imagine, the same sums
    m2 = _model(pivp_amd, 'CDNA', nm, P)
    m2.imagine(np.repeat(imgs[:2], K, axis=1), np.ascontiguousarray(cand.transpose(1, 0, 2)), np.repeat(stas[0], K, axis=0),
               designated=planning.one_hot_planes(np.tile(np.array([[[32, 32]]]), (K, 1, 1)), 64, 64), normalize=True)
    assert torch.equal(torch.stack(m2.gen_images), frames)
    d = m2.pixel_distrib[:, :, 0]
    rows = torch.arange(64, dtype=torch.float32, device=d.device).view(64, 1)
    cols = torch.arange(64, dtype=torch.float32, device=d.device).view(1, 64)
    dist = torch.sqrt((rows - 40.0) ** 2 + (cols - 24.0) ** 2)
    assert torch.equal((d * dist).sum(dim=(-2, -1)).sum(dim=0), cost)
    # candidate 0 replays the recorded actions: its frames are those of a batch-1 imagine up to batching-independent arithmetic
    m3 = _model(pivp_amd, 'CDNA', nm, P)
    alone = m3.imagine(imgs[:2], acts[:steps], stas[0])
    assert float((alone[:, 0] - frames[:, 0]).abs().max()) < 1e-4


def test_predict_cli_designated_pixel(tmp_path):
    """`predict --designated_pixel R,C`: the same frames as the plain CLI (both are feed-self rollouts of the same context) and the pixel's
    normalised distribution beside them; without the flag nothing new is written."""
    torch, pivp_amd = _gpu()
    from pivp_amd import dataset as ds, predict as Pm
    data = tmp_path / 'data'; data.mkdir()
    mdir = tmp_path / 'models' / 'x-y-CDNA-z'; mdir.mkdir(parents=True)
    rs = np.random.RandomState(0)
    T = 5
    np.save(str(data / 'image_batch_0'), rs.rand(T, 64, 64, 3).astype(np.float32))
    np.save(str(data / 'action_batch_0'), (rs.randn(T, 5) * 0.1).astype(np.float32))
    np.save(str(data / 'state_batch_0'), (rs.randn(T, 5) * 0.1).astype(np.float32))
    np.save(str(data / 'image_batch_pred_0'), (rs.rand(T, 96, 120, 3) * 255).astype(np.uint8))
    ds.write_map(str(data), [[0, '', 'image_batch_0.npy', 'action_batch_0.npy', 'state_batch_0.npy', '', 'image_batch_pred_0.npy']])
    P, nm = TR.load_trained('CDNA')
    with open(str(mdir / 'training-0'), 'wb') as f:
        np.savez_compressed(f, **P)
    base = ['x-y-CDNA-z', 'training-0', '0', '--models_dir', str(tmp_path / 'models'), '--data_dir', str(data)]
    Pm.main(base)
    plain = np.load(str(mdir / 'prediction-0.npy'))
    assert sorted(os.listdir(str(mdir))) == ['prediction-0.npy', 'training-0']
    os.remove(str(mdir / 'prediction-0.npy'))
    Pm.main(base + ['--designated_pixel', '20,40'])
    assert sorted(os.listdir(str(mdir))) == ['pixel_distrib-0.npy', 'prediction-0.npy', 'training-0']
    assert np.array_equal(np.load(str(mdir / 'prediction-0.npy')), plain) and plain.shape == (T - 1, 3, 64, 64) and plain.dtype == np.uint8
    d = np.load(str(mdir / 'pixel_distrib-0.npy'))
    assert d.shape == (T - 2, 64, 64) and d.dtype == np.float32 and d.min() >= 0
    assert np.abs(d.sum(axis=(1, 2), dtype=np.float64) - 1.0).max() < 1e-5
    r, c = np.unravel_index(d[0].argmax(), (64, 64))
    assert abs(int(r) - 20) <= 4 and abs(int(c) - 40) <= 4               # one step moves a pixel by at most the 5x5 kernel's reach and m_0 keeps it in place
    with pytest.raises(ValueError):
        Pm.main(base + ['--designated_pixel', '64,0'])
