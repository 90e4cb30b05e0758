"""Float64 restatement of designated-pixel tracking (include/pivp_hip.h: pivp_pixel_track, pivp_rollout_predict).

One timestep composites (oracle/restatement.py `_step`, TM:725-727)
    out = prev * m_0 + sum over zip(transformed, m_1..)        transformed = [sigmoid(enc7), T_1(prev), ...]   CDNA / STP
                                                               transformed = [T(prev)]                          DNA
which is linear in prev apart from the synthesised layer sigmoid(enc7).  Tracked planes D (B, P, H, W) move through the same map with
prev := D and the synthesised layer := 0, reference quirks included (zip drops CDNA's last transform; STP's transforms share one theta; DNA's
slice quirk).  Two forms:

  advect_step(D, masks, model_type, aux)   explicit masks / kernels / theta / enc7, no network: for known answers and for per-op checks
  track_rollout(...)                       a full oracle rollout with taps, then per step the ORACLE'S OWN `_cdna / _stp / _dna` applied to D

Both are built from the oracle's primitives only (depthwise_conv2d, spatial_transformer_*); tests/test_imagine_host.py ties the first to the
`output` tap of `_step`."""
import numpy as np

from oracle import restatement as R

FLAGS = {'CDNA': dict(is_cdna=True), 'STP': dict(is_cdna=False, is_stp=True), 'DNA': dict(is_cdna=False, is_dna=True)}


def cdna_transforms(D, kerns):
    """TM:336-349 on planes: D (B, P, H, W), kerns (B, NM, 5, 5) -> NM arrays (B, P, H, W)."""
    B, P, H, W = D.shape
    NM = kerns.shape[1]
    t = R.depthwise_conv2d(D.transpose(1, 0, 2, 3), kerns.transpose(1, 0, 2, 3), 2)     # (P, B*NM, H, W)
    t = t.reshape(P, B, NM, H, W).transpose(2, 1, 0, 3, 4)
    return [t[m] for m in range(NM)]


def stp_transform(D, theta, border='clamp'):
    """TM:465-471 on planes: theta (B, 2, 3) or (B, 6)."""
    theta = np.asarray(theta, dtype=D.dtype).reshape(D.shape[0], 2, 3)
    return R.spatial_transformer_sampler(D, R.spatial_transformer_grid(theta, D.shape[2:]), border)


def dna_transform(D, enc7):
    """TM:392-415 on planes: enc7 (B, 25, H, W) = relu(Deconv1x1(enc6)), the kernel normalised here as the reference does."""
    B, P, H, W = D.shape
    pad = np.pad(D, ((0, 0), (0, 0), (2, 2), (2, 2)))
    inputs = []
    for xk in range(5):
        for yk in range(5):
            tmp = pad[:, :, xk:H, yk:W]                                  # TM:400, the slice quirk
            inputs.append(np.pad(tmp, ((0, 0), (0, 0), (0, xk), (0, yk)))[:, None])
    kin = np.concatenate(inputs, axis=1)
    kn = R.relu(enc7 - R.RELU_SHIFT) + R.RELU_SHIFT
    kn = kn / kn.sum(axis=1, keepdims=True)
    return (kin * kn[:, :, None]).sum(axis=1)


def _composite(D, masks, transformed):
    out = D * masks[:, 0:1]
    for layer, m in zip(transformed, [masks[:, i:i + 1] for i in range(1, masks.shape[1])]):    # TM:726: zip truncates
        out = out + layer * m
    return out


def advect_step(D, masks, model_type, aux, stp_border='clamp'):
    """One step of the definition.  masks: SOFTMAXED (B, NM+1, H, W); aux: CDNA kernels (B, NM, 5, 5) | STP theta | DNA enc7 (B, 25, H, W)."""
    D = np.asarray(D)
    masks = np.asarray(masks, dtype=D.dtype)
    NM = masks.shape[1] - 1
    zero = np.zeros_like(D)
    if model_type == 'CDNA':
        transformed = [zero] + cdna_transforms(D, np.asarray(aux, dtype=D.dtype).reshape(D.shape[0], NM, 5, 5))
    elif model_type == 'STP':
        warped = stp_transform(D, aux, stp_border)
        transformed = [zero] + [warped] * (NM - 1)
    elif model_type == 'DNA':
        assert NM == 1
        transformed = [dna_transform(D, np.asarray(aux, dtype=D.dtype))]
    else:
        raise ValueError(model_type)
    return _composite(D, masks, transformed)


def head_aux(model, taps):
    """The `aux` of advect_step for one tapped oracle step, recomputed from the taps with the oracle's primitives (TM:321-329 / 457-468)."""
    p, B = model.p, taps['hidden5'].shape[0]
    if model.model_type == 'CDNA':
        k = R.linear(taps['hidden5'].reshape(B, -1), p['model/cdna_kerns/W'], p['model/cdna_kerns/b']).reshape(B, model.num_masks, 5, 5)
        k = R.relu(k - R.RELU_SHIFT) + R.RELU_SHIFT
        return k / k.sum(axis=(2, 3), keepdims=True)
    if model.model_type == 'STP':
        s1 = R.relu(R.linear(taps['hidden5'].reshape(B, -1), p['model/stp_input/W'], p['model/stp_input/b']))
        ident = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], dtype=model.dtype)
        return (R.linear(s1, p['model/identity_params/W'], p['model/identity_params/b']) + ident).reshape(B, 2, 3)
    return taps['enc7']


def advect_with_oracle_heads(model, taps, D):
    """One step through the oracle's own head (three planes at a time: `_cdna` is written for three channels)."""
    head = {'CDNA': model._cdna, 'STP': model._stp, 'DNA': model._dna}[model.model_type]
    B, P, H, W = D.shape
    out = np.empty_like(D)
    for c0 in range(0, P, 3):
        n = min(3, P - c0)
        chunk = np.zeros((B, 3, H, W), dtype=D.dtype)
        chunk[:, :n] = D[:, c0:c0 + n]
        transformed, _ = head(taps['enc6'], taps['hidden5'], chunk)
        if model.model_type != 'DNA':
            transformed = [np.zeros_like(chunk)] + list(transformed[1:])     # the synthesised layer carries no mass
        out[:, c0:c0 + n] = _composite(chunk, taps['masks'], transformed)[:, :n]
    return out


def run_oracle(params, model_type, num_masks, batch, dtype=np.float64, ctx=2, stp_border='clamp'):
    """Feed-self oracle rollout on `batch` = (images, actions, states) with every step tapped -> the oracle model (`.taps`, `.gen_images`)."""
    m = R.Model(num_masks, params=params, dtype=dtype, num_frame_before_prediction=ctx, stp_border=stp_border, **FLAGS[model_type])
    m.train = False
    images, actions, states = batch
    m([images, actions, states], 0, tap_steps=range(len(images) - 1))
    return m


def advect_rollout(m, D0, f):
    """D0 (B, P, H, W), given on frame f, through steps f .. T-2 of a tapped oracle rollout -> (T-1-f, B, P, H, W) in the model's dtype."""
    D = np.asarray(D0, dtype=m.dtype)
    outs = []
    for t in range(f, len(m.taps)):
        D = advect_with_oracle_heads(m, m.taps[t], D)
        outs.append(D)
    return np.stack(outs)


def track_rollout(params, model_type, num_masks, batch, D0, f, dtype=np.float64, ctx=2, stp_border='clamp'):
    """run_oracle + advect_rollout -> (planes, the oracle model)."""
    m = run_oracle(params, model_type, num_masks, batch, dtype, ctx, stp_border)
    return advect_rollout(m, D0, f), m


def standard_planes(B, H=64, W=64):
    """The planes of the rollout checks: one-hot (32, 32), one-hot (20, 40), unit-mass Gaussian (sigma 3 at (30, 30)); float64 (B, 3, H, W)."""
    D = np.zeros((B, 3, H, W))
    D[:, 0, 32, 32] = 1.0
    D[:, 1, 20, 40] = 1.0
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.exp(-((yy - 30.0) ** 2 + (xx - 30.0) ** 2) / (2 * 3.0 ** 2))
    D[:, 2] = g / g.sum()
    return D


def stp_short_planes(B, H=64, W=64):
    """Planes for the trained STP model, which hands most of every pixel to the synthesised layer: a plane's maximum shrinks 6-10x per step
    (0.13, 0.022, 0.0041, 7e-4, 1e-4 for the one-hot at (32, 32)), so over five steps no plane in [0, 1] keeps a maximum of 1e-3.  On a
    FOUR-frame batch (three steps) these do: one-hot (32, 32), one-hot (30, 48) -- the best-kept pixel of the held-out batch --, and the Gaussian
    of standard_planes scaled to peak 1."""
    D = standard_planes(B, H, W)
    D[:, 1] = 0.0
    D[:, 1, 30, 48] = 1.0
    D[:, 2] /= D[:, 2].max()
    return D


# (model, frames T of R.moving_batch(2, T, 64, 64, seed=123), planes, does every step keep a plane maximum >= 1e-3) of the rollout checks
ROLLOUT_CASES = [('CDNA', 6, standard_planes, True), ('DNA', 6, standard_planes, True), ('STP', 6, standard_planes, False),
                 ('STP', 4, stp_short_planes, True)]


def load_trained(model_type):
    """(params, num_masks) of the committed 64 x 64 trained weights."""
    import os
    import sys
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    if gold not in sys.path:
        sys.path.insert(0, gold)
    import trained_weights as TW
    nm = 1 if model_type == 'DNA' else 10
    P0 = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=nm, model_type=model_type, height=64, width=64)
    return TW.load_trained('trained_%s64_q8' % model_type.lower(), P0), nm
