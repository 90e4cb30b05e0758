"""Case tables, seeded inputs and float64 references of tests/test_gpu_forward_heads.py: the forward head kernels (csrc/heads.hip, frame_head.hip,
pixel_track.hip, skinny_linear.h, frame_transform.h) off the 64x64 grid.  No GPU import.

The float64 forwards are those of tests/heads_bwd_reference.py (flat_softmax, composite_cdna / _stp / _dna, cdna_kernels, stp_regressor, heads),
not restated here, and that module's rule holds: a reference is evaluated in float64 FROM THE fp32 ARRAYS THE KERNEL IS HANDED, so a comparison
tests one op's arithmetic and not a chain of roundings.  tests/test_heads_fwd_host.py checks them against oracle/restatement.py at what this
table adds, and asserts the table's own conditions: every case accepted or refused as stated here, every branch it names reached by a case.

Every case is a tuple whose id string (`*_id`) names the branch it exists for."""
import numpy as np
import torch

import heads_bwd_reference as R

F64, t64, f32 = R.F64, R.t64, R.f32
MODE = {'cdna': 0, 'stp': 1, 'dna': 2}
NE = {'cdna': 3, 'stp': 3, 'dna': 25}
B = 2                                    # batch of every case but the skinny linear's and the 1x1 heads'

# ---- the geometry of the kernels, restated (the host test pins the constants to the sources) ---------------------------------------------------------
BAND_TR = 4                              # image rows per block of composite_kernel / pixel_track_kernel / frame_head_kernel
CDNA_KL = 11 * 28
LDS_CAP = 160 * 1024
LIN_KS, LIN_BG, FH_MAXKS = 64, 16, 128


def composite_lds_bytes(W, NM):
    NP = NM + 1
    npx = BAND_TR * W
    return 4 * (NP * (npx + 2 * (NP - 1)) + 2 * NP * (npx // NP + 2) + 3 * (BAND_TR + 4) * (W + 4) + CDNA_KL)


def composite_serves(H, W, NM, mode):
    if H <= 1 or W <= 1 or NM < 1 or NM > 11 or mode not in (0, 1, 2):
        return False
    if mode == 2 and NM != 1:
        return False
    return composite_lds_bytes(W, NM) <= LDS_CAP and W + 4 <= 256


def frame_head_lds_floats(mode, W, NM):
    NP, npx, PW = NM + 1, BAND_TR * W, W + 4
    win, G = npx + 2 * (NP - 1), npx // NP + 2
    f = 32 * 68 + 32 + ((NP * win + 3) & ~3) + (0 if mode == 2 else 3 * npx) + CDNA_KL + 256 + 8
    f += ((3 * (BAND_TR + 4) * PW + 3) & ~3) + max(24 * 68, (2 * NP * G + 3) & ~3)
    return f + 4 * 64 * 36


def frame_head_ok(mode, Bn, H, W, NM):
    if mode not in (0, 1, 2) or Bn <= 0 or H <= 1 or W <= 1 or NM < 1 or NM > 11:
        return False
    if mode == 2 and NM != 1:
        return False
    if H % BAND_TR or (BAND_TR * W) % 64 or W + 4 > 256:
        return False
    return 4 * frame_head_lds_floats(mode, W, NM) <= LDS_CAP


def kslices(K):
    return (K + LIN_KS - 1) // LIN_KS


def frame_head_fits(mode, Bn, H, W, NM, K):
    """pivp_frame_head_fits: 0 refused, 1 the in-kernel finisher serves K, 2 the finisher stays a launch of its own (through aux)."""
    if not frame_head_ok(mode, Bn, H, W, NM):
        return 0
    return 1 if (mode == 2 or kslices(K) <= FH_MAXKS) else 2


def cdna_kernels_serves(NM):
    return NM >= 1 and NM * 25 <= 256


def rstep(W):
    """band_tile_request / _file: tile rows a pass of the 256 threads covers (thread = a column of the padded row)."""
    return 256 // (W + 4)


def logit_window(H, W, NM, band):
    """win of band `band` of composite_kernel: the band's pixels +- NP - 1 flat elements per plane."""
    rows = min(BAND_TR, H - band * BAND_TR)
    return rows * W + 2 * NM


def bands(H):
    return (H + BAND_TR - 1) // BAND_TR


# ---- composite ------------------------------------------------------------------------------------------------------------------------------------
COMPOSITE_FRAMES = [                      # (H, W, the branch the frame reaches)
    (4, 16, 'one-band-first-and-last'),
    (30, 72, 'rstep3-two-row-last-band'),
    (10, 100, 'rstep2-two-row-last-band'),
    (16, 128, 'rstep1'),
    (12, 248, 'widest-plan-frame-window-loop-three-bands'),
    (6, 252, 'widest-entry-frame-partial-band'),
]
CDNA_NM, STP_NM, DNA_NM = (1, 2, 3, 7, 10), (1, 3, 7, 11), (1,)
# (model, H, W, NM, stp_zero)
COMPOSITE_CASES = ([('cdna', H, W, NM, 0) for (H, W, _) in COMPOSITE_FRAMES for NM in CDNA_NM] +
                   [('stp', H, W, NM, zb) for (H, W, _) in COMPOSITE_FRAMES for NM in STP_NM for zb in (0, 1)] +
                   [('dna', H, W, NM, 0) for (H, W, _) in COMPOSITE_FRAMES for NM in DNA_NM])
_FRAME_TAG = {(H, W): tag for (H, W, tag) in COMPOSITE_FRAMES}


def composite_id(case):
    model, H, W, NM, zb = case
    return '%s-%dx%d-%s-NM%d%s' % (model, H, W, _FRAME_TAG[(H, W)], NM, ('-zero' if zb else '-clamp') if model == 'stp' else '')


# the flat softmax's groups straddle planes where HW % NP != 0: at least one frame per straddling NP
STRADDLING_NP = (3, 11, 12)
for _NP in STRADDLING_NP:
    assert any((H * W) % (NM + 1) != 0 for (_, H, W, NM, _) in COMPOSITE_CASES if NM + 1 == _NP), _NP

# ---- pixel track ----------------------------------------------------------------------------------------------------------------------------------
TRACK_FRAMES = [(30, 72), (10, 100), (6, 252)]
# (model, H, W, NM, stp_zero): P = 8 is run, and P = 1 against its plane 0
TRACK_CASES = ([('cdna', H, W, NM, 0) for (H, W) in TRACK_FRAMES for NM in (1, 10)] +
               [('stp', H, W, NM, zb) for (H, W) in TRACK_FRAMES for NM in (1, 10) for zb in (0, 1)] +
               [('dna', H, W, 1, 0) for (H, W) in TRACK_FRAMES])


def track_id(case):
    model, H, W, NM, zb = case
    return '%s-%dx%d-rstep%d-last-band-%d-rows-NM%d%s' % (model, H, W, rstep(W), H - (bands(H) - 1) * BAND_TR, NM,
                                                          ('-zero' if zb else '-clamp') if model == 'stp' else '')


# ---- frame head -----------------------------------------------------------------------------------------------------------------------------------
# (H, W, hidden5's K, the branch): K picks the finisher's slice count KS = K / 64
FRAME_HEAD_FRAMES = [
    (4, 16, 128, 'one-band-tile-three-idle-waves-KS2'),
    (8, 48, 5760, 'three-tiles-KS90-clamped-tail'),
    (16, 80, 8192, 'five-tiles-over-four-waves-KS128-limit'),
    (8, 128, 16384, 'eight-tiles-KS256-finisher-forced-through-aux'),
    (8, 240, 5760, 'widest-frame-KS90'),
]
FH_MODELS = [('cdna', 1, 0), ('cdna', 4, 0), ('cdna', 10, 0), ('stp', 1, 0), ('stp', 1, 1), ('stp', 11, 0), ('stp', 11, 1), ('dna', 1, 0)]
# (model, H, W, NM, stp_zero, K, finisher): train = True always
FRAME_HEAD_CASES = ([(m, H, W, NM, zb, K, fin) for (H, W, K, _) in FRAME_HEAD_FRAMES for (m, NM, zb) in FH_MODELS for fin in (True, False)
                     if fin == (m == 'dna' or fin and kslices(K) <= FH_MAXKS)] +   # (DNA has no motion head, K > 8192 no in-kernel finisher: one form)
                    [('cdna', 64, 64, 10, 0, 8192, True), ('stp', 64, 64, 10, 1, 8192, True), ('stp', 64, 64, 10, 1, 8192, False),
                     ('dna', 64, 64, 1, 0, 8192, True)])                           # the constant-folded instances
_FH_TAG = dict([((H, W), tag) for (H, W, _, tag) in FRAME_HEAD_FRAMES] + [((64, 64), 'constant-folded-instance')])
FH_B = 2


def frame_head_id(case):
    m, H, W, NM, zb, K, fin = case
    return '%s-%dx%d-%s-NM%d%s-K%d-%s' % (m, H, W, _FH_TAG[(H, W)], NM, ('-zero' if zb else '-clamp') if m == 'stp' else '', K,
                                          'finisher' if fin else 'aux')


# ---- skinny linear --------------------------------------------------------------------------------------------------------------------------------
LINEAR_B = (1, 16, 17, 33)
LINEAR_K = (128, 5760, 8192, 16384, 200)
GEN_CASES = [(K, NM, Bn) for K in LINEAR_K for NM in (1, 10) for Bn in LINEAR_B]        # pivp_cdna_kernels
STPP_CASES = [(K, Bn) for K in LINEAR_K for Bn in LINEAR_B]                            # pivp_stp_params


def linear_id(case):
    K, Bn = case[0], case[-1]
    tag = 'K%d-KS%d%s-B%d%s' % (K, kslices(K), '-partial-slice' if K % LIN_KS else '', Bn, '-second-group-of-one' if Bn % LIN_BG == 1 and Bn > 1 else '')
    return tag if len(case) == 2 else tag + '-nout%d' % (25 * case[1])


# ---- 1x1 heads ------------------------------------------------------------------------------------------------------------------------------------
HEADS_SHAPES = [(1, 64, 'one-wave-three-return-early'), (3, 2160, 'wave-across-samples-partial-wave-partial-block'), (2, 4096, 'whole-blocks')]
HEADS_MODELS = [(10, 'cdna'), (11, 'stp'), (1, 'cdna'), (1, 'dna')]
HEADS_CASES = [(Bn, HW, NM, m) for (Bn, HW, _) in HEADS_SHAPES for (NM, m) in HEADS_MODELS]
_HD_TAG = {(Bn, HW): tag for (Bn, HW, tag) in HEADS_SHAPES}


def heads_id(case):
    Bn, HW, NM, m = case
    return '%s-B%d-HW%d-%s-NP%d' % (m, Bn, HW, _HD_TAG[(Bn, HW)], NM + 1)


# ---- refusals: (entry, model, H, W, NM) each entry must answer with the bad-argument status ------------------------------------------------------------
REFUSALS = [('composite', 'cdna', 4, 253, 10), ('composite', 'cdna', 8, 16, 12), ('composite', 'cdna', 1, 16, 10), ('composite', 'dna', 8, 16, 2),
            ('cdna_kernels', 'cdna', 8, 16, 11), ('frame_head', 'cdna', 6, 16, 10), ('frame_head', 'cdna', 8, 24, 10)]


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------------------
def make_fwd_theta(rs, Bn, H):
    """Sample 0: near the identity (R.make_theta, far = 0).  The others: a rotation by about 35 degrees, stretched and shifted, so that a good part of
    the frame samples outside it -- the border rule decides those pixels -- and the rest inside."""
    th = [R.make_theta(rs, 1, H, 0)[0]]
    for b in range(1, Bn):
        th.append(1.15 * np.array(R.rotation_theta(35.0 if b % 2 else -35.0, 0.3, -0.25)) + 0.02 * rs.randn(6))
    return f32(np.stack(th))


def stp_outside_frame(theta, H, W):
    """Per sample, the fraction of pixels whose sampling coordinate lies outside the frame (clamped by one border rule, read as 0 by the other)."""
    gu, gv = [c.numpy() for c in R.stp_coords(t64(theta), H, W)]
    return ((np.abs(gu) > 1.0) | (np.abs(gv) > 1.0)).reshape(theta.shape[0], -1).mean(1)


def make_composite(model, H, W, NM, Bn=B):
    """-> dict(prev, logits, layer0, aux) as [B][planes][H][W] fp32 (aux: kernels [B][NM][5][5] | theta [B][6] | enc7 [B][25][H][W])."""
    rs = R._rs(20, MODE[model], H, W, NM, Bn)
    HW = H * W
    d = dict(prev=f32(rs.rand(Bn, 3, H, W)), logits=R.make_logits(rs, Bn, NM + 1, HW).reshape(Bn, NM + 1, H, W), layer0=None)
    if model == 'dna':
        d['aux'] = f32(np.maximum(rs.randn(Bn, 25, H, W), 0.0))
        return d
    d['layer0'] = f32(rs.rand(Bn, 3, H, W))
    d['aux'] = f32(R.cdna_kernels(t64(rs.randn(Bn, NM * 25)), NM)).reshape(Bn, NM, 5, 5) if model == 'cdna' else make_fwd_theta(rs, Bn, H)
    return d


def make_track(model, H, W, NM, P=8, Bn=B):
    """-> dict(planes [B][P][H][W], masks: the fp32 softmax of seeded logits, aux)."""
    d = make_composite(model, H, W, NM, Bn)
    rs = R._rs(21, MODE[model], H, W, NM, Bn)
    planes = rs.rand(Bn, P, H, W) ** 4                                            # O(1) peaks on a low floor, as a designated-pixel map has
    return dict(planes=f32(planes), masks=f32(ref_masks(d['logits'])), aux=d['aux'])


def make_frame_head(model, H, W, NM, K, Bn=FH_B):
    """The raw enc6 map, norm_enc6's parameters, the 1x1 heads, the previous frame and the motion head's Linear over a K-long hidden5 (as
    (B, 128, K / 128, 1): the wrapper's NHWC-flat index is the reference's), all in the reference's layouts, fp32-exact."""
    rs = R._rs(22, MODE[model], H, W, NM, K, Bn)
    ne, nout = NE[model], (25 * NM if model == 'cdna' else 100)
    d = dict(e6raw=rs.randn(Bn, 64, H, W) * 1.5 + 0.3, gamma=1.0 + 0.1 * rs.randn(64, H, W), beta=0.1 * rs.randn(64, H, W),
             Wm=rs.randn(64, NM + 1, 1, 1) / 4, bm=rs.randn(NM + 1) * 0.1, We=rs.randn(64, ne, 1, 1) / 8, be=rs.randn(ne) * 0.1,
             prev=rs.rand(Bn, 3, H, W), h5=rs.randn(Bn, 128, K // 128, 1), Wh=rs.randn(nout, K) / np.sqrt(K), bh=rs.randn(nout) * 0.1,
             W2=rs.randn(6, 100) * 0.02, b2=rs.randn(6) * 0.01)
    if model == 'stp':      # the regressor's bias carries the warp of make_fwd_theta's far sample, so that theta leaves the frame here too
        d['b2'] = d['b2'] + (1.15 * np.array(R.rotation_theta(35.0, 0.3, -0.25)) - np.array([1.0, 0, 0, 0, 1.0, 0]))
    return {k: f32(v) for k, v in d.items()}


def make_linear(K, nout, Bn):
    """x [B][K] (the NHWC-flat hidden5) and the K-major operand wt [K][256], columns nout.. zero, scaled by 1 / sqrt(K): outputs stay O(1)."""
    rs = R._rs(23, K, nout, Bn)
    wt = np.zeros((K, 256)); wt[:, :nout] = rs.randn(K, nout) / np.sqrt(K)
    return dict(x=f32(rs.randn(Bn, K)), wt=f32(wt), b=f32(0.1 * rs.randn(nout)), w2=f32(rs.randn(6, 100) / 10.0), b2=f32(0.1 * rs.randn(6)))


def make_heads(Bn, HW, NM, model):
    rs = R._rs(24, Bn, HW, NM, MODE[model])
    ne = NE[model]
    return dict(e6=f32(np.maximum(rs.randn(Bn, 64, 1, HW), 0.0)), Wm=f32(rs.randn(64, NM + 1, 1, 1) / 8.0), bm=f32(0.1 * rs.randn(NM + 1)),
                We=f32(rs.randn(64, ne, 1, 1) / 8.0), be=f32(0.1 * rs.randn(ne)))


# ---- float64 references, from the fp32 arrays the kernel is handed -----------------------------------------------------------------------------------
def ref_masks(logits):
    return R.flat_softmax(t64(logits)).numpy()


def _cdna_planes(planes, mk, layer0, kerns):
    """R.composite_cdna on any number of planes: its transform takes three at a time."""
    Bn, P, H, W = planes.shape
    pad = torch.cat((planes, torch.zeros(Bn, -P % 3, H, W, dtype=F64)), 1)
    l0 = torch.cat((layer0, torch.zeros(Bn, -P % 3, H, W, dtype=F64)), 1)
    return torch.cat([R.composite_cdna(pad[:, c:c + 3], mk, l0[:, c:c + 3], kerns) for c in range(0, P, 3)], 1)[:, :P]


def ref_composite(model, prev, masks, layer0, aux, stp_zero=0):
    """The next frame (or the tracked planes: any plane count, layer0 = None for zero) from GIVEN masks [B][NP][H][W]."""
    pv, mk = t64(prev), t64(masks)
    l0 = torch.zeros_like(pv) if layer0 is None else t64(layer0)
    if model == 'cdna':
        Bn, NM = aux.shape[0], mk.shape[1] - 1
        return _cdna_planes(pv, mk, l0, t64(aux).reshape(Bn, NM, 25)).numpy()
    if model == 'stp':
        return R.composite_stp(pv, mk, l0, t64(aux), stp_zero).numpy()
    return R.composite_dna(pv, mk, t64(aux)).numpy()


def layer_norm_relu(x, gamma, beta, eps):
    """norm_enc6 + ReLU (TM:203-208, TM:601): statistics over the whole (C, H, W) map of a sample."""
    x = t64(x)
    flat = x.reshape(x.shape[0], -1)
    mean, var = flat.mean(1, keepdim=True), flat.var(1, unbiased=False, keepdim=True)
    return torch.relu(((flat - mean) / torch.sqrt(var + eps)) * t64(gamma).reshape(1, -1) + t64(beta).reshape(1, -1)).reshape(x.shape)


def ref_heads(e6, Wm, bm, We, be, model):
    """e6 [B][64][H][W] (normalised) -> logits, enc7 (behind the variant's activation), layer0 (None for DNA), as [B][planes][H][W] float64."""
    Bn, _, H, W = e6.shape
    e = (e6 if isinstance(e6, torch.Tensor) else t64(e6)).permute(0, 2, 3, 1).reshape(-1, 64)
    pm, pe = R.heads(e, t64(Wm)[:, :, 0, 0], t64(bm), t64(We)[:, :, 0, 0], t64(be), Bn, H * W)
    if model != 'stp':
        pe = torch.relu(pe)
    shape = lambda t: t.reshape(Bn, -1, H, W).numpy()
    return shape(torch.relu(pm)), shape(pe), (None if model == 'dna' else shape(torch.sigmoid(pe)))


def ref_cdna_kernels(x, wt, b, NM):
    return R.cdna_kernels(t64(x) @ t64(wt)[:, :25 * NM] + t64(b), NM).numpy()


def ref_stp_params(x, wt, b1, w2, b2):
    return R.stp_regressor(t64(x), t64(wt)[:, :100], t64(b1), t64(w2), t64(b2))[0].numpy()


def h5_flat(h5):
    """The NHWC-flat hidden5 the kernels read, from the (B, 128, h, w) array the wrappers take."""
    return np.ascontiguousarray(h5.transpose(0, 2, 3, 1)).reshape(h5.shape[0], -1)


def wt_of(Wh):
    """The K-major operand of a reference-layout (nout, K) Linear weight over (B, 128, K / 128, 1) inputs (checkpoint.to_internal's)."""
    nout, K = Wh.shape
    return np.ascontiguousarray(Wh.reshape(nout, 128, K // 128).transpose(2, 1, 0)).reshape(K, nout)


# every STP case: at least one sample maps a tenth or more of its pixels outside the frame (a condition on the inputs, computed here on the CPU)
for (_m, _H, _W, _NM, _zb) in COMPOSITE_CASES + TRACK_CASES:
    if _m == 'stp' and _zb == 0:
        assert stp_outside_frame(make_composite(_m, _H, _W, _NM)['aux'], _H, _W).max() >= 0.10, (_H, _W, _NM)
