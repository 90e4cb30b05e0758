"""CPU-side tests of the forward head parity suite (tests/test_gpu_forward_heads.py): the float64 references of tests/heads_bwd_reference.py against
oracle/restatement.py at what the forward table adds to the backward's shapes (the one-band frame, NM = 11 and NM = 1, the STP zero border on a
theta that leaves the frame, norm_enc6), and the conditions of tests/heads_fwd_cases.py itself: its restated predicates and constants against the
sources, every case accepted or refused as the table says, every branch the table names reached by at least one case.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import restatement as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_bwd_reference as R  # noqa: E402
import heads_fwd_cases as C  # noqa: E402
from test_backward_heads_host import _close, _head_model, _oracle_composite  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'physical-interaction-video-prediction_amd', 'csrc')
T = R.t64


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the references at the forward table's shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,NP', [(4, 16, 12), (4, 16, 3), (6, 252, 11), (10, 100, 2), (30, 72, 8)])
def test_flat_softmax_agrees_with_the_restatement(H, W, NP):
    lg = R.make_logits(np.random.RandomState(NP), 2, NP, H * W).reshape(2, NP, H, W)
    want = O.softmax_axis1(lg.astype(np.float64).reshape(-1, NP)).reshape(lg.shape)
    _close(C.ref_masks(lg), want, 1e-15)
    if (H * W) % NP:                                                             # a group that holds elements of two planes
        flat = np.arange(NP * H * W).reshape(-1, NP) // (H * W)
        assert (flat[:, 0] != flat[:, -1]).any()


@pytest.mark.parametrize('model,H,W,NM,zb', [('cdna', 4, 16, 1, 0), ('cdna', 4, 16, 10, 0), ('cdna', 6, 20, 7, 0), ('stp', 4, 16, 11, 0), ('stp', 4, 16, 11, 1),
                                             ('stp', 4, 16, 1, 1), ('stp', 10, 12, 3, 1), ('dna', 4, 16, 1, 0), ('dna', 6, 20, 1, 0)])
def test_composites_agree_with_the_restatement(model, H, W, NM, zb):
    """ref_composite on the table's own inputs (the one-band frame, NM = 11, NM = 1, the zero border with a sample that leaves the frame) against the
    model's transform + TM:720-726 as oracle/restatement.py spells them."""
    d = C.make_composite(model, H, W, NM)
    prev, logits = d['prev'].astype(np.float64), d['logits'].astype(np.float64)
    m = _head_model(model, NM, 8, np.random.RandomState(0), 'zeros' if zb else 'clamp')
    if model == 'cdna':
        l0 = d['layer0'].astype(np.float64)
        t = O.depthwise_conv2d(prev.transpose(1, 0, 2, 3), d['aux'].astype(np.float64).transpose(1, 0, 2, 3), 2)
        transformed = [l0] + list(t.reshape(3, C.B, NM, H, W).transpose(2, 1, 0, 3, 4))
    elif model == 'stp':
        assert C.stp_outside_frame(d['aux'], H, W).max() >= 0.10
        grid = O.spatial_transformer_grid(d['aux'].astype(np.float64).reshape(C.B, 2, 3), (H, W))
        transformed = [d['layer0'].astype(np.float64)] + [O.spatial_transformer_sampler(prev, grid, 'zeros' if zb else 'clamp')] * (NM - 1)
    else:
        z = np.where(d['aux'] > 0, d['aux'], -1.0).astype(np.float64)
        transformed, _ = m._dna(z, None, prev)
    want, masks = _oracle_composite(transformed, prev, logits, NM)
    mk = C.ref_masks(d['logits'])
    _close(mk, masks, 1e-15)
    _close(C.ref_composite(model, d['prev'], mk, d['layer0'], d['aux'], zb), want, 1e-13)


def test_tracked_planes_are_the_composite_of_each_plane_without_the_synthesised_layer():
    """ref_composite on 8 planes (what pixel_track is compared with) == on each plane alone with layer0 = 0."""
    for model, NM, zb in (('cdna', 10, 0), ('cdna', 1, 0), ('stp', 10, 1), ('dna', 1, 0)):
        d = C.make_track(model, 6, 20, NM)
        all8 = C.ref_composite(model, d['planes'], d['masks'], None, d['aux'], zb)
        assert all8.shape == d['planes'].shape
        for c in (0, 3, 7):
            three = np.repeat(d['planes'][:, c:c + 1], 3, 1)
            one = C.ref_composite(model, three, d['masks'], np.zeros_like(three), d['aux'], zb)
            _close(all8[:, c], one[:, 0], 1e-15)


def test_small_forwards_agree_with_the_restatement():
    rs = np.random.RandomState(3)
    # cdna_kernels at NM = 1 and through the K-major operand
    d = C.make_linear(200, 25, 3)
    k = O.relu(O.linear(d['x'].astype(np.float64), d['wt'].astype(np.float64)[:, :25].T, d['b'].astype(np.float64)).reshape(3, 1, 25) - 1e-12) + 1e-12
    _close(C.ref_cdna_kernels(d['x'], d['wt'], d['b'], 1), k / k.sum(2, keepdims=True), 1e-15)
    d = C.make_linear(128, 100, 2)
    s1 = O.relu(O.linear(d['x'].astype(np.float64), d['wt'].astype(np.float64)[:, :100].T, d['b'].astype(np.float64)))
    _close(C.ref_stp_params(d['x'], d['wt'], d['b'], d['w2'], d['b2']), O.linear(s1, d['w2'].astype(np.float64), d['b2'].astype(np.float64)) + [1.0, 0, 0, 0, 1.0, 0], 1e-14)
    # the K-major operand and the NHWC-flat hidden5 of the frame-head cases are checkpoint.to_internal's
    import pivp_amd
    Wh, h5 = R.f32(rs.randn(50, 384)), R.f32(rs.randn(2, 128, 3, 1))
    assert np.array_equal(pivp_amd.to_internal('model/cdna_kerns/W', Wh).reshape(384, 256)[:, :50], C.wt_of(Wh))
    _close(C.h5_flat(h5).astype(np.float64) @ C.wt_of(Wh).astype(np.float64), O.linear(h5.astype(np.float64).reshape(2, -1), Wh.astype(np.float64)), 1e-12)
    # norm_enc6 + ReLU and the 1x1 heads of a frame-head case
    f = C.make_frame_head('stp', 4, 16, 11, 128)
    e6 = O.relu(O.layer_norm_conv2d(f['e6raw'].astype(np.float64), f['gamma'].astype(np.float64).reshape(-1), f['beta'].astype(np.float64).reshape(-1), 1e-6))
    mine = C.layer_norm_relu(f['e6raw'], f['gamma'], f['beta'], 1e-6)
    _close(mine, e6, 1e-12)
    lg, e7, l0 = C.ref_heads(mine, f['Wm'], f['bm'], f['We'], f['be'], 'stp')
    w64 = lambda k: f[k].astype(np.float64)
    _close(lg, O.relu(O.deconv2d(e6, w64('Wm'), w64('bm'))), 1e-12)
    _close(e7, O.deconv2d(e6, w64('We'), w64('be')), 1e-12)
    _close(l0, O.sigmoid(O.deconv2d(e6, w64('We'), w64('be'))), 1e-12)
    assert C.stp_outside_frame(C.ref_stp_params(C.h5_flat(f['h5']), C.wt_of(f['Wh']), f['bh'], f['W2'], f['b2']), 4, 16).max() >= 0.10


# ---- the table's restated geometry against the sources ----------------------------------------------------------------------------------------------------
def test_restated_constants_and_predicates_are_the_sources():
    ft, hd, fh, sl = _src('frame_transform.h'), _src('heads.hip'), _src('frame_head.hip'), _src('skinny_linear.h')
    num = lambda pat, s: int(re.search(pat, s).group(1))
    assert num(r'#define PIVP_CP_TR (\d+)', ft) == C.BAND_TR == num(r'constexpr int FH_TR = (\d+);', fh)
    assert re.search(r'constexpr int CDNA_KL = 11 \* 28;', ft) and C.CDNA_KL == 308
    assert num(r'constexpr int LIN_KS = (\d+);', sl) == C.LIN_KS and num(r'constexpr int LIN_BG = (\d+);', sl) == C.LIN_BG
    assert num(r'constexpr int FH_MAXKS = (\d+);', fh) == C.FH_MAXKS
    assert (num(r'constexpr int FH_XP = (\d+);', fh), num(r'constexpr int FH_HP = (\d+);', fh), num(r'constexpr int FH_WP = (\d+);', fh),
            num(r'constexpr int FH_HW = (\d+);', fh)) == (36, 68, 68, 4)                                  # frame_head_lds_floats' 36, 68, 68, 4
    assert 'rstep = 256 / PW' in ft and 'constexpr int BAND_PR = (BAND_TR + 4 + 2) / 3;' in ft
    assert 'return sizeof(float) * ((size_t)NP * win + 2 * NP * G + 3 * (BAND_TR + 4) * (W + 4) + CDNA_KL);' in ft
    assert 'num_masks < 1 || num_masks > 11 || mode < 0 || mode > 2) return false;' in hd
    assert 'return composite_lds_bytes(W, num_masks) <= 160 * 1024 && W + 4 <= 256;' in hd
    assert 'if (H % FH_TR || (FH_TR * W) % 64 || W + 4 > 256 || num_masks + 1 < 2) return false;' in fh
    assert 'return num_masks >= 1 && num_masks * 25 <= 256;' in hd
    assert 'for (int jx = tid + 768; jx < win; jx += 256)' in hd                                         # the window loop the 248-wide frame is for


def test_the_library_accepts_and_refuses_as_the_table_says():
    """The host-only entries of the built library against the restated predicates (the launching entries' refusals are GPU tests)."""
    import __graft_entry__ as g
    g.build()
    from pivp_amd import _lib
    lib = _lib.load()
    for (m, H, W, NM, zb, K, fin) in C.FRAME_HEAD_CASES:
        fits = lib.pivp_frame_head_fits(C.MODE[m], C.FH_B, H, W, NM, 0 if m == 'dna' else K)
        assert fits == C.frame_head_fits(C.MODE[m], C.FH_B, H, W, NM, K), (m, H, W, NM, K)
    for (entry, m, H, W, NM) in C.REFUSALS:
        if entry == 'frame_head':
            assert lib.pivp_frame_head_fits(C.MODE[m], 2, H, W, NM, 128) == 0
    assert lib.pivp_linear_scratch_floats(3, 200) == (3 * 4 + C.FH_MAXKS) * 256


def test_every_case_is_accepted_or_refused_as_the_table_says():
    for (m, H, W, NM, zb) in C.COMPOSITE_CASES + C.TRACK_CASES:
        assert C.composite_serves(H, W, NM, C.MODE[m]), (m, H, W, NM)
    for (m, H, W, NM, zb, K, fin) in C.FRAME_HEAD_CASES:
        fits = C.frame_head_fits(C.MODE[m], C.FH_B, H, W, NM, K)
        assert fits == (2 if (m != 'dna' and K > 8192) else 1), (m, H, W, NM, K)
        assert fin or m != 'dna'
        assert K % 128 == 0                                                      # hidden5 as (B, 128, K / 128, 1)
        assert C.composite_serves(H, W, NM, C.MODE[m])                           # "where both serve the shape": all of them
    for (K, NM, Bn) in C.GEN_CASES:
        assert C.cdna_kernels_serves(NM) and K > 0 and Bn > 0
    refused = {'composite': lambda m, H, W, NM: not C.composite_serves(H, W, NM, C.MODE[m]), 'cdna_kernels': lambda m, H, W, NM: not C.cdna_kernels_serves(NM),
               'frame_head': lambda m, H, W, NM: not C.frame_head_ok(C.MODE[m], 2, H, W, NM)}
    for (entry, m, H, W, NM) in C.REFUSALS:
        assert refused[entry](m, H, W, NM), (entry, m, H, W, NM)
    # one condition each: the neighbouring shape is served
    assert C.composite_serves(4, 252, 10, 0) and C.composite_serves(8, 16, 11, 0) and C.composite_serves(2, 16, 10, 0) and C.composite_serves(8, 16, 1, 2)
    assert C.cdna_kernels_serves(10) and C.frame_head_ok(0, 2, 8, 16, 10) and C.frame_head_ok(0, 2, 4, 32, 10)
    ids = [C.composite_id(c) for c in C.COMPOSITE_CASES] + [C.track_id(c) for c in C.TRACK_CASES] + [C.frame_head_id(c) for c in C.FRAME_HEAD_CASES] + \
          [C.linear_id(c) for c in C.GEN_CASES + C.STPP_CASES] + [C.heads_id(c) for c in C.HEADS_CASES]
    assert len(set(ids)) == len(ids)


def test_every_stp_case_sends_a_sample_outside_the_frame():
    for (m, H, W, NM, zb) in C.COMPOSITE_CASES + C.TRACK_CASES:
        if m == 'stp':
            out = C.stp_outside_frame(C.make_composite(m, H, W, NM)['aux'], H, W)
            assert 0.10 <= out.max() < 0.9, (H, W, NM, out)                       # ... and no sample wholly outside


def _half_zero(lg):
    assert 0.3 < (lg == 0).mean() < 0.7


def test_every_branch_the_table_names_has_a_case():
    comp = C.COMPOSITE_CASES
    frames = {(H, W) for (_, H, W, _, _) in comp}
    # band_tile_request / band_tile_file: rows per pass, the remaining-rows loop, idle threads
    by_rstep = {r: {(H, W) for (H, W) in frames if C.rstep(W) == r} for r in (1, 2, 3)}
    assert all(by_rstep[r] for r in (1, 2, 3)) and {C.rstep(W) for (H, W) in frames} >= {1, 2, 3}
    assert any(C.rstep(W) >= 3 and C.rstep(W) * 3 >= C.BAND_TR + 4 for (H, W) in frames)                   # no remaining rows
    assert any(C.rstep(W) == 2 for (H, W) in frames) and any(C.rstep(W) == 1 for (H, W) in frames)         # rows 6, 7 / rows 3 .. 7 in the loop
    assert all(256 - C.rstep(W) * (W + 4) > 0 for (H, W) in frames if W != 252) and 256 - C.rstep(252) * 256 == 0   # idle threads; none at the widest
    # the logit window loop: win > 768 in a full band, and not in the two-row band of the widest frame
    assert any(C.logit_window(H, W, NM, 0) > 768 for (_, H, W, NM, _) in comp) and any(C.logit_window(H, W, NM, 0) <= 768 for (_, H, W, NM, _) in comp)
    assert {m for (m, H, W, NM, _) in comp if C.logit_window(H, W, NM, 0) > 768} == {'cdna', 'stp', 'dna'}
    assert C.logit_window(12, 192, 1, 0) > 768 >= C.logit_window(12, 191, 1, 0) and C.logit_window(12, 187, 11, 0) > 768 >= C.logit_window(12, 186, 11, 0)
    # partial last band, one band that is first and last, a middle band
    assert {H % 4 for (H, W) in frames} >= {0, 2} and any(C.bands(H) == 1 for (H, W) in frames) and any(C.bands(H) >= 3 for (H, W) in frames)
    assert any(H % 4 and C.rstep(W) == r for (H, W) in frames for r in (1, 2, 3)) and all(any(H % 4 and C.rstep(W) == r for (H, W) in frames) for r in (1, 2, 3))
    assert {H % 4 for (H, W) in C.TRACK_FRAMES} == {2} and {C.rstep(W) for (H, W) in C.TRACK_FRAMES} == {1, 2, 3}
    # flat softmax: plane-aligned and straddling group counts, NP = 12, NP = 2
    nps = {NM + 1 for (_, _, _, NM, _) in comp}
    assert nps >= {2, 3, 4, 8, 11, 12}
    for NP in C.STRADDLING_NP:
        assert any((H * W) % NP for (_, H, W, NM, _) in comp if NM + 1 == NP), NP
    for NP in (2, 4, 8):
        assert any((H * W) % NP == 0 for (_, H, W, NM, _) in comp if NM + 1 == NP), NP
    assert any(m == 'stp' and NM == 11 for (m, _, _, NM, _) in comp) and any(m == 'stp' and NM == 1 for (m, _, _, NM, _) in comp)
    assert any(m == 'cdna' and NM == 1 for (m, _, _, NM, _) in comp)
    assert {zb for (m, _, _, _, zb) in comp if m == 'stp'} == {0, 1}
    _half_zero(C.make_composite('cdna', 30, 72, 10)['logits'])
    # frame head: tiles per band against the four waves, stp_zero, the generic and the folded instances, the finisher's slice counts
    fh = C.FRAME_HEAD_CASES
    ntile = {W: C.BAND_TR * W // 64 for (_, _, W, _, _, _, _) in fh}
    assert min(ntile.values()) == 1 and any(4 < n < 8 for n in ntile.values()) and max(ntile.values()) == 15 and max(ntile) == 240
    assert not C.frame_head_ok(0, 2, 8, 256, 10)                                                      # 240 is the widest
    assert any(m == 'stp' and zb == 1 and (W, NM) != (64, 10) for (m, _, W, NM, zb, _, _) in fh) and any(m == 'stp' and zb == 1 and (W, NM) == (64, 10) for (m, _, W, NM, zb, _, _) in fh)
    assert {m for (m, _, W, NM, _, _, _) in fh if W == 64 and NM == (1 if m == 'dna' else 10)} == {'cdna', 'stp', 'dna'}
    ks_fin = {C.kslices(K) for (m, _, _, _, _, K, fin) in fh if fin and m != 'dna'}
    assert ks_fin >= {2, 90, 128} and any(k % 32 and k % 4 for k in ks_fin) and max(ks_fin) == C.FH_MAXKS
    assert any(C.kslices(K) > C.FH_MAXKS and not fin for (m, _, _, _, _, K, fin) in fh if m != 'dna')
    assert {fin for (m, _, _, _, _, K, fin) in fh if m != 'dna' and C.kslices(K) <= C.FH_MAXKS} == {True, False}
    # skinny linear: a second batch group of one sample, the clamped tail of sum_partials, a partial K slice, nout = 25
    lin = [(K, Bn) for (K, NM, Bn) in C.GEN_CASES] + list(C.STPP_CASES)
    assert {Bn % 16 for (K, Bn) in lin} >= {0, 1} and any(Bn > 16 and Bn % 16 == 1 for (K, Bn) in lin) and any(Bn > 32 for (K, Bn) in lin)
    assert {C.kslices(K) % 32 for (K, Bn) in lin} >= {0, 2, 4, 26} and any(K % 64 for (K, Bn) in lin) and any(C.kslices(K) > 32 and C.kslices(K) % 32 for (K, Bn) in lin)
    assert {NM for (K, NM, Bn) in C.GEN_CASES} == {1, 10}
    # 1x1 heads: a partial block, a wave across two samples, waves past the end, NP = 12
    hd = C.HEADS_CASES
    assert any((Bn * HW) % 256 for (Bn, HW, _, _) in hd) and any(HW % 64 and Bn > 1 for (Bn, HW, _, _) in hd) and any((Bn * HW) % 64 for (Bn, HW, _, _) in hd)
    assert any(-(-(Bn * HW) // 256) * 256 - Bn * HW >= 64 for (Bn, HW, _, _) in hd)                      # a wave with px0 >= total_px
    assert {NM + 1 for (_, _, NM, _) in hd} >= {2, 11, 12} and {m for (_, _, _, m) in hd} == {'cdna', 'stp', 'dna'}
