"""CPU-side tests of the head-side backward parity suite: the float64 reference forwards of tests/heads_bwd_reference.py against
oracle/restatement.py, torch.autograd.gradcheck on them, the C-ABI surface of the new op entries, and the input conditions every case of
tests/test_gpu_backward_heads.py rests on (so a bad seed fails here, not on the device).  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivp_amd  # noqa: F401
from pivp_amd import _lib
from oracle import restatement as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_bwd_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'pivp_composite_backward_tiles': 2, 'pivp_composite_backward': 18, 'pivp_mask_softmax_backward': 6, 'pivp_heads_backward_det_floats': 4,
       'pivp_heads_backward': 16, 'pivp_cdna_kernels_backward': 15, 'pivp_stp_params_backward': 16, 'pivp_enc3_state_backward_det_floats': 3,
       'pivp_enc3_state_backward': 21, 'pivp_enc0_backward_det_floats': 3, 'pivp_enc0_backward': 12}
T = R.t64


def _close(mine, theirs, tol=1e-12):
    mine = mine.detach().numpy() if isinstance(mine, torch.Tensor) else np.asarray(mine)
    assert mine.shape == theirs.shape, (mine.shape, theirs.shape)
    assert np.abs(mine - theirs).max() <= tol, np.abs(mine - theirs).max()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree_on_the_backward_op_entries():
    import __graft_entry__ as g
    g.build()
    header = open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', header)) - {'pivp_config', 'pivp_plan'}
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    for name, nargs in NEW.items():
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header).group(1)
        assert len(proto.split(',')) == nargs, name                                  # the header's parameter count is the table's
    assert declared == set(_lib.SIGNATURES) and declared <= exported
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17                                              # added without a version change: nothing else moved
    # the host-only entries: the tile count the reference assumes, the scratch sizes, refusals
    for H, W in [(64, 64), (16, 16), (24, 40), (72, 40), (16, 128), (32, 128), (8, 64), (96, 64), (64, 128)]:
        assert lib.pivp_composite_backward_tiles(H, W) == R.tiles(H, W)
    assert lib.pivp_composite_backward_tiles(0, 64) == -1
    assert lib.pivp_heads_backward_det_floats(3, 384, 11, 3) == 3 * 65 * 14 and lib.pivp_heads_backward_det_floats(0, 384, 11, 3) == -1
    assert lib.pivp_enc3_state_backward_det_floats(3, 108, 1) == 6 * (74 * 64 + 64 + 55) + 6 * 5
    assert lib.pivp_enc0_backward_det_floats(33, 64, 64) == 512 * (75 * 32 + 32) and lib.pivp_enc0_backward_det_floats(2, 16, 24) == 3 * (75 * 32 + 32)
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc', 'backward_heads.hip')).read()
    assert int(re.search(r'constexpr int CBS_R = (\d+);', src).group(1)) == R.CBS_R   # the window the far-theta cases are built against
    # ... and the launcher's choice between the whole-frame and the windowed scatter, which R.stp_plain_whole restates
    cond = re.search(r'const int whole = \(!det_acc && whole_on > 0 && dprev && lds_head \+ sizeof\(float\) \* 3 \* \(size_t\)H \* W <= (\d+) \* 1024\)', src)
    assert cond and int(cond.group(1)) * 1024 == R.STP_WHOLE_LDS
    assert re.search(r'const size_t lds_head = sizeof\(float\) \* \(\(size_t\)NP \* win \+ 2 \* NP \* G\);', src)
    assert int(re.search(r'constexpr int whole_on = (\d+);', src).group(1)) > 0


# ---- forward agreement with oracle/restatement.py ---------------------------------------------------------------------------------------------
def _oracle_composite(transformed, prev, logits, NM):
    """TM:720-726 as oracle/restatement.py's Model._step spells it."""
    B, _, H, W = prev.shape
    masks = O.softmax_axis1(logits.reshape(-1, NM + 1)).reshape(B, NM + 1, H, W)
    out = prev * masks[:, 0:1]
    for layer, m in zip(transformed, [masks[:, k:k + 1] for k in range(1, NM + 1)]):
        out = out + layer * m
    return out, masks


def _head_model(kind, NM, K, rs, border='clamp'):
    m = O.Model(NM, is_cdna=kind == 'cdna', is_stp=kind == 'stp', is_dna=kind == 'dna', stp_border=border)
    ne = 25 if kind == 'dna' else 3
    m.p = {'model/enc7/W': np.eye(ne).reshape(ne, ne, 1, 1), 'model/enc7/b': np.zeros(ne),          # enc7 = the given pre-activation
           'model/cdna_kerns/W': rs.randn(NM * 25, K) / np.sqrt(K), 'model/cdna_kerns/b': 0.1 * rs.randn(NM * 25),
           'model/stp_input/W': rs.randn(100, K) / np.sqrt(K), 'model/stp_input/b': 0.1 * rs.randn(100),
           'model/identity_params/W': rs.randn(6, 100) / 10.0, 'model/identity_params/b': 0.05 * rs.randn(6)}
    return m


@pytest.mark.parametrize('H,W,NM', [(8, 8, 3), (6, 10, 10), (8, 8, 1)])
def test_forward_cdna_agrees_with_the_restatement(H, W, NM):
    rs = np.random.RandomState(H + NM)
    B, K = 2, 32
    prev, z, logits, h5 = rs.rand(B, 3, H, W), rs.randn(B, 3, H, W), np.maximum(rs.randn(B, NM + 1, H, W), 0), rs.randn(B, K)
    m = _head_model('cdna', NM, K, rs)
    transformed, enc7 = m._cdna(z, h5, prev)
    want, masks = _oracle_composite(transformed, prev, logits, NM)
    kerns = R.cdna_kernels(T(h5) @ T(m.p['model/cdna_kerns/W']).t() + T(m.p['model/cdna_kerns/b']), NM)
    _close(kerns.reshape(B, NM, 5, 5), m.last_cdna_kerns)
    mk = R.flat_softmax(T(logits))
    _close(mk, masks)
    _close(R.composite_cdna(T(prev), mk, torch.sigmoid(torch.relu(T(z))), kerns), want)


@pytest.mark.parametrize('border', ['clamp', 'zeros'])
@pytest.mark.parametrize('H,W,NM,far', [(8, 8, 3, 0), (6, 10, 10, 1), (8, 12, 2, 2)])
def test_forward_stp_agrees_with_the_restatement(H, W, NM, far, border):
    rs = np.random.RandomState(H + NM)
    B, K = 2, 32
    prev, z, logits, h5 = rs.rand(B, 3, H, W), rs.randn(B, 3, H, W), np.maximum(rs.randn(B, NM + 1, H, W), 0), rs.randn(B, K)
    m = _head_model('stp', NM, K, rs, border)
    m.p['model/identity_params/b'] = m.p['model/identity_params/b'] + R.make_theta(rs, 1, H, far)[0].astype(np.float64) - [1, 0, 0, 0, 1, 0]
    transformed, enc7 = m._stp(z, h5, prev)
    want, _ = _oracle_composite(transformed, prev, logits, NM)
    p = m.p
    theta, s1 = R.stp_regressor(T(h5), T(p['model/stp_input/W']).t(), T(p['model/stp_input/b']), T(p['model/identity_params/W']), T(p['model/identity_params/b']))
    grid = O.spatial_transformer_grid(theta.numpy().reshape(B, 2, 3), (H, W))
    gu, gv = R.stp_coords(theta, H, W)
    _close(gu, grid[:, 0]); _close(gv, grid[:, 1])
    zb = int(border == 'zeros')
    _close(R.stp_sample(T(prev), theta, zb), O.spatial_transformer_sampler(prev, grid, border))
    _close(R.composite_stp(T(prev), R.flat_softmax(T(logits)), torch.sigmoid(T(z)), theta, zb), want)


@pytest.mark.parametrize('H,W', [(8, 8), (6, 10)])
def test_forward_dna_agrees_with_the_restatement(H, W):
    rs = np.random.RandomState(H)
    B = 2
    prev, z, logits = rs.rand(B, 3, H, W), rs.randn(B, 25, H, W), np.maximum(rs.randn(B, 2, H, W), 0)
    m = _head_model('dna', 1, 8, rs)
    transformed, enc7 = m._dna(z, None, prev)
    want, _ = _oracle_composite(transformed, prev, logits, 1)
    _close(R.composite_dna(T(prev), R.flat_softmax(T(logits)), torch.relu(T(z))), want)


def test_forward_small_ops_agree_with_the_restatement():
    rs = np.random.RandomState(5)
    B, h, w = 2, 2, 3
    # enc3: smear + 1x1 conv + ReLU, and the state predictor
    e2, action, state = np.maximum(rs.randn(B, 64, h, w), 0), rs.randn(B, 5), rs.randn(B, 5)
    W3, b3, Wcs, bcs = rs.randn(64, 74, 1, 1), rs.randn(64), rs.randn(5, 10), rs.randn(5)
    sa = np.concatenate((action, state), 1)
    for use_state in (0, 1):
        x = np.concatenate((e2, np.tile(sa.reshape(B, 10, 1, 1), (1, 1, h, w))), 1) if use_state else e2
        Wc = W3 if use_state else W3[:, :64]
        want = O.relu(O.conv2d(x, Wc, b3, 1, 0))
        e3, snew, _ = R.enc3_state(T(e2.transpose(0, 2, 3, 1).reshape(B, h * w, 64)), T(action), T(state), T(Wc[:, :, 0, 0].T), T(b3), T(Wcs), T(bcs),
                                   use_state)
        _close(e3.reshape(B, h, w, 64).permute(0, 3, 1, 2), want)
        _close(snew, O.linear(sa, Wcs, bcs))
    # enc0: 5x5 stride 2 pad 2 with the [75][32] weight
    img, W0, b0 = rs.rand(B, 3, 8, 12), rs.randn(32, 3, 5, 5), rs.randn(32)
    w75 = W0.transpose(2, 3, 1, 0).reshape(75, 32)
    _close(R.enc0_weight(T(w75)), W0)
    _close(R.enc0(T(img), T(w75), T(b0)).permute(0, 3, 1, 2), O.conv2d(img, W0, b0, 2, 2))
    # the 1x1 heads (L.Deconvolution2D with a 1x1 kernel) on NHWC input, planar output
    e6, Wm, bm, We, be = rs.randn(B, 64, 4, 6), rs.randn(64, 11, 1, 1), rs.randn(11), rs.randn(64, 3, 1, 1), rs.randn(3)
    pm, pe = R.heads(T(e6.transpose(0, 2, 3, 1).reshape(-1, 64)), T(Wm[:, :, 0, 0]), T(bm), T(We[:, :, 0, 0]), T(be), B, 24)
    _close(pm.reshape(B, 11, 4, 6), O.deconv2d(e6, Wm, bm)); _close(pe.reshape(B, 3, 4, 6), O.deconv2d(e6, We, be))
    # kernel normalisation
    v = rs.randn(B, 75)
    k = O.relu(v.reshape(B, 3, 25) - 1e-12) + 1e-12
    _close(R.cdna_kernels(T(v), 3), k / k.sum(2, keepdims=True))


# ---- gradcheck ----------------------------------------------------------------------------------------------------------------------------------
def _g(a):
    return T(a, True)


GC_CASES = ['softmax', 'cdna', 'dna', 'small'] + ['stp-%d-%d' % (far, zb) for far in (0, 1, 2) for zb in (0, 1)]


@pytest.mark.parametrize('case', GC_CASES)
def test_gradcheck_on_8x8_inputs(case):
    rs = np.random.RandomState(8)
    B, H, W, NM = 1, 8, 8, 3
    gc = lambda f, *a: torch.autograd.gradcheck(f, a, eps=1e-6, atol=1e-6, rtol=1e-5)
    gcf = lambda f, *a: torch.autograd.gradcheck(f, a, eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)   # the weight-heavy ops: thousands of inputs
    prev, z, pre = rs.rand(B, 3, H, W), rs.randn(B, 3, H, W), 2 * rs.randn(B, NM + 1, H, W)
    mk = R.flat_softmax(torch.relu(T(pre))).numpy()
    if case == 'softmax':
        assert gc(lambda p: R.flat_softmax(torch.relu(p)), _g(pre))
    elif case == 'cdna':
        kerns = R.cdna_kernels(T(rs.randn(B, NM * 25)), NM).numpy()
        assert gc(lambda p, m, zz, k: R.composite_cdna(p, m, torch.sigmoid(torch.relu(zz)), k), _g(prev), _g(mk), _g(z), _g(kerns))
        assert gc(lambda v: R.cdna_kernels(v, NM), _g(rs.randn(B, NM * 25)))
    elif case.startswith('stp'):
        far, zb = int(case[4]), int(case[6])
        theta = R.make_theta(rs, B, H, far)
        assert gc(lambda p, m, zz, th: R.composite_stp(p, m, torch.sigmoid(zz), th, zb), _g(prev), _g(mk), _g(z), _g(theta))
    elif case == 'dna':
        # the frame reaches the output through mask 0 only (the shifted copies are detached, TM:404), so the frame is no gradcheck input
        mk2 = R.flat_softmax(torch.relu(T(pre[:, :2]))).numpy()
        assert gc(lambda m, e: R.composite_dna(T(prev), m, torch.relu(e)), _g(mk2), _g(rs.randn(B, 25, H, W)))
    else:
        assert gcf(lambda x, w1, b1, w2, b2: R.stp_regressor(x, w1, b1, w2, b2)[0], _g(rs.randn(B, 16)), _g(rs.randn(16, 100) / 4), _g(rs.randn(100)),
                   _g(rs.randn(6, 100)), _g(rs.randn(6)))
        for us in (0, 1):
            assert gcf(lambda e2, a, s, w3, b3, wcs, bcs: R.enc3_state(e2, a, s, w3, b3, wcs, bcs, us)[:2], _g(rs.randn(B, 4, 64)), _g(rs.randn(B, 5)),
                       _g(rs.randn(B, 5)), _g(rs.randn(74 if us else 64, 64) / 8), _g(rs.randn(64)), _g(rs.randn(5, 10)), _g(rs.randn(5)))
        assert gcf(R.enc0, _g(rs.rand(B, 3, H, W)), _g(rs.randn(75, 32) / 8), _g(rs.randn(32)))
        assert gcf(lambda e6, wm, bm, we, be: R.heads(e6, wm, bm, we, be, B, 8), _g(rs.randn(B * 8, 64)), _g(rs.randn(64, 4)), _g(rs.randn(4)),
                   _g(rs.randn(64, 3)), _g(rs.randn(3)))


def test_inverted_activations_reproduce_the_saved_ones():
    rs = np.random.RandomState(9)
    z = 1.5 * rs.randn(1000)
    for relu in (False, True):
        l0 = R.f32(torch.sigmoid(torch.relu(T(z)) if relu else T(z)))
        zz = R.z_of_layer0(l0, relu)
        back = torch.sigmoid(torch.relu(zz) if relu else zz).numpy()
        assert np.abs(back - l0.astype(np.float64)).max() < 1e-15
    r = R.f32(np.maximum(rs.randn(1000), 0))
    assert np.array_equal(torch.relu(R.pre_of_relu(r)).numpy(), r.astype(np.float64))


# ---- the input conditions of every GPU case -------------------------------------------------------------------------------------------------
def _half_zero(lg):
    assert 0.3 < (lg == 0).mean() < 0.7 and not ((lg > 0) & (lg < 1e-6)).any()


@pytest.mark.parametrize('H,W,NM,B', R.CDNA_CASES)
def test_input_conditions_cdna(H, W, NM, B):
    d = R.make_composite('cdna', H, W, NM, B)
    R.check_composite('cdna', d, H, W)
    _half_zero(d['logits'])
    assert all(v.dtype == np.float32 for v in d.values())


@pytest.mark.parametrize('H,W,far', R.STP_FRAMES)
def test_input_conditions_stp(H, W, far):
    for NM in (10, 3, 2):
        d = R.make_composite('stp', H, W, NM, R.STP_B, far)
        _half_zero(d['logits'])
        assert np.abs(d['aux'] - np.array([1, 0, 0, 0, 1, 0], np.float32)).max() > 1e-3          # never the exact identity
        # the scatter a plain launch of this case runs: checked, not assumed (a deterministic one is windowed whatever the frame)
        assert R.stp_plain_whole(H, W, NM) == (NM in R.STP_PLAIN_WHOLE[(H, W)]), (H, W, NM)
        for zb in (0, 1):
            assert (H, W, NM, zb, far) in R.STP_CASES
            R.check_composite('stp', d, H, W, zb)
            frac = R.stp_outside_fraction(d['aux'], H, W, zb)
            if far:
                assert frac > R.STP_FAR_OUTSIDE[(H, W, far, zb)], (frac, H, W, far, zb)
            else:
                assert frac < 0.05, frac
    # a frame that runs the float window in plain mode sends more than half of its taps outside it with the far theta itself, in both border modes
    if far and not all(R.stp_plain_whole(H, W, NM) for NM in (10, 3, 2)):
        assert far == 1 and R.STP_FAR_OUTSIDE[(H, W, far, 0)] >= 0.5 and R.STP_FAR_OUTSIDE[(H, W, far, 1)] >= 0.5
    # every far frame has, in each border mode, a theta that sends more than half of its in-frame taps outside the window
    for zb in (0, 1):
        for (h, w) in {(h, w) for (h, w, f) in R.STP_FRAMES if f}:
            assert any(R.STP_FAR_OUTSIDE[(h, w, f, zb)] >= 0.5 for (hh, ww, f) in R.STP_FRAMES if f and (hh, ww) == (h, w))


@pytest.mark.parametrize('H,W,B', R.DNA_CASES)
def test_input_conditions_dna(H, W, B):
    d = R.make_composite('dna', H, W, 1, B)
    R.check_composite('dna', d, H, W)
    _half_zero(d['logits']); _half_zero(d['aux'])


def test_input_conditions_small_ops():
    for NP, B, HW in R.SOFTMAX_CASES:
        _half_zero(R.make_mask_softmax(NP, B, HW)['logits'])
    for K, NM, B, nt in R.GEN_CASES:
        d = R.make_cdna_kernels(K, NM, B, nt)
        R.check_preact(d['vpre'][:, :NM * 25] - 1e-12)
    for K, B, nt in R.STPP_CASES:
        R.check_preact(R.make_stp_params(K, B, nt)['s1'][:, :100])
    for HW8, us, B in R.ENC3_CASES:
        d = R.make_enc3(HW8, us, B)
        R.check_preact(d['pre']); R.check_preact(d['e2'])
        assert np.array_equal(d['e3'] > 0, d['pre'] > 0)                          # fp32 rounding moved no unit across its threshold


def test_both_instances_run_the_float_window_with_a_far_theta():
    """The cases the windowed float scatter is checked by: the 8-row instance at (96, 64, NM = 10), the 4-row one (W > 64) at (64, 128) for every NM,
    each with the far theta in both border modes; the small-cotangent test runs the first of them."""
    windowed = {(H, W, NM) for (H, W, NM, zb, far) in R.STP_CASES if far == 1 and not R.stp_plain_whole(H, W, NM)}
    assert windowed == {(96, 64, 10), (64, 128, 10), (64, 128, 3), (64, 128, 2)}
    assert {R.tile_rows(W) for (H, W, NM) in windowed} == {4, 8}
    for (H, W, NM) in windowed:
        assert all((H, W, NM, zb, 1) in R.STP_CASES and (H, W, NM, zb, 0) in R.STP_CASES for zb in (0, 1))


@pytest.mark.parametrize('H,W,NM,far,zb', [(96, 64, 10, 1, 0), (96, 64, 10, 1, 1), (64, 128, 3, 1, 0), (64, 128, 3, 1, 1), (64, 128, 10, 1, 0)])
def test_far_theta_cases_see_a_dropped_out_of_window_scatter(H, W, NM, far, zb):
    """What the far cases are for: were the scatters outside the tile's window lost, d prev would move by far more than the 2e-5 gate.  On cases
    that a plain launch really runs windowed."""
    assert not R.stp_plain_whole(H, W, NM)
    d = R.make_composite('stp', H, W, NM, R.STP_B, far)
    B = R.STP_B
    g, mk = T(d['go']).reshape(B, 3, H, W), R.flat_softmax(T(d['logits']).reshape(B, NM + 1, H, W))
    grads = []
    for window_only in (False, True):
        pv = T(d['prev'], True)
        (R.stp_sample(pv.reshape(B, 3, H, W), T(d['aux']), zb, window_only) * mk[:, 2:].sum(1, keepdim=True) * g).sum().backward()
        grads.append(pv.grad.numpy())
    full = R.ref_composite('stp', d['prev'], d['logits'], d['layer0'], d['aux'], d['go'], H, W, stp_zero=zb)['dprev']
    assert np.abs(grads[0] - grads[1]).max() / np.abs(full).max() > 1e-2
