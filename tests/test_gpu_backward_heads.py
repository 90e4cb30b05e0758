"""GPU parity tests of the head-side backward kernels (csrc/backward_heads.hip), one op at a time through the C ABI, against the float64
autograd reference of tests/heads_bwd_reference.py on the same fp32 inputs.  Gate: the per-op backward gate of test_gpu_backward_ops.py,
max|got - ref| / max|ref| < 2e-5, on EVERY element of EVERY output (nothing is masked out).  Overwritten outputs start as NaN and accumulated ones
from a random prior, so a missing write or a stray overwrite fails the gate.  The input conditions the comparison rests on (no threshold within
1e-6, no sampling coordinate on a pixel centre) are asserted for every case by tests/test_backward_heads_host.py, on the CPU.

Every gated figure is printed (`pytest -s`) before it is asserted; profiles/r10/NOTES.md has the worst figure per op from the MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_bwd_reference as R  # noqa: E402

GATE = 2e-5
BADARG = -1


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd  # noqa: F401
    import heads_bwd_ops
    return heads_bwd_ops


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


def _gate(what, got, ref, gate=GATE):
    r = _rel(got, ref)
    print('%-64s %.3e' % (what, r))
    assert r < gate, (what, r)          # (a NaN -- an element the kernel never wrote -- fails this comparison too)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _prior(shape, seed):
    return R.f32(np.random.RandomState(seed).randn(*shape))


# ---- composite backward, CDNA: the folded 64x64x10 instance, the generic 8-row one, the 4-row one for W > 64 ---------------------------------
@pytest.mark.parametrize('H,W,NM,B', R.CDNA_CASES)
def test_composite_backward_cdna(ops, H, W, NM, B):
    d = R.make_composite('cdna', H, W, NM, B)
    ref = R.ref_composite('cdna', d['prev'], d['logits'], d['layer0'], d['aux'], d['go'], H, W)
    prior = _prior((B, 3, H * W), 1)
    tag = 'cdna %dx%d NM=%d B=%d ' % (H, W, NM, B)
    for mode in ('null', 'overwrite', 'accum'):
        rc, o = ops.composite_backward('cdna', d, H, W, NM, dprev_prior=prior if mode == 'accum' else None, dprev_accum=int(mode == 'accum'),
                                       want_dprev=mode != 'null')
        assert rc == 0
        assert o['part'].shape[1] == R.tiles(H, W)
        _gate(tag + mode + ' dmk', o['dmk'], ref['dmk'])
        _gate(tag + mode + ' dz', o['dz'], ref['dz'])
        # the tiles' partial sums added on the host; the unused last kernel's slots are not read
        _gate(tag + mode + ' dkern', o['part'].astype(np.float64).sum(1)[:, :(NM - 1) * 25].reshape(B, NM - 1, 25), ref['daux'])
        if mode == 'overwrite':
            _gate(tag + mode + ' dprev', o['dprev'], ref['dprev'])
        elif mode == 'accum':
            _gate(tag + mode + ' dprev', o['dprev'].astype(np.float64) - prior, ref['dprev'])


# ---- composite backward, STP: whole-frame LDS window, +-12-row window with global atomics outside it, fixed-point accumulator -------------------
# Which of the first two a 'plain' launch runs is the launcher's choice, restated by R.stp_plain_whole and pinned to the source on the host: the
# float window runs at (96, 64, NM = 10) (8-row instance) and at (64, 128) for every NM (4-row instance); the other plain cases keep the whole frame
# in LDS.  The 'det' launches run the fixed-point window on every frame.
@pytest.mark.parametrize('H,W,NM,zb,far', R.STP_CASES)
def test_composite_backward_stp(ops, H, W, NM, zb, far):
    B = R.STP_B
    d = R.make_composite('stp', H, W, NM, B, far)
    ref = R.ref_composite('stp', d['prev'], d['logits'], d['layer0'], d['aux'], d['go'], H, W, stp_zero=zb)
    prior = _prior((B, 3, H * W), 2)
    tag = 'stp %dx%d NM=%d zero=%d theta=%d (plain: %s) ' % (H, W, NM, zb, far, 'whole frame' if R.stp_plain_whole(H, W, NM) else 'window')
    runs = {}
    for mode in ('plain', 'det', 'det2', 'null'):
        rc, o = ops.composite_backward('stp', d, H, W, NM, dprev_prior=prior, dprev_accum=1, want_dprev=mode != 'null', stp_zero=zb,
                                       det=mode.startswith('det'))
        assert rc == 0
        runs[mode] = o
        if mode == 'det2':
            continue
        _gate(tag + mode + ' dmk', o['dmk'], ref['dmk'])
        _gate(tag + mode + ' dz', o['dz'], ref['dz'])
        _gate(tag + mode + ' dtheta', o['part'].astype(np.float64).sum(1)[:, :6], ref['daux'])
        if mode != 'null':
            _gate(tag + mode + ' dprev', o['dprev'].astype(np.float64) - prior, ref['dprev'])
    for k in ('dmk', 'dz', 'dprev'):
        assert _same_bits(runs['det'][k], runs['det2'][k]), k                  # two deterministic calls: the same bits
    assert _same_bits(runs['det']['part'][:, :, :6], runs['det2']['part'][:, :, :6])
    assert not runs['det']['acc'].any() and not runs['det2']['acc'].any()      # the accumulator is handed back all zero
    for k in ('dmk', 'dz'):                                                     # without d prev: the other outputs are what they were
        assert _same_bits(runs['null'][k], runs['plain'][k]), k
    assert _same_bits(runs['null']['part'][:, :, :6], runs['plain']['part'][:, :, :6])


@pytest.mark.parametrize('det', [0, 1])
def test_composite_backward_stp_small_cotangent(ops, det):
    """The windowed and the fixed-point scatter with a cotangent of 1e-6: the same relative gate (2^-48 is 3.6e-9 of 1e-6).  Onto a zero prior:
    an O(1) prior would round the sum to 6e-8, far above this gradient's scale."""
    H, W, NM, zb, far, B = 96, 64, 10, 0, 1, R.STP_B
    d = R.make_composite('stp', H, W, NM, B, far)
    d['go'] = R.f32(d['go'] * np.float32(1e-6))
    ref = R.ref_composite('stp', d['prev'], d['logits'], d['layer0'], d['aux'], d['go'], H, W, stp_zero=zb)
    rc, o = ops.composite_backward('stp', d, H, W, NM, dprev_prior=np.zeros((B, 3, H * W), np.float32), dprev_accum=1, stp_zero=zb, det=bool(det))
    assert rc == 0
    tag = 'stp 96x64 go*1e-6 det=%d ' % det
    _gate(tag + 'dprev', o['dprev'], ref['dprev'])
    _gate(tag + 'dmk', o['dmk'], ref['dmk'])
    _gate(tag + 'dz', o['dz'], ref['dz'])
    _gate(tag + 'dtheta', o['part'].astype(np.float64).sum(1)[:, :6], ref['daux'])


# ---- composite backward, DNA ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,B', R.DNA_CASES)
def test_composite_backward_dna(ops, H, W, B):
    d = R.make_composite('dna', H, W, 1, B)
    ref = R.ref_composite('dna', d['prev'], d['logits'], None, d['aux'], d['go'], H, W)
    prior = _prior((B, 3, H * W), 3)
    tag = 'dna %dx%d B=%d ' % (H, W, B)
    for mode in ('null', 'overwrite', 'accum'):
        rc, o = ops.composite_backward('dna', d, H, W, 1, dprev_prior=prior if mode == 'accum' else None, dprev_accum=int(mode == 'accum'),
                                       want_dprev=mode != 'null')
        assert rc == 0
        _gate(tag + mode + ' dmk', o['dmk'], ref['dmk'])
        _gate(tag + mode + ' dz', o['dz'], ref['dz'])
        if mode == 'overwrite':
            _gate(tag + mode + ' dprev', o['dprev'], ref['dprev'])
        elif mode == 'accum':
            _gate(tag + mode + ' dprev', o['dprev'].astype(np.float64) - prior, ref['dprev'])


# ---- flat softmax + ReLU backward: 256 groups per block over planar data -----------------------------------------------------------------------
@pytest.mark.parametrize('NP,B,HW', R.SOFTMAX_CASES)
def test_mask_softmax_backward(ops, NP, B, HW):
    d = R.make_mask_softmax(NP, B, HW)
    rc, got = ops.mask_softmax_backward(d['logits'], d['dmk'])
    assert rc == 0
    _gate('softmax NP=%d B=%d HW=%d dlogits' % (NP, B, HW), got, R.ref_mask_softmax(d['logits'], d['dmk']))


# ---- 1x1 heads backward: 512-pixel blocks over the flat B*HW range ---------------------------------------------------------------------------------
@pytest.mark.parametrize('NP,NE,B,HW', R.HEADS_CASES)
def test_heads_backward(ops, NP, NE, B, HW):
    d = R.make_heads(NP, NE, B, HW)
    ref = R.ref_heads(d['e6'], d['wm'], d['we'], d['dpm'], d['dpe'], B, HW)
    tag = 'heads NP=%d NE=%d B=%d HW=%d ' % (NP, NE, B, HW)
    runs = {}
    for mode in ('plain', 'det', 'det2'):
        rc, o = ops.heads_backward(d, B, HW, det=mode != 'plain')
        assert rc == 0
        runs[mode] = o
        if mode == 'det2':
            continue
        _gate(tag + mode + ' de6', o['de6'], ref['de6'])
        for k, p in zip(('dwm', 'dbm', 'dwe', 'dbe'), d['prior']):
            _gate(tag + mode + ' ' + k, o[k].astype(np.float64) - p, ref[k])
    for k in runs['det']:
        assert _same_bits(runs['det'][k], runs['det2'][k]), k


# ---- CDNA kernel generator backward: 32 samples per pass of the data gradient ----------------------------------------------------------------------
@pytest.mark.parametrize('K,NM,B,ntiles', R.GEN_CASES)
def test_cdna_kernels_backward(ops, K, NM, B, ntiles):
    d = R.make_cdna_kernels(K, NM, B, ntiles)
    ref = R.ref_cdna_kernels(d['hidden5'], d['wt'], d['vpre'], d['dkpart'], NM)
    tag = 'generator K=%d NM=%d B=%d tiles=%d ' % (K, NM, B, ntiles)
    last = slice((NM - 1) * 25, NM * 25)
    for accum_dx in (0, 1):
        for det in (False, True):
            rc, o = ops.cdna_kernels_backward(d, NM, accum_dx, det=det)
            assert rc == 0
            t = tag + 'accum=%d det=%d ' % (accum_dx, det)
            _gate(t + 'dv', o['dv'], ref['dv'])
            _gate(t + 'dhidden5', o['dx'].astype(np.float64) - (d['prior_dx'] if accum_dx else 0.0), ref['dx'])
            _gate(t + 'dwt', o['dwt'].astype(np.float64) - d['prior_dwt'], ref['dwt'])
            _gate(t + 'db', o['db'][:NM * 25].astype(np.float64) - d['prior_db'][:NM * 25], ref['db'])
            # the last generated kernel never reaches the output (TM:726): exactly no gradient, like the padding columns
            assert not o['dv'][:, (NM - 1) * 25:].any()
            assert _same_bits(o['dwt'][:, (NM - 1) * 25:], d['prior_dwt'][:, (NM - 1) * 25:])
            assert _same_bits(o['db'][last], d['prior_db'][last]) and _same_bits(o['db'][NM * 25:], d['prior_db'][NM * 25:])


# ---- STP regressor backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,B,ntiles', R.STPP_CASES)
def test_stp_params_backward(ops, K, B, ntiles):
    d = R.make_stp_params(K, B, ntiles)
    ref = R.ref_stp_params(d['hidden5'], d['wt1'], d['s1'], d['w2'], d['dthpart'])
    tag = 'regressor K=%d B=%d tiles=%d ' % (K, B, ntiles)
    for det in (False, True):
        rc, o = ops.stp_params_backward(d, det=det)
        assert rc == 0
        t = tag + 'det=%d ' % det
        _gate(t + 'dv', o['dv'], ref['dv'])
        _gate(t + 'dhidden5', o['dx'], ref['dx'])
        _gate(t + 'dwt1', o['dwt1'].astype(np.float64) - d['prior_dwt1'], ref['dwt1'])
        for k, p in zip(('db1', 'dw2', 'db2'), d['prior']):
            _gate(t + k, o[k].astype(np.float64) - p, ref[k])
        assert not o['dv'][:, 100:].any()
        assert _same_bits(o['dwt1'][:, 100:], d['prior_dwt1'][:, 100:])


# ---- enc3 + state predictor backward: 64-pixel tiles, partial last tile --------------------------------------------------------------------------
@pytest.mark.parametrize('HW8,use_state,B', R.ENC3_CASES)
def test_enc3_state_backward(ops, HW8, use_state, B):
    d = R.make_enc3(HW8, use_state, B)
    for mask_e2 in (0, 1):
        ref = R.ref_enc3_state(d['e2'], d['action'], d['state'], d['w3'], d['b3'], d['wcs'], d['de3'], d['dsnew'], use_state, mask_e2)
        for ldd3 in (64, 192):
            for det in (False, True):
                rc, o = ops.enc3_state_backward(d, use_state, mask_e2, ldd3, det=det)
                assert rc == 0
                t = 'enc3 HW8=%d state=%d B=%d mask=%d ld=%d det=%d ' % (HW8, use_state, B, mask_e2, ldd3, det)
                _gate(t + 'de2', o['de2'], ref['de2'])
                for k, p in zip(('dw3', 'db3', 'dwcs', 'dbcs', 'dstate'), d['prior']):
                    _gate(t + k, o[k].astype(np.float64) - p, ref[k])


# ---- enc0 backward: the weight gradient's grid is capped at 512 blocks (first hit at B = 33 on 64x64) -------------------------------------------
@pytest.mark.parametrize('B,H,W', R.ENC0_CASES)
def test_enc0_backward(ops, B, H, W):
    d = R.make_enc0(B, H, W)
    ref = R.ref_enc0(d['img'], d['w'], d['d'], B, H, W)
    for dimg_mode in (None, 0, 1):
        for det in (False, True):
            rc, o = ops.enc0_backward(d, B, H, W, dimg_mode, det=det)
            assert rc == 0
            t = 'enc0 B=%d %dx%d dimg=%s det=%d ' % (B, H, W, dimg_mode, det)
            _gate(t + 'dw', o['dw'].astype(np.float64) - d['prior'][0], ref['dw'])
            _gate(t + 'db', o['db'].astype(np.float64) - d['prior'][1], ref['db'])
            if dimg_mode is not None:
                _gate(t + 'dimg', o['dimg'].astype(np.float64) - (d['prior'][2] if dimg_mode else 0.0), ref['dimg'])


# ---- refusals: PIVP_ERR_BADARG before anything is launched (the NaN-filled outputs stay NaN) -------------------------------------------------------
def test_refusals(ops):
    from pivp_amd import _lib
    lib = _lib.load()
    rc, o = ops.composite_backward('cdna', R.make_composite('cdna', 8, 256, 10, 1), 8, 256, 10)            # W = 256: the tile's window outgrows the block
    assert rc == BADARG and np.isnan(o['dmk']).all() and np.isnan(o['dz']).all() and np.isnan(o['dprev']).all()
    for NM in (1, 11):
        d = R.make_composite('stp', 16, 16, NM, 1)
        rc, o = ops.composite_backward('stp', d, 16, 16, NM, dprev_prior=np.zeros((1, 3, 256), np.float32), dprev_accum=1)
        assert rc == BADARG and np.isnan(o['dmk']).all() and not o['dprev'].any()
    rc, o = ops.heads_backward(R.make_heads(8, 25, 1, 64), 1, 64)                                          # NP + NE = 33
    assert rc == BADARG and np.isnan(o['de6']).all()
    d = R.make_enc0(1, 16, 16)
    d['prior'][2] = d['prior'][2][:, :, :15 * 16]
    rc, o = ops.enc0_backward(d, 1, 15, 16, 1)                                                              # a data gradient on an odd height
    assert rc == BADARG and _same_bits(o['dw'], d['prior'][0]) and _same_bits(o['dimg'], d['prior'][2])
    # a null required pointer
    m = R.make_mask_softmax(4, 1, 64)
    lg = ops.dev(m['logits'])
    assert lib.pivp_mask_softmax_backward(lg.data_ptr(), None, 1, 64, 4, None) == BADARG
    assert lib.pivp_mask_softmax_backward(None, lg.data_ptr(), 1, 64, 4, None) == BADARG
    # (one NaN buffer stands for every argument and is smaller than these shapes ask for, on purpose: the pointers are checked before anything
    # else, so nothing may be launched and nothing may touch it)
    buf = ops.nan(1, 5, 256)
    assert lib.pivp_composite_backward(0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(),
                                       buf.data_ptr(), None, 0, 1, 16, 16, 4, 0, None, None) == BADARG
    assert lib.pivp_enc0_backward(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), None, 0, 1, 16, 16, None, None) == BADARG
    torch.cuda.synchronize()
    assert np.isnan(buf.cpu().numpy()).all()
