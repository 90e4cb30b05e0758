"""GPU parity tests of the forward head kernels off the 64x64 grid: pivp_composite, pivp_pixel_track, pivp_frame_head, pivp_cdna_kernels,
pivp_stp_params and pivp_heads, one op at a time through the C ABI, against the float64 forwards of tests/heads_bwd_reference.py evaluated from
the fp32 arrays the kernel is handed.  The cases, their inputs and the references are tests/heads_fwd_cases.py's; each case's id names the branch
it exists for, and tests/test_heads_fwd_host.py asserts on the CPU that every named branch has a case.

Gates: those the 64x64 tests of the same ops hold (tests/test_gpu_ops.py), absolute on O(1) values, unchanged: masks 1e-6, CDNA / DNA out 1e-5,
STP out 3e-5, heads (and norm_enc6) 2e-5, cdna_kernels 1e-6, stp_params 1e-5.  Every gated figure is printed (`pytest -s`) before it is asserted,
and the worst per quantity at the end of the module.

Worst figures on the MI355X over all cases of each table (max |got - float64|, and the case that gave it):
  composite      masks 4.8e-07 (cdna 12x248 NM10)   out CDNA 4.4e-07 (16x128 NM7)   STP 6.2e-07 (16x128 NM11 clamp)   DNA 2.6e-07 (12x248)
  pixel_track    CDNA 1.8e-07 (30x72 NM10)   STP 2.9e-07 (10x100 NM10 clamp)   DNA 1.2e-07 (30x72)
  frame_head     enc6 1.0e-06 (8x240)   logits 2.0e-06 (8x128 NM1)   enc7 1.2e-06 (dna 64x64)   layer0 1.4e-07   masks 2.9e-07 (stp 8x128 NM11)
                 out CDNA 2.5e-07 (64x64)   STP 3.9e-07 (8x48 NM11 clamp)   DNA 2.4e-07 (64x64)   kerns 1.1e-07 (4x16, KS 2)   theta 6.1e-08 (16x80, KS 128)
  cdna_kernels   1.3e-07 (K 200, B 33)        stp_params 1.3e-07 (K 8192, B 33); at K = 16384 1.1e-07 / 1.2e-07: the gates hold there as at 8192
  heads          logits 7.7e-07 (B3 HW2160 NP11)   enc7 1.1e-06 (dna B2 HW4096)   layer0 1.4e-07
No case needs a looser gate than the 64x64 test of its op; the nearest is frame_head logits at a tenth of its gate.

What the value mutations of the shared code do to this file (each applied alone, the library rebuilt, this file run once):
  cdna_kernel_paired k < NM for k < NM - 1        the 36 CDNA cases of composite and pixel_track fail, through _without_last_kernel only: the extra
                                                  kernel meets a zero mask, so only a non-finite tap shows it; no 64x64 test of tests/test_gpu_ops.py fails
  stp_gather with wu1 and wv1 swapped             every STP case of composite, pixel_track and frame_head (62)
  window loop from tid + 1024 for tid + 768       every case 248 or 252 wide, frame_head's 240-wide through its bit-equality (45); no test narrower than 188 can
  FlatSoftmax::groups < glast for <= glast        every case with masks (162); the 64x64 tests fail as well, the last group of a band holds pixels at any shape"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_fwd_cases as C  # noqa: E402

GATE_MASKS, GATE_OUT, GATE_OUT_STP, GATE_HEADS, GATE_KERNS, GATE_THETA = 1e-6, 1e-5, 3e-5, 2e-5, 1e-6, 1e-5
BADARG = -1
SENTINEL = -7.0


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd  # noqa: F401
    import hip_ops
    import track_ops
    hip_ops.track = track_ops
    return hip_ops


@pytest.fixture(scope='module')
def worst():
    w = {}
    yield w
    for k in sorted(w):
        print('WORST %-40s %.3e  (%s)' % (k, w[k][0], w[k][1]))


def _gate(worst, quantity, case_id, got, ref, gate):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), (quantity, case_id)
    err = np.abs(got - ref).max()
    print('%-28s %-80s %.3e' % (quantity, case_id, err))
    if quantity not in worst or err > worst[quantity][0]:
        worst[quantity] = (err, case_id)
    assert err < gate, (quantity, case_id, err)


def _out_gate(model):
    return GATE_OUT_STP if model == 'stp' else GATE_OUT


# ---- composite -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.COMPOSITE_CASES, ids=C.composite_id)
def test_composite(ops, worst, case):
    model, H, W, NM, zb = case
    cid = C.composite_id(case)
    d = C.make_composite(model, H, W, NM)
    out, masks = ops.composite(d['prev'], d['logits'], d['layer0'], d['aux'], NM, C.MODE[model], zb)
    mk = C.ref_masks(d['logits'])
    _gate(worst, 'composite masks', cid, masks, mk, GATE_MASKS)
    _gate(worst, 'composite out ' + model, cid, out, C.ref_composite(model, d['prev'], mk, d['layer0'], d['aux'], zb), _out_gate(model))
    if model == 'cdna':
        out2, _ = ops.composite(d['prev'], d['logits'], d['layer0'], _without_last_kernel(d['aux']), NM, 0, 0)
        assert np.array_equal(out, out2)


def _without_last_kernel(kerns):
    """zip truncation (TM:725): the last generated kernel pairs with no mask.  composite_kernel and pixel_track_kernel leave it out of the blend
    (cdna_kernel_paired), they do not weigh it with a zero: NaNs in its place must not reach the output."""
    k = kerns.copy()
    k[:, -1] = np.nan
    return k


@pytest.mark.parametrize('H,W', [(H, W) for (H, W, _) in C.COMPOSITE_FRAMES])
def test_composite_constant_logits_give_equal_masks(ops, H, W):
    for model, NM in (('cdna', 10), ('stp', 11), ('dna', 1)):
        d = C.make_composite(model, H, W, NM)
        _, masks = ops.composite(d['prev'], np.full_like(d['logits'], 0.25), d['layer0'], d['aux'], NM, C.MODE[model], 0)
        assert np.abs(masks - 1.0 / (NM + 1)).max() < 1e-7, (model, H, W)


# ---- pixel track -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.TRACK_CASES, ids=C.track_id)
def test_pixel_track(ops, worst, case):
    model, H, W, NM, zb = case
    cid = C.track_id(case)
    d = C.make_track(model, H, W, NM, P=8)
    got = ops.track.pixel_track(d['planes'], d['masks'], d['aux'], NM, C.MODE[model], zb)
    _gate(worst, 'pixel_track ' + model, cid, got, C.ref_composite(model, d['planes'], d['masks'], None, d['aux'], zb), _out_gate(model))
    one = ops.track.pixel_track(d['planes'][:, :1], d['masks'], d['aux'], NM, C.MODE[model], zb)
    assert np.array_equal(one[:, 0], got[:, 0])                                   # P = 1 is plane 0 of P = 8
    if model == 'cdna':
        assert np.array_equal(ops.track.pixel_track(d['planes'], d['masks'], _without_last_kernel(d['aux']), NM, 0, 0), got)


# ---- frame head ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.FRAME_HEAD_CASES, ids=C.frame_head_id)
def test_frame_head(ops, worst, case):
    model, H, W, NM, zb, K, finisher = case
    cid = C.frame_head_id(case)
    mt = C.MODE[model]
    d = C.make_frame_head(model, H, W, NM, K)
    sep, fused = ops.frame_head_pair(d['e6raw'], d['gamma'], d['beta'], 1e-6, d['Wm'], d['bm'], d['We'], d['be'], d['prev'], d['h5'], d['Wh'], d['bh'],
                                     d['W2'], d['b2'], NM, mt, zb, finisher, True)
    in_kernel = fused['kerns'] is not None
    assert model == 'dna' or in_kernel == (finisher and C.frame_head_fits(mt, C.FH_B, H, W, NM, K) == 1)
    # (1) norm_enc6 + ReLU + the 1x1 heads, from the raw input
    e6 = C.layer_norm_relu(d['e6raw'], d['gamma'], d['beta'], 1e-6)
    lg, e7, l0 = C.ref_heads(e6, d['Wm'], d['bm'], d['We'], d['be'], model)
    _gate(worst, 'frame_head enc6', cid, fused['enc6'], e6.numpy(), GATE_HEADS)
    _gate(worst, 'frame_head logits', cid, fused['logits'], lg, GATE_HEADS)
    _gate(worst, 'frame_head enc7', cid, fused['enc7'], e7, GATE_HEADS)
    if model != 'dna':
        _gate(worst, 'frame_head layer0', cid, fused['layer0'], l0, GATE_HEADS)
    # (2) the motion head's generator (the in-kernel finisher's output, or the separate finisher's that went in through aux)
    aux = None
    if model != 'dna':
        aux = (fused['kerns'] if in_kernel else sep['kerns']).reshape((C.FH_B, NM, 5, 5) if model == 'cdna' else (C.FH_B, 6))
        x, wt = C.h5_flat(d['h5']), C.wt_of(d['Wh'])
        if model == 'cdna':
            _gate(worst, 'frame_head kerns', cid, aux.reshape(C.FH_B, NM, 25), C.ref_cdna_kernels(x, wt, d['bh'], NM), GATE_KERNS)
        else:
            _gate(worst, 'frame_head theta', cid, aux, C.ref_stp_params(x, wt, d['bh'], d['W2'], d['b2']), GATE_THETA)
            assert C.stp_outside_frame(aux, H, W).max() >= 0.10
    # (3) softmax + transform + compositing, from the fused launch's OWN fp32 logits, layer0 / enc7 and kernels / theta
    mk = C.ref_masks(fused['logits'])
    _gate(worst, 'frame_head masks', cid, fused['masks'], mk, GATE_MASKS)
    ref = C.ref_composite(model, d['prev'], mk, None if model == 'dna' else fused['layer0'], fused['enc7'] if model == 'dna' else aux, zb)
    _gate(worst, 'frame_head out ' + model, cid, fused['out'], ref, _out_gate(model))
    # (4) and bit for bit the separate kernels'
    for k in ('out', 'masks', 'enc7', 'logits', 'enc6') + (() if model == 'dna' else ('layer0',)):
        assert np.array_equal(sep[k], fused[k]), (k, np.abs(sep[k] - fused[k]).max())
    if in_kernel:
        assert np.array_equal(sep['kerns'].reshape(C.FH_B, -1), fused['kerns'].reshape(C.FH_B, -1))
    assert np.all(np.isfinite(fused['stat'])) and np.all(fused['stat'][:, 1] > 0)


# ---- skinny linear -----------------------------------------------------------------------------------------------------------------------------------
def _skinny_call(fn, key, d, nout, K, *more):
    """Through checkpoint.to_internal where it can lay the operand out (K a multiple of 128), else the K-major operand as it is."""
    import pivp_amd
    if K % 128:
        return fn(d['x'], d['wt'], *more, internal=True)
    Bn = d['x'].shape[0]
    h5 = np.ascontiguousarray(d['x'].reshape(Bn, K // 128, 128).transpose(0, 2, 1)).reshape(Bn, 128, K // 128, 1)
    W = pivp_amd.from_internal(key, d['wt'].ravel(), (nout, K))
    assert np.array_equal(C.wt_of(W), d['wt'][:, :nout]) and np.array_equal(C.h5_flat(h5), d['x'])
    return fn(h5, W, *more)


@pytest.mark.parametrize('case', C.GEN_CASES, ids=C.linear_id)
def test_cdna_kernels(ops, worst, case):
    K, NM, Bn = case
    d = C.make_linear(K, 25 * NM, Bn)
    got = _skinny_call(ops.cdna_kernels, 'model/cdna_kerns/W', d, 25 * NM, K, d['b'], NM).reshape(Bn, NM, 25)
    _gate(worst, 'cdna_kernels', C.linear_id(case), got, C.ref_cdna_kernels(d['x'], d['wt'], d['b'], NM), GATE_KERNS)
    assert np.abs(got.astype(np.float64).sum(2) - 1.0).max() < 1e-6


@pytest.mark.parametrize('case', C.STPP_CASES, ids=C.linear_id)
def test_stp_params(ops, worst, case):
    K, Bn = case
    d = C.make_linear(K, 100, Bn)
    got = _skinny_call(ops.stp_params, 'model/stp_input/W', d, 100, K, d['b'], d['w2'], d['b2'])
    _gate(worst, 'stp_params', C.linear_id(case), got, C.ref_stp_params(d['x'], d['wt'], d['b'], d['w2'], d['b2']), GATE_THETA)


# ---- 1x1 heads ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.HEADS_CASES, ids=C.heads_id)
def test_heads(ops, worst, case):
    Bn, HW, NM, model = case
    cid = C.heads_id(case)
    d = C.make_heads(Bn, HW, NM, model)
    logits, enc7, layer0 = ops.heads(d['e6'], d['Wm'], d['bm'], d['We'], d['be'], NM, C.MODE[model])
    lg, e7, l0 = C.ref_heads(d['e6'], d['Wm'], d['bm'], d['We'], d['be'], model)
    _gate(worst, 'heads logits', cid, logits, lg, GATE_HEADS)
    _gate(worst, 'heads enc7', cid, enc7, e7, GATE_HEADS)
    if model != 'dna':
        _gate(worst, 'heads layer0', cid, layer0, l0, GATE_HEADS)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,model,H,W,NM', C.REFUSALS, ids=lambda v: str(v))
def test_refusals_leave_the_outputs_untouched(ops, entry, model, H, W, NM):
    from pivp_amd import _lib
    lib = _lib.load()
    mt = C.MODE[model]
    dev = lambda *shape: torch.full(shape, 0.5, dtype=torch.float32, device=ops.DEV)
    sent = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=ops.DEV)
    Bn, NP, ne = 2, NM + 1, C.NE[model]
    outs = [sent(Bn, 3, H, W), sent(Bn, NP, H, W)]
    if entry == 'composite':
        prev, logits, l0, aux = dev(Bn, 3, H, W), dev(Bn, NP, H, W), dev(Bn, 3, H, W), dev(Bn, 25 * max(NM, H * W))
        rc = lib.pivp_composite(prev.data_ptr(), logits.data_ptr(), l0.data_ptr(), aux.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), Bn, H, W, NM, mt, 0,
                                ops.stream())
    elif entry == 'cdna_kernels':
        K = 128
        x, wt, b, scr = dev(Bn, K), dev(K, 512), dev(512), dev(lib.pivp_linear_scratch_floats(Bn, K))
        outs = [sent(Bn, NM, 25)]
        rc = lib.pivp_cdna_kernels(x.data_ptr(), wt.data_ptr(), b.data_ptr(), scr.data_ptr(), outs[0].data_ptr(), Bn, K, NM, ops.stream())
    else:
        a = _lib.PivpFrameHeadArgs()
        keep = dict(e6raw=dev(Bn, H * W, 64), ln_part=dev(Bn, 64, 4), gamma=dev(H * W, 64), beta=dev(H * W, 64), masks_w=dev(64, NP), masks_b=dev(NP), enc7_w=dev(64, ne),
                    enc7_b=dev(ne), prev=dev(Bn, 3, H, W), aux=dev(Bn, NM, 25))
        outs += [sent(Bn, ne, H, W)]
        for k, v in keep.items():
            setattr(a, k, v.data_ptr())
        a.ln_nparts, a.ln_eps = 1, 1e-6
        a.out, a.masks_out, a.enc7 = [o.data_ptr() for o in outs]
        a.B, a.H, a.W, a.num_masks, a.model_type, a.stp_zero_border = Bn, H, W, NM, mt, 0
        rc = lib.pivp_frame_head(ctypes.byref(a), ops.stream())
    torch.cuda.synchronize()
    assert rc == BADARG, rc
    for o in outs:
        assert torch.all(o == SENTINEL).item()
