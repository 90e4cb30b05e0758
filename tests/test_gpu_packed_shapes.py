"""The packed-operand ConvLSTM kernels (bf16, bf16x3, bf16x6, fp16x3: convlstm_bf16.hip, convlstm_ring.h, convlstm_l2direct.h) on the maps packed_tiles_serve
(wgrad_form.h) accepts beyond the square powers of two of tests/test_gpu_bf16.py, each against the float64 restatement with that file's gates unchanged; then
inference rollouts of the split modes on rectangular frames against the float64 model.

A block decodes its tile from blockIdx.x with three divisions -- by the tiles of the launch, by tpi (tiles per image) and by tpr (tiles per row) -- that the
launcher turns into multiply-high / shift pairs (packed_decode_divisors).  On a square power-of-two map all three divisors are powers of two, a 16-wide tile
row is a whole image row, and on the 8 x 8 map a two-image tile is a whole image pair.  The shapes below are the smallest that leave each of these cases:

  (B, cx, C, H, W)        tiles                                                      grid, 16- / 32-channel blocks
  (1, 32, 32,  8, 48)     16 wide, tpr = 3, odd batch                                     6 /  3
  (3, 32, 64, 24, 16)     16 wide, tpi = 3, tpr = 1, odd batch                           36 / 18
  (2, 32, 32, 40, 32)     16 wide, tpi = 10, tpr = 2 (lstm1 of an 80 x 64 frame)         40 / 20
  (2, 64, 128, 16, 8)     two images, two tile rows (lstm5 of 128 x 64)                  16 /  8
  (4, 32, 32, 24, 8)      two images, tpi = 3, two image pairs                           12 /  6
  (2, 64, 128, 8, 24)     two images, three tiles per row (lstm5 of 64 x 192)            24 / 12
  (2, 32, 32, 16, 40)     two images, tpr = 5, tpi = 10                                  20 / 10

grid = (B / images per tile) * tpi * (C / channels per block).  A grid that is a multiple of 8 takes the kernels' XCD-aware blockIdx remap, any other does
not: with 16-channel blocks 40, 16 and 24 take it and 6, 36, 12, 20 do not; with 32-channel blocks 8 takes it and 3, 18, 20, 6, 12, 10 do not (_grid and the
assertion under SHAPES keep this true).  Two-image tiles with several tiles per row run on both sides (24 / 12), as do 16-wide tiles with tpr = 2 (40 / 20).

The LayerNorm partials of the epilogue are checked image by image: slot trem * n_nblk + nblk under image b0 + ti.  Two images of a tile that wrote each
other's slots, or a tile that wrote the slots of another, would give every image a wrong count, mean or variance.

What fails when an index is wrong (shown on the CPU by breaking the reference instead of a kernel): h and c of an image whose tile origin is misplaced differ
from the reference by O(1) at most pixels against gates of 2e-5 .. 5e-5; with H and W exchanged in the reference's gate reshape every rectangular shape fails;
with the two images' partial slots exchanged in _ln_check the per-image means differ by 4e-4 .. 6e-3 (each is a mean of 6,144 .. 40,960 values of spread 0.3)
against the 1e-6 gate on every shape with B > 1, and a partial written to another tile's slot of its own image breaks that image's count."""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import restatement as R
from test_gpu_bf16 import TOL, _bf16, _lstm_ref

pytestmark = pytest.mark.gpu
BADARG = -1

SHAPES = [(1, 32, 32, 8, 48), (3, 32, 64, 24, 16), (2, 32, 32, 40, 32), (2, 64, 128, 16, 8), (4, 32, 32, 24, 8), (2, 64, 128, 8, 24), (2, 32, 32, 16, 40)]
REFUSED = [(1, 32, 32, 8, 24), (3, 32, 32, 16, 40), (2, 32, 32, 12, 16)]      # 8-wide tiles with an odd batch (twice); a height that is no multiple of 8
CONCAT = (2, 64, 128, 8, 24)


def _tiles(B, H, W):
    """(images per tile, tiles per image, tiles per row) as the kernels take them from the map"""
    tw = 16 if W % 16 == 0 else 8
    return (1 if tw == 16 else 2), (H // 8) * (W // tw), W // tw


def _grid(shape, nch):
    B, cx, C, H, W = shape
    ti_n, tpi, _ = _tiles(B, H, W)
    return (B // ti_n) * tpi * (C // nch)


for _nch in (16, 32):      # both sides of `(gridDim.x & 7) == 0` for either block width
    assert {_grid(s, _nch) % 8 == 0 for s in SHAPES} == {True, False}, _nch


def _sid(s):
    return 'B%d-%d+%d-%dx%d' % s


def _nid(n):
    return 'nch%d' % n


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import hip_ops
    return hip_ops


def _case(B, cx, C, H, W, seed):
    """test_gpu_bf16._case with a width of its own"""
    rs = np.random.RandomState(seed)
    x = rs.randn(B, cx, H, W); h = rs.randn(B, C, H, W) * 0.5; c = rs.randn(B, C, H, W)
    Wt = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
    return x, h, c, Wt, b


_CASES = {}


def _operands(shape, kind):
    """One input per shape and operand kind ('bf16': x, h and the weights are bf16 numbers; 'f32': every operand is an fp32 number) with its float64 results
    (h, c, gates) for the given h and for h = 0: computed once, shared by every test of the shape, left unchanged."""
    if (shape, kind) not in _CASES:
        B, cx, C, H, W = shape
        x, h, c, Wt, b = _case(B, cx, C, H, W, 1000 + 97 * B + 31 * C + 7 * H + W)
        if kind == 'bf16':
            x, h, Wt = _bf16(x), _bf16(h), _bf16(Wt)
        else:
            x, h, c, Wt, b = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in (x, h, c, Wt, b)]
        t0 = time.time()
        ref, ref0 = _lstm_ref(x, h, c, Wt, b), _lstm_ref(x, h * 0, c, Wt, b)
        print('float64 reference %s %s: %.2f s for two cells' % (_sid(shape), kind, time.time() - t0))
        for a in (x, h, c, Wt, b) + ref[:2] + ref[2] + ref0[:2]:
            a.setflags(write=False)
        _CASES[(shape, kind)] = ((x, h, c, Wt, b), ref, ref0)
    return _CASES[(shape, kind)]


def _err(hg, cg, ref):
    return max(np.abs(hg - ref[0]).max(), np.abs(cg - ref[1]).max())


_F32 = {}


def _fp32_kernel(ops, shape):
    """the fp32 kernel's (max |err|, rms err of c) against float64 on the shape's 'f32' operands: the yardstick of the fp32-grade forms"""
    if shape not in _F32:
        args, ref, _ = _operands(shape, 'f32')
        hf, cf = ops.convlstm(*args)
        _F32[shape] = (_err(hf, cf, ref), float(np.sqrt(((cf - ref[1]) ** 2).mean())))
    return _F32[shape]


_BF16_ERR = {}


def _plain_bf16_error(ops, shape):
    """the plain bf16 kernel's error on fp32 operands (its operand rounding): what the two-piece form must undercut fifty times"""
    if shape not in _BF16_ERR:
        args, ref, _ = _operands(shape, 'f32')
        _BF16_ERR[shape] = _err(*ops.convlstm_bf16(*args), ref)
    return _BF16_ERR[shape]


def _ln_merge(part, s):
    """Chan merge of image s's (count, mean, M2) partials -> (count, mean, variance) of the image"""
    cnt, mean, m2 = (part[s, :, k].astype(np.float64) for k in range(3))
    tot = cnt.sum()
    tot_mean = (cnt * mean).sum() / tot
    return tot, tot_mean, (m2.sum() + (cnt * (mean - tot_mean) ** 2).sum()) / tot


def _ln_check(part, n, hk, shape, nch):
    """the epilogue's partials, image by image, against the h the same launch wrote (hk, itself held to the reference by the caller)"""
    B, cx, C, H, W = shape
    _, tpi, _ = _tiles(B, H, W)
    assert n == tpi * C // nch, (n, tpi, C, nch)
    assert part.shape == (B, n, 4)
    for s in range(B):
        tot, mean, var = _ln_merge(part, s)
        assert tot == C * H * W, (s, tot)
        assert abs(mean - hk[s].mean()) < 1e-6, (s, mean, hk[s].mean())
        assert np.allclose(var, hk[s].var(), rtol=1e-4), (s, var, hk[s].var())


# ---- 1. per-op forward parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nch', [0, 16, 32], ids=_nid)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_bf16_is_exact_on_bf16_operands(ops, shape, nch):
    """test_convlstm_bf16_exact_on_bf16_operands' gate; then the stored gate planes and the LayerNorm partials of the same launch, and the first step"""
    B, cx, C, H, W = shape
    args, ref, ref0 = _operands(shape, 'bf16')
    hg, cg = ops.convlstm_bf16(*args, nch)
    print('%s nch %d bf16: max |err| %.2e' % (_sid(shape), nch, _err(hg, cg, ref)))
    assert np.abs(hg - ref[0]).max() < TOL and np.abs(cg - ref[1]).max() < TOL
    h2, c2, gates, (part, n) = ops.convlstm_bf16(*args, nch, want_gates=True, want_ln=True)
    assert np.array_equal(h2, hg) and np.array_equal(c2, cg)      # the same blocks in the same order, two more stores each
    gn = gates.reshape(B, H, W, 4, C).transpose(3, 0, 4, 1, 2)      # NHWC rows of [gate][channel] -> [gate][B][C][H][W]
    for k in range(4):
        assert np.abs(gn[k] - ref[2][k]).max() < TOL, k
    _ln_check(part, n, hg, shape, nch or 16)      # (nch = 0: 16-channel blocks below 256 blocks of 32)
    h0, c0 = ops.convlstm_bf16(*args, nch, h_is_zero=True)
    assert np.abs(h0 - ref0[0]).max() < TOL and np.abs(c0 - ref0[1]).max() < TOL


@pytest.mark.parametrize('nch', [16, 32], ids=_nid)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_bf16x3_on_fp32_operands(ops, shape, nch):
    """test_convlstm_bf16x3_on_fp32_operands' gate: 5e-5, and a fiftieth of the plain bf16 kernel's error on the same input"""
    args, ref, ref0 = _operands(shape, 'f32')
    e1 = _plain_bf16_error(ops, shape)
    hg, cg = ops.convlstm_bf16x3(*args, nch=nch)
    e3 = _err(hg, cg, ref)
    print('%s nch %d: max |err| two bf16 pieces %.2e, plain bf16 %.2e' % (_sid(shape), nch, e3, e1))
    assert e3 < 5e-5 and e3 < e1 / 50
    h0, c0 = ops.convlstm_bf16x3(*args, h_is_zero=True, nch=nch)
    assert _err(h0, c0, ref0) < 5e-5


# (entry, absolute bound, bound on max |err| and on the rms error of c in units of the fp32 kernel's): test_convlstm_bf16x6_is_fp32_grade and
# test_convlstm_fp16x3_is_fp32_grade.  The absolute bounds were measured on square maps at the same K = 25 (cx + C) and hold unchanged here.  Measured on the
# seven shapes, both block widths: three bf16 pieces 5.2e-7 .. 1.23e-6 (0.66 .. 1.26 of the fp32 kernel's 6.7e-7 .. 1.12e-6; rms of c 0.67 .. 0.92 of its),
# two fp16 pieces 5.4e-7 .. 1.27e-6 (0.69 .. 1.72; rms 0.73 .. 0.97); two bf16 pieces 7.6e-6 .. 1.22e-5 against the plain bf16 kernel's 4.1e-3 .. 6.5e-3
# (1/410 .. 1/650 of it); plain bf16 on bf16 operands 4.7e-7 .. 1.31e-6.
FP32_GRADE = {'bf16x6': (2e-6, 2.0, 1.2), 'fp16x3': (3e-6, 2.5, 1.5)}


@pytest.mark.parametrize('nch', [16, 32], ids=_nid)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
@pytest.mark.parametrize('entry', sorted(FP32_GRADE))
def test_fp32_grade_forms(ops, entry, shape, nch):
    args, ref, ref0 = _operands(shape, 'f32')
    ef, rf = _fp32_kernel(ops, shape)
    run = getattr(ops, 'convlstm_' + entry)
    absb, kmax, krms = FP32_GRADE[entry]
    hg, cg, (part, n) = run(*args, nch=nch, want_ln=True)
    e = _err(hg, cg, ref); r = float(np.sqrt(((cg - ref[1]) ** 2).mean()))
    print('%s nch %d %s: max |err| %.2e, fp32 kernel %.2e; rms of c %.2e vs %.2e' % (_sid(shape), nch, entry, e, ef, r, rf))
    assert e < absb and e < kmax * ef and r < krms * rf
    _ln_check(part, n, hg, shape, nch)
    h0, c0 = run(*args, h_is_zero=True, nch=nch)
    assert _err(h0, c0, ref0) < absb


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
@pytest.mark.parametrize('entry', sorted(FP32_GRADE))
def test_block_widths_agree_and_a_second_call_repeats_the_bits(ops, entry, shape):
    """16- and 32-channel blocks sum the same terms in another tap rotation; the same launch twice walks the same order"""
    args = _operands(shape, 'f32')[0]
    run = getattr(ops, 'convlstm_' + entry)
    h16, c16 = run(*args, nch=16)
    h32, c32 = run(*args, nch=32)
    assert np.abs(h16 - h32).max() < 2e-6 and np.abs(c16 - c32).max() < 2e-6
    for nch, hh, cc in ((16, h16, c16), (32, h32, c32)):
        hb, cb = run(*args, nch=nch)
        assert np.array_equal(hh, hb) and np.array_equal(cc, cb), nch


@pytest.mark.parametrize('entry', ['bf16', 'bf16x3', 'bf16x6', 'fp16x3'])
def test_x_as_the_last_channels_of_a_concat(entry):
    """tests/test_gpu_conv_forms.py::test_convlstm_reads_the_last_channels_of_a_concat on two-image tiles, three to a row: x is the last 64 of 96 columns, the
    others NaN.  The stride moves addresses only (the bits of the contiguous call), and the result is the float64 cell's within the entry's own bound."""
    import conv_ops
    kind = 'bf16' if entry == 'bf16' else 'f32'
    args, ref, _ = _operands(CONCAT, kind)
    hs, cs = conv_ops.convlstm(entry, *args, ld=CONCAT[1] + 32)
    hc, cc = conv_ops.convlstm(entry, *args)
    err = _err(hs, cs, ref)
    print('%s %s, x at columns 32..96 of 96: max |err| %.2e' % (_sid(CONCAT), entry, err))
    assert np.isfinite(hs).all() and np.isfinite(cs).all()
    assert np.array_equal(hs, hc) and np.array_equal(cs, cc)
    assert err < {'bf16': TOL, 'bf16x3': 5e-5, 'bf16x6': 2e-6, 'fp16x3': 3e-6}[entry]


@pytest.mark.parametrize('shape', REFUSED, ids=_sid)
@pytest.mark.parametrize('entry', ['bf16', 'bf16x3', 'bf16x6', 'fp16x3'])
def test_entries_refuse_maps_their_tiles_do_not_serve(ops, entry, shape):
    """PIVP_ERR_BADARG in front of the launch, with a valid weight pack and every buffer in place: h, c, the gate planes and the partials keep their 7.0"""
    import conv_ops
    from pivp_amd import _lib, to_internal
    lib = _lib.load()
    B, cx, C, H, W = shape
    x, h, c, Wt, b = _case(B, cx, C, H, W, 3)
    pack, run, pieces, tail = conv_ops._PACK[entry]
    wd = ops._t(to_internal('lstm1/conv/W', Wt))
    wb = torch.empty(pieces * lib.pivp_lstm_bf16_weight_elems(cx + C, C) + tail, dtype=torch.int16, device=ops.DEV)
    _lib.check(getattr(lib, pack)(*((wd.data_ptr(), wb.data_ptr(), cx + C, C) + ((W,) if entry == 'fp16x3' else ()) + (ops.stream(),))), pack)
    xd, hd, cd, bd = ops.nhwc(x), ops.nhwc(h), ops.nhwc(c), ops._t(b)
    cap = (H // 8 + 1) * (W // 8 + 1) * (C // 16)
    outs = [torch.full(sz, conv_ops.PREFILL, dtype=torch.float32, device=ops.DEV)
            for sz in ((B, H, W, C), (B, H, W, C), (B * H * W, 4 * C), (B, cap, 4))]
    h_out, c_out, gates, part = outs
    npart = ctypes.c_int(-7)
    for hp in (hd.data_ptr(), None):
        for nch in (0, 16, 32):
            rc = getattr(lib, run)(xd.data_ptr(), cx, cx, hp, C, wb.data_ptr(), bd.data_ptr(), cd.data_ptr(), c_out.data_ptr(), h_out.data_ptr(),
                                   gates.data_ptr(), part.data_ptr(), cap, ctypes.addressof(npart), B, H, W, nch, ops.stream())
            assert rc == BADARG, (entry, shape, nch, rc)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == conv_ops.PREFILL).all())


# ---- 3. inference rollouts of the split modes on rectangular frames -------------------------------------------------------------------------------------------
# Maps of the cells at frame H x W: H/2 x W/2 (lstm1, 2, 7), H/4 x W/4 (lstm3, 4, 6), H/8 x W/8 (lstm5).
#   128 x 64   64 x 32, 32 x 16, 16 x 8: every cell packed, lstm5 on two-image tiles in two rows
#   64 x 96    32 x 48 (16-wide tiles, tpr = 3), 16 x 24 (two-image tiles, three to a row), 8 x 12: lstm5 is not served -- the split modes run it on the fp32
#              kernel, the bf16 mode has no fall-back and refuses the frame
# Which of norm(hidden1) / norm(hidden3) an inference plan applies inside lstm2 / lstm4's staging (step_form, plan.h): the L2-direct forms on a map that is a
# multiple of 16 wide, from 128 tiles (lstm2: B * H2/8 * W2/16) or 64 tiles (lstm4) on.  At B = 2 that is neither norm at either frame (32 and 8 tiles at
# 128 x 64; 24 tiles at 64 x 96, where lstm4's 16 x 24 map rules the fold out by its width whatever the batch): both run as launches of their own.  At
# B = 12 a 64 x 96 frame gives lstm2 144 tiles -- hidden1's norm moves into lstm2 -- while hidden3's must stay a launch of its own in front of lstm4's
# two-image tiles, which have no norm-on-load form.  The tile counts are a tuning choice, so no test holds the plan to them: _taps_case reads from outside
# what the plan did with hidden1 and prints it (observed: not folded in the four B = 2 cases, folded at B = 12), and only the B = 12 case needs the fold.
FRAMES = [(128, 64), (64, 96)]
FRAME_IDS = ['%dx%d' % f for f in FRAMES]
MODES = ['bf16x6', 'fp16x3']
PRECISION_CODE = {'fp32': 0, 'bf16': 1, 'bf16x6': 3, 'fp16x3': 4}
TAPS = ('hidden1', 'hidden2', 'hidden3', 'hidden4', 'hidden5')


_INPUTS, _ORACLE, _RUNS = {}, {}, {}


def _inputs(H, W, B, T):
    if (H, W, B, T) not in _INPUTS:
        P = R.init_params(seed=1, dtype=np.float32, scale=1.0, num_masks=10, model_type='CDNA', height=H, width=W)
        _INPUTS[(H, W, B, T)] = (P, R.synthetic_batch(B, T, H, W))
    return _INPUTS[(H, W, B, T)]


def _oracle(H, W, B=2, T=3):
    """the float64 model's frames and loss: once per frame size"""
    if (H, W, B, T) not in _ORACLE:
        P, (imgs, acts, stas) = _inputs(H, W, B, T)
        t0 = time.time()
        ref = R.Model(10, params=P, dtype=np.float64, prefix='x'); ref.train = False
        loss = float(ref([imgs, acts, stas], 0))
        gen = np.stack(ref.gen_images)
        gen.setflags(write=False)
        print('float64 model at %dx%d, B = %d, T = %d: %.1f s' % (H, W, B, T, time.time() - t0))
        _ORACLE[(H, W, B, T)] = (gen, loss)
    return _ORACLE[(H, W, B, T)]


def _run(precision, H, W, B=2, T=3, keep=False, taps=()):
    """an inference rollout -> (frames, loss, taps of the last step); the fp32 plan's runs are kept for the tests that share them"""
    import pivp_amd
    key = (precision, H, W, B, T, keep, tuple(taps))
    if key in _RUNS:
        return _RUNS[key]
    P, (imgs, acts, stas) = _inputs(H, W, B, T)
    m = pivp_amd.Model(10, prefix='t', precision=precision, keep_activations=keep)
    m.load_state_dict_reference(P)
    with pivp_amd.using_config('train', False):
        loss = float(m([imgs, acts, stas], 0))
    assert m._active.lib.pivp_plan_get_precision(m._active.h) == PRECISION_CODE[precision]
    out = (torch.stack(m.gen_images).cpu().numpy(), loss, {k: m.tap(k).cpu().numpy() for k in taps})
    if precision == 'fp32':
        _RUNS[key] = out
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H,W', FRAMES, ids=FRAME_IDS)
def test_split_mode_rollouts_are_as_close_to_float64_as_the_fp32_plan(mode, H, W):
    """test_rollout_fp16x3_is_as_close_to_float64_as_the_fp32_path's gate, frame by frame, at B = 2, T = 3"""
    gref, lref = _oracle(H, W)
    genf, lossf, _ = _run('fp32', H, W)
    gen, loss, _ = _run(mode, H, W)
    assert gen.shape == (2, 2, 3, H, W)
    l3 = R.per_pixel_l2(gen, gref); lf = R.per_pixel_l2(genf, gref)
    per3 = l3.reshape(l3.shape[0], -1).max(axis=1); perf = lf.reshape(lf.shape[0], -1).max(axis=1)
    print('%s rollout at %dx%d: per-pixel L2 vs float64 per frame %s (fp32 plan %s); loss %.8f vs %.8f (fp32 plan %.8f)'
          % (mode, H, W, ' '.join('%.2e' % v for v in per3), ' '.join('%.2e' % v for v in perf), loss, lref, lossf))
    assert (per3 < 2.0 * np.maximum(perf, 1e-6)).all() and abs(loss - lref) < 1e-6


def _taps_case(mode, H, W, B):
    """hidden1 .. hidden5 of the mode's inference plan against the fp32 plan's (test_split_modes_apply_hidden1_and_hidden3_inside_lstm2_and_lstm4's gate).
    hidden4 and hidden5 are only right if lstm4 consumed the normalised hidden3, hidden2 only if lstm2 consumed the normalised hidden1.  Whether lstm2 applied
    that norm itself shows from outside: a plan that keeps its activations never does, and writes hidden1 with the launches an unfolded inference plan runs --
    the same bits (step 1 is fed a ground-truth frame in both) --, while a folding plan never writes hidden1 and the tap rebuilds it from recomputed
    statistics, equal to the fused ones up to summation order only."""
    tf = _run('fp32', H, W, B, taps=TAPS)[2]
    tm = _run(mode, H, W, B, taps=TAPS)[2]
    tk = _run(mode, H, W, B, keep=True, taps=TAPS[:1])[2]
    rebuilt1 = not np.array_equal(tm['hidden1'], tk['hidden1'])
    worst = {k: float(np.abs(tm[k] - tf[k]).max()) for k in TAPS}
    print('%s taps at %dx%d, B = %d: norm(hidden1) applied inside lstm2 (the tap is a rebuild): %s; max |tap - fp32 plan| %s'
          % (mode, H, W, B, rebuilt1, ' '.join('%s %.2e' % kv for kv in worst.items())))
    for k, d in worst.items():
        assert d < 2e-5, (mode, k, d)
    return rebuilt1


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H,W', FRAMES, ids=FRAME_IDS)
def test_split_mode_taps_on_rectangular_frames(mode, H, W):
    _taps_case(mode, H, W, 2)


@pytest.mark.parametrize('mode', MODES)
def test_hidden3_keeps_its_own_norm_launch_in_front_of_two_image_tiles(mode):
    """64 x 96 at B = 12: lstm2 (32 x 48, 144 tiles) applies norm(hidden1) while it stages its patch; lstm4 (16 x 24: two-image tiles, three to a row) has no
    such form and must read a hidden3 that a launch of its own wrote -- hidden4 and hidden5 show that it did.  The case is only worth its name while lstm2
    folds: if the plan's tile threshold moves, raise B until it does again."""
    assert (96 // 4) % 16 != 0      # lstm4's map is no multiple of 16 wide: its tiles hold two images
    assert _taps_case(mode, 64, 96, 12), 'lstm2 no longer applies norm(hidden1) itself at B = 12 (step_form, plan.h): raise the batch of this case'


def test_bf16_mode_on_rectangular_frames():
    """128 x 64: every map is served; the error is reported and held to test_rollout_bf16_reports_error_against_the_golden_fixture's sanity bound.
    64 x 96: lstm5's 8 x 12 map is not served and the mode has no fall-back: refused at pivp_plan_set_precision (test_bf16_precision_is_refused_on_a_72x40_frame)"""
    import pivp_amd
    gref, lref = _oracle(128, 64)
    genf, lossf, _ = _run('fp32', 128, 64)
    gen, loss, _ = _run('bf16', 128, 64)
    l32 = R.per_pixel_l2(genf, gref); l16 = R.per_pixel_l2(gen, gref)
    print('bf16 rollout at 128x64: per-pixel L2 vs float64: fp32 max %.2e rms %.2e | bf16 max %.2e rms %.2e | loss %.6f / %.6f / %.6f'
          % (l32.max(), np.sqrt((l32 ** 2).mean()), l16.max(), np.sqrt((l16 ** 2).mean()), lref, lossf, loss))
    assert l32.max() < 1e-4
    assert 1e-6 < l16.max() < 5e-2 and abs(loss - lref) < 1e-3
    P, (imgs, acts, stas) = _inputs(64, 96, 2, 3)
    m = pivp_amd.Model(10, prefix='t', precision='bf16')
    m.load_state_dict_reference(P)
    with pytest.raises(RuntimeError, match='pivp_plan_set_precision'):
        with pivp_amd.using_config('train', False):
            m([imgs, acts, stas], 0)


def test_odd_batch_on_a_rectangular_frame():
    """B = 3 at 128 x 64 in the bf16x6 mode: the 64 x 32 and 32 x 16 cells stay packed (16-wide tiles take any batch), lstm5's 16 x 8 map cannot pair its
    images and runs on the fp32 kernel; test_split_modes_with_odd_batches' gate against the fp32 plan"""
    genf = _run('fp32', 128, 64, B=3)[0]
    gen = _run('bf16x6', 128, 64, B=3)[0]
    l2 = R.per_pixel_l2(gen, genf)
    print('B = 3 at 128x64, bf16x6 against the fp32 plan: max per-pixel L2 %.2e' % l2.max())
    assert np.isfinite(gen).all() and l2.max() < 2e-5
