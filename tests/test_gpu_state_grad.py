"""GPU tests of the gradients through a carried recurrent state (include/pivp_state_grad.h): `Model(carry_state=True, keep_activations=True,
state_backward=True)` -- truncated BPTT across calls, `backward(initial_state_grad=, final_state_grad=)`, `pivp_amd.chunked_backward` -- against
float64 autograd through the torch restatement called on consecutive windows without reset_state() (tests/state_grad_reference.py, computed once per
case and shared), the neutrality of the new flag, the two kernels of csrc/state_grad.hip alone, and the refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_grad_reference as SR  # noqa: E402
from input_grad_reference import rel_errors  # noqa: E402
from test_gpu_train import _check_grads  # noqa: E402
from test_gpu_bf16 import _relu_mismatches  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CX = (32, 32, 32, 64, 64, 128, 96)      # x channels of the seven cells (TM:509-515)


@pytest.fixture(scope='module')
def pivp():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    return pivp_amd


def _model(pivp, name, flag=True, batch_seed=None, **kw):
    mkw, nm, P, wins = SR.case_inputs(name, batch_seed)
    extra = dict(carry_state=True, state_backward=True) if flag else {}
    m = pivp.Model(nm, prefix='t', keep_activations=True, **dict(mkw, **dict(extra, **kw)))
    m.load_state_dict_reference(P)
    return m, wins


def _two_windows(m, wins):
    """window 1 from zeros, window 2 from the state it left, gradients cleared in front of the sweep the caller runs -> (loss1, loss2) device scalars"""
    m.reset_state()
    l1 = m(wins[0], 0)
    l2 = m(wins[1], 0)
    m.cleargrads()
    return l1, l2


def _state_of(pivp, flat, B, hw):
    return pivp.RecurrentState(torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32)).to(DEV), B, hw)


def _check_state_grad(got, ref, B, H, W, what):
    worst = 0.0
    for g, (a, b) in enumerate(zip(SR.segments(got, B, H, W), SR.segments(ref, B, H, W))):
        assert np.abs(b).max() > 0, 'segment %d of the reference is zero: the comparison would mean nothing' % g
        e = max(rel_errors(a, b))
        worst = max(worst, e)
        assert np.isfinite(a).all() and e < SR.STATE_GATE, '%s, segment %d (%s of cell %d): %.2e' % (what, g, 'h' if g % 2 else 'c', g // 2, e)
    return worst


# ---- 1. truncated BPTT: parameter gradients ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,det', [('cdna_T3', False), ('cdna_T5', False), ('stp_T4', False), ('dna_T4', False), ('ctx3_T5', False),
                                      ('nostate_T3', False), ('cdna_T3', True)])
def test_truncated_bptt_parameter_gradients(pivp, name, det):
    """Window 2's sweep, the state it started from a constant, against float64 with the state detached (det: the fixed-order slot form, whose t = 0
    now has an h operand).  On a model without the flag this raises."""
    ref = SR.reference(name, 'truncated')
    m, wins = _model(pivp, name, deterministic=det)
    l1, l2 = _two_windows(m, wins)
    m.backward()
    assert abs(float(l1) - ref['loss1']) < 1e-6 and abs(float(l2) - ref['loss2']) < 1e-6
    worst = _check_grads(m.grads_reference(), ref['grads'], SR.PARAM_GATE[SR.model_type(name)])
    print('truncated BPTT %s%s: worst relative gradient error %.2e (%s)' % (name, ' deterministic' if det else '', worst[0], worst[1]))


# ---- 2. d loss / d (the state the call started from) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cdna_T3', 'stp_T4', 'dna_T4'])
def test_initial_state_grad_matches_float64(pivp, name):
    ref = SR.reference(name, 'truncated')
    m, wins = _model(pivp, name)
    _two_windows(m, wins)
    m.backward(initial_state_grad=True)
    isg = m.initial_state_grad
    assert (isg.batch, isg.hw) == (2, (64, 64))
    worst = _check_state_grad(isg.data.cpu().numpy(), ref['state_grad'], 2, 64, 64, name)
    # the parameter gradients are those of the plain sweep (t = 0 now also forms the h columns of its data gradients)
    _check_grads(m.grads_reference(), ref['grads'], SR.PARAM_GATE[SR.model_type(name)])
    print('initial_state_grad %s: worst segment error %.2e' % (name, worst))
    # overwritten, not accumulated, and reused by the next call of the same shape
    first, ptr = isg.data.clone(), isg.data.data_ptr()
    m.backward(initial_state_grad=True)
    assert m.initial_state_grad.data.data_ptr() == ptr
    assert float((m.initial_state_grad.data - first).norm() / first.norm()) < 1e-3


# ---- 3. the seed on the final state, alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SR.SEED_CASES)
def test_final_state_grad_alone(pivp, name):
    """builtin_loss=False: the cost is sum(w * final state) for a fixed random w, from zeros and from a carried state."""
    w = _state_of(pivp, SR.seed_weights(2, 64, 64), 2, (64, 64))
    tol = SR.PARAM_GATE[SR.model_type(name)]
    m, wins = _model(pivp, name)
    m.reset_state()
    m(wins[1], 0)
    m.cleargrads()
    m.backward(builtin_loss=False, final_state_grad=w)
    worst = _check_grads(m.grads_reference(), SR.reference(name, 'seed_zeros')['grads'], tol)
    print('final_state_grad from zeros: worst relative gradient error %.2e (%s)' % worst)
    ref = SR.reference(name, 'seed_carried')
    _two_windows(m, wins)
    m.backward(builtin_loss=False, final_state_grad=w, initial_state_grad=True)
    worst = _check_grads(m.grads_reference(), ref['grads'], tol)
    ws = _check_state_grad(m.initial_state_grad.data.cpu().numpy(), ref['state_grad'], 2, 64, 64, name)
    print('final_state_grad from a carried state: worst relative gradient error %.2e (%s), worst state segment %.2e' % (worst + (ws,)))
    with pytest.raises(ValueError, match='nothing to differentiate'):
        m.backward(builtin_loss=False)


# ---- 4. exact BPTT over two windows in the memory of one --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('det', [False, True])      # (the fixed-order forms must ACCUMULATE in _flat_grads over the windows' sweeps too)
def test_chunked_backward_is_full_bptt(pivp, det):
    name = SR.CHUNKED_CASE
    tol = SR.PARAM_GATE[SR.model_type(name)]
    full, trunc = SR.reference(name, 'full'), SR.reference(name, 'truncated')
    dist = SR.lstm_weight_distance(trunc['grads'], full['grads'])
    assert dist >= 10 * tol, 'truncated and full references differ by %.2e on the ConvLSTM weights: the test could not tell them apart' % dist
    m, wins = _model(pivp, name, deterministic=det)
    m.reset_state()
    m(wins[0], 0)                     # (parameters are lazily sized: cleargrads needs one call)
    m.reset_state()
    m.cleargrads()
    total = pivp.chunked_backward(m, wins, iter_num=0)
    assert abs(float(total) - (full['loss1'] + full['loss2'])) < 2e-6
    worst = _check_grads(m.grads_reference(), full['grads'], tol)
    print('chunked_backward over two windows%s: worst relative gradient error %.2e (%s); truncated vs full on the ConvLSTM weights %.2e'
          % ((' (deterministic)' if det else '',) + worst + (dist,)))
    # the model carries the state the last window left
    ref_final = m.recurrent_state().data.clone()
    m.reset_state()
    m(wins[0], 0); m(wins[1], 0)
    assert torch.equal(m.recurrent_state().data, ref_final)


def test_chunked_backward_over_one_window_is_the_plain_sweep(pivp):
    m, wins = _model(pivp, 'cdna_T3', deterministic=True)
    m.reset_state()
    m(wins[0], 0)
    m.cleargrads(); m.backward()
    plain = m._flat_grads.clone()
    m.reset_state(); m.cleargrads()
    loss = pivp.chunked_backward(m, [wins[0]], iter_num=0)
    assert torch.equal(m._flat_grads, plain) and float(loss) == float(m.loss)


# ---- 5. deterministic, and the neutrality of the flag -----------------------------------------------------------------------------------------------
def test_deterministic_carried_sweep_and_neutrality(pivp):
    m, wins = _model(pivp, 'cdna_T3', deterministic=True)
    out = []
    for _ in range(2):
        _two_windows(m, wins)
        m.backward(initial_state_grad=True)
        out.append((m._flat_grads.clone(), m.initial_state_grad.data.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # enable registered, but a start from zeros: the default sweep's bits
    plain, _ = _model(pivp, 'cdna_T3', flag=False, deterministic=True)
    grads = []
    for mm in (m, plain):
        mm.reset_state()
        mm(wins[0], 0)
        mm.cleargrads(); mm.backward()
        grads.append(mm._flat_grads.clone())
    assert torch.equal(grads[0], grads[1])
    # two alternating buffers against one advanced in place: the same frames and states over three calls
    inplace, _ = _model(pivp, 'cdna_T3', flag=False, carry_state=True, deterministic=True)
    m.reset_state()
    for k, w in enumerate((wins[0], wins[1], wins[0])):
        m(w, 0); inplace(w, 0)
        assert torch.equal(m._gen, inplace._gen) and torch.equal(m._gen_states, inplace._gen_states), 'call %d' % k
        assert torch.equal(m.recurrent_state().data, inplace.recurrent_state().data), 'call %d' % k
    # ... and the refusal stays on a model built without the flag
    inplace.cleargrads()
    with pytest.raises(RuntimeError, match='truncated BPTT'):
        inplace.backward()


# ---- 6. the precision modes ---------------------------------------------------------------------------------------------------------------------------
def _forward_pair(pivp, prec, seed):
    """the fp32 and the `prec` model after both windows of 'cdna_T3' at a batch seed -> (models, ReLU units on different sides of zero in the two
    modes, counted over both windows)"""
    models, flips = {}, 0
    for p in ('fp32', prec):
        m, wins = _model(pivp, 'cdna_T3', precision=p, batch_seed=seed)
        m.reset_state()
        m(wins[0], 0)
        models[p] = m
    flips += _relu_mismatches(models['fp32'], models[prec], 2)
    for p in ('fp32', prec):
        models[p](wins[1], 0)
    flips += _relu_mismatches(models['fp32'], models[prec], 2)
    return models, flips


@pytest.mark.parametrize('prec', ['bf16', 'fp16x3', 'bf16x6'])
def test_precision_modes_track_the_fp32_carried_sweep(pivp, prec):
    """Form and bounds of tests/test_gpu_bf16.py's train-step tests: relative L2 distance of the flat gradients to the fp32 path's, bf16 < 5e-2, fp16x3 <
    1e-4 (2e-3 when ReLU units sit on different sides of zero in the two modes), bf16x6 < 1e-4.  The fp32-grade modes hold every segment of
    initial_state_grad to their bound as well; the bf16 mode's state gradient is printed per segment and only has to be finite (the project has no
    bound for it: profiles/r16/NOTES.md).  Batch seeds: state_grad_reference.PRECISION_SEEDS."""
    models, flips = _forward_pair(pivp, prec, SR.PRECISION_SEEDS[prec])
    outs = {}
    for p in ('fp32', prec):
        m = models[p]
        m.cleargrads()
        m.backward(initial_state_grad=True)
        outs[p] = (m._flat_grads.clone(), m.initial_state_grad.data.cpu().numpy())
    rel = float((outs[prec][0] - outs['fp32'][0]).norm() / outs['fp32'][0].norm())
    segs = [float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(SR.segments(outs[prec][1], 2, 64, 64), SR.segments(outs['fp32'][1], 2, 64, 64))]
    print('%s carried sweep against fp32: relative gradient difference %.2e, ReLU units on different sides of zero: %d; initial_state_grad per segment '
          '(c, h of cell 0 .. 6): %s' % (prec, rel, flips, ' '.join('%.1e' % e for e in segs)))
    bound = {'bf16': 5e-2, 'fp16x3': 1e-4 if flips == 0 else 2e-3, 'bf16x6': 1e-4}[prec]
    assert torch.isfinite(outs[prec][0]).all() and np.isfinite(outs[prec][1]).all()
    assert rel < bound
    if prec != 'bf16':
        assert max(segs) < bound


def test_bf16x6_batch_seed_outside(pivp):
    """Why PRECISION_SEEDS['bf16x6'] is not 0: at the seeds listed as outside the two modes' forward passes disagree on a ReLU unit."""
    for seed in SR.PRECISION_SEEDS_OUTSIDE['bf16x6']:
        assert _forward_pair(pivp, 'bf16x6', seed)[1] > 0, seed
    assert _forward_pair(pivp, 'bf16x6', SR.PRECISION_SEEDS['bf16x6'])[1] == 0


def test_chunked_backward_in_bf16_tracks_fp32(pivp):
    """The seed path (final_state_grad: the scatter, dh_b read in place) in a precision mode: chunked_backward over two windows, bf16 against fp32,
    test_gpu_bf16.py's form and bound for the bf16 mode's gradients (relative L2 of the flat gradient < 5e-2)."""
    out = {}
    for p in ('fp32', 'bf16'):
        m, wins = _model(pivp, SR.CHUNKED_CASE, precision=p)
        m.reset_state()
        m(wins[0], 0)
        m.reset_state()
        m.cleargrads()
        pivp.chunked_backward(m, wins, iter_num=0)
        out[p] = m._flat_grads.clone()
    rel = float((out['bf16'] - out['fp32']).norm() / out['fp32'].norm())
    print('bf16 chunked_backward against fp32: relative gradient difference %.2e' % rel)
    assert torch.isfinite(out['bf16']).all() and 1e-6 < rel < 5e-2


# ---- 7. input gradients after a carried start -----------------------------------------------------------------------------------------------------------
def test_input_gradients_after_a_carried_start(pivp):
    name = 'cdna_T3'
    ref = SR.reference(name, 'truncated')
    m, wins = _model(pivp, name)
    _two_windows(m, wins)
    m.backward(input_grad=True, params=False)
    T = wins[1][0].shape[0]
    ea = rel_errors(m.action_grad.cpu().numpy(), ref['action_grad'][:T - 1])
    es = rel_errors(m.state_grad.cpu().numpy(), ref['state0_grad'][0])
    print('input gradients after a carried start: actions rel L2 %.2e max %.2e, state0 rel L2 %.2e max %.2e' % (ea + es))
    assert np.abs(ref['action_grad'][:T - 1]).max() > 0 and max(ea + es) < 2e-3


# ---- 8. the kernels alone ---------------------------------------------------------------------------------------------------------------------------------
def _guarded(n, lead, fill=7.0):
    """a float32 buffer of n elements with `lead` guard floats in front and 64 behind -> (whole, view)"""
    whole = torch.full((lead + n + 64,), fill, dtype=torch.float32, device=DEV)
    return whole, whole[lead:lead + n]


def _guards_intact(whole, lead, n, fill=7.0):
    return bool((whole[:lead] == fill).all()) and bool((whole[lead + n:] == fill).all())


# off 1: destinations one float off 16 bytes: every segment takes the 4-byte form of the same runs.  2: only the sources of lstm4's c and lstm6's h are off
# 16 bytes: those two segments take the 4-byte form, the other twelve keep their 16-byte accesses (the choice is made per segment)
@pytest.mark.parametrize('off', [0, 1, 2])
@pytest.mark.parametrize('H,W,B', [(16, 16, 1), (64, 64, 2), (128, 64, 3)])
def test_gather_and_scatter_kernels_are_exact(pivp, H, W, B, off):
    lib = pivp._lib.load()
    cfg = pivp._lib.PivpConfig(batch=B, seq_len=3, height=H, width=W, num_masks=10, model_type=0, use_state=1, context_frames=2, keep_activations=1,
                               ln_eps=1e-6, stp_zero_border=0)
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device='cpu').manual_seed(H + W + B)
    shapes = [(B, H // lv, W // lv, C) for lv, C in zip(SR.CELL_LEVELS, SR.CELL_CHANNELS)]
    dc = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    din = [torch.randn(s[:3] + (cx + s[3],), generator=gen).to(DEV) for s, cx in zip(shapes, CX)]
    if off == 2:
        shifted = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)      # the same values one float further on
        dc[3], din[5] = shifted(dc[3]), shifted(din[5])
        assert dc[3].data_ptr() % 16 == 4 and din[5].data_ptr() % 16 == 4
    n = SR.state_numel(B, H, W)
    lead = 64 + (off == 1)
    whole, dst = _guarded(n, lead)
    ptrs = lambda ts: (ctypes.c_void_p * 7)(*[t.data_ptr() for t in ts])
    assert lib.pivp_state_grad_gather(ctypes.byref(cfg), ptrs(dc), ptrs(din), dst.data_ptr(), st) == 0
    want = torch.cat([t.reshape(-1) for c, d, cx in zip(dc, din, CX) for t in (c, d[..., cx:])])
    torch.cuda.synchronize()
    assert torch.equal(dst, want) and _guards_intact(whole, lead, n)
    # the scatter: the c segments of a state into seven buffers, each between guards; the h segments go nowhere
    seed = torch.randn(n, generator=gen).to(DEV)
    outs = [_guarded(int(np.prod(s)), lead) for s in shapes]
    assert lib.pivp_state_grad_scatter(ctypes.byref(cfg), seed.data_ptr(), (ctypes.c_void_p * 7)(*[v.data_ptr() for _, v in outs]), st) == 0
    torch.cuda.synchronize()
    segs = SR.segments(seed, B, H, W)
    for i, (wh, v) in enumerate(outs):
        assert torch.equal(v, segs[2 * i]) and _guards_intact(wh, lead, v.numel()), 'cell %d' % i
    # refused in front of the launch
    assert lib.pivp_state_grad_gather(None, ptrs(dc), ptrs(din), dst.data_ptr(), st) == -1
    assert lib.pivp_state_grad_gather(ctypes.byref(cfg), ptrs(dc), ptrs(din), None, st) == -1
    assert lib.pivp_state_grad_scatter(ctypes.byref(cfg), None, ptrs(dc), st) == -1
    bad = (ctypes.c_void_p * 7)(*([dc[0].data_ptr()] * 6 + [None]))
    assert lib.pivp_state_grad_gather(ctypes.byref(cfg), bad, ptrs(din), dst.data_ptr(), st) == -1


# ---- 9. refusals launch nothing -------------------------------------------------------------------------------------------------------------------------------
def _raw_sweep(m):
    plan = m._active
    return plan.lib.pivp_rollout_backward(plan.h, m._inputs[0].data_ptr(), m._inputs[1].data_ptr(), m._inputs[2].data_ptr(), None, m._gen.data_ptr(),
                                          m._gen_states.data_ptr(), m._stream())


def test_refusals_launch_nothing(pivp):
    m, wins = _model(pivp, 'cdna_T3', deterministic=True)
    m.reset_state()
    m(wins[0], 0)
    m.cleargrads(); m.backward()
    g0 = m._flat_grads.clone()
    plan, lib = m._active, m._active.lib
    buf = torch.full((SR.state_numel(2, 64, 64) + 64,), 3.0, dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    unchanged = lambda mm, g: (torch.cuda.synchronize(), torch.equal(mm._flat_grads, g))[1]
    # d_state_in after a start from zeros
    assert lib.pivp_plan_set_state_grad(plan.h, 1, None, p) == 0
    assert _raw_sweep(m) == -3 and unchanged(m, g0) and bool((buf == 3.0).all())
    # misaligned or overlapping pointers, d_state_in without enable, enable out of range: refused, and the registration stays what it was
    for bad in ((1, p + 4, None), (1, None, p + 8), (1, p, p + 16), (1, p, p), (0, None, p), (2, None, None), (-1, None, None)):
        assert lib.pivp_plan_set_state_grad(plan.h, *bad) == -1, bad
    en, so, si = ctypes.c_int(-7), ctypes.c_void_p(1), ctypes.c_void_p(1)
    assert lib.pivp_plan_get_state_grad(plan.h, ctypes.byref(en), ctypes.byref(so), ctypes.byref(si)) == 0
    assert (en.value, so.value, si.value) == (1, None, p)
    assert lib.pivp_plan_set_state_grad(plan.h, 0, None, None) == 0
    # enable = 0 after a carried start (and d_state_in over the state the rollout read)
    m(wins[1], 0)
    assert _raw_sweep(m) == -3 and unchanged(m, g0)
    assert lib.pivp_plan_set_state_grad(plan.h, 1, None, m._spare_state.data.data_ptr()) == -1
    assert lib.pivp_plan_set_state_grad(plan.h, 1, None, None) == 0 and _raw_sweep(m) == 0      # (enabled: served)
    torch.cuda.synchronize()
    assert not torch.equal(m._flat_grads, g0)
    assert lib.pivp_plan_set_state_grad(plan.h, 0, None, None) == 0
    # a forward registered with state_in == state_out has overwritten the state it started from
    inplace, _ = _model(pivp, 'cdna_T3', flag=False, carry_state=True, deterministic=True)
    inplace(wins[0], 0)
    inplace.cleargrads(); inplace.backward()
    g1 = inplace._flat_grads.clone()
    inplace(wins[1], 0)
    h2 = inplace._active.h
    assert lib.pivp_plan_set_state_grad(h2, 1, None, None) == 0
    try:
        assert _raw_sweep(inplace) == -3 and unchanged(inplace, g1)
    finally:
        lib.pivp_plan_set_state_grad(h2, 0, None, None)
    assert _raw_sweep(inplace) == -3 and unchanged(inplace, g1)


# ---- 10. 128 x 128 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_truncated_bptt_128x128(pivp):
    """One carried window at T = 3 against float64, with tests/test_gpu_train.py::test_bptt_gradients_128x128's bounds (relative L2 and median element)."""
    name = 'cdna_128_T3'
    ref = SR.reference(name, 'truncated')
    m, wins = _model(pivp, name)
    l1, l2 = _two_windows(m, wins)
    m.backward(initial_state_grad=True)
    assert abs(float(l2) - ref['loss2']) < 1e-6
    got = m.grads_reference()
    for kname, g in ref['grads'].items():
        d = got[kname].astype(np.float64) - g
        rel_l2 = np.linalg.norm(d) / (np.linalg.norm(g) + 1e-30)
        med = np.median(np.abs(d)) / (np.abs(g).max() + 1e-12)
        assert rel_l2 < 1e-2 and med < 1e-3, '%s: relative L2 %.2e, median %.2e' % (kname, rel_l2, med)
    isg = m.initial_state_grad.data.cpu().numpy()
    errs = [rel_errors(a, b)[0] for a, b in zip(SR.segments(isg, 2, 128, 128), SR.segments(ref['state_grad'], 2, 128, 128))]
    print('128 x 128 carried window: worst state segment relative L2 %.2e' % max(errs))
    assert max(errs) < 1e-2
