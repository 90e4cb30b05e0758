"""The 5x5 data gradient's fused epilogue (IgemmDesc::ep_*), per op and in every operand form, and the ConvLSTM cell backward around it.

The backward sweep lets the data gradient of lstm7, lstm6 and lstm1 apply the ReLU mask of the enc conv in front of the cell (mode 1) or add a second gradient
path (mode 2) while it stores -- but only on an unsplit grid, which the suite's small batches never produce.  pivp_conv5x5_ep and pivp_convlstm_backward_form
run that code at B = 2 (no_split, or a shape whose launcher decides for an unsplit grid on its own):
  * the hooked launch is BIT-IDENTICAL to the unhooked one followed by the fp32 elementwise operation on the host: the hook meets the same accumulator;
  * with operands that are bf16 numbers the hooked result agrees with the float64 convolution + hook to fp32 summation accuracy (tests/test_gpu_bf16.py's gate);
  * the cell in the forms 1..4 against float64 autograd, with the gates of the per-form convolution tests.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 2e-5                                  # tests/test_gpu_bf16.py's exact-operand gate, here relative to max |ref|
FORMS = ['bf16', 'bf16x3', 'bf16x6', 'fp16x3']
BADARG = -1


@pytest.fixture(scope='module')
def ops():
    import hip_ops
    return hip_ops


@pytest.fixture(scope='module')
def env():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import pivp_amd
    from pivp_amd import _lib
    return pivp_amd, _lib, _lib.load()


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _relu_source(rs, shape, ncols):
    """relu(randn): about half exact +0.0, as the post-ReLU activations the hook meets; a handful of -0.0 (must mask) and of tiny positive normals (must not)
    among the first ncols channels (the ones a launch reads)."""
    ep = np.maximum(rs.randn(*shape), 0.0).astype(np.float32)
    idx = [tuple(rs.randint(0, n) for n in (shape[0], ncols) + tuple(shape[2:])) for _ in range(16)]
    for k, i in enumerate(idx):
        ep[i] = np.float32(-0.0) if k < 8 else np.float32(1e-30)
    assert np.signbit(ep[idx[0]]) and ep[idx[8]] > 0
    return ep


def _host_hook(base, src, n, mode):
    """the fp32 elementwise operation the hook fuses, on columns < n of an NCHW (or [M][C] with axis 1 = channel) float32 array"""
    exp = np.array(base, dtype=np.float32, copy=True)
    s = np.asarray(src[:, :n], dtype=np.float32)
    if mode == 1:
        exp[:, :n] = np.where(s > 0, base[:, :n], np.float32(0.0))
    else:
        exp[:, :n] = base[:, :n] + s
    return exp


# ---- the hook on its own: pivp_conv5x5_ep ---------------------------------------------------------------------------------------------------------------------
# name: (B, cin, cout, H, W, source channels, ep_cols, ep_ld, modes, no_split, ldo)
HOOK_CASES = {
    'lstm7': (2, 128, 128, 32, 32, 96, 96, 96, (1,), True, None),                 # ep6
    'lstm6_padded_rows': (2, 256, 192, 16, 16, 128, 128, 128, (1,), True, None),  # ep5; 192 columns of the pack's conv5x5_bf16_rows(192)
    'lstm1_channel_slice': (2, 128, 64, 32, 32, 32, 32, 64, (2,), True, None),    # ep0: the source is the last 32 channels of a 64-wide buffer
    'non_square_map': (2, 128, 128, 16, 32, 96, 96, 96, (1, 2), True, None),      # the row decode: H != W
    'two_image_tiles': (2, 512, 192, 8, 8, 64, 64, 64, (1, 2), True, None),       # 8-wide map
    'one_k_group': (2, 64, 64, 16, 16, 32, 32, 32, (1,), False, None),            # ncg == 1: the launcher decides for the unsplit grid alone
    'strided_destination': (2, 128, 64, 32, 32, 32, 32, 64, (2,), False, 96),     # ldo != cout: never split
    'cols_beyond_cout': (2, 128, 64, 32, 32, 96, 96, 96, (1,), True, None),       # ep_cols >= cout: clamped
}


@functools.lru_cache(maxsize=None)
def _hook_case(name):
    B, cin, cout, H, W, c_ep, cols, ld, modes, no_split, ldo = HOOK_CASES[name]
    rs = np.random.RandomState(1000 + sorted(HOOK_CASES).index(name))
    x = _bf16(rs.randn(B, cin, H, W)); Wt = _bf16(rs.randn(cout, cin, 5, 5) / np.sqrt(25 * cin))
    ref = R.conv2d(x, Wt, np.zeros(cout), 1, 2)
    ep = _relu_source(rs, (B, c_ep, H, W), min(c_ep, cols, cout))
    return _frozen(x, Wt, ref, ep)


def _check_hooked(got, base_out, ref, ep, cols, mode, ldo, label):
    out, applied = got[0], got[1]
    cout = out.shape[1]
    n = min(cols, cout)
    assert applied == 1, label
    exp = _host_hook(base_out, ep, n, mode)
    same = _bits(out) == _bits(exp)
    print('%s mode %d: %d of %d elements differ in bits from the unhooked launch + host operation (%d of them in hooked columns)'
          % (label, mode, int((~same).sum()), same.size, int((~same[:, :n]).sum())))
    assert same.all(), label
    assert np.array_equal(_bits(out[:, n:]), _bits(base_out[:, n:]))            # columns >= ep_cols: untouched by the hook
    ref_h = ref.copy()
    s64 = ep[:, :n].astype(np.float64)
    ref_h[:, :n] = np.where(s64 > 0, ref[:, :n], 0.0) if mode == 1 else ref[:, :n] + s64
    err = np.abs(out - ref_h).max() / np.abs(ref_h).max()
    print('%s mode %d: max |err| vs float64 conv + hook %.2e of max |ref|' % (label, mode, err))
    assert err < TOL, label
    if ldo:
        tail = got[2]
        assert tail.shape[-1] == ldo - cout and np.all(tail == 7.0), label      # the destination's columns cout .. ldo-1: never written


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', list(HOOK_CASES))
def test_conv5x5_hook_is_the_unhooked_launch_plus_the_elementwise_op(ops, name, form):
    B, cin, cout, H, W, c_ep, cols, ld, modes, no_split, ldo = HOOK_CASES[name]
    x, Wt, ref, ep = _hook_case(name)
    assert ops.conv5x5_ep_ksplit(form, cin, cout, ldo or cout, 0, no_split, B, H, W) == 1       # the table's "unsplit because"
    base = ops.conv5x5_ep(x, Wt, form, no_split=no_split, ldo=ldo)
    assert base[1] == 0                                                          # no hook asked for, none reported
    e0 = np.abs(base[0] - ref).max() / np.abs(ref).max()
    print('%s %s: unhooked max |err| vs float64 conv %.2e of max |ref|' % (name, form, e0))
    assert e0 < TOL
    for mode in modes:
        got = ops.conv5x5_ep(x, Wt, form, ep=ep, ep_cols=cols, ep_ld=ld, mode=mode, no_split=no_split, ldo=ldo)
        _check_hooked(got, base[0], ref, ep, cols, mode, ldo, '%s %s' % (name, form))


@pytest.mark.parametrize('form', FORMS)
def test_conv5x5_split_grid_leaves_the_hook_to_the_caller(ops, form):
    """lstm7's data gradient at B = 2 without no_split: where the device splits K (the library says so: it depends on the CU count), the launch must not take the
    hook at all -- applied == 0 and the plain conv's bits.  Two K groups (cin = 128) bound the split at 2, and 0 + a + b is the same fp32 number in either order
    of the two atomic adds, so the split launch is reproducible bit for bit."""
    B, cin, cout, H, W, c_ep, cols, ld, _, _, _ = HOOK_CASES['lstm7']
    x, Wt, ref, ep = _hook_case('lstm7')
    ks = ops.conv5x5_ep_ksplit(form, cin, cout, cout, 0, 0, B, H, W)
    base = ops.conv5x5_ep(x, Wt, form)
    got = ops.conv5x5_ep(x, Wt, form, ep=ep, ep_cols=cols, ep_ld=ld, mode=1)
    assert base[1] == 0 and np.abs(base[0] - ref).max() < TOL * np.abs(ref).max()
    if ks > 1:
        assert ks == 2
        assert got[1] == 0
        assert np.array_equal(_bits(got[0]), _bits(base[0]))                     # not half-applied
    else:
        print('%s: this device runs lstm7 at B = 2 unsplit (K split %d): the launch takes the hook' % (form, ks))
        _check_hooked(got, base[0], ref, ep, cols, 1, None, 'lstm7 unsplit by the launcher %s' % form)


# ---- the cell around it: pivp_convlstm_backward_form ----------------------------------------------------------------------------------------------------------
CELL_SHAPES = [(2, 96, 32, 32), (2, 128, 64, 16), (2, 32, 32, 32), (2, 64, 128, 8)]      # lstm7, lstm6, lstm1, lstm5 (8-wide map: an even batch)
# the hook as pivp_rollout_backward sets it for the cell: (source channels, ep_ld, ep_cols, mode); lstm5 has none
CELL_HOOKS = [(96, 96, 96, 1), (128, 128, 128, 1), (32, 64, 32, 2), None]
# the gates of the per-form convolution tests (tests/test_gpu_bf16.py).  test_conv5x5_bf16x3: max |err| < 5e-5 on outputs of unit rms (x ~ N(0, 1), W ~ N(0, 1 / K))
# and < 1/50 of the bf16 form's; the split form's error is relative to the products, so on a gradient of another size the same gate is 5e-5 of its rms.
# test_conv5x5_bf16x6 and test_conv5x5_fp16x3 allow their forms 1.2 and 1.5 times the rms error of the kernel they are measured against: here of the fp32 entry
# (precision 0) on the same inputs with the same det / dx_only.
# (Measured on an MI355X, lstm7's cell: the split form 5.4e-6 = 2.2e-5 of the gradient's rms against the 5e-5 gate and 1/490 of the bf16 form's 2.65e-3; the
# fp32-grade forms 0.45 .. 0.85 of the fp32 entry's rms error against the 1.2 / 1.5 allowed.)
BF16X3_ABS, BF16X3_OF_BF16, RATIO = 5e-5, 1.0 / 50, {3: 1.2, 4: 1.5}


def _shape(si):
    """a cell's (B, cx, C, H, W): an index into CELL_SHAPES (square maps), or such a tuple itself (tests/test_gpu_backward_shapes.py: H != W)"""
    return tuple(si) if isinstance(si, tuple) else CELL_SHAPES[si] + (CELL_SHAPES[si][3],)


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(DEV)      # (a copy: the cached cases are read-only)


def _nhwc(a):
    return _t(np.asarray(a).transpose(0, 2, 3, 1))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / (np.abs(b).max() + 1e-300)


def _rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))


@functools.lru_cache(maxsize=None)
def _cell_case(si, gscale=1.0):
    """inputs and float64 autograd as tests/test_gpu_backward_ops.py::test_convlstm_backward; gscale multiplies every cotangent"""
    B, cx, C, H, Wd = _shape(si)
    rs = np.random.RandomState(C + cx)
    x = rs.randn(B, cx, H, Wd); h = rs.randn(B, C, H, Wd) * 0.5; c = rs.randn(B, C, H, Wd)
    W = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
    dh = rs.randn(B, C, H, Wd) * gscale; dh2 = rs.randn(B, C, H, Wd) * 0.5 * gscale; dcn = rs.randn(B, C, H, Wd) * gscale
    tx, th, tc = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, h, c)]
    tW = torch.tensor(W, dtype=torch.float64, requires_grad=True); tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    g = F.conv2d(torch.cat((tx, th), 1), tW, tb, padding=2)
    g.retain_grad()
    j, i, f, o = torch.split(g, C, dim=1)
    cn = tc * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    hn = torch.tanh(cn) * torch.sigmoid(o)
    (hn * torch.tensor(dh + dh2) + cn * torch.tensor(dcn)).sum().backward()
    ref = dict(din=np.concatenate([tx.grad.numpy(), th.grad.numpy()], 1), dc=tc.grad.numpy(), dG=g.grad.numpy(), dW=tW.grad.numpy(), db=tb.grad.numpy())
    inp = dict(x=x, h=h, c=c, W=W, b=b, dh=dh, dh2=dh2, dcn=dcn)
    _frozen(*ref.values()); _frozen(*inp.values())
    return inp, ref


_DEV_CACHE = {}


def _cell_dev(env, si, gscale=1.0):
    """the case on the device, with the forward through pivp_convlstm_train; nothing in it is written by a backward run"""
    key = (si, gscale)
    if key in _DEV_CACHE:
        return _DEV_CACHE[key]
    pivp, _lib, lib = env
    B, cx, C, H, Wd = _shape(si)
    inp, _ = _cell_case(si, gscale)
    M = B * H * Wd
    d = dict(xd=_nhwc(inp['x']), hd=_nhwc(inp['h']), cd=_nhwc(inp['c']), wd=_t(pivp.to_internal('lstm1/conv/W', inp['W'])), bd=_t(inp['b']))
    d['c_out'] = torch.empty_like(d['cd']); d['h_out'] = torch.empty_like(d['hd'])
    d['gates'] = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_convlstm_train(d['xd'].data_ptr(), cx, cx, d['hd'].data_ptr(), C, d['wd'].data_ptr(), d['bd'].data_ptr(), d['cd'].data_ptr(),
                                       d['c_out'].data_ptr(), d['h_out'].data_ptr(), d['gates'].data_ptr(), B, H, Wd, _st()), 'fwd')
    # dh_b arrives as the last C channels of a wider buffer (the next step's d_in)
    d['wide'] = torch.zeros((M, cx + C), dtype=torch.float32, device=DEV)
    d['wide'][:, cx:] = _nhwc(inp['dh2']).reshape(M, C)
    d['dha'] = _nhwc(inp['dh']); d['dc0'] = _nhwc(inp['dcn'])
    torch.cuda.synchronize()
    _DEV_CACHE[key] = d
    return d


@functools.lru_cache(maxsize=None)
def _cell_hook_source(si):
    c_src, ld, cols, mode = CELL_HOOKS[si]
    B, cx, C, H, Wd = _shape(si)
    rs = np.random.RandomState(77 + si)
    if mode == 1:
        src = _relu_source(rs, (B * H * Wd, c_src), cols)
    else:
        src = rs.randn(B * H * Wd, c_src).astype(np.float32)
    return _frozen(src)[0]


def _run_cell(env, si, prec, det=0, dx_only=0, hook=False, gscale=1.0, legacy=False):
    """one cell backward; d_in prefilled with 1e3.  legacy: through pivp_convlstm_backward."""
    pivp, _lib, lib = env
    B, cx, C, H, Wd = _shape(si)
    d = _cell_dev(env, si, gscale)
    M, cin = B * H * Wd, cx + C
    dc = d['dc0'].clone()
    dG = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    wt = torch.empty_like(d['wd'])
    d_in = torch.full((M, cin), 1e3, dtype=torch.float32, device=DEV)
    dW = torch.zeros_like(d['wd']); db = torch.zeros_like(d['bd'])
    applied = ctypes.c_int(-1)
    head = (d['xd'].data_ptr(), cx, cx, d['hd'].data_ptr(), C, d['wd'].data_ptr(), d['gates'].data_ptr(), d['cd'].data_ptr(), d['c_out'].data_ptr(),
            d['dha'].data_ptr(), C, d['wide'].data_ptr() + cx * 4, cin, dc.data_ptr(), 1, dG.data_ptr(), wt.data_ptr(), d_in.data_ptr(), dW.data_ptr(),
            db.data_ptr())
    if legacy:
        _lib.check(lib.pivp_convlstm_backward(*head, B, H, Wd, _st()), 'pivp_convlstm_backward')
    else:
        scratch = torch.zeros(lib.pivp_convlstm_backward_form_scratch_floats(cx, C), dtype=torch.float32, device=DEV)
        ep = (None, 0, 0, 0)
        if hook:
            c_src, ld, cols, mode = CELL_HOOKS[si]
            buf = torch.full((M, ld), float('nan'), dtype=torch.float32, device=DEV)      # (a channel slice: the source is the buffer's last c_src channels)
            buf[:, ld - c_src:] = _t(_cell_hook_source(si))
            ep = (buf.data_ptr() + (ld - c_src) * 4, ld, cols, mode)
        _lib.check(lib.pivp_convlstm_backward_form(prec, *head, scratch.data_ptr() if prec else None, *ep, ctypes.byref(applied), det, dx_only,
                                                   B, H, Wd, _st()), 'pivp_convlstm_backward_form')
    torch.cuda.synchronize()
    nchw = lambda t, ch: t.cpu().numpy().reshape(B, H, Wd, ch).transpose(0, 3, 1, 2)
    return dict(din=nchw(d_in, cin), din_flat=d_in.cpu().numpy(), dG=nchw(dG, 4 * C), dG_flat=dG.cpu().numpy(), dc=nchw(dc, C), dc_flat=dc.cpu().numpy(),
                dW=pivp.from_internal('lstm1/conv/W', dW.cpu().numpy(), (4 * C, cin, 5, 5)), db=db.cpu().numpy(), applied=applied.value)


_ERR_CACHE = {}


def _form_err(env, si, prec, det, dx_only=0, gscale=1.0):
    """d_in error against autograd of a form's entry (cached: the fp32 entry is every fp32-grade form's yardstick, the bf16 form the split form's)"""
    key = (si, prec, det, dx_only, gscale)
    if key not in _ERR_CACHE:
        _ERR_CACHE[key] = _run_cell(env, si, prec, det=det, dx_only=dx_only, gscale=gscale)['din'] - _cell_case(si, gscale)[1]['din']
    return _ERR_CACHE[key]


def _check_cell(env, si, prec, r, det, dx_only=0, gscale=1.0, label=''):
    """the gates of one run: dG and dc from the fp32 gate kernel, no element of d_in left at its 1e3 prefill, d_in by the form's rule"""
    B, cx, C, H, Wd = _shape(si)
    _, ref = _cell_case(si, gscale)
    cols = slice(0, cx) if dx_only else slice(None)      # dx_only: the h columns are not asserted (left alone, cleared or computed: all within the contract)
    eG, eC = _rel(r['dG'], ref['dG']), _rel(r['dc'], ref['dc'])
    print('%s: dG %.2e, dc %.2e of max |ref|' % (label, eG, eC))
    assert eG < 2e-5 and eC < 2e-5, label
    din, rd = r['din'][:, cols], ref['din'][:, cols]
    assert np.isfinite(din).all() and np.abs(din).max() < 100.0 * max(1.0, np.abs(rd).max()), label      # nothing stays near the 1e3 prefill
    err = din - rd
    if prec == 1:
        # the float64 convolution of the operands the kernel multiplies: bf16(dG as the gate kernel left it) with bf16(W), flipped and transposed
        Wt = np.ascontiguousarray(_bf16(_cell_case(si, gscale)[0]['W'])[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        refq = R.conv2d(_bf16(r['dG']), Wt, np.zeros(cx + C), 1, 2)[:, cols]
        e = _rel(din, refq)
        print('%s: d_in vs the float64 conv of the bf16 operands %.2e of max |ref| (vs autograd %.2e)' % (label, e, _rel(din, rd)))
        assert e < 2e-5, label
    elif prec == 2:
        e3, e1 = np.abs(err).max(), np.abs(_form_err(env, si, 1, det, dx_only, gscale)[:, cols]).max()
        print('%s: d_in max |err| split %.2e, plain bf16 %.2e, rms of the gradient %.2e' % (label, e3, e1, _rms(rd)))
        assert e3 < BF16X3_ABS * _rms(rd) and e3 < e1 * BF16X3_OF_BF16, label
    else:
        ef = _form_err(env, si, 0, det, dx_only, gscale)[:, cols]
        print('%s: d_in rms err %.2e (max %.2e), fp32 entry %.2e (max %.2e), of a gradient of rms %.2e' % (label, _rms(err), np.abs(err).max(), _rms(ef), np.abs(ef).max(), _rms(rd)))
        assert _rel(din, rd) < 2e-5 and _rms(err) < RATIO[prec] * _rms(ef), label


@pytest.mark.parametrize('prec,si', [(p, s) for s in range(len(CELL_SHAPES)) for p in (1, 3, 4)] + [(2, 0)])
def test_convlstm_backward_in_every_form(env, prec, si):
    label = 'form %d cell %s' % (prec, CELL_SHAPES[si])
    _, ref = _cell_case(si)
    runs = {}
    for det in (0, 1):
        runs[det] = _run_cell(env, si, prec, det=det)
        _check_cell(env, si, prec, runs[det], det, label='%s det %d' % (label, det))
    if prec != 1:       # the weight gradient stays the fp32 kernel's in every form but bf16
        assert _rel(runs[0]['dW'], ref['dW']) < 2e-5 and _rel(runs[0]['db'], ref['db']) < 2e-5
    again = _run_cell(env, si, prec, det=1)
    assert np.array_equal(_bits(again['din_flat']), _bits(runs[1]['din_flat']))      # det: one block's plain store per element
    if CELL_HOOKS[si] is not None:
        c_src, ld, cols, mode = CELL_HOOKS[si]
        hooked = _run_cell(env, si, prec, det=1, hook=True)
        assert hooked['applied'] == 1
        exp = _host_hook(runs[1]['din_flat'], _cell_hook_source(si), cols, mode)
        assert np.array_equal(_bits(hooked['din_flat']), _bits(exp))
        assert np.array_equal(_bits(hooked['dG_flat']), _bits(runs[1]['dG_flat'])) and np.array_equal(_bits(hooked['dc_flat']), _bits(runs[1]['dc_flat']))
    assert runs[0]['applied'] == 0 and runs[1]['applied'] == 0


@pytest.mark.parametrize('prec', [1, 2, 3, 4])
def test_convlstm_backward_form_dx_only(env, prec):
    r = _run_cell(env, 0, prec, det=0, dx_only=1)
    _check_cell(env, 0, prec, r, 0, dx_only=1, label='form %d dx_only' % prec)


def test_convlstm_backward_fp16x3_with_gradient_sized_cotangents(env):
    """all cotangents x 1e-6: dG lies far below fp16's normal range, which is what the dg_absmax scale is for; the same relative gates"""
    r = _run_cell(env, 0, 4, det=0, gscale=1e-6)
    _check_cell(env, 0, 4, r, 0, gscale=1e-6, label='fp16x3 tiny cotangents')
    assert np.abs(r['dG']).max() < 1e-5


def test_convlstm_backward_form_at_precision_0_is_the_fp32_entry(env):
    """dG and dc (the gate kernel: no atomics) bit for bit.  d_in cannot be asked bit for bit: the fp32 data gradient splits K up to ten ways at this batch and
    its partial sums meet by atomic adds in any order, so two runs of pivp_convlstm_backward itself differ in the last bits.  Bound of that reordering: at most ten
    fp32 additions of partial sums no larger than max |d_in|, 2^-24 relative each: 6e-7 of max |ref|; gated at 2e-6.  (Measured on an MI355X: the two entries'
    d_in differ by 9.9e-8 and 1.2e-7 of max |ref| at the two shapes -- so they do differ, and by a twentieth of the gate.)"""
    for si in (0, 3):
        _, ref = _cell_case(si)
        a = _run_cell(env, si, 0, legacy=True)
        b = _run_cell(env, si, 0, hook=CELL_HOOKS[si] is not None)      # (the fp32 kernels have no hook: reported as not applied)
        assert b['applied'] == 0
        assert np.array_equal(_bits(a['dG_flat']), _bits(b['dG_flat'])) and np.array_equal(_bits(a['dc_flat']), _bits(b['dc_flat']))
        d = np.abs(a['din'] - b['din']).max() / np.abs(ref['din']).max()
        print('cell %s: precision 0 vs pivp_convlstm_backward: d_in differs by %.2e of max |ref|' % (CELL_SHAPES[si], d))
        assert d < 2e-6
        for r in (a, b):
            assert _rel(r['din'], ref['din']) < 2e-5 and _rel(r['dW'], ref['dW']) < 2e-5 and _rel(r['db'], ref['db']) < 2e-5


# ---- refusals: PIVP_ERR_BADARG in front of the first launch ------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(env):
    pivp, _lib, lib = env
    z = torch.zeros(1 << 21, dtype=torch.float32, device=DEV)             # every operand of the largest shape below fits: a call that is NOT refused stays in bounds
    out = torch.full((1 << 19,), 7.0, dtype=torch.float32, device=DEV)
    wb = torch.zeros(3 * lib.pivp_conv5x5_bf16_weight_elems(128, 128) + 256, dtype=torch.int16, device=DEV)
    scr = torch.zeros(lib.pivp_convlstm_backward_form_scratch_floats(96, 32), dtype=torch.float32, device=DEV)
    applied = ctypes.c_int(-1)

    def conv(prec, ldx=128, ep_ld=96, ep_cols=96, mode=1, B=2, H=32, W=32):
        return lib.pivp_conv5x5_ep(prec, z.data_ptr(), 128, ldx, z.data_ptr(), wb.data_ptr(), out.data_ptr(), 128, 128, 0, z.data_ptr(), ep_ld, ep_cols, mode, 1,
                                   scr.data_ptr(), ctypes.byref(applied), B, H, W, _st())

    def cell(prec, ep_ld=96, ep_cols=96, mode=1, B=2, H=32, W=32):
        p = z.data_ptr()
        return lib.pivp_convlstm_backward_form(prec, p, 96, 96, p, 32, p, p, p, p, p, 32, None, 0, out.data_ptr(), 0, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                               out.data_ptr(), out.data_ptr(), scr.data_ptr(), p, ep_ld, ep_cols, mode, ctypes.byref(applied), 1, 0, B, H, W, _st())

    for fn, bad in ((conv, (0, 5, -1)), (cell, (-1, 5))):
        for prec in bad:
            assert fn(prec) == BADARG, (fn.__name__, 'precision', prec)
        for prec in (1, 2, 3, 4):
            assert fn(prec, mode=3) == BADARG, (fn.__name__, 'ep_mode 3', prec)
            assert fn(prec, ep_ld=64, ep_cols=96) == BADARG, (fn.__name__, 'ep_ld < ep_cols', prec)
        for prec in (3, 4):
            assert fn(prec, B=3, H=8, W=8) == BADARG, (fn.__name__, '8-wide map, odd batch', prec)
    assert conv(4, ldx=160) == BADARG                                      # fp16x3: x contiguous
    assert lib.pivp_conv5x5_ep_ksplit(0, 128, 128, 128, 0, 0, 2, 32, 32) == BADARG
    torch.cuda.synchronize()
    assert applied.value == 0
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(z.abs().max()) == 0.0      # nothing ran
