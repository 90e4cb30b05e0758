"""GPU parity tests for every launch form of the plain convolutions (enc0, the 3x3 stride-2 convs, the transposed convs): each row of
tests/conv_form_cases.py first asserts the form the launcher takes (pivp_conv_form / pivp_conv_enc0_form, include/pivp_conv_forms.h), then holds
the kernel to the float64 oracle at test_gpu_ops.TOL (K <= 1,440 here, below the K <= 4,800 that constant was set for).  Then the strides a plan
passes on every step (channel slices of concat buffers, with guards on the neighbouring columns), the LayerNorm-on-load conv with its training
write-back and its fused enc3 epilogue (pivp_conv3x3s2_ln), and the LayerNorm partials the producers' epilogues write (pivp_conv_layernorm).
Every test prints its worst error (pytest -s); profiles/r22/NOTES.md records them."""
import numpy as np
import pytest

from oracle import restatement as R
import conv_form_cases as CF
from test_gpu_ops import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    import conv_ops
    return conv_ops


@pytest.fixture(scope='module')
def hops():
    import hip_ops
    return hip_ops


def _report(what, **errs):
    print('conv_forms %s: %s' % (what, '  '.join('%s = %.3e' % kv for kv in errs.items())))


def _cid(c):
    return '%s-B%d-%dx%dx%d-to%d-%s%s' % (c.op, c.B, c.cin, c.H, c.W, c.cout, c.form, '-bias+%d' % c.bias_off if c.bias_off else '')


# ---- form parity ----------------------------------------------------------------------------------------------------------------------------------
_refs = {}      # one input and one float64 pre-activation per group of rows (rows of a group differ in cout: the first columns of one weight)


def _operands(c):
    key = c.group or _cid(c)
    if key not in _refs:
        rows = [r for r in CF.CASES if (r.group or _cid(r)) == key]
        cmax = max(r.cout for r in rows)
        rs = np.random.RandomState(len(key) * 1000 + c.B * 10 + c.cin)
        x = rs.randn(c.B, c.cin, c.H, c.W)
        if c.op == 'conv':
            W = rs.randn(cmax, c.cin, 3, 3) / np.sqrt(9 * c.cin)
        else:
            W = rs.randn(c.cin, cmax, 3, 3) / np.sqrt(9 * c.cin)
        b = rs.randn(cmax) * 0.1
        f32 = lambda a: a.astype(np.float32).astype(np.float64)       # the values the kernel receives
        pre = R.conv2d(f32(x), f32(W), f32(b), 2, 1) if c.op == 'conv' else R.deconv2d(f32(x), f32(W), f32(b), 2, 1, (2 * c.H, 2 * c.W))
        _refs[key] = (x, W, b, pre)
    x, W, b, pre = _refs[key]
    return x, (W[:c.cout] if c.op == 'conv' else W[:, :c.cout]), b[:c.cout], pre[:, :c.cout]


@pytest.mark.parametrize('c,relu', [pytest.param(c, relu, id='%s-relu%d' % (_cid(c), relu)) for c in CF.CASES for relu in c.relus])
def test_form_parity(ops, c, relu):
    assert ops.conv_form(c.op, c.cin, c.cout, c.B, c.H, c.W, aligned=c.bias_off == 0) == CF.FORM[c.form], c
    x, W, b, pre = _operands(c)
    ref = R.relu(pre) if relu else pre
    got, guard = ops.conv(c.op, x, W, b, relu, bias_off=c.bias_off)
    err = np.abs(got - ref).max()
    _report('%s relu=%d' % (_cid(c), relu), err=err)
    assert guard.size == 0 and err < TOL


@pytest.mark.parametrize('c', CF.ENC0_CASES, ids=lambda c: 'enc0-B%d-%dx%d-%s' % (c.B, c.H, c.W, c.form))
def test_enc0_form_parity(ops, hops, c):
    assert ops.enc0_form(c.B, c.H, c.W) == CF.ENC0_FORM[c.form], c
    rs = np.random.RandomState(c.H * 10 + c.W)
    img = rs.rand(c.B, 3, c.H, c.W); W = rs.randn(32, 3, 5, 5) / np.sqrt(75); b = rs.randn(32) * 0.1
    err = np.abs(hops.conv_enc0(img, W, b) - R.conv2d(img, W, b, 2, 2)).max()
    _report('enc0 %dx%d %s' % (c.H, c.W, c.form), err=err)
    assert err < TOL


# ---- strides and guards ---------------------------------------------------------------------------------------------------------------------------
# (op, B, cin, H, W, cout, form, ld of the input buffer, ldo, column offset of the output slice)
STRIDED = [
    ('conv', 3, 32, 16, 16, 32, 'small1', 64, 96, 64),          # enc1's output: cat6[:, 64:96]; its input as the skip cat7 + 32 is read
    ('deconv', 3, 64, 48, 60, 64, 'small2', 96, 128, 32),       # a 64-channel slice of a 96-wide concat
    ('deconv', 3, 96, 48, 60, 96, 'small3', 96, 160, 32),       # enc5 reading 96 of 96
    ('deconv', 1, 64, 32, 32, 64, 'deconv_tile', 96, 128, 64),
    ('deconv', 3, 96, 16, 16, 96, 'deconv_tile', 96, 128, 0),   # enc5 at the product size: 96 of 96 into the leading columns
]


@pytest.mark.parametrize('op,B,cin,H,W,cout,form,ld,ldo,ooff', STRIDED, ids=['%s-%s-ld%d-ldo%d+%d' % (s[0], s[6], s[7], s[8], s[9]) for s in STRIDED])
def test_conv_on_channel_slices_leaves_the_neighbours_alone(ops, op, B, cin, H, W, cout, form, ld, ldo, ooff):
    assert ops.conv_form(op, cin, cout, B, H, W) == CF.FORM[form]
    rs = np.random.RandomState(ld + ldo + ooff)
    x = rs.randn(B, cin, H, W)
    Wt = (rs.randn(cout, cin, 3, 3) if op == 'conv' else rs.randn(cin, cout, 3, 3)) / np.sqrt(9 * cin)
    b = rs.randn(cout) * 0.1
    ref = R.relu(R.conv2d(x, Wt, b, 2, 1) if op == 'conv' else R.deconv2d(x, Wt, b, 2, 1, (2 * H, 2 * W)))
    got, guard = ops.conv(op, x, Wt, b, True, ld=ld, ldo=ldo, ooff=ooff)
    err = np.abs(got - ref).max()      # (NaN if a neighbouring input column was read)
    _report('strided %s %s ld=%d ldo=%d+%d' % (op, form, ld, ldo, ooff), err=err)
    assert guard.shape[-1] == ldo - cout and np.all(guard == ops.PREFILL)
    assert err < TOL
    plain, _ = ops.conv(op, x, Wt, b, True)
    assert np.array_equal(got, plain)      # the strides change addresses, not arithmetic


@pytest.mark.parametrize('B,C,H,ldo,ooff,relu', [(3, 32, 32, 64, 32, True), (3, 64, 16, 96, 0, False)])
def test_layernorm_into_a_channel_slice(ops, B, C, H, ldo, ooff, relu):
    """ln() of a rollout: norm_enc0 writes cat7[:, 32:64] (with the ReLU), hidden6's norm cat6[:, :64]"""
    rs = np.random.RandomState(ldo)
    x = rs.randn(B, C, H, H) * 2 + 0.7
    n = C * H * H
    g = 1 + 0.1 * rs.randn(n); be = 0.1 * rs.randn(n)
    ref = R.layer_norm_conv2d(x, g, be, 1e-6)
    if relu:
        ref = R.relu(ref)
    got, guard = ops.layernorm(x, g, be, 1e-6, relu, ldo=ldo, ooff=ooff)
    err = np.abs(got - ref).max()
    _report('layernorm %d of %d at %d' % (C, ldo, ooff), err=err)
    assert guard.shape[-1] == ldo - C and np.all(guard == ops.PREFILL) and err < TOL


def _lstm_ref(x, h, c, W, b):
    g = R.conv2d(np.concatenate((x, h), 1), W, b, 1, 2)
    j, i, f, o = np.split(g, 4, axis=1)
    cn = c * R.sigmoid(f + 1.0) + R.sigmoid(i) * np.tanh(j)
    return np.tanh(cn) * R.sigmoid(o), cn


_lstm_cache = {}


def _lstm_case(C):
    if C not in _lstm_cache:
        rs = np.random.RandomState(500 + C)
        B, cx, H = 2, 32, 16
        x = rs.randn(B, cx, H, H); h = rs.randn(B, C, H, H) * 0.5; c = rs.randn(B, C, H, H)
        W = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
        _lstm_cache[C] = (x, h, c, W, b) + _lstm_ref(x, h, c, W, b)
    return _lstm_cache[C]


@pytest.mark.parametrize('C,ld', [(32, 64), (64, 96)], ids=['lstm1-cat7+32', 'lstm3-cat6+64'])
@pytest.mark.parametrize('entry,variant', [('f32', v) for v in range(5)] + [(e, 0) for e in ('bf16', 'bf16x3', 'bf16x6', 'fp16x3')])
def test_convlstm_reads_the_last_channels_of_a_concat(ops, entry, variant, C, ld):
    """lstm1 reads cx = 32 at cat7 + 32 (ld 64), lstm3 at cat6 + 64 (ld 96): the other columns are NaN here.  The stride moves addresses only, so the result has
    the bits of the same entry on a contiguous x; the fp32 variants are held to the float64 oracle besides (the packed forms' own accuracy: test_gpu_bf16.py)."""
    x, h, c, W, b, hr, cr = _lstm_case(C)
    hs, cs = ops.convlstm(entry, x, h, c, W, b, ld=ld, variant=variant)
    hc, cc = ops.convlstm(entry, x, h, c, W, b, variant=variant)
    err = max(np.abs(hs - hr).max(), np.abs(cs - cr).max())
    _report('convlstm %s v%d C=%d ld=%d' % (entry, variant, C, ld), err_vs_float64=err)
    assert np.isfinite(hs).all() and np.isfinite(cs).all()
    assert np.array_equal(hs, hc) and np.array_equal(cs, cc)
    if entry == 'f32':
        assert err < TOL


# ---- the LayerNorm-on-load conv -------------------------------------------------------------------------------------------------------------------
# (B, cin, H, W, cout, the igemm_small form, with the enc3 epilogue).  The fourth shape stands for the issue's (8, 32, 120, 140) to 96: that map has
# 60 * 70 = 4,200 anchors per sample, no multiple of 32, so the LayerNorm-on-load form refuses it (below); 128 x 128 reaches <3, true> at the same batch.
LN_CONV = [(3, 32, 16, 8, 32, 'small1', False), (2, 64, 16, 16, 64, 'small1', True), (8, 64, 128, 128, 64, 'small2', False), (8, 32, 128, 128, 96, 'small3', False)]


@pytest.mark.parametrize('B,cin,H,W,cout,form,with_ep', LN_CONV, ids=['B%d-%dx%dx%d-to%d-%s%s' % (s[0], s[1], s[2], s[3], s[4], s[5], '-ep' if s[6] else '') for s in LN_CONV])
def test_conv3x3s2_of_norm_in_one_launch(ops, hops, B, cin, H, W, cout, form, with_ep):
    """enc1 / enc2 behind hidden2 / hidden4 (TM:560-563): within TOL of the float64 conv of the float64 norm and BIT-identical to pivp_layernorm followed by
    pivp_conv3x3s2; the training write-back is pivp_layernorm's output bit for bit, with the samples' (mean, rstd); the fused epilogue is pivp_enc3_state on the
    conv's own output, bit for bit (it replaces the form the table names by <2, true, true>: all 64 channels of a pixel in one block)."""
    lib = ops._lib.load()
    assert lib.pivp_conv3x3s2_ln_fits(cin, cout, B, H, W) == 1 and ops.conv_form('conv', cin, cout, B, H, W) == CF.FORM[form]
    rs = np.random.RandomState(B * 100 + cin + W)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = f32(rs.randn(B, cin, H, W) * 0.3 + 0.1)
    n = cin * H * W
    g = f32(1 + 0.1 * rs.randn(n)); be = f32(0.1 * rs.randn(n))
    Wt = f32(rs.randn(cout, cin, 3, 3) / np.sqrt(9 * cin)); b = f32(rs.randn(cout) * 0.1)
    xn = R.layer_norm_conv2d(x, g, be, 1e-6)
    ref = R.relu(R.conv2d(xn, Wt, b, 2, 1))
    one = ops.conv3x3s2_ln(x, g, be, Wt, b, True)
    err = np.abs(one['out'] - ref).max()
    # the two launches a plan without the fold runs
    two_n, _ = ops.layernorm(x, g, be, 1e-6, False)
    two, _ = ops.conv('conv', two_n, Wt, b, True)
    # the training form: the same launch also writes the normalised input (into the leading columns of a wider buffer) and the statistics
    kept = ops.conv3x3s2_ln(x, g, be, Wt, b, True, keep_ld=cin + 32)
    mu = x.reshape(B, -1).mean(1); rstd = 1.0 / np.sqrt(x.reshape(B, -1).var(1) + 1e-6)
    stat_err = max(np.abs(kept['stat'][:, 0] / mu - 1).max(), np.abs(kept['stat'][:, 1] / rstd - 1).max())
    _report('conv3x3s2_ln B=%d %dx%dx%d to %d %s' % (B, cin, H, W, cout, form), err=err, keep_err=np.abs(kept['keep'] - xn).max(), stat_rel_err=stat_err)
    assert err < TOL
    assert np.array_equal(one['out'], two)
    assert np.array_equal(kept['out'], one['out']) and np.array_equal(kept['keep'], two_n) and np.all(kept['keep_guard'] == ops.PREFILL)
    assert stat_err < 1e-6
    if with_ep:
        act = rs.randn(B, 5) * 0.1; st = rs.randn(B, 5) * 0.1
        W3 = rs.randn(64, 74, 1, 1) / np.sqrt(74); b3 = rs.randn(64) * 0.1
        Wcs = rs.randn(5, 10); bcs = rs.randn(5)
        for use_state in (True, False):
            w3 = W3 if use_state else W3[:, :64]
            fused = ops.conv3x3s2_ln(x, g, be, Wt, b, True, ep=dict(action=act, state=st, W3=w3, b3=b3, Wcs=Wcs, bcs=bcs, use_state=use_state))
            e3, snew = hops.enc3_state(fused['out'], act, st, w3, b3, Wcs, bcs, use_state=use_state)
            assert np.array_equal(fused['out'], one['out'])
            assert np.array_equal(fused['e3'], e3) and np.array_equal(fused['state'], snew), use_state
            # ... and both against float64
            sa = np.concatenate((act, st), 1)
            xin = np.concatenate((ref, np.tile(sa[:, :, None, None], (1, 1, H // 2, W // 2))), 1) if use_state else ref
            e3_err = np.abs(fused['e3'] - R.relu(R.conv2d(xin, w3, b3, 1, 0))).max()
            s_err = np.abs(fused['state'] - R.linear(sa, Wcs, bcs)).max()
            _report('conv3x3s2_ln epilogue use_state=%d' % use_state, e3_err=e3_err, state_err=s_err)
            assert e3_err < TOL and s_err < TOL


@pytest.mark.parametrize('cin,cout,B,H,W,ep,why', [
    (32, 32, 3, 10, 6, False, '15 anchors per sample'), (32, 96, 8, 120, 140, False, '4,200 anchors per sample'), (48, 32, 3, 16, 8, False, 'cin % 32'),
    (32, 32, 3, 16, 8, True, 'the epilogue needs cout == 64'), (64, 96, 2, 16, 16, True, 'the epilogue needs cout == 64')])
def test_conv3x3s2_of_norm_refusals_launch_nothing(ops, cin, cout, B, H, W, ep, why):
    rc, untouched = ops.conv3x3s2_ln_refused(cin, cout, B, H, W, ep=ep)
    assert rc == -1 and untouched, why
    if not ep:
        assert ops._lib.load().pivp_conv3x3s2_ln_fits(cin, cout, B, H, W) == 0


def test_conv3x3s2_of_norm_refuses_a_bad_write_back(ops):
    for keep_ld in (16, 34):      # narrower than cin; no multiple of 4
        rc, untouched = ops.conv3x3s2_ln_refused(32, 32, 3, 16, 8, keep_ld=keep_ld)
        assert rc == -1 and untouched, keep_ld
    rc, untouched = ops.conv3x3s2_ln_refused(64, 64, 2, 16, 16, ep=True, keep_ld=64)      # the write-back and the epilogue exclude each other
    assert rc == -1 and untouched


# ---- the producers' LayerNorm partials ------------------------------------------------------------------------------------------------------------
# (kind, B, cin, H, W, cout, form): one row per form that writes partials -- igemm_small's layout depends on ntb -- and per kind one that writes none
PARTIALS = [
    ('enc0', 3, 3, 32, 32, 32, 'rows'), ('enc0', 3, 3, 64, 64, 32, 'rows'), ('enc0', 3, 3, 24, 16, 32, 'generic'),
    ('conv', 3, 32, 16, 16, 32, 'small1'), ('conv', 3, 32, 16, 16, 64, 'small1'), ('conv', 3, 32, 10, 6, 32, 'small1'),
    ('deconv', 3, 64, 48, 60, 64, 'small2'), ('deconv', 3, 96, 48, 60, 96, 'small3'),
    ('deconv', 2, 128, 32, 60, 128, 'small1'), ('deconv', 2, 128, 40, 60, 128, 'small2'),      # four and two column blocks: the partial index runs over them
    ('deconv', 1, 64, 32, 32, 64, 'deconv_tile'), ('deconv', 3, 64, 50, 55, 64, 'small2'),
]


def _producer(kind, B, cin, H, W, cout, rs, scale=1.0, offset=0.0):
    x = rs.rand(B, 3, H, W) if kind == 'enc0' else rs.randn(B, cin, H, W)
    if kind == 'enc0':
        Wt = rs.randn(32, 3, 5, 5) / np.sqrt(75)
    else:
        Wt = (rs.randn(cout, cin, 3, 3) if kind == 'conv' else rs.randn(cin, cout, 3, 3)) / np.sqrt(9 * cin)
    Wt = Wt * scale
    b = rs.randn(cout) * 0.1 * scale + offset
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x, Wt, b = f32(x), f32(Wt), f32(b)
    raw = R.conv2d(x, Wt, b, 2, 2) if kind == 'enc0' else R.conv2d(x, Wt, b, 2, 1) if kind == 'conv' else R.deconv2d(x, Wt, b, 2, 1, (2 * H, 2 * W))
    return x, Wt, b, raw


def _form_of(ops, kind, B, cin, H, W, cout):
    if kind == 'enc0':
        return {v: k for k, v in CF.ENC0_FORM.items()}[ops.enc0_form(B, H, W)]
    return {v: k for k, v in CF.FORM.items()}[ops.conv_form(kind, cin, cout, B, H, W)]


@pytest.mark.parametrize('kind,B,cin,H,W,cout,form', PARTIALS, ids=['%s-B%d-%dx%dx%d-to%d-%s' % (p[0], p[1], p[2], p[3], p[4], p[5], p[6]) for p in PARTIALS])
def test_producer_partials_feed_the_norm(ops, hops, kind, B, cin, H, W, cout, form):
    """norm(conv(x)) with the statistics from the producer's epilogue, as a rollout runs norm_enc0 and norm_enc6: the count of partials is the launcher's
    formula, the norm within 1e-4 of float64 (it divides by std(raw) ~ 0.3 .. 1: the gate of test_convlstm_layernorm_fused_stats) and within 2e-6 of
    pivp_layernorm (its own statistics pass) on the kernel's raw output."""
    assert _form_of(ops, kind, B, cin, H, W, cout) == form
    rs = np.random.RandomState(B * 1000 + H * 10 + cout)
    x, Wt, b, raw_ref = _producer(kind, B, cin, H, W, cout, rs)
    n = raw_ref[0].size
    g = 1 + 0.1 * rs.randn(n); be = 0.1 * rs.randn(n)
    relu_ln = kind != 'conv'      # norm_enc0 and norm_enc6 are followed by a ReLU
    ref = R.layer_norm_conv2d(raw_ref, g, be, 1e-6)
    raw, ln, fused, guard = ops.conv_layernorm(kind, x, Wt, b, False, g, be, 1e-6, relu_ln, ldo=cout + 32, ooff=32)
    own = hops.layernorm(raw, g, be, 1e-6, relu_ln)
    if relu_ln:
        ref = R.relu(ref)
    raw_err, err, own_err = np.abs(raw - raw_ref).max(), np.abs(ln - ref).max(), np.abs(ln - own).max()
    _report('partials %s %s B=%d %dx%d to %d' % (kind, form, B, H, W, cout), fused=fused, raw_err=raw_err, err=err, vs_own_stats=own_err)
    assert fused == CF.partials_per_sample(kind, form, cout, H, W)
    assert np.all(guard == ops.PREFILL)
    assert raw_err < TOL and err < 1e-4 and own_err < 2e-6


@pytest.mark.parametrize('kind,B,cin,H,W,cout,form', [('enc0', 2, 3, 64, 64, 32, 'rows'), ('conv', 2, 32, 64, 64, 32, 'small1'), ('deconv', 2, 64, 32, 32, 64, 'deconv_tile'),
                                                       ('deconv', 3, 64, 48, 60, 64, 'small2')])
def test_producer_partials_with_a_large_offset(ops, kind, B, cin, H, W, cout, form):
    """raw output mean ~ 100, std ~ 0.01 (through a large bias): per-tile (count, mean, M2) partials merged by Chan's formula keep the variance a
    sum / sum-of-squares form would lose.  The bound of test_layernorm_large_offset_is_stable, 2e-3: the fp32 quantisation of the raw output dominates
    (half an ulp of 100, 3.8e-6, over a std of 0.01).  Against the float64 norm of the kernel's OWN raw output -- the statistics alone -- every producer is held
    to it.  Against the float64 norm of the float64 conv, the igemm kernels and the tile kernel are too: they add the bias once, to the finished sum.  enc0's
    kernels start their 75-term fmaf chain FROM the bias, so each of its 76 roundings is one of a number near 100: |raw error| <= 76 * 2^-18 = 2.9e-4, which
    the norm divides by std(raw).  (Measured: 8.6e-3 for enc0 against 8e-4 .. 1.3e-3 for the others; profiles/r22/NOTES.md.  Real biases are O(0.1).)"""
    assert _form_of(ops, kind, B, cin, H, W, cout) == form
    rs = np.random.RandomState(H + cout)
    x, Wt, b, raw_ref = _producer(kind, B, cin, H, W, cout, rs, scale={'enc0': 0.0175, 'conv': 0.01, 'deconv': 0.02}[kind], offset=100.0)
    n = raw_ref[0].size
    ref = R.layer_norm_conv2d(raw_ref, np.ones(n), np.zeros(n), 1e-6)
    raw, ln, fused, _ = ops.conv_layernorm(kind, x, Wt, b, False, np.ones(n), np.zeros(n), 1e-6, False)
    own = R.layer_norm_conv2d(raw.astype(np.float64), np.ones(n), np.zeros(n), 1e-6)
    err, own_err, raw_err = np.abs(ln - ref).max(), np.abs(ln - own).max(), np.abs(raw - raw_ref).max()
    _report('partials %s %s large offset' % (kind, form), fused=fused, raw_mean=raw_ref.mean(), raw_std=raw_ref.std(), raw_err=raw_err, err=err, vs_norm_of_own_raw=own_err)
    assert fused == CF.partials_per_sample(kind, form, cout, H, W) > 0
    assert 99.9 < raw_ref.mean() < 100.1 and 0.007 < raw_ref.std() < 0.014
    bound = 2e-2 * 0.05 + 1e-3
    assert own_err < bound
    assert err < bound + (76 * 2.0 ** -18 / raw_ref.std() if kind == 'enc0' else 0.0)
