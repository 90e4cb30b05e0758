"""The per-op backward parity checks with the map's height and width as separate arguments: HIP (through the C ABI) against PyTorch autograd or NumPy in
float64 on the CPU, on the same seeded inputs.  tests/test_gpu_backward_ops.py runs them on the model's square power-of-two maps (H, H),
tests/test_gpu_backward_shapes.py on maps that are neither.  Every function takes env = (pivp_amd, _lib, the loaded library) and asserts the op's gate."""
import numpy as np
import torch
import torch.nn.functional as F

DEV = 'cuda:0'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def _nhwc(a):
    return _t(np.asarray(a).transpose(0, 2, 3, 1))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / (np.abs(b).max() + 1e-30)


def _cell_autograd(x, h, c, W, b, C, dh, dcn):
    """float64 autograd of one ConvLSTM cell with cotangents dh on h_t and dcn on c_t -> (tx, th, tc, tW, tb) with .grad"""
    tx, th, tc = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, h, c)]
    tW = torch.tensor(W, dtype=torch.float64, requires_grad=True); tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    g = F.conv2d(torch.cat((tx, th), 1), tW, tb, padding=2)
    j, i, f, o = torch.split(g, C, dim=1)
    cn = tc * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    hn = torch.tanh(cn) * torch.sigmoid(o)
    (hn * torch.tensor(dh) + cn * torch.tensor(dcn)).sum().backward()
    return tx, th, tc, tW, tb


def convlstm_backward(env, B, cx, C, H, Wd, first):
    pivp, _lib, lib = env
    rs = np.random.RandomState(C + cx)
    x = rs.randn(B, cx, H, Wd); h = np.zeros((B, C, H, Wd)) if first else rs.randn(B, C, H, Wd) * 0.5
    c = np.zeros((B, C, H, Wd)) if first else rs.randn(B, C, H, Wd)
    W = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
    dh = rs.randn(B, C, H, Wd); dh2 = rs.randn(B, C, H, Wd) * 0.5; dcn = rs.randn(B, C, H, Wd)
    # reference: autograd
    tx, th, tc, tW, tb = _cell_autograd(x, h, c, W, b, C, dh + dh2, dcn)
    # HIP
    xd, hd, cd = _nhwc(x), _nhwc(h), _nhwc(c)
    wd, bd = _t(pivp.to_internal('lstm1/conv/W', W)), _t(b)
    c_out = torch.empty_like(cd); h_out = torch.empty_like(hd)
    M = B * H * Wd
    gates = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_convlstm_train(xd.data_ptr(), cx, cx, None if first else hd.data_ptr(), C, wd.data_ptr(), bd.data_ptr(),
                                       cd.data_ptr(), c_out.data_ptr(), h_out.data_ptr(), gates.data_ptr(), B, H, Wd, _st()), 'fwd')
    # dh_b arrives as the last C channels of a wider buffer (the next step's d_in), exercise that stride
    wide = torch.zeros((M, cx + C), dtype=torch.float32, device=DEV)
    wide[:, cx:] = _nhwc(dh2).reshape(M, C)
    dha = _nhwc(dh)
    dc = _nhwc(dcn).clone()
    dG = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    wt = torch.empty_like(wd)
    d_in = torch.empty((M, cx + C), dtype=torch.float32, device=DEV)
    dW = torch.zeros_like(wd); db = torch.zeros_like(bd)
    _lib.check(lib.pivp_convlstm_backward(xd.data_ptr(), cx, cx, None if first else hd.data_ptr(), C, wd.data_ptr(), gates.data_ptr(),
                                          cd.data_ptr(), c_out.data_ptr(), dha.data_ptr(), C, (wide.data_ptr() + cx * 4), cx + C,
                                          dc.data_ptr(), 1, dG.data_ptr(), wt.data_ptr(), d_in.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                          B, H, Wd, _st()), 'bwd')
    torch.cuda.synchronize()
    din = d_in.cpu().numpy().reshape(B, H, Wd, cx + C).transpose(0, 3, 1, 2)
    dW_ref = tW.grad.numpy().copy()
    if first:
        dW_ref[:, cx:] = 0          # the skipped zero-h K range gets no gradient (h == 0 => it is exactly 0 anyway)
    got_dW = pivp.from_internal('lstm1/conv/W', dW.cpu().numpy(), W.shape)
    errs = dict(dx=_rel(din[:, :cx], tx.grad.numpy()), dh=0.0 if first else _rel(din[:, cx:], th.grad.numpy()),
                dc=_rel(dc.cpu().numpy().reshape(B, H, Wd, C).transpose(0, 3, 1, 2), tc.grad.numpy()),
                dW=_rel(got_dW, dW_ref), db=_rel(db.cpu().numpy(), tb.grad.numpy()))
    print('convlstm backward B %d %d+%d @%dx%d first %d: ' % (B, cx, C, H, Wd, first) + ', '.join('%s %.2e' % kv for kv in errs.items()) + ' of max |ref|')
    assert errs['dx'] < 2e-5
    if not first:
        assert errs['dh'] < 2e-5
    assert errs['dc'] < 2e-5
    assert errs['dW'] < 2e-5
    assert errs['db'] < 2e-5


def _conv_case(rs, mode, cin, cout):
    if mode:
        return rs.randn(cin, cout, 3, 3) / np.sqrt(9 * cin), 'enc4/W'
    return rs.randn(cout, cin, 3, 3) / np.sqrt(9 * cin), 'enc1/W'


def _conv_fwd(mode, tx, tW, tb):
    return F.conv_transpose2d(tx, tW, tb, stride=2, padding=1, output_padding=1) if mode else F.conv2d(tx, tW, tb, stride=2, padding=1)


def conv_deconv_backward(env, mode, B, cin, cout, H, Wd):
    pivp, _lib, lib = env
    rs = np.random.RandomState(cin + mode)
    x = rs.randn(B, cin, H, Wd)
    Ho, Wo = (2 * H, 2 * Wd) if mode else (H // 2, Wd // 2)
    dy = rs.randn(B, cout, Ho, Wo)
    W, key = _conv_case(rs, mode, cin, cout)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True); tW = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (_conv_fwd(mode, tx, tW, tb) * torch.tensor(dy)).sum().backward()
    xd, dyd = _nhwc(x), _nhwc(dy)
    wd = _t(pivp.to_internal(key, W))
    wt = torch.empty_like(wd); dW = torch.zeros_like(wd); db = torch.zeros(cout, dtype=torch.float32, device=DEV)
    prior = rs.randn(B, H, Wd, cin).astype(np.float32)
    dx = _t(prior)
    _lib.check(lib.pivp_conv_backward(mode, xd.data_ptr(), cin, cin, wd.data_ptr(), dyd.data_ptr(), cout, cout, wt.data_ptr(),
                                      dx.data_ptr(), cin, 1, dW.data_ptr(), db.data_ptr(), B, H, Wd, _st()), 'conv_backward')
    torch.cuda.synchronize()
    got_dx = (dx.cpu().numpy() - prior).transpose(0, 3, 1, 2)      # accum_dx = 1 adds into the existing buffer
    errs = (_rel(got_dx, tx.grad.numpy()), _rel(pivp.from_internal(key, dW.cpu().numpy(), W.shape), tW.grad.numpy()), _rel(db.cpu().numpy(), tb.grad.numpy()))
    print('conv backward mode %d B %d %d->%d @%dx%d: dx %.2e, dW %.2e, db %.2e of max |ref|' % ((mode, B, cin, cout, H, Wd) + errs))
    assert errs[0] < 2e-5
    assert errs[1] < 2e-5
    assert errs[2] < 2e-5


def layernorm_backward(env, B, C, H, Wd, relu):
    pivp, _lib, lib = env
    rs = np.random.RandomState(C)
    n = C * H * Wd
    x = rs.randn(B, C, H, Wd) * 2 + 0.5; g = 1 + 0.1 * rs.randn(n); be = 0.1 * rs.randn(n); dy = rs.randn(B, C, H, Wd)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(g, dtype=torch.float64, requires_grad=True); tb = torch.tensor(be, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(tx.reshape(B, -1), (n,), tg, tb, 1e-6).reshape(x.shape)
    if relu:
        y = F.relu(y)
    (y * torch.tensor(dy)).sum().backward()
    perm = lambda v: _t(np.asarray(v).reshape(C, H * Wd).T)
    xd, gd, bd = _nhwc(x), perm(g), perm(be)
    ldo = C + 32                                               # output / dy live in a wider concat buffer
    out = torch.zeros((B, H, Wd, ldo), dtype=torch.float32, device=DEV)
    scratch = torch.empty(lib.pivp_layernorm_scratch_floats(B, n), dtype=torch.float32, device=DEV)
    stat = torch.empty((B, 2), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_layernorm_train(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr() + 32 * 4, scratch.data_ptr(),
                                        stat.data_ptr(), B, n, C, ldo, 1e-6, int(relu), _st()), 'ln fwd')
    dyw = torch.zeros((B, H, Wd, ldo), dtype=torch.float32, device=DEV)
    dyw[..., 32:] = _nhwc(dy)
    dx = torch.empty_like(xd); dg = torch.zeros_like(gd); dbt = torch.zeros_like(bd)
    sc2 = torch.empty(lib.pivp_layernorm_backward_scratch_floats(B, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_layernorm_backward(dyw.data_ptr() + 32 * 4, ldo, out.data_ptr() + 32 * 4, ldo, xd.data_ptr(), stat.data_ptr(),
                                           gd.data_ptr(), sc2.data_ptr(), dx.data_ptr(), dg.data_ptr(), dbt.data_ptr(), B, n, C,
                                           int(relu), _st()), 'ln bwd')
    torch.cuda.synchronize()
    unperm = lambda t: t.cpu().numpy().reshape(H * Wd, C).T.ravel()
    errs = (_rel(dx.cpu().numpy().transpose(0, 3, 1, 2), tx.grad.numpy()), _rel(unperm(dg), tg.grad.numpy()), _rel(unperm(dbt), tb.grad.numpy()))
    print('layernorm backward B %d C %d @%dx%d relu %d: dx %.2e, dgamma %.2e, dbeta %.2e of max |ref|' % ((B, C, H, Wd, int(relu)) + errs))
    assert errs[0] < 3e-5
    assert errs[1] < 3e-5 and errs[2] < 3e-5


def conv_weight_gradient_batched_over_timesteps(env, mode, B, cin, cout, H, Wd, T):
    pivp, _lib, lib = env
    rs = np.random.RandomState(cin + mode + B + T)
    Ho, Wo = (2 * H, 2 * Wd) if mode else (H // 2, Wd // 2)
    x = rs.randn(T, B, cin, H, Wd); dy = rs.randn(T, B, cout, Ho, Wo)
    W, key = _conv_case(rs, mode, cin, cout)
    tW = torch.tensor(W, dtype=torch.float64, requires_grad=True); tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    tot = 0
    for t in range(T):
        tot = tot + (_conv_fwd(mode, torch.tensor(x[t], dtype=torch.float64), tW, tb) * torch.tensor(dy[t])).sum()
    tot.backward()
    # forward slabs hold x[t] at slab t; the sweep runs t = T-1 .. 0 and its dY ring slot j holds timestep T-1-j
    xd = _t(np.ascontiguousarray(x.transpose(0, 1, 3, 4, 2)))
    dyd = _t(np.ascontiguousarray(dy[::-1].transpose(0, 1, 3, 4, 2)))
    n = lib.pivp_conv_backward_part_floats(mode, cin, cout, B, H, Wd)
    assert n > 0
    part = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV)
    prior = rs.randn(W.size).astype(np.float32) * 0.01
    dW = _t(prior); db = torch.zeros(cout, dtype=torch.float32, device=DEV)
    xs, ys = xd[0].numel() * 4, dyd[0].numel() * 4
    first = max(1, T - 1)          # a batch of T - 1 timesteps (stored), then the last one alone (added)
    _lib.check(lib.pivp_conv_wgrad_partial_batch(mode, xd.data_ptr() + (T - 1) * xs, cin, cin, -xs, dyd.data_ptr(), cout, cout, ys, first, 1,
                                                 part.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, Wd, _st()), 'batch 1')
    if first < T:
        _lib.check(lib.pivp_conv_wgrad_partial_batch(mode, xd.data_ptr(), cin, cin, -xs, dyd.data_ptr() + (T - 1) * ys, cout, cout, ys, 1, 0,
                                                     part.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, Wd, _st()), 'batch 2')
    _lib.check(lib.pivp_conv_wgrad_partial_reduce(mode, cin, cout, part.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, Wd, _st()), 'reduce')
    torch.cuda.synchronize()
    got = pivp.from_internal(key, dW.cpu().numpy() - prior, W.shape)
    errs = (_rel(got, tW.grad.numpy()), _rel(db.cpu().numpy(), tb.grad.numpy()))
    print('conv weight gradient in partial planes mode %d B %d %d->%d @%dx%d T %d: dW %.2e, db %.2e of max |ref|' % ((mode, B, cin, cout, H, Wd, T) + errs))
    assert errs[0] < 2e-5
    assert errs[1] < 2e-5


def convlstm_backward_dx_only(env, B, cx, C, H, Wd):
    pivp, _lib, lib = env
    rs = np.random.RandomState(C + cx + B)
    x = rs.randn(B, cx, H, Wd); h = rs.randn(B, C, H, Wd) * 0.5; c = rs.randn(B, C, H, Wd)
    W = rs.randn(4 * C, cx + C, 5, 5) / np.sqrt(25 * (cx + C)); b = rs.randn(4 * C) * 0.1
    dh = rs.randn(B, C, H, Wd); dcn = rs.randn(B, C, H, Wd)
    tx, th, tc, tW, tb = _cell_autograd(x, h, c, W, b, C, dh, dcn)
    xd, hd, cd = _nhwc(x), _nhwc(h), _nhwc(c)
    wd, bd = _t(pivp.to_internal('lstm1/conv/W', W)), _t(b)
    c_out = torch.empty_like(cd); h_out = torch.empty_like(hd)
    M = B * H * Wd
    gates = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_convlstm_train(xd.data_ptr(), cx, cx, hd.data_ptr(), C, wd.data_ptr(), bd.data_ptr(), cd.data_ptr(), c_out.data_ptr(),
                                       h_out.data_ptr(), gates.data_ptr(), B, H, Wd, _st()), 'fwd')
    dha = _nhwc(dh); dc = _nhwc(dcn).clone()
    dG = torch.empty((M, 4 * C), dtype=torch.float32, device=DEV)
    wt = torch.empty_like(wd)
    d_in = torch.full((M, cx + C), 7.0, dtype=torch.float32, device=DEV)
    dW = torch.zeros_like(wd); db = torch.zeros_like(bd)
    _lib.check(lib.pivp_convlstm_backward_dx_only(xd.data_ptr(), cx, cx, hd.data_ptr(), C, wd.data_ptr(), gates.data_ptr(), cd.data_ptr(),
                                                  c_out.data_ptr(), dha.data_ptr(), C, None, 0, dc.data_ptr(), 1, dG.data_ptr(), wt.data_ptr(),
                                                  d_in.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, Wd, _st()), 'bwd')
    torch.cuda.synchronize()
    din = d_in.cpu().numpy().reshape(B, H, Wd, cx + C).transpose(0, 3, 1, 2)
    errs = (_rel(din[:, :cx], tx.grad.numpy()), _rel(dc.cpu().numpy().reshape(B, H, Wd, C).transpose(0, 3, 1, 2), tc.grad.numpy()),
            _rel(pivp.from_internal('lstm1/conv/W', dW.cpu().numpy(), W.shape), tW.grad.numpy()), _rel(db.cpu().numpy(), tb.grad.numpy()))
    print('convlstm backward dx only B %d %d+%d @%dx%d: dx %.2e, dc %.2e, dW %.2e, db %.2e of max |ref|' % ((B, cx, C, H, Wd) + errs))
    assert errs[0] < 2e-5
    assert np.all((din[:, cx:] == 7.0) | (din[:, cx:] == 0.0))     # d h_{-1}: not computed (untouched, or cleared with the rest of d_in)
    assert np.abs(din[:, cx:] - th.grad.numpy()).max() > 1e-3
    assert errs[1] < 2e-5
    assert errs[2] < 2e-5
    assert errs[3] < 2e-5


def layernorm_plus_gate_backward_pair(env, B, C, H, Wd, lddy, recurrent):
    pivp, _lib, lib = env
    rs = np.random.RandomState(100 * C + B)
    npix, n = H * Wd, H * Wd * C
    # forward pieces in NHWC: pre-activation gates, c_{t-1}; h_t = tanh(c_t) s(o) goes through the norm, whose output meets dy
    pre = rs.randn(B, npix, 4, C); c_old = rs.randn(B, npix, C)
    gamma = 1.0 + 0.3 * rs.randn(npix, C); beta = 0.1 * rs.randn(npix, C)
    dy = rs.randn(B, npix, C); dh_b = rs.randn(B, npix, C) * 0.5; dc_in = rs.randn(B, npix, C)
    tp, tco = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (pre, c_old)]
    tg, tb = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (gamma, beta)]
    aj, ai, af, ao = torch.tanh(tp[:, :, 0]), torch.sigmoid(tp[:, :, 1]), torch.sigmoid(tp[:, :, 2] + 1.0), torch.sigmoid(tp[:, :, 3])
    cn = tco * af + ai * aj
    hn = torch.tanh(cn) * ao
    mean = hn.reshape(B, -1).mean(1)[:, None, None]; var = hn.reshape(B, -1).var(1, unbiased=False)[:, None, None]
    eps = 1e-6
    y = (hn - mean) / torch.sqrt(var + eps) * tg + tb
    loss = (y * torch.tensor(dy)).sum() + (cn * torch.tensor(dc_in)).sum()
    if recurrent:
        loss = loss + (hn * torch.tensor(dh_b)).sum()
    loss.backward()
    # HIP: stored activations j, i, f, o; stat = (mean, rstd)
    gates = _t(torch.stack((aj, ai, af, ao), 2).detach().numpy().reshape(B * npix, 4 * C))
    stat = _t(np.stack((mean.detach().numpy().reshape(B), 1.0 / np.sqrt(var.detach().numpy().reshape(B) + eps)), 1))
    dyw = torch.full((B * npix, lddy), 7.0, dtype=torch.float32, device=DEV)
    off = lddy - C                                                           # the slice sits at the end of a wider concat row
    dyw[:, off:] = _t(dy.reshape(B * npix, C))
    dc = _t(dc_in.reshape(B * npix, C)); dG = torch.empty((B * npix, 4 * C), dtype=torch.float32, device=DEV)
    dgm = torch.full((n,), 0.5, dtype=torch.float32, device=DEV); dbt = torch.full((n,), -0.25, dtype=torch.float32, device=DEV)   # accumulated into
    scratch = torch.empty(lib.pivp_gates_backward_ln_scratch_floats(B, n), dtype=torch.float32, device=DEV)
    hb = _t(dh_b.reshape(B * npix, C)) if recurrent else None
    cod, cnd, gmd, hd = _t(c_old.reshape(B * npix, C)), _t(cn.detach().numpy().reshape(B * npix, C)), _t(gamma.reshape(-1)), _t(hn.detach().numpy().reshape(B * npix, C))
    _lib.check(lib.pivp_gates_backward_ln(gates.data_ptr(), cod.data_ptr(), cnd.data_ptr(),
                                          dyw.data_ptr() + off * 4, lddy, gmd.data_ptr(), stat.data_ptr(),
                                          hd.data_ptr(), hb.data_ptr() if recurrent else None, C,
                                          dc.data_ptr(), 1, dG.data_ptr(), dgm.data_ptr(), dbt.data_ptr(), scratch.data_ptr(), B, npix, C, _st()),
               'pivp_gates_backward_ln')
    torch.cuda.synchronize()
    ref_dG = tp.grad.numpy().reshape(B * npix, 4 * C)
    errs = (_rel(dG.cpu().numpy(), ref_dG), _rel(dc.cpu().numpy(), tco.grad.numpy().reshape(B * npix, C)),
            _rel(dgm.cpu().numpy() - 0.5, tg.grad.numpy().reshape(-1)), _rel(dbt.cpu().numpy() + 0.25, tb.grad.numpy().reshape(-1)))
    print('norm + gate backward B %d C %d @%dx%d: dG %.2e, dc %.2e, dgamma %.2e, dbeta %.2e of max |ref|' % ((B, C, H, Wd) + errs))
    assert errs[0] < 2e-5
    assert errs[1] < 2e-5
    assert errs[2] < 2e-5
    assert errs[3] < 2e-5
    assert off == 0 or float(dyw[:, :off].min()) == 7.0


def lstm_wgrad_ref(x, h, dG):
    """dW[n, ci, ky, kx] = sum_{b,y,x} concat(x, h)[b, ci, y+ky-2, x+kx-2] * dG[b, n, y, x] (zero outside the image), float64 (TM:262-266 backward)."""
    xin = np.concatenate([x, h], 1) if h is not None else x
    H, W = xin.shape[2:]
    pad = np.pad(xin, ((0, 0), (0, 0), (2, 2), (2, 2)))
    dW = np.zeros((dG.shape[1], xin.shape[1], 5, 5))
    for ky in range(5):
        for kx in range(5):
            dW[:, :, ky, kx] = np.einsum('bnyx,bcyx->nc', dG, pad[:, :, ky:ky + H, kx:kx + W])
    return dW


def convlstm_weight_gradient_in_partial_slots(B, cx, C, H, Wd, Ts, form):
    import hip_ops as ops
    rs = np.random.RandomState(B * 7 + cx + C + H)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    launches = []
    ref = 0.0; dbr = 0.0
    for T in Ts:
        xs = [f32(rs.randn(B, cx, H, Wd)) for _ in range(T)]; hs = [f32(rs.randn(B, C, H, Wd) * 0.5) for _ in range(T)]
        dGs = [f32(rs.randn(B, 4 * C, H, Wd) * 0.1) for _ in range(T)]
        launches.append((xs, hs, dGs))
        ref = ref + sum(lstm_wgrad_ref(x, h, g) for x, h, g in zip(xs, hs, dGs))
        dbr = dbr + sum(g.sum(axis=(0, 2, 3)) for g in dGs)
    got, db, raw = ops.wgrad5x5_f32_batch(launches, form=form)
    unit = np.sqrt((ref ** 2).mean())
    err = np.abs(got - ref).max() / unit
    old, dbo, _ = ops.wgrad5x5_f32_batch(launches, slots=False)
    err_old = np.abs(old - ref).max() / unit
    print('lstm wgrad form %d %d+%d @%dx%d B %d launches %s: slots max |err| %.2e of the gradient rms, round-2 kernel %.2e' % (form, cx, C, H, Wd, B, Ts, err, err_old))
    assert np.isfinite(got).all() and err < 2e-5 and err <= 3.0 * err_old + 1e-7
    assert np.abs(db - dbr).max() < 2e-5 * np.abs(dbr).max() + 1e-6
    got2, db2, raw2 = ops.wgrad5x5_f32_batch(launches, form=form)
    assert np.array_equal(raw, raw2) and np.array_equal(db, db2)          # no atomics: bit-identical
    if len(Ts) == 1 and Ts[0] == 1:      # the sweep's t = 0: no h operand, only the x rows are differentiated (their own partition of the slots)
        xs, hs, dGs = launches[0]
        got0, db0, _ = ops.wgrad5x5_f32_batch(launches, h_is_zero=True, form=form)
        assert np.abs(got0[:, :cx] - ref[:, :cx]).max() < 2e-5 * unit and np.all(got0[:, cx:] == 0)
        assert np.abs(db0 - dbr).max() < 2e-5 * np.abs(dbr).max() + 1e-6
