"""Float64 restatement of the forward of the head-side ops (torch, differentiable), written from the formulas in the comments of
csrc/backward_heads.hip and from oracle/torch_restatement.py, and their gradients by autograd against a given cotangent: the reference of
tests/test_gpu_backward_heads.py.  tests/test_backward_heads_host.py checks the forwards against oracle/restatement.py and with gradcheck.

Every `ref_*` takes the fp32 arrays the kernel is handed (in the kernel's layouts) and evaluates the float64 forward FROM THOSE VALUES: a saved
activation (the ReLU'd logits, layer0 = sigmoid(.), enc7, s1, vpre, e3) is inverted to the pre-activation it stands for, so no threshold is decided
differently on the two sides.  `make_*` build the seeded inputs of a test case and `check_*` assert the conditions the comparison rests on."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
RELU_SHIFT = 1e-12
CBS_R = 12           # rows above / below a tile in the LDS window of composite_bwd_stp (csrc/backward_heads.hip)


def t64(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    return t.requires_grad_() if grad else t


def f32(a):
    return np.ascontiguousarray(np.asarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32))


def tile_rows(W):
    return 8 if W <= 64 else 4


def tiles(H, W):
    return (H + tile_rows(W) - 1) // tile_rows(W)


# ---- forwards -----------------------------------------------------------------------------------------------------------------------------
def flat_softmax(r):
    """TM:720-722: softmax over groups of NP CONSECUTIVE elements of the planar [B][NP][H][W] tensor (the reference's reshape(-1, NP))."""
    return torch.softmax(r.reshape(-1, r.shape[1]), dim=1).reshape(r.shape)


def cdna_transform(prev, kerns):
    """TM:336-349: kernel k of sample b cross-correlated (pad 2) with each colour plane of sample b.  kerns [B][NM][25] -> [B][NM][3][H][W]."""
    B, _, H, W = prev.shape
    NM = kerns.shape[1]
    t = F.conv2d(prev.permute(1, 0, 2, 3), kerns.reshape(B * NM, 1, 5, 5), padding=2, groups=B)
    return t.reshape(3, B, NM, H, W).permute(1, 2, 0, 3, 4)


def composite_cdna(prev, mk, layer0, kerns):
    """TM:725-726: prev * mk0 + layer0 * mk1 + sum_k transformed_k * mk_{k+2}; zip() drops the last generated kernel."""
    t = cdna_transform(prev, kerns)
    out = prev * mk[:, 0:1] + layer0 * mk[:, 1:2]
    for k in range(kerns.shape[1] - 1):
        out = out + t[:, k] * mk[:, k + 2:k + 3]
    return out


def stp_coords(theta, H, W):
    """F.spatial_transformer_grid + the sampler's map to pixels, BEFORE any clamp: (gu, gv) in [-1, 1] units.  theta [B][6]."""
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H, dtype=F64), torch.linspace(-1, 1, W, dtype=F64), indexing='ij')
    th = theta.reshape(-1, 6, 1, 1)
    return th[:, 0] * xs + th[:, 1] * ys + th[:, 2], th[:, 3] * xs + th[:, 4] * ys + th[:, 5]


def stp_taps(theta, H, W, zero_border):
    """-> u, v (pixel coordinates, clamped in 'clamp' mode), u0, v0 (the top-left tap as integers)."""
    gu, gv = stp_coords(theta, H, W)
    if not zero_border:
        gu, gv = gu.clamp(-1, 1), gv.clamp(-1, 1)
    u, v = (gu + 1) * (W - 1) / 2.0, (gv + 1) * (H - 1) / 2.0
    u0, v0 = torch.floor(u).detach(), torch.floor(v).detach()
    if not zero_border:
        u0, v0 = u0.clamp(0, W - 2), v0.clamp(0, H - 2)
    return u, v, u0, v0


def stp_sample(prev, theta, zero_border, window_only=False):
    """F.spatial_transformer_sampler, bilinear; 'clamp' clips the coordinates, 'zeros' samples a zero-padded frame.  window_only (the host test's
    measure of what a case can see, never the reference): the taps outside the +-CBS_R-row window of the source pixel's tile are dropped."""
    B, C, H, W = prev.shape
    u, v, u0, v0 = stp_taps(theta, H, W, zero_border)
    y0 = (torch.arange(H) // tile_rows(W) * tile_rows(W)).reshape(1, H, 1)
    wu1, wv1 = u - u0, v - v0
    bidx = torch.arange(B).reshape(B, 1, 1)
    out = 0
    for a, wv in ((0, 1 - wv1), (1, wv1)):
        for e, wu in ((0, 1 - wu1), (1, wu1)):
            uu, vv = (u0 + e).long(), (v0 + a).long()
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            if window_only:
                ok = ok & (vv >= y0 - CBS_R) & (vv < y0 + tile_rows(W) + CBS_R)
            ok = ok.to(F64)
            val = prev[bidx, :, vv.clamp(0, H - 1), uu.clamp(0, W - 1)].permute(0, 3, 1, 2)
            out = out + val * (wv * wu * ok)[:, None]
    return out


def composite_stp(prev, mk, layer0, theta, zero_border):
    """TM:465-471 + 725-726: the num_masks - 1 transforms share one theta, so masks 2.. all weigh the same warp."""
    return prev * mk[:, 0:1] + layer0 * mk[:, 1:2] + stp_sample(prev, theta, zero_border) * mk[:, 2:].sum(1, keepdim=True)


def kernel_normalise(v, dim):
    """TM:327-329 / TM:408-410: relu(v - 1e-12) + 1e-12, divided by its sum over `dim`."""
    u = torch.relu(v - RELU_SHIFT) + RELU_SHIFT
    return u / u.sum(dim, keepdim=True)


def dna_transform(prev, e7):
    """TM:392-415: 25 shifted copies of the zero-padded frame (with the reference's slice quirk, TM:400; DETACHED, TM:404) weighted by the
    normalised per-pixel kernels.  e7 [B][25][H][W] behind its ReLU."""
    B, C, H, W = prev.shape
    pad = F.pad(prev.detach(), (2, 2, 2, 2))
    kin = []
    for xk in range(5):
        for yk in range(5):
            kin.append(F.pad(pad[:, :, xk:H, yk:W], (0, yk, 0, xk)))
    kin = torch.stack(kin, 1)
    return (kin * kernel_normalise(e7, 1)[:, :, None]).sum(1)


def composite_dna(prev, mk, e7):
    return prev * mk[:, 0:1] + dna_transform(prev, e7) * mk[:, 1:2]


def cdna_kernels(v, NM):
    """v [B][NM*25] -> normalised kernels [B][NM][25]."""
    return kernel_normalise(v.reshape(v.shape[0], NM, 25), 2)


def stp_regressor(x, w1, b1, w2, b2):
    """TM:457-468: theta = W2 relu(W1 x + b1) + b2 + identity.  w1 [K][100] ([in][out]), w2 [6][100]."""
    s1 = torch.relu(x @ w1 + b1)
    return s1 @ w2.t() + b2 + torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=F64), s1


def enc3_state(e2, action, state, w3, b3, wcs, bcs, use_state):
    """TM:556-567, 503, 730.  e2 [B][HW8][64]; w3 [64 | 74][64] ([in][out]); wcs [5][10].  -> e3 [B][HW8][64], new state [B][5], pre-activation."""
    sa = torch.cat((action, state), 1)
    x = torch.cat((e2, sa[:, None, :].expand(-1, e2.shape[1], -1)), 2) if use_state else e2
    pre = x @ w3 + b3
    return torch.relu(pre), sa @ wcs.t() + bcs, pre


def enc0_weight(w):
    """[75][32] with k = (ky*5 + kx)*3 + ci  ->  (32, 3, 5, 5)."""
    return w.reshape(5, 5, 3, 32).permute(3, 2, 0, 1)


def enc0(img, w, b):
    """TM:500: 5x5 stride 2 pad 2.  img [B][3][H][W] -> NHWC [B][H/2][W/2][32]."""
    return F.conv2d(img, enc0_weight(w), b, stride=2, padding=2).permute(0, 2, 3, 1)


def heads(e6, wm, bm, we, be, B, HW):
    """1x1 heads on NHWC e6 [B*HW][64] -> planar pre-activations [B][NP][HW], [B][NE][HW]."""
    pm = (e6 @ wm + bm).reshape(B, HW, -1).permute(0, 2, 1)
    pe = (e6 @ we + be).reshape(B, HW, -1).permute(0, 2, 1)
    return pm, pe


# ---- inverses of the saved activations ----------------------------------------------------------------------------------------------------
def pre_of_relu(r):
    """A pre-activation whose ReLU is r exactly: r where positive, -1 where the unit is off."""
    r = t64(r)
    return torch.where(r > 0, r, torch.full_like(r, -1.0))


def z_of_layer0(layer0, relu):
    """The enc7 pre-activation z with sigmoid(relu(z)) == layer0 (CDNA) or sigmoid(z) == layer0 (STP), in float64."""
    l0 = t64(layer0)
    z = torch.log(l0) - torch.log1p(-l0)
    return torch.where(l0 > 0.5, z, torch.full_like(z, -1.0)) if relu else z


def _np(t):
    return None if t is None else t.detach().numpy()


# ---- gradients ------------------------------------------------------------------------------------------------------------------------------
def ref_composite(model, prev, logits, layer0, aux, go, H, W, stp_zero=0):
    """Gradients of sum(out * go).  -> dict(dmk, dz, daux (kernels [B][NM-1][25] | theta [B][6] | None), dprev), all planar."""
    B = prev.shape[0]
    leaf = (lambda a: a.detach().requires_grad_())
    pv = t64(prev, True).reshape(B, 3, H, W)
    pv.retain_grad()
    mk = leaf(flat_softmax(t64(logits).reshape(B, -1, H, W)))
    g = t64(go).reshape(B, 3, H, W)
    if model == 'cdna':
        z = leaf(z_of_layer0(layer0, True).reshape(B, 3, H, W)); k = t64(aux, True)
        out = composite_cdna(pv, mk, torch.sigmoid(torch.relu(z)), k)
    elif model == 'stp':
        z = leaf(z_of_layer0(layer0, False).reshape(B, 3, H, W)); k = t64(aux, True)
        out = composite_stp(pv, mk, torch.sigmoid(z), k, stp_zero)
    else:
        z = leaf(pre_of_relu(aux).reshape(B, 25, H, W)); k = None
        out = composite_dna(pv, mk, torch.relu(z))
    (out * g).sum().backward()
    daux = None if k is None else (k.grad[:, :-1] if model == 'cdna' else k.grad)
    return dict(dmk=_np(mk.grad.reshape(B, -1, H * W)), dz=_np(z.grad.reshape(B, -1, H * W)), daux=_np(daux), dprev=_np(pv.grad.reshape(B, 3, H * W)))


def ref_mask_softmax(logits, dmk):
    pre = pre_of_relu(logits).requires_grad_()
    B, NP = logits.shape[:2]
    mk = flat_softmax(torch.relu(pre).reshape(B, NP, 1, -1))
    (mk * t64(dmk).reshape(mk.shape)).sum().backward()
    return _np(pre.grad)


def ref_heads(e6, wm, we, dpm, dpe, B, HW):
    e6, wm, we = t64(e6, True), t64(wm, True), t64(we, True)
    bm, be = torch.zeros(wm.shape[1], dtype=F64, requires_grad=True), torch.zeros(we.shape[1], dtype=F64, requires_grad=True)
    pm, pe = heads(e6, wm, bm, we, be, B, HW)
    ((pm * t64(dpm)).sum() + (pe * t64(dpe)).sum()).backward()
    return dict(de6=_np(e6.grad), dwm=_np(wm.grad), dbm=_np(bm.grad), dwe=_np(we.grad), dbe=_np(be.grad))


def _linear_stage(x, wt, dv):
    """Gradients of sum((x wt + b) * dv) for a given dv: dx, dwt, db."""
    x, wt = t64(x, True), t64(wt, True)
    b = torch.zeros(wt.shape[1], dtype=F64, requires_grad=True)
    ((x @ wt + b) * dv).sum().backward()
    return _np(x.grad), _np(wt.grad), _np(b.grad)


def ref_cdna_kernels(hidden5, wt, vpre, dkpart, NM):
    """dkpart [B][ntiles][256]: summed over the tiles; the last kernel and the padding columns get no gradient."""
    B = vpre.shape[0]
    v = t64(vpre[:, :NM * 25], True)
    dk = t64(dkpart).sum(1)[:, :(NM - 1) * 25].reshape(B, NM - 1, 25)
    (cdna_kernels(v, NM)[:, :NM - 1] * dk).sum().backward()
    dv = torch.zeros(B, 256, dtype=F64); dv[:, :NM * 25] = v.grad
    dx, dwt, db = _linear_stage(hidden5, wt, dv)
    return dict(dv=_np(dv), dx=dx, dwt=dwt, db=db[:NM * 25])


def ref_stp_params(hidden5, wt1, s1, w2, dthpart):
    B = s1.shape[0]
    pre = pre_of_relu(s1[:, :100]).requires_grad_()
    w2t = t64(w2, True); b2 = torch.zeros(6, dtype=F64, requires_grad=True)
    dth = t64(dthpart).sum(1)[:, :6]
    ((torch.relu(pre) @ w2t.t() + b2) * dth).sum().backward()
    dv = torch.zeros(B, 256, dtype=F64); dv[:, :100] = pre.grad
    dx, dwt, db = _linear_stage(hidden5, wt1, dv)
    return dict(dv=_np(dv), dx=dx, dwt1=dwt, db1=db[:100], dw2=_np(w2t.grad), db2=_np(b2.grad))


def ref_enc3_state(e2, action, state, w3, b3, wcs, de3, dsnew, use_state, mask_e2):
    """e2 [B][HW8][64] behind enc2's ReLU; de3 [B][HW8][64].  mask_e2: the gradient in front of that ReLU."""
    x2 = pre_of_relu(e2).requires_grad_() if mask_e2 else t64(e2, True)
    st, w3t, b3t, wcst = t64(state, True), t64(w3, True), t64(b3, True), t64(wcs, True)
    bcs = torch.zeros(5, dtype=F64, requires_grad=True)
    e3, snew, _ = enc3_state(torch.relu(x2) if mask_e2 else x2, t64(action), st, w3t, b3t, wcst, bcs, use_state)
    ((e3 * t64(de3)).sum() + (snew * t64(dsnew)).sum()).backward()
    return dict(de2=_np(x2.grad), dw3=_np(w3t.grad), db3=_np(b3t.grad), dwcs=_np(wcst.grad), dbcs=_np(bcs.grad), dstate=_np(st.grad))


def ref_enc0(img, w, d, B, H, W):
    im, wt = t64(img, True), t64(w, True)
    b = torch.zeros(32, dtype=F64, requires_grad=True)
    (enc0(im.reshape(B, 3, H, W), wt, b) * t64(d).reshape(B, H // 2, W // 2, 32)).sum().backward()
    return dict(dimg=_np(im.grad), dw=_np(wt.grad), db=_np(b.grad))


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------------
def _rs(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def make_logits(rs, B, NP, HW):
    """relu(2 randn): about half of the units are exact zeros."""
    return f32(np.maximum(2.0 * rs.randn(B, NP, HW), 0.0))


def rotation_theta(deg, tx, ty):
    a = np.deg2rad(deg)
    return [np.cos(a), -np.sin(a), tx, np.sin(a), np.cos(a), ty]


def make_theta(rs, B, H, far):
    """far = 0, near: the identity plus a 0.05 perturbation (never the exact identity: its coordinates are integers).  far = 1: a rotation of about
    80 degrees and a vertical shift well over CBS_R rows.  far = 2, flip: the rows mirrored and stretched twofold, so a pixel's target row runs
    against its own (the only way past one half outside the window on a frame hardly taller than the window, see STP_FRAMES).  Both with a 0.02
    perturbation."""
    if not far:
        return f32(np.array([1.0, 0, 0, 0, 1.0, 0]) + 0.05 * rs.randn(B, 6))
    if far == 2:
        return f32(np.array([0.9, 0.3, 0.05, 0.2, -2.0, 0.1]) + 0.02 * rs.randn(B, 6))
    shift = max(2.0 * (CBS_R + 4) / (H - 1), 1.5 if H <= 32 else 0.0)           # rows -> [-1, 1] units (16 rows; 23 on the 32-row frame)
    base = np.array([rotation_theta(80.0 if b % 2 == 0 else -80.0, 0.1, -shift if b % 2 == 0 else shift) for b in range(B)])
    return f32(base + 0.02 * rs.randn(B, 6))


def make_composite(model, H, W, NM, B, far=0):
    """-> dict(prev, logits, layer0, aux, go) in the kernel's layouts, fp32; the saved activations are the float64 forward rounded to fp32."""
    rs = _rs({'cdna': 0, 'stp': 1, 'dna': 2}[model], H, W, NM, B, int(far))
    HW = H * W
    d = dict(prev=f32(rs.rand(B, 3, HW)), logits=make_logits(rs, B, NM + 1, HW), go=f32(rs.randn(B, 3, HW)), layer0=None)
    if model == 'dna':
        d['aux'] = f32(np.maximum(rs.randn(B, 25, HW), 0.0))
        return d
    z = t64(1.5 * rs.randn(B, 3, HW))
    d['layer0'] = f32(torch.sigmoid(torch.relu(z) if model == 'cdna' else z))
    if model == 'cdna':
        d['aux'] = f32(cdna_kernels(t64(rs.randn(B, NM * 25)), NM))
    else:
        d['aux'] = make_theta(rs, B, H, far)
    return d


def check_composite(model, d, H, W, stp_zero=0):
    """The conditions the comparison rests on (asserted on the host for every case)."""
    if model == 'dna':
        e7 = d['aux']
        assert not ((e7 > 0) & (e7 < 1e-6)).any()
        return
    z = z_of_layer0(d['layer0'], model == 'cdna').numpy()
    if model == 'cdna':
        on = d['layer0'] > 0.5
        assert on.any() and (~on).any() and np.all(d['layer0'][~on] == 0.5) and z[on].min() > 1e-6
        return
    gu, gv = [c.numpy() for c in stp_coords(t64(d['aux']), H, W)]
    for g, n in ((gu, W), (gv, H)):
        assert np.abs(np.abs(g) - 1.0).min() > 1e-9                         # no coordinate on a clamp bound
        p = (g + 1) * (n - 1) / 2.0
        live = np.ones_like(p, dtype=bool) if stp_zero else (np.abs(g) < 1.0)   # (clamped coordinates sit on the border pixel by construction)
        assert np.abs(p[live] - np.round(p[live])).min() > 1e-9           # ... nor on a pixel centre, where floor() jumps


def stp_outside_fraction(theta, H, W, stp_zero):
    """Of the bilinear taps that land inside the frame, the fraction outside the +-CBS_R-row LDS window of the source pixel's tile."""
    _, _, u0, v0 = [c.numpy() for c in stp_taps(t64(theta), H, W, stp_zero)]
    tr = tile_rows(W)
    y0 = (np.arange(H) // tr * tr).reshape(1, H, 1)
    inside = outside = 0
    for a in (0, 1):
        for e in (0, 1):
            uu, vv = u0 + e, v0 + a
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            inwin = (vv >= y0 - CBS_R) & (vv < y0 + tr + CBS_R)
            inside += (ok & inwin).sum(); outside += (ok & ~inwin).sum()
    return outside / float(inside + outside)


STP_WHOLE_LDS = 96 * 1024   # composite_bwd_stp: the whole-frame window is taken while it fits in this much LDS with the softmax staging


def stp_plain_whole(H, W, NM):
    """The launcher's choice (composite_bwd_stp in csrc/backward_heads.hip) for a plain launch with d prev: True, the block keeps the whole frame's
    d prev in LDS; False, the tile's rows +-CBS_R, with global atomics for what lands outside.  A deterministic launch (det_acc) is always windowed."""
    NP, npix = NM + 1, tile_rows(W) * W
    win, G = npix + 2 * (NP - 1), npix // NP + 2
    lds_head = 4 * (NP * win + 2 * NP * G)
    return lds_head + 4 * 3 * H * W <= STP_WHOLE_LDS


def make_mask_softmax(NP, B, HW):
    rs = _rs(10, NP, B, HW)
    return dict(logits=make_logits(rs, B, NP, HW), dmk=f32(rs.randn(B, NP, HW)))


def make_heads(NP, NE, B, HW):
    rs = _rs(11, NP, NE, B, HW)
    return dict(e6=f32(np.maximum(rs.randn(B * HW, 64), 0.0)), wm=f32(rs.randn(64, NP) / 8.0), we=f32(rs.randn(64, NE) / 8.0),
                dpm=f32(rs.randn(B, NP, HW)), dpe=f32(rs.randn(B, NE, HW)),
                prior=[f32(rs.randn(64, NP)), f32(rs.randn(NP)), f32(rs.randn(64, NE)), f32(rs.randn(NE))])


def make_cdna_kernels(K, NM, B, ntiles):
    """vpre is the float64 Linear rounded to fp32; dkpart's slots of the unused last kernel and of the padding hold large values that must not be read."""
    rs = _rs(12, K, NM, B, ntiles)
    x = f32(rs.randn(B, K)); wt = f32(rs.randn(K, 256) / np.sqrt(K)); b = f32(0.1 * rs.randn(256))
    vpre = f32(t64(x) @ t64(wt) + t64(b))
    dkpart = f32(rs.randn(B, ntiles, 256)); dkpart[:, :, (NM - 1) * 25:] = 1.0e6
    return dict(hidden5=x, wt=wt, vpre=vpre, dkpart=dkpart, prior_dx=f32(rs.randn(B, K) / np.sqrt(K)), prior_dwt=f32(rs.randn(K, 256)), prior_db=f32(rs.randn(256)))


def check_preact(v):
    """No pre-activation within 1e-6 of its threshold, exact ReLU zeros aside; both sides of the threshold occur."""
    v = np.asarray(v, dtype=np.float64)
    assert (v > 0).any() and (v <= 0).any() and not ((v != 0) & (np.abs(v) < 1e-6)).any()


def make_stp_params(K, B, ntiles):
    rs = _rs(13, K, B, ntiles)
    x = f32(rs.randn(B, K)); wt1 = f32(rs.randn(K, 256) / np.sqrt(K)); b1 = f32(0.1 * rs.randn(256))
    s1 = f32(torch.relu(t64(x) @ t64(wt1) + t64(b1))); s1[:, 100:] = 0.0
    dthpart = f32(rs.randn(B, ntiles, 8)); dthpart[:, :, 6:] = 1.0e6
    return dict(hidden5=x, wt1=wt1, s1=s1, w2=f32(rs.randn(6, 100) / 10.0), dthpart=dthpart, prior_dwt1=f32(rs.randn(K, 256)),
                prior=[f32(rs.randn(100)), f32(rs.randn(6, 100)), f32(rs.randn(6))])


def make_enc3(HW8, use_state, B):
    rs = _rs(14, HW8, use_state, B)
    cin = 74 if use_state else 64
    d = dict(e2=f32(np.maximum(rs.randn(B, HW8, 64), 0.0)), action=f32(rs.randn(B, 5)), state=f32(rs.randn(B, 5)),
             w3=f32(rs.randn(cin, 64) / np.sqrt(cin)), b3=f32(0.1 * rs.randn(64)), wcs=f32(rs.randn(5, 10) / 3.0),
             de3=f32(rs.randn(B, HW8, 64)), dsnew=f32(rs.randn(B, 5)))
    e3, _, pre = enc3_state(t64(d['e2']), t64(d['action']), t64(d['state']), t64(d['w3']), t64(d['b3']), t64(d['wcs']), torch.zeros(5, dtype=F64), use_state)
    d['e3'], d['pre'] = f32(e3), pre.numpy()
    d['prior'] = [f32(rs.randn(cin, 64)), f32(rs.randn(64)), f32(rs.randn(5, 10)), f32(rs.randn(5)), f32(rs.randn(B, 5))]
    return d


def make_enc0(B, H, W):
    rs = _rs(15, B, H, W)
    return dict(img=f32(rs.rand(B, 3, H * W)), w=f32(rs.randn(75, 32) / np.sqrt(75.0)), d=f32(rs.randn(B * (H // 2) * (W // 2), 32)),
                prior=[f32(rs.randn(75, 32)), f32(rs.randn(32)), f32(rs.randn(B, 3, H * W))])


# ---- the cases of tests/test_gpu_backward_heads.py (the host test asserts the input conditions on every one) ---------------------------------
CDNA_CASES = [(64, 64, 10, 2), (16, 16, 10, 3), (24, 40, 4, 2), (72, 40, 2, 2), (16, 128, 10, 2), (32, 128, 3, 1)]      # H, W, NM, B
# H, W, theta (0 near, 1 far, 2 flip).  Which scatter of d prev a plain launch runs is the launcher's choice (stp_plain_whole below): (64, 64),
# (8, 64) and (32, 128) whole-frame for every NM, (96, 64) windowed at NM = 10 only, (64, 128) windowed for every NM -- the one frame on which the
# 4-row instance (W > 64) runs the float window with global atomics outside it.  A deterministic launch is windowed on every frame.
# STP_FAR_OUTSIDE: (H, W, theta, stp_zero_border) -> the fraction of the in-frame taps that must land outside the tile's window.  More than half on
# (96, 64) and (64, 128) with the far theta in both border modes.  On the 32-row frame (windowed in deterministic launches only) the window spans 28
# rows; a rotation by 80 degrees sends a pixel to a row that hardly depends on its own, and with every tap in the frame ('clamp') at most half of the
# (tile, target row) pairs then lie outside whatever the shift is: the far theta passes one half with the zero border only, and the flip is added for
# 'clamp'.
STP_FRAMES = [(64, 64, 0), (8, 64, 0), (96, 64, 0), (96, 64, 1), (32, 128, 0), (32, 128, 1), (32, 128, 2), (64, 128, 0), (64, 128, 1)]
STP_FAR_OUTSIDE = {(96, 64, 1, 0): 0.5, (96, 64, 1, 1): 0.5, (64, 128, 1, 0): 0.5, (64, 128, 1, 1): 0.5,
                   (32, 128, 1, 1): 0.5, (32, 128, 2, 0): 0.5, (32, 128, 1, 0): 0.4, (32, 128, 2, 1): 0.4}
# (H, W) -> the mask counts at which a plain launch with d prev keeps the whole frame in LDS (the others run the +-CBS_R-row window)
STP_PLAIN_WHOLE = {(64, 64): (10, 3, 2), (8, 64): (10, 3, 2), (96, 64): (3, 2), (32, 128): (10, 3, 2), (64, 128): ()}
STP_CASES = [(H, W, NM, zb, far) for (H, W, far) in STP_FRAMES for NM in (10, 3, 2) for zb in (0, 1)]
STP_B = 2
DNA_CASES = [(64, 64, 2), (24, 40, 3), (16, 128, 2), (64, 64, 3), (24, 40, 2), (16, 128, 3)]                               # H, W, B
SOFTMAX_CASES = [(2, 3, 384), (4, 3, 384), (11, 3, 384), (12, 3, 384), (11, 2, 4096)]                                     # NP, B, HW
HEADS_CASES = [(NP, NE, B, HW) for (NP, NE) in ((11, 3), (2, 25), (4, 3), (7, 25)) for (B, HW) in ((3, 384), (2, 4096))]
GEN_CASES = [(K, NM, B, nt) for K in (512, 8192) for NM in (10, 2) for B in (1, 3, 33) for nt in (2, 8)]
STPP_CASES = [(K, B, nt) for K in (512, 8192) for B in (3, 33) for nt in (2, 8)]
ENC3_CASES = [(HW8, us, B) for HW8 in (4, 6, 64, 108) for us in (0, 1) for B in (1, 3)]
ENC0_CASES = [(2, 64, 64), (3, 16, 24), (2, 24, 40), (33, 64, 64)]                                                         # B, H, W
