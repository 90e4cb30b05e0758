"""NumPy-in / NumPy-out wrappers around the head-side backward entry points (pivp_composite_backward, pivp_mask_softmax_backward,
pivp_heads_backward, pivp_cdna_kernels_backward, pivp_stp_params_backward, pivp_enc3_state_backward, pivp_enc0_backward), for
tests/test_gpu_backward_heads.py.  Overwritten outputs start as NaN (a missing write shows), accumulated ones from the given prior."""
import numpy as np
import torch

from pivp_amd import _lib

DEV = 'cuda:0'
MODEL = {'cdna': _lib.MODEL_CDNA, 'stp': _lib.MODEL_STP, 'dna': _lib.MODEL_DNA}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def host(t):
    return None if t is None else t.cpu().numpy()


def _st():
    return torch.cuda.current_stream().cuda_stream


def composite_backward(model, d, H, W, NM, dprev_prior=None, dprev_accum=0, want_dprev=True, stp_zero=0, det=False, go_scale=1.0):
    """-> (rc, dict(dmk, dz, part, dprev, acc)).  dprev_prior: the buffer's contents before the call (None: NaN).  det: with the fixed-point accumulator
    (zeroed before, returned after)."""
    lib = _lib.load()
    B, HW, T = d['prev'].shape[0], H * W, max(lib.pivp_composite_backward_tiles(H, W), 1)
    prev, logits, aux = dev(d['prev']), dev(d['logits']), dev(d['aux'])
    go = dev(d['go'] * np.float32(go_scale))
    layer0 = None if d['layer0'] is None else dev(d['layer0'])
    dmk, dz = nan(B, NM + 1, HW), nan(B, 25 if model == 'dna' else 3, HW)
    part = None if model == 'dna' else nan(B, T, 256 if model == 'cdna' else 8)
    dprev = None
    if want_dprev:
        dprev = nan(B, 3, HW) if dprev_prior is None else dev(dprev_prior)
    acc = torch.zeros(B * 3 * HW, dtype=torch.int64, device=DEV) if det else None
    rc = lib.pivp_composite_backward(MODEL[model], ptr(prev), ptr(logits), ptr(layer0), ptr(aux), ptr(go), ptr(dmk), ptr(dz), ptr(part), ptr(dprev),
                                     dprev_accum, B, H, W, NM, stp_zero, ptr(acc), _st())
    torch.cuda.synchronize()
    return rc, dict(dmk=host(dmk), dz=host(dz), part=host(part), dprev=host(dprev), acc=host(acc))


def mask_softmax_backward(logits, dmk):
    lib = _lib.load()
    B, NP, HW = logits.shape
    lg, dm = dev(logits), dev(dmk)
    rc = lib.pivp_mask_softmax_backward(ptr(lg), ptr(dm), B, HW, NP, _st())
    torch.cuda.synchronize()
    return rc, host(dm)


def heads_backward(d, B, HW, det=False):
    lib = _lib.load()
    NP, NE = d['wm'].shape[1], d['we'].shape[1]
    e6, wm, we, dpm, dpe = [dev(d[k]) for k in ('e6', 'wm', 'we', 'dpm', 'dpe')]
    de6 = nan(B * HW, 64)
    dwm, dbm, dwe, dbe = [dev(p) for p in d['prior']]
    part = nan(max(lib.pivp_heads_backward_det_floats(B, HW, NP, NE), 1)) if det else None
    rc = lib.pivp_heads_backward(ptr(e6), ptr(wm), ptr(we), ptr(dpm), ptr(dpe), ptr(de6), ptr(dwm), ptr(dbm), ptr(dwe), ptr(dbe), B, HW, NP, NE,
                                 ptr(part), _st())
    torch.cuda.synchronize()
    return rc, dict(de6=host(de6), dwm=host(dwm), dbm=host(dbm), dwe=host(dwe), dbe=host(dbe))


def cdna_kernels_backward(d, NM, accum_dx, det=False):
    lib = _lib.load()
    B, K = d['hidden5'].shape
    ntiles = d['dkpart'].shape[1]
    x, wt, vpre, dk = [dev(d[k]) for k in ('hidden5', 'wt', 'vpre', 'dkpart')]
    dv = nan(B, 256)
    dx = dev(d['prior_dx']) if accum_dx else nan(B, K)
    dwt, db = dev(d['prior_dwt']), dev(d['prior_db'])
    part = nan(B * 256) if det else None
    rc = lib.pivp_cdna_kernels_backward(ptr(x), ptr(wt), ptr(vpre), ptr(dk), ntiles, ptr(dv), ptr(dx), accum_dx, ptr(dwt), ptr(db), B, K, NM,
                                        ptr(part), _st())
    torch.cuda.synchronize()
    return rc, dict(dv=host(dv), dx=host(dx), dwt=host(dwt), db=host(db))


def stp_params_backward(d, det=False):
    lib = _lib.load()
    B, K = d['hidden5'].shape
    ntiles = d['dthpart'].shape[1]
    x, wt1, s1, w2, dth = [dev(d[k]) for k in ('hidden5', 'wt1', 's1', 'w2', 'dthpart')]
    dv, dx = nan(B, 256), nan(B, K)
    dwt1 = dev(d['prior_dwt1'])
    db1, dw2, db2 = [dev(p) for p in d['prior']]
    part = nan(B * 706) if det else None
    rc = lib.pivp_stp_params_backward(ptr(x), ptr(wt1), ptr(s1), ptr(w2), ptr(dth), ntiles, ptr(dv), ptr(dx), ptr(dwt1), ptr(db1), ptr(dw2), ptr(db2),
                                      B, K, ptr(part), _st())
    torch.cuda.synchronize()
    return rc, dict(dv=host(dv), dx=host(dx), dwt1=host(dwt1), db1=host(db1), dw2=host(dw2), db2=host(db2))


def enc3_state_backward(d, use_state, mask_e2, ldd3, det=False):
    """de3 is handed over as the first 64 columns of rows of ldd3 floats (the other columns NaN: never read)."""
    lib = _lib.load()
    B, HW8 = d['e2'].shape[:2]
    e2, e3, action, state, w3, wcs, dsnew = [dev(d[k]) for k in ('e2', 'e3', 'action', 'state', 'w3', 'wcs', 'dsnew')]
    de3 = nan(B * HW8, ldd3)
    de3[:, :64] = dev(d['de3']).reshape(B * HW8, 64)
    de2 = nan(B, HW8, 64)
    dw3, db3, dwcs, dbcs, dstate = [dev(p) for p in d['prior']]
    part = nan(max(lib.pivp_enc3_state_backward_det_floats(B, HW8, use_state), 1)) if det else None
    rc = lib.pivp_enc3_state_backward(ptr(e2), ptr(e3), ptr(de3), ldd3, ptr(action), ptr(state), ptr(w3), ptr(wcs), ptr(dsnew), ptr(de2), ptr(dw3),
                                      ptr(db3), ptr(dwcs), ptr(dbcs), ptr(dstate), B, HW8, use_state, mask_e2, ptr(part), _st())
    torch.cuda.synchronize()
    return rc, dict(de2=host(de2), dw3=host(dw3), db3=host(db3), dwcs=host(dwcs), dbcs=host(dbcs), dstate=host(dstate))


def enc0_backward(d, B, H, W, dimg_mode, det=False):
    """dimg_mode: None (null), 0 (overwrite NaN), 1 (accumulate onto the prior)."""
    lib = _lib.load()
    img, w, dd = dev(d['img']), dev(d['w']), dev(d['d'])
    dw, db = dev(d['prior'][0]), dev(d['prior'][1])
    dimg = None if dimg_mode is None else (dev(d['prior'][2]) if dimg_mode else nan(B, 3, H * W))
    part = nan(max(lib.pivp_enc0_backward_det_floats(B, H, W), 1)) if det else None
    rc = lib.pivp_enc0_backward(ptr(img), ptr(w), ptr(dd), ptr(dw), ptr(db), ptr(dimg), int(bool(dimg_mode)), B, H, W, ptr(part), _st())
    torch.cuda.synchronize()
    return rc, dict(dw=host(dw), db=host(db), dimg=host(dimg))
