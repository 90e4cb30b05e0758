"""NumPy-in / NumPy-out wrappers for tests/test_gpu_conv_forms.py: the plain convolutions with the strides a plan passes, and the op entries of
include/pivp_conv_forms.h.  By the method of hip_ops.conv5x5_ep: an input is the LAST channels of an ld-wide NaN-filled device buffer (a channel slice
of a concat), an output a channel slice of an ldo-wide buffer prefilled with 7.0 whose other columns are returned beside the result."""
import ctypes

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib
from hip_ops import DEV, _t, nhwc, nchw, stream

pytestmark = pytest.mark.gpu

PREFILL = 7.0


def conv_form(op, cin, cout, B, H, W, aligned=True):
    return _lib.load().pivp_conv_form(int(op == 'deconv'), cin, cout, B, H, W, int(aligned))


def enc0_form(B, H, W):
    return _lib.load().pivp_conv_enc0_form(B, H, W)


def _in_slice(x, ld):
    """x NCHW as the last channels of an ld-wide NaN-filled NHWC buffer -> (buffer, pointer to the slice)"""
    B, c, H, W = x.shape
    ld = c if ld is None else ld
    buf = torch.full((B, H, W, ld), float('nan'), dtype=torch.float32, device=DEV)
    buf[..., ld - c:] = nhwc(x)
    return buf, buf.data_ptr() + (ld - c) * 4, ld


def _out_slice(B, H, W, c, ldo, ooff):
    ldo = c if ldo is None else ldo
    assert ooff + c <= ldo and ooff % 4 == 0
    buf = torch.full((B, H, W, ldo), PREFILL, dtype=torch.float32, device=DEV)
    return buf, buf.data_ptr() + ooff * 4, ldo


def _split(buf, c, ooff):
    """-> (the slice as NCHW, every other column [B, H, W, ldo - c])"""
    full = buf.cpu().numpy()
    return np.ascontiguousarray(full[..., ooff:ooff + c].transpose(0, 3, 1, 2)), np.concatenate((full[..., :ooff], full[..., ooff + c:]), axis=-1)


def _bias(b, off=0):
    """the bias `off` floats past a 16-byte boundary -> (buffer, pointer)"""
    buf = torch.zeros(len(b) + 4, dtype=torch.float32, device=DEV)
    buf[off:off + len(b)] = _t(b)
    return buf, buf.data_ptr() + off * 4


def _perm(v, C, HW):            # gamma / beta of a LayerNormalizationConv2D, (C, H, W)-flat -> [HW][C]
    return _t(np.asarray(v).reshape(C, HW).T)


def conv(op, x, W, b, relu, ld=None, ldo=None, ooff=0, bias_off=0):
    """pivp_conv3x3s2 (op 'conv', W (cout, cin, 3, 3)) / pivp_deconv3x3s2 ('deconv', W (cin, cout, 3, 3)) -> (out NCHW, the columns outside the slice)"""
    lib = _lib.load()
    B, cin, H, Wd = x.shape
    up = op == 'deconv'
    cout = W.shape[1] if up else W.shape[0]
    Ho, Wo = (2 * H, 2 * Wd) if up else (H // 2, Wd // 2)
    xbuf, xptr, ld = _in_slice(x, ld)
    wd = _t(pivp_amd.to_internal('enc4/W' if up else 'enc1/W', W))
    bbuf, bptr = _bias(b, bias_off)
    obuf, optr, ldo = _out_slice(B, Ho, Wo, cout, ldo, ooff)
    fn = lib.pivp_deconv3x3s2 if up else lib.pivp_conv3x3s2
    _lib.check(fn(xptr, cin, ld, wd.data_ptr(), bptr, optr, cout, ldo, int(relu), B, H, Wd, stream()), op)
    torch.cuda.synchronize()
    return _split(obuf, cout, ooff)


def layernorm(x, gamma, beta, eps, relu, ldo=None, ooff=0):
    """pivp_layernorm into a channel slice -> (out NCHW float32, the columns outside the slice)"""
    lib = _lib.load()
    B, C, H, Wd = x.shape
    n = C * H * Wd
    xd = nhwc(x)
    gd, bd = _perm(gamma, C, H * Wd), _perm(beta, C, H * Wd)
    obuf, optr, ldo = _out_slice(B, H, Wd, C, ldo, ooff)
    scratch = torch.empty(lib.pivp_layernorm_scratch_floats(B, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.pivp_layernorm(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), optr, scratch.data_ptr(), B, n, C, ldo, eps, int(relu), stream()), 'layernorm')
    torch.cuda.synchronize()
    return _split(obuf, C, ooff)


def conv3x3s2_ln_refused(cin, cout, B, H, Wd, ep=False, keep_ld=None):
    """pivp_conv3x3s2_ln on arguments it must refuse, every buffer large enough for the launch it must not make.  -> (rc, is the output still its prefill)"""
    lib = _lib.load()
    new = lambda n, v=0.5: torch.full((max(int(n), 64),), v, dtype=torch.float32, device=DEV)
    x, g, be = new(B * H * Wd * cin), new(H * Wd * cin), new(H * Wd * cin)
    w, b = new(9 * (cin + 32) * (cout + 32)), new(cout + 32)
    out = new(B * (H // 2 + 1) * (Wd // 2 + 1) * cout, PREFILL)
    scratch = new(B * (H * Wd * cin // 4096 + 2) * 4)
    keep = None if keep_ld is None else new(B * H * Wd * max(keep_ld, cin), PREFILL)
    e, hold = None, []
    if ep:
        e = _lib.PivpEnc3Epilogue()
        hold = [new(74 * 64), new(64), new(B * 5), new(B * 5), new(50), new(5), new(B * (H // 2 + 1) * (Wd // 2 + 1) * 64, PREFILL), new(B * 5, PREFILL)]
        e.w3, e.b3, e.action, e.state, e.wcs, e.bcs, e.e3_out, e.state_out = [t.data_ptr() for t in hold]
        e.use_state = 1
    rc = lib.pivp_conv3x3s2_ln(x.data_ptr(), cin, w.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), 1e-6, scratch.data_ptr(), out.data_ptr(), cout, cout, 1,
                               None if keep is None else keep.data_ptr(), 0 if keep_ld is None else keep_ld, None,
                               None if e is None else ctypes.byref(e), B, H, Wd, stream())
    torch.cuda.synchronize()
    untouched = bool((out == PREFILL).all()) and (keep is None or bool((keep == PREFILL).all())) and (not hold or bool((hold[6] == PREFILL).all()))
    return rc, untouched


def conv3x3s2_ln(x, gamma, beta, W, b, relu, eps=1e-6, keep_ld=None, ep=None, ldo=None, ooff=0):
    """pivp_conv3x3s2_ln.  keep_ld: ask for the write-back of the normalised input (pixel stride keep_ld) and the samples' (mean, rstd).
    ep: dict(action, state, W3, b3, Wcs, bcs, use_state) for the fused enc3 + state predictor.  -> dict(rc, out, guard[, keep, keep_guard, stat][, e3, state])"""
    lib = _lib.load()
    B, cin, H, Wd = x.shape
    cout = W.shape[0]
    Ho, Wo = H // 2, Wd // 2
    n = cin * H * Wd
    xd = nhwc(x)
    gd, bed = _perm(gamma, cin, H * Wd), _perm(beta, cin, H * Wd)
    wd = _t(pivp_amd.to_internal('enc1/W', W))
    bbuf, bptr = _bias(b)
    obuf, optr, ldo = _out_slice(B, Ho, Wo, cout, ldo, ooff)
    scratch = torch.empty(max(lib.pivp_layernorm_scratch_floats(B, max(n, 4)), 4), dtype=torch.float32, device=DEV)
    kbuf = kptr = sbuf = None
    if keep_ld is not None:
        kbuf = torch.full((B, H, Wd, max(keep_ld, 1)), PREFILL, dtype=torch.float32, device=DEV)
        sbuf = torch.full((B, 2), PREFILL, dtype=torch.float32, device=DEV)
        kptr = kbuf.data_ptr()
    e = None
    hold = []
    if ep is not None:
        e = _lib.PivpEnc3Epilogue()
        hold = [_t(pivp_amd.to_internal('enc3/W', ep['W3'])), _t(ep['b3']), _t(ep['action']), _t(ep['state']), _t(ep['Wcs']), _t(ep['bcs']),
                torch.full((B, Ho, Wo, 64), PREFILL, dtype=torch.float32, device=DEV), torch.full((B, 5), PREFILL, dtype=torch.float32, device=DEV)]
        e.w3, e.b3, e.action, e.state, e.wcs, e.bcs, e.e3_out, e.state_out = [t.data_ptr() for t in hold]
        e.use_state = int(ep['use_state'])
    rc = lib.pivp_conv3x3s2_ln(xd.data_ptr(), cin, wd.data_ptr(), bptr, gd.data_ptr(), bed.data_ptr(), eps, scratch.data_ptr(), optr, cout, ldo, int(relu),
                               kptr, 0 if keep_ld is None else keep_ld, None if sbuf is None else sbuf.data_ptr(),
                               None if e is None else ctypes.byref(e), B, H, Wd, stream())
    _lib.check(rc, 'conv3x3s2_ln')
    torch.cuda.synchronize()
    res = dict(rc=rc)
    res['out'], res['guard'] = _split(obuf, cout, ooff)
    if kbuf is not None:
        res['keep'], res['keep_guard'] = _split(kbuf, min(cin, kbuf.shape[-1]), 0)
        res['stat'] = sbuf.cpu().numpy()
    if e is not None:
        res['e3'] = nchw(hold[6], B, Ho, Wo, 64)
        res['state'] = hold[7].cpu().numpy()
    return res


KIND = {'enc0': 0, 'conv': 1, 'deconv': 2}      # PIVP_CONV_KIND_*


def conv_layernorm(kind, x, W, b, relu, gamma, beta, eps, relu_ln, ldo=None, ooff=0):
    """pivp_conv_layernorm: the producer with its LayerNorm partials requested, then the norm from them.  x NCHW (enc0: the frames), W in the reference's layout.
    -> (raw NCHW, norm NCHW, partials per sample the producer reported, the norm's columns outside its slice)"""
    lib = _lib.load()
    B, cin, H, Wd = x.shape
    up = kind == 'deconv'
    cout = W.shape[1] if up else W.shape[0]
    Ho, Wo = (2 * H, 2 * Wd) if up else (H // 2, Wd // 2)
    if kind == 'enc0':
        xd, wd, ldx = _t(x), _t(pivp_amd.to_internal('enc0/W', W)), 3
    else:
        xd, wd, ldx = nhwc(x), _t(pivp_amd.to_internal('enc4/W' if up else 'enc1/W', W)), cin
    bbuf, bptr = _bias(b)
    gd, bed = _perm(gamma, cout, Ho * Wo), _perm(beta, cout, Ho * Wo)
    raw = torch.full((B, Ho, Wo, cout), PREFILL, dtype=torch.float32, device=DEV)
    obuf, optr, ldo = _out_slice(B, Ho, Wo, cout, ldo, ooff)
    nfl = lib.pivp_conv_layernorm_scratch_floats(KIND[kind], cout, B, H, Wd)
    assert nfl > 0, nfl
    scratch = torch.full((nfl,), float('nan'), dtype=torch.float32, device=DEV)
    fused = ctypes.c_int(-1)
    _lib.check(lib.pivp_conv_layernorm(KIND[kind], xd.data_ptr(), cin, ldx, wd.data_ptr(), bptr, raw.data_ptr(), cout, int(relu), gd.data_ptr(), bed.data_ptr(),
                                       optr, ldo, scratch.data_ptr(), eps, int(relu_ln), B, H, Wd, ctypes.byref(fused), stream()), 'conv_layernorm')
    torch.cuda.synchronize()
    out, guard = _split(obuf, cout, ooff)
    return nchw(raw, B, Ho, Wo, cout), out, fused.value, guard


_PACK = {'bf16': ('pivp_pack_lstm_bf16', 'pivp_convlstm_bf16', 1, 0), 'bf16x3': ('pivp_pack_lstm_bf16x3', 'pivp_convlstm_bf16x3', 2, 0),
         'bf16x6': ('pivp_pack_lstm_bf16x6', 'pivp_convlstm_bf16x6', 3, 0), 'fp16x3': ('pivp_pack_lstm_fp16x3', 'pivp_convlstm_fp16x3', 2, 256)}


def convlstm(entry, x, h, c, W, b, ld=None, variant=0):
    """One ConvLSTM step with x read as the last cx channels of an ld-wide NaN-filled buffer.  entry: 'f32' (pivp_convlstm_v with `variant`) or a packed-operand
    form of _PACK (its pack built here).  -> (h, c) NCHW"""
    lib = _lib.load()
    B, cx, H, Wd = x.shape
    C = h.shape[1]
    xbuf, xptr, ld = _in_slice(x, ld)
    hd, cd = nhwc(h), nhwc(c)
    wd, bd = _t(pivp_amd.to_internal('lstm1/conv/W', W)), _t(b)
    c_out = torch.empty_like(cd); h_out = torch.empty_like(hd)
    if entry == 'f32':
        _lib.check(lib.pivp_convlstm_v(xptr, cx, ld, hd.data_ptr(), C, wd.data_ptr(), bd.data_ptr(), cd.data_ptr(), c_out.data_ptr(), h_out.data_ptr(),
                                       B, H, Wd, variant, stream()), 'convlstm_v')
    else:
        pack, run, pieces, tail = _PACK[entry]
        wb = torch.empty(pieces * lib.pivp_lstm_bf16_weight_elems(cx + C, C) + tail, dtype=torch.int16, device=DEV)
        args = (wd.data_ptr(), wb.data_ptr(), cx + C, C) + ((Wd,) if entry == 'fp16x3' else ()) + (stream(),)
        _lib.check(getattr(lib, pack)(*args), pack)
        _lib.check(getattr(lib, run)(xptr, cx, ld, hd.data_ptr(), C, wb.data_ptr(), bd.data_ptr(), cd.data_ptr(), c_out.data_ptr(), h_out.data_ptr(),
                                     None, None, 0, None, B, H, Wd, 0, stream()), run)
    torch.cuda.synchronize()
    return nchw(h_out, B, H, Wd, C), nchw(c_out, B, H, Wd, C)
