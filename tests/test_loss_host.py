"""CPU-side tests of the image loss: the float64 restatement (tests/loss_reference.py) against metrics_reference, its autograd gradient against the
three-map closed form the kernel uses and against central differences, `ImageLoss` validation, the train.py flags, the C-ABI surface of
include/pivp_loss.h against `_lib.LOSS_SIGNATURES` and the built library, and the off switch of `Model(image_loss=...)`.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_reference as LR  # noqa: E402
import metrics_reference as MR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(seed, shape, kind='noise'):
    rs = np.random.RandomState(seed)
    if kind == 'noise':
        return rs.rand(*shape).astype(np.float32), rs.rand(*shape).astype(np.float32)
    x = (0.9 + 0.02 * rs.rand(*shape)).astype(np.float32)                 # bright and flat: the variances cancel
    return (x + 0.01 * rs.randn(*shape)).astype(np.float32), x


@pytest.mark.parametrize('win,sigma', [(11, 1.5), (7, 1.5), (3, 0.0)])
def test_restated_ssim_is_the_metrics_ssim(win, sigma):
    y, x = _pair(1, (3, 3, 16, 24))
    vals = LR.per_image_terms(torch.tensor(y, dtype=torch.float64), torch.tensor(x, dtype=torch.float64), ('dssim', 'mse'), win, sigma)
    s64, m64 = MR.ssim_mse(y, x, win, sigma)
    assert np.abs((1.0 - vals['dssim'].numpy()) - s64).max() <= 1e-14 and np.abs(vals['mse'].numpy() - m64).max() <= 1e-16


@pytest.mark.parametrize('kind', ['noise', 'flat'])
@pytest.mark.parametrize('win,sigma', [(11, 1.5), (7, 1.5), (5, 0.0)])
def test_autograd_equals_the_three_map_form_and_central_differences(kind, win, sigma):
    """11 x 13: with win = 11 a 1 x 3 strip of positions, everything halo."""
    y, x = _pair(2, (2, 2, 11, 13), kind)
    ref = LR.loss_and_grad(y, x, (0, 0, 0, 1.0), win, sigma)
    N = y.shape[0]
    closed = -LR.ssim_grad_closed_form(y, x, win, sigma) / N               # d mean_n (1 - ssim_n) / d pred
    scale = np.abs(ref['grad']).max()
    assert scale > 0 and np.abs(closed - ref['grad']).max() <= 1e-11 * scale
    # central differences of the float64 total on a handful of pixels: h = 1e-5 leaves 1e-10 of curvature and 1e-11 of rounding
    rs = np.random.RandomState(3)
    y64 = y.astype(np.float64)
    for _ in range(6):
        idx = tuple(rs.randint(0, s) for s in y.shape)
        hi, lo = y64.copy(), y64.copy()
        hi[idx] += 1e-5; lo[idx] -= 1e-5
        fd = (LR.loss_and_grad(hi, x, (0, 0, 0, 1.0), win, sigma)['terms'][4] - LR.loss_and_grad(lo, x, (0, 0, 0, 1.0), win, sigma)['terms'][4]) / 2e-5
        assert abs(fd - ref['grad'][idx]) <= 1e-5 * scale + 1e-9, (idx, fd, ref['grad'][idx])


def test_pointwise_terms_by_hand():
    """A 2 x 2 image: every term written out."""
    y = np.array([[[[0.5, 0.25], [0.75, 0.25]]]])
    x = np.array([[[[0.5, 0.5], [0.25, 0.25]]]])
    r = LR.loss_and_grad(y, x, (1.0, 1.0, 1.0, 0.0))
    assert np.isclose(r['values'][0, 0], (0.0625 + 0.25) / 4) and np.isclose(r['values'][1, 0], (0.25 + 0.5) / 4)
    # vertical edges: | |0.25| - |-0.25| | + | |0| - |-0.25| | = 0.25, over C (H-1) W = 2; horizontal: | |-0.25| - |0| | + | |-0.5| - |0| | = 0.75, over 2
    assert np.isclose(r['values'][2, 0], 0.125 + 0.375) and r['values'][3, 0] == 0 and np.isclose(r['terms'][4], r['terms'][:3].sum())
    # sign(0) = 0: the pixel where pred equals truth gets no L1 gradient; the first vertical edge's outer |.| sits at 0 and passes nothing on
    g = LR.loss_and_grad(y, x, (0.0, 1.0, 0.0, 0.0))['grad']
    assert g[0, 0, 0, 0] == 0 and g[0, 0, 0, 1] == -0.25 and g[0, 0, 1, 0] == 0.25 and g[0, 0, 1, 1] == 0
    gg = LR.loss_and_grad(y, x, (0.0, 0.0, 1.0, 0.0))['grad']
    assert np.isclose(gg[0, 0, 0, 0], 0.5)      # only its horizontal edge passes: dh = y01 - y00 < 0 with |dh| > |dx|, y00 is the subtrahend, over C H (W-1) = 2


def test_image_loss_validation():
    s = pivp_amd.ImageLoss()
    assert s.weights() == (1.0, 0.0, 0.0, 0.0) and s.is_reference() and (s.win, s.sigma, s.data_range) == (11, 1.5, 1.0)
    t = pivp_amd.ImageLoss(mse=0.5, l1=0.2, gdl=0.1, dssim=0.3, win=7, sigma=0, data_range=2)
    assert not t.is_reference() and t.weights() == (0.5, 0.2, 0.1, 0.3) and (t.win, t.sigma, t.data_range) == (7, 0.0, 2.0)
    assert not pivp_amd.ImageLoss(mse=2).is_reference() and not pivp_amd.ImageLoss(mse=0).is_reference()
    for bad in (dict(l1=float('nan')), dict(gdl=float('inf')), dict(mse='1'), dict(dssim=None), dict(l1=True), dict(mse=1e39),
                dict(win=4), dict(win=13), dict(win=1), dict(win=7.0), dict(sigma=float('nan')), dict(data_range=0), dict(data_range=-1.0),
                dict(data_range=float('inf'))):
        with pytest.raises(ValueError):
            pivp_amd.ImageLoss(**bad)
    t.check_frames((3, 7, 9))
    with pytest.raises(ValueError, match='smaller than the 7 x 7 window'):
        t.check_frames((3, 6, 9))
    with pytest.raises(ValueError, match='at least 2 x 2'):
        pivp_amd.ImageLoss(gdl=1.0).check_frames((3, 1, 9))
    pivp_amd.ImageLoss(l1=1.0).check_frames((3, 1, 1))
    # the wrapper checks its arguments before it needs a GPU or the library
    x = np.zeros((2, 3, 8, 8), np.float32)
    for args in ((x, x[:1], t), (x[0, 0], x[0, 0], t), (x, x, (1, 0, 0, 0)), (x[..., :6, :], x[..., :6, :], t)):
        with pytest.raises(ValueError):
            pivp_amd.image_loss(*args)


def test_model_without_an_image_loss_calls_nothing_new():
    """None and the reference's weights leave the model on its old path: no spec is kept active, so neither pivp_image_loss nor the seed hook is
    ever reached (the GPU tests compare the bits)."""
    plain, none, ref = pivp_amd.Model(10), pivp_amd.Model(10, image_loss=None), pivp_amd.Model(10, image_loss=pivp_amd.ImageLoss())
    assert not plain._extra_loss and not none._extra_loss and not ref._extra_loss
    assert plain.loss_terms is None and plain._loss_grad is None and plain.image_loss is None
    on = pivp_amd.Model(10, image_loss=pivp_amd.ImageLoss(l1=0.1))
    assert on._extra_loss and on.loss_terms is None
    for bad in ((1, 0, 0, 0), 'l1', 1.0):
        with pytest.raises(ValueError, match='ImageLoss'):
            pivp_amd.Model(10, image_loss=bad)
    import inspect
    assert 'frame_grad' in inspect.signature(pivp_amd.Model.backward).parameters
    src = inspect.getsource(pivp_amd.Model)
    assert src.count('pivp_plan_set_frame_grad(') == 2 and 'if seed is not None' in src and 'if self._extra_loss:' in src


def test_train_parser_keeps_the_reference_objective_by_default():
    from pivp_amd import train
    a = train.build_parser().parse_args([])
    assert (a.loss_mse, a.loss_l1, a.loss_gdl, a.loss_dssim) == (1.0, 0.0, 0.0, 0.0) and train.image_loss_from_args(a) is None
    b = train.build_parser().parse_args(['--loss_mse', '0.5', '--loss_l1', '0.2', '--loss_gdl', '0.1', '--loss_dssim', '0.3'])
    spec = train.image_loss_from_args(b)
    assert type(spec).__name__ == 'ImageLoss' and spec.weights() == (0.5, 0.2, 0.1, 0.3)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(['--loss_l1', 'some'])
    with pytest.raises(SystemExit):
        train.image_loss_from_args(train.build_parser().parse_args(['--loss_gdl', 'nan']))


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_loss_header_library_and_ctypes_table_agree():
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_loss.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.LOSS_SIGNATURES) == {'pivp_image_loss_ws_bytes', 'pivp_image_loss', 'pivp_plan_set_frame_grad'}
    assert declared <= exported
    assert not any(declared & set(table) for header, table in _lib.HEADER_SIGNATURES.items() if header != 'pivp_loss.h')
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17                                       # pivp_hip.h keeps its symbols and its version
    i, ll, vp, sp = _lib._i, _lib._ll, _lib._vp, ctypes.POINTER(_lib.PivpImageLoss)
    assert _lib.LOSS_SIGNATURES['pivp_image_loss_ws_bytes'] == (ll, [i, i, i, i, sp])
    assert _lib.LOSS_SIGNATURES['pivp_image_loss'] == (i, [vp, vp, i, i, i, i, sp, vp, vp, vp, vp, vp])
    assert _lib.LOSS_SIGNATURES['pivp_plan_set_frame_grad'] == (i, [vp, vp])
    for name, (res, args) in _lib.LOSS_SIGNATURES.items():                    # load() bound the fourth table too
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert 'image_loss.hip' in build.SOURCES and 'pivp_loss.h' in [os.path.basename(f) for f in _digest.source_files()]
    # the struct as the header lays it out: four floats, an int, two floats
    m = re.search(r'typedef struct \{([^}]*)\} pivp_image_loss_t;', open(os.path.join(ROOT, 'include', 'pivp_loss.h')).read())
    fields = [(t, n.strip()) for t, names in re.findall(r'(float|int) ([^;]+);', m.group(1)) for n in names.split(',')]
    assert fields == [({_lib._f: 'float', _lib._i: 'int'}[t], n) for n, t in _lib.PivpImageLoss._fields_]
    assert ctypes.sizeof(_lib.PivpImageLoss) == 28


def test_host_side_argument_checks_need_no_gpu():
    """Sizes, null pointers, the window and the weights are refused before anything is launched: the calls return on a machine without a device."""
    lib = _lib.load()
    sp = _lib.PivpImageLoss(1.0, 0.0, 0.0, 1.0, 11, 1.5, 1.0)
    assert lib.pivp_image_loss_ws_bytes(1, 1, 11, 11, ctypes.byref(sp)) == 32 and lib.pivp_image_loss_ws_bytes(256, 3, 64, 64, ctypes.byref(sp)) == 8192
    for n, c, h, w in ((0, 3, 64, 64), (-1, 3, 64, 64), (2, 0, 64, 64), (2, 3, 0, 64), (2, 3, 64, 0)):
        assert lib.pivp_image_loss_ws_bytes(n, c, h, w, ctypes.byref(sp)) == -1
    assert lib.pivp_image_loss_ws_bytes(2, 3, 64, 64, None) == -1
    assert lib.pivp_image_loss(None, None, 2, 3, 64, 64, ctypes.byref(sp), None, None, None, None, None) == -1
    buf = (ctypes.c_double * 4096)()          # host memory with the right alignment: the checks below fail before anything could read it
    p = ctypes.addressof(buf)
    call = lambda s, N=1, C=1, H=16, W=16, pred=p, ws=p: lib.pivp_image_loss(pred, p, N, C, H, W, ctypes.byref(s) if s else None, p, p, p, ws, None)
    S = _lib.PivpImageLoss
    for bad in (S(1, 0, 0, 1, 4, 1.5, 1), S(1, 0, 0, 1, 13, 1.5, 1), S(1, 0, 0, 0, 1, 1.5, 1), S(float('nan'), 0, 0, 0, 11, 1.5, 1),
                S(1, float('inf'), 0, 0, 11, 1.5, 1), S(1, 0, 0, 1, 11, float('nan'), 1), S(1, 0, 0, 1, 11, 1.5, 0), S(1, 0, 0, 1, 11, 1.5, float('inf')), None):
        assert call(bad) == -1
    assert call(S(0, 0, 0, 1, 11, 1.5, 1), H=10) == -1 and call(S(0, 0, 0, 1, 11, 1.5, 1), W=10) == -1          # smaller than the window
    assert call(S(0, 0, 1, 0, 11, 1.5, 1), H=1) == -1 and call(S(0, 0, 1, 0, 11, 1.5, 1), W=1) == -1            # no edge for the GDL
    assert call(sp, pred=p + 2) == -1 and call(sp, ws=p + 4) == -1 and call(sp, N=0) == -1 and call(sp, C=0) == -1
    assert lib.pivp_plan_set_frame_grad(None, None) == -1


def test_stale_library_is_refused_after_an_edit_to_the_loss_header(monkeypatch, tmp_path):
    from pivp_amd import _digest
    before = _digest.source_digest()
    include = shutil.copytree(_digest.INCLUDE, str(tmp_path / 'include'))      # the public headers, one of them edited
    with open(os.path.join(include, 'pivp_loss.h'), 'ab') as f:
        f.write(b'\n/* edited */\n')
    monkeypatch.setattr(_digest, 'INCLUDE', include)
    assert _digest.source_digest() != before
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(RuntimeError, match='stale'):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load().pivp_abi_version() == 17
