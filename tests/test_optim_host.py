"""CPU-side tests of the guarded Adam step: the C-ABI surface of include/pivp_optim.h against `_lib.OPTIM_SIGNATURES` and the built library, the
build and digest lists, the argument errors of `GradientClipping` / `Adam.add_hook`, the train.py flags, and the float64 restatement
(tests/optim_reference.py) against closed forms.  No GPU."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pivp_amd
from pivp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_reference as OR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_optim_header_library_and_ctypes_table_agree():
    """The guarded step's entry points have a header and a table of their own; the model's ABI and the data feed's stay as they were."""
    import __graft_entry__ as g
    from pivp_amd import _digest, build
    g.build()
    declared = _declared('pivp_optim.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.OPTIM_SIGNATURES) == {'pivp_grad_stats_ws_bytes', 'pivp_grad_stats', 'pivp_adam_step_guarded'}
    assert declared <= exported
    assert not declared & set(_lib.SIGNATURES) and not declared & set(_lib.DATA_SIGNATURES)
    assert len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 and _declared('pivp_data.h') == {'pivp_gather_batch'}
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17
    i, ll, vp, d = _lib._i, _lib._ll, _lib._vp, _lib._c.c_double
    assert _lib.OPTIM_SIGNATURES['pivp_grad_stats_ws_bytes'] == (ll, [ll, i])
    assert _lib.OPTIM_SIGNATURES['pivp_grad_stats'] == (i, [vp, ll, vp, vp, i, i, d, d, vp, vp, vp])
    assert _lib.OPTIM_SIGNATURES['pivp_adam_step_guarded'] == (i, [vp] * 4 + [ll] + [d] * 5 + [vp, i, vp, vp])
    for name, (res, args) in _lib.OPTIM_SIGNATURES.items():                  # load() bound the third table too
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert 'optim.hip' in build.SOURCES and 'pivp_optim.h' in [os.path.basename(f) for f in _digest.source_files()]
    header = open(os.path.join(ROOT, 'include', 'pivp_optim.h')).read()
    assert int(re.search(r'#define PIVP_OPTIM_MAX_SEGMENTS (\d+)', header).group(1)) == _lib.OPTIM_MAX_SEGMENTS >= 256
    assert int(re.search(r'#define PIVP_GRAD_GROUPS (\d+)', open(os.path.join(ROOT, 'include', 'pivp_hip.h')).read()).group(1)) == _lib.GRAD_GROUPS


def test_host_side_argument_checks_of_the_entry_points_need_no_gpu():
    """Sizes and null pointers are refused before anything is launched: the calls return on a machine without a device."""
    lib = _lib.load()
    cap = _lib.OPTIM_MAX_SEGMENTS
    assert lib.pivp_grad_stats_ws_bytes(1, 1) == 16 and lib.pivp_grad_stats_ws_bytes(197, 3) == (4 + 3) * 8
    assert lib.pivp_grad_stats_ws_bytes(2 ** 33 + 1, cap) == (2 ** 27 + 1 + cap) * 8
    for n, nseg in ((0, 1), (-5, 1), (64, 0), (64, -1), (64, cap + 1)):
        assert lib.pivp_grad_stats_ws_bytes(n, nseg) == -1
    assert lib.pivp_grad_stats(None, 64, None, None, 1, 1, 1.0, 0.0, None, None, None) == -1
    assert lib.pivp_adam_step_guarded(None, None, None, None, 64, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, 0, None, None) == -1


def test_stale_library_is_refused_after_an_edit_to_the_optim_header(monkeypatch, tmp_path):
    from pivp_amd import _digest
    before = _digest.source_digest()
    include = shutil.copytree(_digest.INCLUDE, str(tmp_path / 'include'))      # the public headers, one of them edited ...
    with open(os.path.join(include, 'pivp_optim.h'), 'ab') as f:
        f.write(b'\n/* edited */\n')
    monkeypatch.setattr(_digest, 'INCLUDE', include)
    assert _digest.source_digest() != before
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(RuntimeError, match='stale'):
        _lib.load()
    os.remove(os.path.join(include, 'pivp_optim.h'))                           # ... then absent
    with pytest.raises(RuntimeError, match=r'pivp_optim\.h is missing .*include/.*pivp_optim\.h.* next to it'):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load().pivp_abi_version() == 17


def test_gradient_clipping_and_add_hook_argument_errors(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_library)
    assert 'GradientClipping' in pivp_amd.__all__ and 'Adam' in pivp_amd.__all__            # exported from the package as Adam is
    h = pivp_amd.GradientClipping(5)
    assert h.name == 'GradientClipping' and h.threshold == 5.0 and isinstance(h.threshold, float)
    for bad in (0, 0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            pivp_amd.GradientClipping(bad)
    for bad in (None, '1.0', True, [1.0]):
        with pytest.raises(TypeError):
            pivp_amd.GradientClipping(bad)
    opt = pivp_amd.Adam(alpha=1e-3)
    assert (opt.skip_nonfinite, opt.track_grad_norm) == (False, False) and not opt._guarded()
    with pytest.raises(RuntimeError, match='setup'):                          # Chainer 2: add_hook before setup
        opt.add_hook(h)
    assert opt.setup(pivp_amd.Model(10)) is opt and not opt._guarded()
    for bad in (lambda o: None, object(), 'GradientClipping', None):
        with pytest.raises(TypeError, match='only GradientClipping'):
            opt.add_hook(bad)
    opt.add_hook(h)
    assert opt._guarded()
    with pytest.raises(KeyError):                                             # a duplicate name
        opt.add_hook(pivp_amd.GradientClipping(1.0))
    with pytest.raises(KeyError):
        opt.remove_hook('clip')
    opt.remove_hook('GradientClipping')
    assert not opt._guarded()
    opt.add_hook(pivp_amd.GradientClipping(2.0), name='clip')
    with pytest.raises(KeyError):
        opt.add_hook(h, name='clip')
    with pytest.raises(ValueError, match='one GradientClipping'):             # a second clipping hook under another name
        opt.add_hook(h)
    opt.remove_hook('clip')
    assert pivp_amd.Adam(skip_nonfinite=True)._guarded() and pivp_amd.Adam(track_grad_norm=True)._guarded()
    o = pivp_amd.Adam(track_grad_norm=True)
    assert o.grad_norm is None and o.clip_rate is None and o.grad_nonfinite is None and o.group_norms is None and o.skipped_steps == 0
    with pytest.raises(RuntimeError, match='no guarded step'):
        o.param_norms()


def test_train_parser_leaves_the_guard_off():
    from pivp_amd import train
    a = train.build_parser().parse_args([])
    assert (a.grad_clip, a.skip_nonfinite, a.log_grad_norm) == (0.0, 0, 0)
    b = train.build_parser().parse_args(['--grad_clip', '2.5', '--skip_nonfinite', '1', '--log_grad_norm', '1'])
    assert (b.grad_clip, b.skip_nonfinite, b.log_grad_norm) == (2.5, 1, 1)
    for bad in (['--skip_nonfinite', '2'], ['--log_grad_norm', '-1'], ['--grad_clip', 'much']):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(bad)
    stat = lambda v: [float(np.mean(v)), float(np.std(v)), float(np.min(v)), float(np.max(v)), float(np.median(v))]
    assert train.grad_norm_stat([1.0, float('nan'), 3.0, float('inf')], stat) == [2.0, 1.0, 1.0, 3.0, 2.0]
    assert np.isnan(train.grad_norm_stat([float('nan')], stat)).all() and len(train.grad_norm_stat([], stat)) == 5


def test_reference_closed_forms():
    """Constant gradients: every norm is c * sqrt(count), exactly representable pieces, float64 sums: 1e-15 relative."""
    n, c = 1000, 0.75
    ends, groups = [64, 640, 1000], [0, 3, 3]
    r = OR.grad_stats(np.full(n, c, np.float32), ends, groups, gscale=0.5, threshold=0.0)
    assert abs(r['norm'] - 0.5 * c * math.sqrt(n)) <= 1e-15 * r['norm'] and r['nonfinite'] == 0 and r['rate'] == np.float32(1)
    want_seg = [0.5 * c * math.sqrt(k) for k in (64, 576, 360)]
    assert np.abs(r['seg_norms'] - want_seg).max() <= 1e-14
    want_grp = [want_seg[0], 0, 0, 0.5 * c * math.sqrt(936), 0, 0]
    assert r['group_norms'].shape == (6,) and np.abs(r['group_norms'] - want_grp).max() <= 1e-14
    # a threshold above the norm: rate exactly 1; below: threshold / norm rounded to float32; Chainer's rule on the clipped gradient
    norm = c * math.sqrt(n)
    assert OR.grad_stats(np.full(n, c, np.float32), ends, groups, threshold=norm * 1.0001)['rate'] == np.float32(1)
    half = OR.grad_stats(np.full(n, c, np.float32), ends, groups, threshold=norm / 2)['rate']
    assert half.dtype == np.float32 and abs(float(half) - 0.5) < 1e-7
    assert abs(np.linalg.norm(OR.clipped(np.full(n, c, np.float32), half)) - norm / 2) < 1e-6
    # a zero gradient: rate 1 and no NaN anywhere
    z = OR.grad_stats(np.zeros(n, np.float32), ends, groups, threshold=1.0)
    assert z['norm'] == 0 and z['rate'] == np.float32(1) and z['nonfinite'] == 0 and not np.isnan(z['seg_norms']).any() and not np.isnan(z['group_norms']).any()
    # magnitudes whose squares leave float32, and the detector
    big = OR.grad_stats(np.full(n, 1e30, np.float32), ends, groups)
    assert big['nonfinite'] == 0 and abs(big['norm'] - float(np.float32(1e30)) * math.sqrt(n)) <= 1e-15 * big['norm']
    g = np.full(n, c, np.float32)
    g[700] = np.nan
    bad = OR.grad_stats(g, ends, groups, threshold=1.0)
    assert bad['nonfinite'] == 1 and np.isnan(bad['norm']) and bad['rate'] == np.float32(1)
    assert np.isfinite(bad['seg_norms']).tolist() == [True, True, False] and np.isfinite(bad['group_norms']).tolist() == [True, True, True, False, True, True]
    # one Adam step from zero state moves every weight by alpha * sign(g) (m / sqrt(v) = (1 - b1) g / (sqrt(1 - b2) |g|), bias-corrected to 1)
    p, m, v = OR.guarded_adam_steps(np.zeros(4), [np.array([3.0, -2.0, 0.5, -8.0])], [np.float32(0.5)])
    assert np.abs(p - (-1e-3 * np.sign([3.0, -2.0, 0.5, -8.0]))).max() < 1e-8 and np.allclose(m, 0.1 * 0.5 * np.array([3.0, -2.0, 0.5, -8.0]))
