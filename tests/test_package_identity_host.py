"""CPU-side tests of the package boundary: under the directory's name and under the `pivp_amd` alias, whichever comes first, every file of the
package is ONE module object per process (each order in an interpreter of its own), the `-m` entry points start without a warning, a
`RecurrentState` is recognised by its class and a look-alike is refused, and the public headers are listed once (`_digest.PUBLIC_HEADERS`), each
with the table of exactly what it declares (`_lib.HEADER_SIGNATURES`).  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivp_amd
from pivp_amd import _digest, _lib, planning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = 'physical-interaction-video-prediction_amd'

FIRST = {'alias': 'import pivp_amd', 'own': "importlib.import_module(OWN)\nimport pivp_amd"}
SEQUENCE = r'''
import importlib, os, runpy, sys
OWN = %r
%s
from pivp_amd.planning import cem_plan
import pivp_amd.predict, pivp_amd.evaluate
from pivp_amd import build, _digest
importlib.import_module(OWN + '.planning')
ran = runpy.run_module('pivp_amd.train', run_name='x')
import pivp_amd.train

here = os.path.join(os.getcwd(), OWN) + os.sep
objects = {}
for mod in list(sys.modules.values()):
    f = getattr(mod, '__file__', None)
    if f and os.path.abspath(f).startswith(here):
        objects.setdefault(os.path.basename(f), set()).add(id(mod))
assert all(len(ids) == 1 for ids in objects.values()), {f: len(ids) for f, ids in objects.items() if len(ids) != 1}
assert set(objects) == {n for n in os.listdir(here) if n.endswith('.py')}, sorted(objects)
for name, mod in list(sys.modules.items()):
    for a, b in (('pivp_amd', OWN), (OWN, 'pivp_amd')):
        if name.startswith(a + '.'):
            assert sys.modules.get(b + name[len(a):], mod) is mod, name
assert sys.modules['pivp_amd'] is sys.modules[OWN] and sys.modules['pivp_amd.train'] is sys.modules[OWN + '.train']
assert ran['Model'] is pivp_amd.Model and ran['__package__'] == 'pivp_amd' and ran['__file__'] == pivp_amd.train.__file__
assert pivp_amd.train.Model is pivp_amd.Model
assert pivp_amd.model.config is pivp_amd.config
assert pivp_amd.config.train is True
with pivp_amd.using_config('train', False):      # the `config` that predict's and the run train.py's Model read
    for obj in (pivp_amd.predict.Model, pivp_amd.predict.using_config, ran['Model'], ran['using_config']):
        assert sys.modules[obj.__module__].config.train is False
assert pivp_amd._lib is pivp_amd.model._lib is importlib.import_module(OWN + '._lib')
print('files', len(objects))
'''


@pytest.mark.parametrize('first', sorted(FIRST))
def test_one_module_object_per_file_whichever_name_comes_first(first):
    out = subprocess.run([sys.executable, '-c', SEQUENCE % (OWN, FIRST[first])], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()
    # every .py file of the package directory, __init__.py included
    assert int(out.stdout.decode().split()[-1]) == len([n for n in os.listdir(os.path.join(ROOT, OWN)) if n.endswith('.py')]) >= 18


@pytest.mark.parametrize('entry', ['train', 'predict', 'evaluate'])
def test_the_documented_entry_points_start_without_a_warning(entry):
    out = subprocess.run([sys.executable, '-m', 'pivp_amd.' + entry, '--help'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0 and b'usage' in out.stdout, out.stderr.decode()
    assert b'RuntimeWarning' not in out.stderr, out.stderr.decode()


def test_in_this_process_too_the_alias_names_the_package_s_own_modules():
    import pivp_amd.state
    assert sys.modules['pivp_amd'] is sys.modules[OWN] is pivp_amd
    assert pivp_amd.state is sys.modules[OWN + '.state'] is sys.modules['pivp_amd.state']
    assert pivp_amd.state.__spec__.name == OWN + '.state'      # the module keeps the spec it was loaded with
    assert isinstance(pivp_amd.RecurrentState.__new__(pivp_amd.RecurrentState), pivp_amd.state.RecurrentState)
    assert len([f for f in sys.meta_path if type(f).__name__ == '_AliasFinder']) == 1
    with pytest.raises(ModuleNotFoundError):
        import pivp_amd.no_such_module  # noqa: F401


def test_a_look_alike_of_a_recurrent_state_is_refused():
    """The surface the state used to be recognised by (its class's name, six attributes) no longer passes: the class does."""
    fake = type('RecurrentState', (object,), dict(expand=None, select=None, clone=None))()
    fake.data, fake.batch, fake.hw = torch.zeros(311296), 1, (64, 64)
    on = pivp_amd.Model(10, carry_state=True)
    with pytest.raises(ValueError, match=r'a RecurrentState \(or None\) is expected'):
        on.set_recurrent_state(fake)
    frame, robot = np.zeros((1, 1, 3, 64, 64), np.float32), np.zeros((1, 5), np.float32)
    with pytest.raises(ValueError, match='belief must be a RecurrentState'):
        planning.cem_plan(on, frame, robot, [[32, 32]], [[40, 24]], 3, belief=fake)
    with pytest.raises(ValueError, match='belief must be a RecurrentState'):
        planning.score_actions(on, frame, robot, np.zeros((4, 3, 5)), (32, 32), (40, 24), belief=fake)
    real = pivp_amd.RecurrentState(fake.data, 1, (64, 64))     # (the same buffer in the class itself passes both checks)
    host = pivp_amd.Model(10, carry_state=True, device='cpu')
    host.set_recurrent_state(real)
    assert host._state is not real and torch.equal(host._state.data, real.data)
    with pytest.raises(ValueError, match='past_actions'):
        planning.cem_plan(on, frame, robot, [[32, 32]], [[40, 24]], 3, past_actions=np.zeros((1, 5)), belief=real)


def test_one_list_of_the_public_headers_and_one_table_per_header():
    present = sorted(n for n in os.listdir(os.path.join(ROOT, 'include')) if re.fullmatch(r'pivp_\w+\.h', n))
    assert tuple(_lib.HEADER_SIGNATURES) == _digest.PUBLIC_HEADERS and sorted(_digest.PUBLIC_HEADERS) == present and len(present) == 10
    assert os.path.samefile(_digest.INCLUDE, os.path.join(ROOT, 'include'))
    assert [os.path.basename(p) for p in _digest.source_files()][-10:] == list(_digest.PUBLIC_HEADERS)
    seen = {}
    for header, table in _lib.HEADER_SIGNATURES.items():
        text = open(os.path.join(ROOT, 'include', header)).read()
        declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', text)) - {'pivp_config', 'pivp_plan'}
        assert declared == set(table), (header, declared ^ set(table))
        for name in table:
            assert seen.setdefault(name, header) == header, (name, seen[name], header)      # every symbol in exactly one table
    tables = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'HEADER_SIGNATURES']
    assert len(tables) == 10 and all(any(t is u for u in _lib.HEADER_SIGNATURES.values()) for t in tables)      # no table outside the mapping
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    for name, (res, args) in ((n, s) for t in _lib.HEADER_SIGNATURES.values() for n, s in t.items()):
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res                         # load() bound them all
