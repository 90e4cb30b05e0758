"""Digest of the HIP sources a libpivp_hip.so is built from.

build.py embeds it in the library (`pivp_build_digest()`, include/pivp_hip.h) and `_lib.load()` recomputes it from the sources that
travel with the package: a library older than the code it claims to implement refuses to load, so a GPU test can never pass on a stale
build.  Sources only (csrc/*.hip, csrc/*.h, the public headers of PUBLIC_HEADERS): objects, the .so and compile flags are not part of it -- an
instrumented build (PIVP_EXTRA_FLAGS) of the same sources is still the same code."""
import hashlib
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
INCLUDE = os.path.join(HERE, '..', 'include')
# the public headers, in the order the digest takes them (_lib.HEADER_SIGNATURES: what each declares)
PUBLIC_HEADERS = ('pivp_data.h', 'pivp_hip.h', 'pivp_optim.h', 'pivp_loss.h', 'pivp_input_grad.h', 'pivp_state.h', 'pivp_state_grad.h',
                  'pivp_goal_cost.h', 'pivp_mpc.h', 'pivp_conv_forms.h')


def source_files():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith('.hip') or n.endswith('.h'))
    return [os.path.join(CSRC, n) for n in names] + [os.path.join(INCLUDE, n) for n in PUBLIC_HEADERS]


def source_digest(paths=None):
    """The digest of `paths` (default: every source file); build.py takes the headers' alone, as its key for recompiling every object."""
    h = hashlib.sha256()
    for path in source_files() if paths is None else paths:
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()
