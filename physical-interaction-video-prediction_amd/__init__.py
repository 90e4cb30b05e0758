"""MI355X-native ConvLSTM + CDNA/STP/DNA next-frame prediction hot path.

Drop-in for the `Model` of kristofbc/physical-interaction-video-prediction
(src/models/train_model.py:478-764) on gfx950: Python host code on PyTorch-ROCm for memory and
streams, hand-written HIP kernels behind the C ABI in include/pivp_hip.h for the arithmetic.

The directory name carries a hyphen (it mirrors the reference repository's name), so import it
with importlib or through the `pivp_amd` alias module at the repo root:
    import pivp_amd
    model = pivp_amd.Model(num_masks=10, is_cdna=True, prefix='predict')
Under either name, in either order, every file of the package is one module object per process.
"""
import importlib.abc
import importlib.machinery
import importlib.util
import sys

_ALIAS = 'pivp_amd' if __name__ != 'pivp_amd' else 'physical-interaction-video-prediction_amd'


class _AliasFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """`<alias>.<x>` IS the module `<this package>.<x>`: imported under the package's own name, handed out under the other, never executed again."""

    def find_spec(self, fullname, path=None, target=None):
        if not fullname.startswith(_ALIAS + '.'):      # (the package's own name goes the ordinary way: answering for it would recurse)
            return None
        real = importlib.util.find_spec(__name__ + fullname[len(_ALIAS):])
        return real and importlib.machinery.ModuleSpec(fullname, self, origin=real.origin, loader_state=real)      # (origin: `python -m`'s __file__)

    def create_module(self, spec):
        module = importlib.import_module(spec.loader_state.name)
        spec.loader_state = module.__spec__      # module_from_spec() is about to overwrite it with `spec` ...
        return module

    def exec_module(self, module):
        module.__spec__ = module.__spec__.loader_state      # ... and a later find_spec() of the own name must not answer with the alias's

    def get_code(self, fullname):      # runpy (`python -m <alias>.<x>`)
        real = importlib.util.find_spec(__name__ + fullname[len(_ALIAS):])
        return real.loader.get_code(real.name)


sys.modules.setdefault(_ALIAS, sys.modules[__name__])
if not any(type(f).__name__ == '_AliasFinder' for f in sys.meta_path):
    sys.meta_path.insert(0, _AliasFinder())

from .model import Model, config, using_config, reference_param_shapes, default_init, scheduled_sampling_masks
from .checkpoint import save_npz, load_npz, to_internal, from_internal, save_optimizer_npz, load_optimizer_npz
from . import dataset
from .dataset import DeviceDataset, DeviceBatcher
from . import planning
from . import metrics
from .metrics import frame_metrics, StepCurves
from . import losses
from .losses import ImageLoss, image_loss
from . import state
from .state import RecurrentState
from . import tbptt
from .tbptt import chunked_backward
from .data import concat_examples
from .optimizer import Adam, GradientClipping
from .parallel import GradAllReduce, shard_batch

__all__ = ['Model', 'config', 'using_config', 'reference_param_shapes', 'default_init',
           'scheduled_sampling_masks', 'save_npz', 'load_npz', 'to_internal', 'from_internal', 'concat_examples',
           'Adam', 'GradientClipping', 'GradAllReduce', 'shard_batch', 'save_optimizer_npz', 'load_optimizer_npz', 'dataset', 'planning',
           'metrics', 'frame_metrics', 'StepCurves', 'DeviceDataset', 'DeviceBatcher', 'losses', 'ImageLoss', 'image_loss', 'state', 'RecurrentState',
           'tbptt', 'chunked_backward']
