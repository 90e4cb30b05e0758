"""Digest of the HIP sources a libpivp_hip.so is built from.

build.py embeds it in the library (`pivp_build_digest()`, include/pivp_hip.h) and `_lib.load()` recomputes it from the sources that
travel with the package: a library older than the code it claims to implement refuses to load, so a GPU test can never pass on a stale
build.  Sources only (csrc/*.hip, csrc/*.h, the nine public headers): objects, the .so and compile flags are not part of it -- an
instrumented build (PIVP_EXTRA_FLAGS) of the same sources is still the same code."""
import hashlib
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
HEADER = os.path.join(HERE, '..', 'include', 'pivp_hip.h')
DATA_HEADER = os.path.join(HERE, '..', 'include', 'pivp_data.h')      # the data-feed entry points (pivp_gather_batch)
OPTIM_HEADER = os.path.join(HERE, '..', 'include', 'pivp_optim.h')    # the guarded optimizer step (pivp_grad_stats, pivp_adam_step_guarded)
LOSS_HEADER = os.path.join(HERE, '..', 'include', 'pivp_loss.h')      # the image loss and the sweep's seed hook (pivp_image_loss, pivp_plan_set_frame_grad)
INPUT_GRAD_HEADER = os.path.join(HERE, '..', 'include', 'pivp_input_grad.h')      # the sweep's input gradients and its mode (pivp_plan_set_input_grad, pivp_plan_set_sweep_mode)
STATE_HEADER = os.path.join(HERE, '..', 'include', 'pivp_state.h')      # the recurrent state across rollouts (pivp_plan_set_rollout_state, pivp_state_copy)
STATE_GRAD_HEADER = os.path.join(HERE, '..', 'include', 'pivp_state_grad.h')      # gradients through that state (pivp_plan_set_state_grad)
GOAL_COST_HEADER = os.path.join(HERE, '..', 'include', 'pivp_goal_cost.h')      # the planner's goal-image cost (pivp_goal_image_cost)
MPC_HEADER = os.path.join(HERE, '..', 'include', 'pivp_mpc.h')      # closed-loop planning (pivp_cem_update_ex, pivp_cem_shift)


def source_files():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith('.hip') or n.endswith('.h'))
    return [os.path.join(CSRC, n) for n in names] + [DATA_HEADER, HEADER, OPTIM_HEADER, LOSS_HEADER, INPUT_GRAD_HEADER, STATE_HEADER, STATE_GRAD_HEADER, GOAL_COST_HEADER, MPC_HEADER]


def source_digest(paths=None):
    """The digest of `paths` (default: every source file); build.py takes the headers' alone, as its key for recompiling every object."""
    h = hashlib.sha256()
    for path in source_files() if paths is None else paths:
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()
