"""Back-propagation through time over a sequence that is processed in consecutive windows, on a `Model(carry_state=True, keep_activations=True,
state_backward=True)` (include/pivp_state_grad.h).

Two ways to train on a long sequence in pieces:
  * truncated: call the model on a window, `backward()`, step the optimizer, go on with the next window without `reset_state()` -- the state the
    window started from is a constant of its sweep (train.py --tbptt_windows N does this);
  * exact, `chunked_backward`: the full gradient of the summed loss of all windows in the activation memory of ONE window, at the price of running
    every window but the last forward twice."""
import numpy as np

from .state import RecurrentState


def split_windows(x, n):
    """[images, actions, states] (time-major, T frames) -> n consecutive windows of T // n frames each; T must be divisible by n."""
    images, actions, states = x
    T = len(images)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError('the number of windows must be a positive integer, not %r' % (n,))
    if T % n or T // n < 2:
        raise ValueError('%d frames cannot be cut into %d consecutive windows of at least 2 frames each' % (T, n))
    w = T // n
    return [[images[k * w:(k + 1) * w], actions[k * w:(k + 1) * w], states[k * w:(k + 1) * w]] for k in range(n)]


def _rng_of(model):
    return model.sampling_rng if model.sampling_rng is not None else np.random


def _rng_state(rng):
    """the state of what scheduled sampling draws from: NumPy's global stream, a RandomState, or a Generator (which has no get_state)"""
    return rng.get_state() if hasattr(rng, 'get_state') else rng.bit_generator.state


def _rng_restore(rng, state):
    if hasattr(rng, 'set_state'):
        rng.set_state(state)
    else:
        rng.bit_generator.state = state


def _check(model, windows):
    if not getattr(model, 'state_backward', False):
        raise ValueError('chunked_backward needs Model(..., carry_state=True, keep_activations=True, state_backward=True)')
    if not isinstance(windows, (list, tuple)) or len(windows) < 1:
        raise ValueError('windows must be a non-empty list of [images, actions, states]')
    for w in windows:
        if not isinstance(w, (list, tuple)) or len(w) != 3:
            raise ValueError('every window is [images, actions, states], time-major')
    rng = _rng_of(model)
    if not (hasattr(rng, 'get_state') and hasattr(rng, 'set_state')) and not hasattr(rng, 'bit_generator'):
        raise ValueError('model.sampling_rng must be a numpy RandomState or Generator (its state is put back for the second pass), not %r' % (type(rng).__name__,))


def chunked_backward(model, windows, iter_num=-1.0):
    """Exact BPTT over consecutive `windows` ([images, actions, states] each, time-major, one batch and frame size) in the memory of one window.

    1. The windows run forward in order from the state the model carries (zeros after `reset_state()`), a snapshot of the state in front of each is kept.
    2. Backwards over the windows: the state is set back to the window's snapshot, the window runs forward again (the last one still holds its
       activations and is not repeated) and `backward(final_state_grad=<the next window's initial_state_grad>, initial_state_grad=True)` sweeps it.
    Gradients ACCUMULATE in `model._flat_grads` as with `backward()`: `cleargrads()` first.  Returns the summed loss of the windows (a device scalar).
    Behind the call the model carries the state the last window left; `loss`, `gen_images` and the other per-call results are those of the window
    swept last, the first one.  Scheduled sampling draws the same ground-truth selection in both passes (the host RNG's state is put back for the
    second).  Nothing synchronises with the host."""
    _check(model, windows)
    rng = _rng_of(model)
    snaps, draws, total = [], [], None
    for w in windows:
        snaps.append(model.recurrent_state())
        draws.append(_rng_state(rng))
        loss = model(w, iter_num)
        total = loss if total is None else total + loss
    final = model.recurrent_state()
    after = _rng_state(rng)
    seed = None
    try:
        for k in reversed(range(len(windows))):
            if k != len(windows) - 1:
                model.set_recurrent_state(snaps[k])
                _rng_restore(rng, draws[k])
                model(windows[k], iter_num)
            carried = snaps[k] is not None
            model.backward(final_state_grad=seed, initial_state_grad=carried)
            seed = model.initial_state_grad if carried else None      # (only the first window can have started from zeros)
    finally:
        _rng_restore(rng, after)
        if isinstance(final, RecurrentState):
            model._adopt_state(final)
    return total
