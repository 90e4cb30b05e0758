"""Everything a plan decides on the host, as text: python scripts/plan_table.py LIB > table.txt

For a host-side refactor of the plan (csrc/plan*.hip): run it on the library before and after, and `cmp` the two outputs.  A CPU-ONLY tool: it
hides every GPU from its process before the library is loaded and refuses to run if the runtime still reports one.  The table: the parameter
table, the workspace size of every configuration, the return code of every setter (good and bad arguments, before and after a workspace is
bound), and the frame-size checks of every entry point that has one.  Pointers are made-up addresses with
the alignment an entry asks for; nothing dereferences them.  The state-copy and state-gradient entries with a frame size they accept do try to launch:
without a device that fails in the runtime, and its code is part of the table -- with one the kernels would touch those addresses, hence the refusal."""
import os
os.environ['HIP_VISIBLE_DEVICES'] = ''      # before the HIP runtime is loaded: this process sees no device
os.environ['ROCR_VISIBLE_DEVICES'] = ''
os.environ['CUDA_VISIBLE_DEVICES'] = ''
import ctypes
import hashlib
import itertools
import sys

_i, _f, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong


class Config(ctypes.Structure):      # pivp_config_t
    _fields_ = [('batch', _i), ('seq_len', _i), ('height', _i), ('width', _i), ('num_masks', _i), ('model_type', _i), ('use_state', _i),
                ('context_frames', _i), ('keep_activations', _i), ('ln_eps', _f), ('stp_zero_border', _i),
                ('action_dim', _i), ('state_dim', _i)]      # 0 / 0 (config() below leaves them out) = the reference data's 5 / 5


MODELS = (('CDNA', 0, 10), ('STP', 1, 10), ('DNA', 2, 1))
SIZES = ((64, 64), (128, 128), (48, 80))
PRECISIONS = ('f32', 'bf16', 'bf16x3', 'bf16x6', 'fp16x3')
OPT_WGRAD_BATCH, OPT_COUNT = 4, 5
A = 1 << 20      # a made-up address, aligned for every entry


def config(model, nm, h, w, b, t, keep=1):
    return Config(b, t, h, w, nm, model, 1, 2 if t > 2 else 1, keep, 1e-6, 0)


def main(path):
    lib = ctypes.CDLL(path)
    count = _i(-1)
    ctypes.CDLL('libamdhip64.so').hipGetDeviceCount(ctypes.byref(count))      # (the runtime the library has just loaded; an error leaves 0 devices)
    if count.value != 0:
        sys.exit('plan_table.py: the runtime reports %d GPU(s) to this process: refusing to run (made-up pointers; run it on a machine without one)' % count.value)
    lib.pivp_param_name.restype = ctypes.c_char_p
    lib.pivp_param_numel.restype = _ll
    lib.pivp_plan_workspace_bytes.restype = _ll
    lib.pivp_get_tap.restype = _ll
    out = sys.stdout.write

    def create(cfg):
        plan = _vp()
        rc = lib.pivp_plan_create(ctypes.byref(cfg), ctypes.byref(plan))
        return rc, plan

    out('abi %d\n' % lib.pivp_abi_version())
    # ---- the parameter table, per model and frame size ----
    for (name, model, nm), (h, w) in itertools.product(MODELS, SIZES):
        rc, plan = create(config(model, nm, h, w, 2, 10))
        n = lib.pivp_param_count(plan)
        out('params %s %dx%d rc=%d count=%d\n' % (name, h, w, rc, n))
        for k in range(n):
            pname = lib.pivp_param_name(plan, k)
            out('  %d %s %d group=%d by_name=%d\n' % (k, pname.decode(), lib.pivp_param_numel(plan, k), lib.pivp_param_group(plan, k),
                                                    lib.pivp_param_group_by_name(pname)))
        out('  out of range: %s %d %d\n' % (lib.pivp_param_name(plan, n), lib.pivp_param_numel(plan, -1), lib.pivp_param_group(plan, n)))
        lib.pivp_plan_destroy(plan)
    # ---- the workspace of every configuration, with the setters that size it ----
    for (name, model, nm), (h, w), b, t, keep, prec, det, wb in itertools.product(MODELS, SIZES, (2, 3, 32), (3, 4, 10, 20), (0, 1), range(5), (0, 1), (0, 3)):
        rc, plan = create(config(model, nm, h, w, b, t, keep))
        rcs = (rc, lib.pivp_plan_set_option(plan, OPT_WGRAD_BATCH, wb), lib.pivp_plan_set_precision(plan, prec), lib.pivp_plan_set_deterministic(plan, det))
        out('ws %s %dx%d B=%d T=%d keep=%d %s det=%d wb=%d rc=%s bytes=%d prec=%d det=%d\n' % (
            name, h, w, b, t, keep, PRECISIONS[prec], det, wb, rcs, lib.pivp_plan_workspace_bytes(plan), lib.pivp_plan_get_precision(plan),
            lib.pivp_plan_get_deterministic(plan)))
        lib.pivp_plan_destroy(plan)
    # ---- every setter's return codes, before and after a workspace is bound ----
    for (name, model, nm), keep in itertools.product(MODELS, (0, 1)):
        cfg = config(model, nm, 64, 64, 2, 10, keep)
        rc, plan = create(cfg)
        n = lib.pivp_param_count(plan)
        for bound in (0, 1):
            r = []
            call = lambda fn, *a: r.append('%s%s=%d' % (fn, a, getattr(lib, fn)(plan, *[_vp(x) if isinstance(x, int) and x >= A or x is None else x for x in a])))
            for idx, ptr in ((-1, A), (n, A), (0, None), (0, A)):
                call('pivp_plan_set_param', idx, ptr)
                call('pivp_plan_set_grad', idx, ptr)
            for opt, v in itertools.product(range(-1, OPT_COUNT + 1), (-1, 0, 1, 2, 8, 9)):
                call('pivp_plan_set_option', opt, v)
                call('pivp_plan_get_option', opt)
            for v in range(-1, 6):
                call('pivp_plan_set_precision', v)
                call('pivp_plan_set_deterministic', 1)
                call('pivp_plan_set_deterministic', 0)
            call('pivp_plan_set_precision', 0)
            for p in (None, A, A + 2):
                call('pivp_plan_set_frame_grad', p)
            for pa, pb in ((None, None), (A, A + 4096), (A + 1, None), (None, A + 2)):
                call('pivp_plan_set_input_grad', pa, pb)
            for pa, pb, obs in ((None, None, 0), (A, A, 0), (A, A + 16, 9), (A + 4, None, 0), (None, A + 8, 0), (A, None, -1), (A, None, 10)):
                call('pivp_plan_set_rollout_state', pa, pb, obs)
            for en, pa, pb in ((0, None, None), (2, None, None), (-1, None, None), (0, None, A), (1, None, A), (1, A, A + 64), (1, A, A + (1 << 30)), (1, A + 8, None),
                               (0, A, None), (0, None, None)):
                call('pivp_plan_set_state_grad', en, pa, pb)
            for v in range(-1, 5):
                call('pivp_plan_set_sweep_mode', v)
                call('pivp_plan_get_sweep_mode')
            call('pivp_plan_set_sweep_mode', 3)
            for v in range(-2, 3):
                call('pivp_plan_set_main_priority', v)
            call('pivp_plan_set_main_priority', -1)
            for v in (0, 1, 2):
                call('pivp_plan_set_group_join', v)
                call('pivp_plan_set_pack_cache', v)
            call('pivp_plan_params_changed')
            call('pivp_plan_set_grad_callback', None, None)
            for g in (-1, 0, 5, 6):
                call('pivp_plan_group_wait', g, None)      # (no side stream yet: nothing to wait for)
            call('pivp_reset_state', None) if not bound else None
            call('pivp_get_tap', b'enc0', 0, A, None)
            call('pivp_rollout_backward', A, A, A, None, A, A, None)      # (no rollout yet: refused before any launch)
            call('pivp_rollout_backward', None, A, A, None, A, A, None)
            call('pivp_rollout_forward', None, A, A, None, A, A, A, None)
            ws = lib.pivp_plan_workspace_bytes(plan)
            for ptr, nbytes in ((None, ws), (A + 128, ws), (A, ws - 4), (A, ws)):
                r.append('set_workspace(%s,%d)=%d' % (ptr, nbytes - ws, lib.pivp_plan_set_workspace(plan, _vp(ptr), _ll(nbytes))))
            out('setters %s keep=%d bound=%d sha=%s\n' % (name, keep, bound, hashlib.sha256('\n'.join(r).encode()).hexdigest()[:16]))
            for line in r:
                out('  ' + line + '\n')
        lib.pivp_plan_destroy(plan)
    # ---- the frame-size checks: every entry point that has one ----
    seg = (_ll * 14)()
    total = _ll()
    tab = (_vp * 7)(*[A + 4096 * k for k in range(7)])
    for h, w, b in itertools.product((8, 16, 20, 24), (8, 16, 20, 24), (0, 1)):
        cfg = config(0, 10, h, w, b, 3)
        rc, plan = create(cfg)
        if rc == 0:
            lib.pivp_plan_destroy(plan)
        r = ['create=%d' % rc]
        for s, tot in ((None, None), (seg, None), (None, ctypes.byref(total)), (seg, ctypes.byref(total))):
            total.value = -1
            r.append('layout=%d:%d' % (lib.pivp_state_layout(ctypes.byref(cfg), s, tot), total.value))
        for index in (None, _vp(A)):
            r.append('copy=%d' % lib.pivp_state_copy(ctypes.byref(cfg), _vp(A), 1, _vp(A + (1 << 24)), 1, index, None))
        r.append('copy(B 1->2, no index)=%d' % lib.pivp_state_copy(ctypes.byref(cfg), _vp(A), 1, _vp(A + (1 << 24)), 2, None, None))
        r.append('gather=%d' % lib.pivp_state_grad_gather(ctypes.byref(cfg), tab, tab, _vp(A + (1 << 24)), None))
        r.append('gather(null out)=%d' % lib.pivp_state_grad_gather(ctypes.byref(cfg), tab, tab, None, None))
        r.append('scatter=%d' % lib.pivp_state_grad_scatter(ctypes.byref(cfg), _vp(A + (1 << 24)), tab, None))
        r.append('scatter(null seed)=%d' % lib.pivp_state_grad_scatter(ctypes.byref(cfg), None, tab, None))
        out('frame %dx%d B=%d %s\n' % (h, w, b, ' '.join(r)))
    out('null cfg: %d %d %d %d %d\n' % (lib.pivp_plan_create(None, None), lib.pivp_state_layout(None, seg, ctypes.byref(total)),
                                        lib.pivp_state_copy(None, _vp(A), 1, _vp(A), 1, None, None),
                                        lib.pivp_state_grad_gather(None, tab, tab, _vp(A), None), lib.pivp_state_grad_scatter(None, _vp(A), tab, None)))


if __name__ == '__main__':
    main(sys.argv[1])
