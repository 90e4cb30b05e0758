"""What feeding the training loop costs: the host feed (`dataset.DeviceFeeder`) against the device-resident data set (`dataset.DeviceDataset` +
`DeviceBatcher`, one pivp_gather_batch launch per batch).  profiles/r11/NOTES.md holds the results.

Part 1, per batch, for three shapes -- config 2 (B = 32, T = 10, 64 x 64), config 5 (B = 32, T = 20, 128 x 128) and one rank's share of a global
batch of 256 over 8 ranks (T = 10, 64 x 64; no process group: a rank is a slice):
    host_ms     wall time of what `DeviceFeeder.prefetch` does: draw, `concat_examples`, the rank's slice, the copy into pinned memory and the
                host-to-device copy until its event
    gather_us   `DeviceDataset.gather` per batch between two HIP events (the index copy and the kernel, as training issues them), and
    kernel_us   200 back-to-back pivp_gather_batch launches on one index buffer between two HIP events, for uint8 and for float32 storage, with the
                bytes moved (stored bytes read + batch bytes written) and their share of the 8 TB/s HBM peak.  Both are upper bounds of the
                kernel's own time wherever the host issues launches more slowly than the GPU retires them
Part 2, ms per step of `get(); optimizer.update(); prefetch(); read the loss` at config 2 on a synthetic set of 512 sequences, in fp32 and bf16,
fed three ways: by `DeviceFeeder`, by `DeviceBatcher` (uint8 storage), and with one resident batch.
Every figure: `--rounds` (at least 7) rounds, the legs interleaved round by round in one process; median, minimum and maximum over the rounds.
The command sets no thread counts.  Prints one JSON line.

    python scripts/bench_feed.py [--rounds 7] [--steps 10] [--skip_loop]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
# name: (sequences in the synthetic set, T, H, W, drawn batch, ranks)
SHAPES = {'config2_B32_T10_64x64': (512, 10, 64, 64, 32, 1),
          'config5_B32_T20_128x128': (64, 20, 128, 128, 32, 1),
          'rank_of_8_global_B256_T10_64x64': (512, 10, 64, 64, 256, 8)}


def stats(v, nd=3):
    return {'median': round(float(np.median(v)), nd), 'min': round(float(min(v)), nd), 'max': round(float(max(v)), nd)}


def synthetic_set(N, T, H, W, seed=0):
    """Frames on the k / 255 grid (what 8-bit images give), so that both storages hold the same set."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(N, T, H, W, 3), dtype=np.uint8).astype(np.float32) / np.float32(255)
    return img, (rs.randn(N, T, 5) * 0.1).astype(np.float32), (rs.randn(N, T, 5) * 0.1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip_loop', action='store_true')
    args = ap.parse_args()
    assert args.rounds >= 7, 'at least 7 interleaved rounds'
    import torch
    import pivp_amd
    from pivp_amd import dataset as ds
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    out = {'rounds': args.rounds, 'steps': args.steps, 'per_batch': {}, 'loop_ms_per_step': {}}

    for name, (N, T, H, W, B, world) in SHAPES.items():
        img, act, sta = synthetic_set(N, T, H, W)
        np.random.seed(0)
        feeder = ds.DeviceFeeder(ds.SerialIterator(ds.group_examples(img, act, sta), B, repeat=True, shuffle=True), rank=0, world=world, device=dev)
        sets = {s: ds.DeviceDataset(img, act, sta, dev, storage=s) for s in ('uint8', 'float32')}
        per = B // world
        bufs = {s: sets[s].gather(list(range(per))) for s in sets}
        rs = np.random.RandomState(1)
        draws = [rs.randint(0, N, size=per) for _ in range(args.steps)]

        def host_feed():
            t0 = time.perf_counter()
            feeder.prefetch()
            feeder._slots[feeder._staged[0]]['copied'].synchronize()
            dt = time.perf_counter() - t0
            feeder.get()                                   # hand the batch over: the next prefetch draws again
            return dt * 1e3

        def gather(storage):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dd = sets[storage]
            for idx in draws[:2]:
                dd.gather(idx, out=bufs[storage])
            torch.cuda.synchronize()
            # the indices travel in front of every launch, as in training; the events bracket index copies and kernels of `steps` batches
            e0.record()
            for idx in draws:
                dd.gather(idx, out=bufs[storage])
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / len(draws) * 1e3
        from pivp_amd import _lib
        lib = _lib.load()
        fixed = torch.from_numpy(draws[0].astype(np.int32)).to(dev)
        stream = torch.cuda.current_stream().cuda_stream

        def kernel(storage, n=200):
            dd, o = sets[storage], bufs[storage]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call = lambda: lib.pivp_gather_batch(dd.frames.data_ptr(), int(storage == 'uint8'), dd.actions.data_ptr(), dd.states.data_ptr(),
                                                 fixed.data_ptr(), per, dd.N, dd.T, dd.H, dd.W, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream)
            for _ in range(3):
                _lib.check(call(), 'pivp_gather_batch')
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n * 1e3
        for _ in range(3):
            host_feed()
        series = {'host_ms': [], 'gather_uint8_us': [], 'gather_float32_us': [], 'kernel_uint8_us': [], 'kernel_float32_us': []}
        for _ in range(args.rounds):
            series['host_ms'].append(float(np.median([host_feed() for _ in range(args.steps)])))
            series['gather_uint8_us'].append(gather('uint8'))
            series['gather_float32_us'].append(gather('float32'))
            series['kernel_uint8_us'].append(kernel('uint8'))
            series['kernel_float32_us'].append(kernel('float32'))
        rec = {k: stats(v) for k, v in series.items()}
        batch_bytes = T * per * (3 * H * W + 10) * 4
        for s, item in (('uint8', 1), ('float32', 4)):
            moved = batch_bytes + T * per * (3 * H * W * item + 40)
            rec['kernel_%s_bytes' % s] = moved
            rec['kernel_%s_hbm_share' % s] = round(moved / (rec['kernel_%s_us' % s]['median'] * 1e-6) / HBM_PEAK, 4)
        rec['batch_bytes'] = batch_bytes
        rec['host_over_gather_uint8'] = round(rec['host_ms']['median'] * 1e3 / rec['gather_uint8_us']['median'], 1)
        out['per_batch'][name] = rec
        del feeder, sets, bufs, img
        torch.cuda.empty_cache()

    if not args.skip_loop:
        N, T, H, W, B, _ = SHAPES['config2_B32_T10_64x64']
        img, act, sta = synthetic_set(N, T, H, W)
        dd = ds.DeviceDataset(img, act, sta, dev, storage='uint8')
        examples = ds.group_examples(img, act, sta)
        for precision in ('fp32', 'bf16'):
            model = pivp_amd.Model(10, prefix='bench', device=dev, keep_activations=True, precision=precision, scheduled_sampling_k=-1)
            opt = pivp_amd.Adam(alpha=0.001).setup(model)
            np.random.seed(0)
            feeder = ds.DeviceFeeder(ds.SerialIterator(examples, B, repeat=True, shuffle=True), device=dev)
            batcher = ds.DeviceBatcher(dd, ds.SerialIterator(range(N), B, repeat=True, shuffle=True))
            resident = dd.gather(list(range(B)))

            class Resident(object):
                def get(self):
                    return resident, 0, False

                def prefetch(self):
                    pass
            feeds = {'device_feeder': feeder, 'device_batcher': batcher, 'resident_batch': Resident()}

            def loop(feed, n):
                itr = 0
                for k in range(2 + n):
                    if k == 2:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    x, _, _ = feed.get()
                    opt.update(model, x, itr)
                    feed.prefetch()
                    float(model.loss)                      # the step's host synchronisation
                    model.reset_state()
                    itr += 1
                return (time.perf_counter() - t0) / n * 1e3
            for feed in feeds.values():
                loop(feed, 2)
            series = {k: [] for k in feeds}
            for _ in range(args.rounds):
                for k, feed in feeds.items():
                    series[k].append(loop(feed, args.steps))
            rec = {k: stats(v) for k, v in series.items()}
            res, bat, fed = rec['resident_batch'], rec['device_batcher'], rec['device_feeder']
            rec['batcher_median_inside_resident_range'] = bool(res['min'] <= bat['median'] <= res['max'])
            rec['batcher_minus_resident_ms'] = round(bat['median'] - res['median'], 3)
            rec['feeder_over_resident'] = round(fed['median'] / res['median'], 3)
            rec['feeder_over_batcher'] = round(fed['median'] / bat['median'], 3)
            out['loop_ms_per_step'][precision] = rec
            del model, opt, feeder, batcher
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
