"""GPU tests of pivp_gather_batch (one training batch gathered out of a device-resident data set) and of `dataset.DeviceDataset` /
`dataset.DeviceBatcher` / `train --device_dataset 1` on top of it.  The oracle is `data.concat_examples` on the host arrays and every comparison
is `np.array_equal`: the gather moves bits (float32 storage) or produces the correctly rounded k / 255 (uint8 storage)."""
import os

import numpy as np
import pytest
import torch

from pivp_amd import dataset as ds
from pivp_amd import concat_examples
import gather_ops as GO

pytestmark = pytest.mark.gpu


def _set(N, T, H, W, storage, seed=0):
    """-> (what the device stores, float32 images as the host path sees them, actions, states)."""
    rs = np.random.RandomState(seed)
    act = rs.randn(N, T, 5).astype(np.float32)
    sta = rs.randn(N, T, 5).astype(np.float32)
    if storage == 'uint8':
        lev = rs.randint(0, 256, size=(N, T, H, W, 3)).astype(np.uint8)
        return lev, lev.astype(np.float32) / np.float32(255), act, sta
    img = rs.rand(N, T, H, W, 3).astype(np.float32)
    return img, img, act, sta


def _oracle(img, act, sta, idx):
    return concat_examples([[img[i], act[i], sta[i]] for i in idx])


def _same_bits(got, ref):
    return all(g.shape == r.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(r).view(np.uint32)) for g, r in zip(got, ref))


# (5, 7): no frame or plane base on 16 bytes; (33, 64): a ragged last band (2,112 = 2 x 1,024 + 64 pixels); the two product sizes
@pytest.mark.parametrize('storage', ['float32', 'uint8'])
@pytest.mark.parametrize('H,W', [(5, 7), (33, 64), (64, 64), (128, 128)])
def test_gather_equals_concat_examples(H, W, storage):
    rs = np.random.RandomState(H * 1000 + W)
    for T in (1, 3):
        for N in (1, 7):
            stored, img, act, sta = _set(N, T, H, W, storage, seed=T * 10 + N)
            on_device = [GO._dev(stored), GO._dev(act), GO._dev(sta)]           # uploaded once per set
            for B in (1, 2, 5, 32):
                drawn = rs.randint(0, N, size=B)                                  # repeats whenever B > N (and often otherwise)
                for idx in (drawn, np.sort(drawn)[::-1], np.arange(B)[::-1] % N):  # ... and two descending orders
                    got = GO.gather_batch(*on_device, idx)
                    assert _same_bits(got, _oracle(img, act, sta, idx)), (T, N, B, idx.tolist())


@pytest.mark.parametrize('H,W', [(16, 16), (10, 9)])      # 16-B path / element-wise path; 768 and 270 stored bytes: every level at least once
def test_every_uint8_level_is_the_correctly_rounded_quotient(H, W):
    lev = (np.arange(H * W * 3) % 256).astype(np.uint8).reshape(1, 1, H, W, 3)
    assert len(np.unique(lev)) == 256
    zero = np.zeros((1, 1, 5), np.float32)
    img = GO.gather_batch(lev, zero, zero, [0])[0]
    want = (lev.astype(np.float32) / np.float32(255))[0].transpose(0, 3, 1, 2)[:, None]       # (T, B, 3, H, W)
    assert img.shape == want.shape and np.array_equal(img.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    table = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(img.view(np.uint32), table[lev[0].transpose(0, 3, 1, 2)[:, None]].view(np.uint32))


@pytest.mark.parametrize('storage', ['float32', 'uint8'])
def test_same_bits_call_after_call_and_sentinels_intact(storage):
    stored, img, act, sta = _set(7, 3, 33, 64, storage)
    idx = [6, 0, 3, 3, 1]
    rc, a, intact_a = GO.gather_batch_rc(stored, act, sta, idx)
    rc2, b, intact_b = GO.gather_batch_rc(stored, act, sta, idx)
    assert rc == 0 and rc2 == 0 and intact_a and intact_b      # 4,096 sentinel floats behind each of the three outputs
    assert _same_bits(a, b) and _same_bits(a, _oracle(img, act, sta, idx))


def test_offsets_into_a_set_larger_than_4_gib():
    T, H, W = 3, 64, 64
    N = 2 ** 32 // (T * H * W * 3) + 100
    assert N * T * H * W * 3 > 2 ** 32
    frames = torch.empty((N, T, H, W, 3), dtype=torch.uint8, device=GO.DEV)      # no fill: only the three gathered sequences are written
    actions = torch.empty((N, T, 5), dtype=torch.float32, device=GO.DEV)
    states = torch.empty((N, T, 5), dtype=torch.float32, device=GO.DEV)
    idx = [0, N // 2, N - 1]
    lev, img, act, sta = _set(3, T, H, W, 'uint8', seed=9)
    for j, i in enumerate(idx):
        frames[i] = torch.from_numpy(lev[j]).to(GO.DEV)
        actions[i] = torch.from_numpy(act[j]).to(GO.DEV)
        states[i] = torch.from_numpy(sta[j]).to(GO.DEV)
    got = GO.gather_batch(frames, actions, states, idx[::-1])
    assert _same_bits(got, _oracle(img, act, sta, [2, 1, 0]))


def test_bad_arguments_return_badarg_and_write_nothing():
    stored, img, act, sta = _set(3, 2, 8, 8, 'float32')
    bad = [dict(null=k) for k in ('frames', 'actions', 'states', 'index', 'out_images', 'out_actions', 'out_states')]
    bad += [dict(B=0), dict(N=0), dict(T=0), dict(H=0), dict(W=-1), dict(frames_u8=2)]
    for kw in bad:
        rc, outs, intact = GO.gather_batch_rc(stored, act, sta, [2, 0], **kw)
        assert rc == -1 and intact and all((o == GO.SENTINEL).all() for o in outs), kw
    rc, outs, intact = GO.gather_batch_rc(stored, act, sta, [], B=0)
    assert rc == -1 and intact
    rc, outs, intact = GO.gather_batch_rc(stored, act, sta, [2, 0])               # the same call with good arguments runs
    assert rc == 0 and intact and _same_bits(outs, _oracle(img, act, sta, [2, 0]))


@pytest.mark.parametrize('storage', ['float32', 'uint8', 'auto'])
def test_device_dataset_gather_and_attributes(storage):
    stored, img, act, sta = _set(7, 3, 33, 64, 'uint8')
    dd = ds.DeviceDataset(img, act, sta, GO.DEV, storage=storage, chunk=3)        # three chunks through the staging buffer
    held = 'float32' if storage == 'float32' else 'uint8'
    assert (dd.N, dd.T, dd.H, dd.W, dd.storage) == (7, 3, 33, 64, held)
    assert dd.nbytes == 7 * 3 * (33 * 64 * 3 * (4 if held == 'float32' else 1) + 40)
    idx = np.array([5, 5, 0, 6])
    got = dd.gather(idx)
    assert _same_bits([g.cpu().numpy() for g in got], _oracle(img, act, sta, idx))
    out = [torch.full_like(g, -1.0) for g in got]
    again = dd.gather(idx.tolist(), out=out)
    assert all(a.data_ptr() == o.data_ptr() for a, o in zip(again, out)) and all(torch.equal(a, g) for a, g in zip(again, got))
    with pytest.raises(ValueError):
        dd.gather([0, 7])
    with pytest.raises(ValueError):
        dd.gather(idx, out=[o[:, :2].contiguous() for o in out])
    off_grid = ds.DeviceDataset(_set(2, 1, 5, 7, 'float32')[0], act[:2, :1], sta[:2, :1], GO.DEV)      # 'auto' on arbitrary floats
    assert off_grid.storage == 'float32'


def test_gather_and_batcher_never_synchronise():
    stored, img, act, sta = _set(7, 4, 64, 64, 'uint8')
    dd = ds.DeviceDataset(img, act, sta, GO.DEV, storage='uint8')
    batcher = ds.DeviceBatcher(dd, ds.SerialIterator(range(7), 2, repeat=True, shuffle=False))      # five batches of 2 out of 7: one epoch boundary
    plain = ds.SerialIterator(range(7), 2, repeat=True, shuffle=False)
    warm = dd.gather([1, 2])                         # the library, the index buffers and the allocator's blocks exist from here on
    torch.cuda.synchronize()
    probe = torch.ones(1, device=GO.DEV)
    kept = []
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        one = dd.gather([1, 2])
        for _ in range(5):
            x, epoch, new_epoch = batcher.get()
            kept.append([t.clone() for t in x])      # the batcher reuses its buffers
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert detects, 'torch.cuda.set_sync_debug_mode("error") does not flag .item() on this torch build: the no-sync assertion cannot be made'
    assert all(torch.equal(a, b) for a, b in zip(one, warm))
    for x in kept:
        assert _same_bits([t.cpu().numpy() for t in x], _oracle(img, act, sta, plain.next()))


@pytest.mark.parametrize('storage', ['float32', 'uint8'])
def test_device_batcher_matches_device_feeder(storage):
    """Same seed, 7 sequences of T = 4 at 64 x 64, batches of 2, 9 steps across epoch boundaries: every batch bit-identical, every
    (epoch, is_new_epoch) equal -- on one rank and on each of two (no process group: a rank is a slice)."""
    stored, img, act, sta = _set(7, 4, 64, 64, 'uint8', seed=2)
    dd = ds.DeviceDataset(img, act, sta, GO.DEV, storage=storage)
    for world in (1, 2):
        for rank in range(world):
            np.random.seed(11)
            feeder = ds.DeviceFeeder(ds.SerialIterator(ds.group_examples(img, act, sta), 2, repeat=True, shuffle=True), rank=rank, world=world,
                                     device=GO.DEV)
            fed = []
            for step in range(9):
                x, epoch, new_epoch = feeder.get()
                fed.append(([t.cpu().numpy() for t in x], epoch, new_epoch, np.random.rand()))      # the step's own draws from the global RNG
                if step + 1 < 9:
                    feeder.prefetch()
            np.random.seed(11)
            batcher = ds.DeviceBatcher(dd, ds.SerialIterator(range(7), 2, repeat=True, shuffle=True), rank=rank, world=world)
            for step in range(9):
                x, epoch, new_epoch = batcher.get()
                draw = np.random.rand()
                batcher.prefetch()
                ref, e0, n0, d0 = fed[step]
                assert (epoch, new_epoch, draw) == (e0, n0, d0), (world, rank, step)
                assert x[0].shape == (4, 2 // world, 3, 64, 64) and _same_bits([t.cpu().numpy() for t in x], ref), (world, rank, step)
            assert [f[2] for f in fed].count(True) == 2


def _make_grid_dataset(root, n=6, T=4):
    rs = np.random.RandomState(0)
    rows = []
    for j in range(n):
        lev = rs.randint(0, 256, size=(T, 64, 64, 3)).astype(np.float32)
        np.save(os.path.join(root, 'image_batch_%d' % j), lev / np.float32(255))
        np.save(os.path.join(root, 'action_batch_%d' % j), (rs.randn(T, 5) * 0.1).astype(np.float32))
        np.save(os.path.join(root, 'state_batch_%d' % j), (rs.randn(T, 5) * 0.1).astype(np.float32))
        rows.append([j, '', 'image_batch_%d.npy' % j, 'action_batch_%d.npy' % j, 'state_batch_%d.npy' % j, '', ''])
    ds.write_map(root, rows)


def _checkpoints(d):
    return sorted(f for f in os.listdir(d) if f.split('-')[0] in ('training', 'state') and f.split('-', 1)[1][:1].isdigit())


def test_train_main_writes_the_same_checkpoints_from_either_feed(tmp_path):
    from pivp_amd import train as T
    data = tmp_path / 'data'
    data.mkdir()
    _make_grid_dataset(str(data))
    dirs = []
    for r, feed in enumerate((['--device_dataset', '0'], ['--device_dataset', '1', '--device_storage', 'float32'],
                              ['--device_dataset', '1', '--device_storage', 'uint8'])):
        out = tmp_path / ('models%d' % r)
        out.mkdir()
        dirs.append(T.main(['--data_dir', str(data), '--output_dir', str(out), '--num_iterations', '4', '--batch_size', '2', '--schedsamp_k', '900',
                            '--save_interval', '1', '--validation_interval', '1', '--train_val_split', '0.7', '--deterministic', '1'] + feed))
    files = _checkpoints(dirs[0])
    assert any(f.startswith('training-') for f in files) and any(f.startswith('state-') for f in files)
    for other in dirs[1:]:
        assert _checkpoints(other) == files
        for f in files:
            with np.load(os.path.join(dirs[0], f)) as a, np.load(os.path.join(other, f)) as b:
                assert sorted(a.files) == sorted(b.files)
                for k in a.files:
                    assert np.array_equal(a[k], b[k]), '%s: %s differs between the host feed and %s' % (f, k, other)
        for f in ('training-global_losses.npy', 'training-global_losses_valid.npy'):
            assert np.array_equal(np.load(os.path.join(dirs[0], f)), np.load(os.path.join(other, f))), f


def test_evaluate_walks_the_device_resident_raw_frames(tmp_path):
    """`evaluate --device_dataset 1` over predict's raw frames (column 6 of map.csv, levels 0..255 at 96 x 120): held as float32 the walk writes the
    host walk's arrays bit for bit (the gather copies the levels, the resize scales by 1/255 as before); held as uint8 the gather hands back
    k / 255 and the resize scales by 1, so a frame may move by a few roundings, bounded below on the frames themselves."""
    import pivp_amd
    from oracle import restatement as R
    from pivp_amd import evaluate as E, _lib
    from pivp_amd.predict import resize_images
    data = tmp_path / 'data'; data.mkdir()
    mdir = tmp_path / 'models' / '20240101-000000-CDNA-2'; mdir.mkdir(parents=True)
    rs = np.random.RandomState(0)
    rows = []
    for j in range(5):
        np.save(str(data / ('action_%d' % j)), (rs.randn(4, 5) * 0.1).astype(np.float32))
        np.save(str(data / ('state_%d' % j)), (rs.randn(4, 5) * 0.1).astype(np.float32))
        np.save(str(data / ('pred_%d' % j)), (rs.rand(4, 96, 120, 3) * 255).astype(np.uint8))
        rows.append([j, '', 'pred_%d.npy' % j, 'action_%d.npy' % j, 'state_%d.npy' % j, '', 'pred_%d.npy' % j])
    ds.write_map(str(data), rows)
    m = pivp_amd.Model(10, prefix='e')
    m.load_state_dict_reference(R.init_params_widened(seed=1, scale=1.0))
    pivp_amd.save_npz(str(mdir / 'training-0'), m)
    base = [mdir.name, 'training-0', '1', '--models_dir', str(tmp_path / 'models'), '--data_dir', str(data), '--batch_size', '2', '--max_sequences', '3']
    got = {}
    for name, extra in (('host', []), ('float32', ['--device_dataset', '1', '--device_storage', 'float32']),
                        ('uint8', ['--device_dataset', '1', '--device_storage', 'uint8']), ('auto', ['--device_dataset', '1'])):
        out = str(tmp_path / ('metrics-%s.npz' % name))
        E.main(base + extra + ['--out', out])
        with np.load(out) as z:
            got[name] = {k: z[k] for k in z.files}
    for k, v in got['host'].items():
        assert np.array_equal(got['float32'][k], v), k                      # bit for bit
        assert np.array_equal(got['uint8'][k], got['auto'][k]), k           # 'auto' holds raw 8-bit frames as uint8
        assert got['uint8'][k].shape == v.shape and np.isfinite(got['uint8'][k][np.isfinite(v)]).all(), k
    assert got['uint8']['count'].tolist() == got['host']['count'].tolist() == [3, 3]
    # the frames the uint8 walk feeds the model against the host walk's: level k reaches the bilinear resize as fl(k / 255) instead of the result
    # being scaled by fl(1 / 255).  Either way a frame value in [0, 1] is a convex combination of four levels with one rounding per level
    # (<= 2^-24 relative), the interpolation's own roundings (the same <= 4 operations in both forms, <= 2^-24 each of a value <= 1) and, in the
    # host form, the scale's two roundings: the two differ by less than 8 * 2^-24
    dset = ds.DeviceDataset.from_dir(str(data), GO.DEV, storage='uint8', raw=True)
    assert (dset.storage, dset.scale, dset.H, dset.W) == ('uint8', 1.0, 96, 120)
    assert ds.DeviceDataset.from_dir(str(data), GO.DEV, storage='float32', raw=True).scale == 1.0 / 255.0
    img = dset.gather([1, 2])[0]
    small = torch.empty((4, 2, 3, 64, 64), dtype=torch.float32, device=GO.DEV)
    _lib.check(_lib.load().pivp_resize_images(img.data_ptr(), small.data_ptr(), 4 * 2 * 3, 96, 120, 64, 64, dset.scale, GO.stream()), 'pivp_resize_images')
    raw = np.stack([np.float32(np.load(str(data / ('pred_%d.npy' % j)))) for j in (1, 2)]).transpose(1, 0, 4, 2, 3)
    host = torch.stack([resize_images(raw[t], (64, 64), GO.DEV, 1.0 / 255.0) for t in range(4)])
    diff = float((small - host).abs().max())
    print('uint8 walk: frames differ from the host walk by at most %.3e (bound %.3e)' % (diff, 8 * 2.0 ** -24))
    assert diff < 8 * 2.0 ** -24
    with pytest.raises(ValueError, match='sequence 0 '):                    # frames in [0, 1] are no raw levels
        ds.FrameStorage('uint8', raw=True).encode(np.full((1, 1, 2, 2, 3), 0.5, np.float32))
