"""CPU tests of the host side of the device-resident data set (dataset.DeviceDataset / DeviceBatcher): the rule that admits uint8 storage, index and
shape validation, the iterator over sequence numbers, rank slices, and the command-line flags.  No GPU, no library."""
import numpy as np
import pytest

import pivp_amd
from pivp_amd import dataset as ds

LEVELS = np.arange(256, dtype=np.float32) / np.float32(255)


def _frames(values, n=1):
    """(n, 1, 2, 128, 3) frames filled with `values` (768 numbers per sequence)."""
    return np.resize(np.asarray(values, dtype=np.float32), (n, 1, 2, 128, 3)).copy()


def test_uint8_storage_takes_exactly_the_k_over_255_grid():
    k, bad = ds.uint8_levels(_frames(LEVELS))
    assert bad is None and k.dtype == np.uint8 and np.array_equal(k.ravel()[:256], np.arange(256))      # all 256 levels survive the round trip
    assert np.array_equal(k.astype(np.float32) / np.float32(255), _frames(LEVELS))
    for policy in ('uint8', 'auto'):
        st = ds.FrameStorage(policy)
        enc = st.encode(_frames(LEVELS))
        assert st.storage == 'uint8' and enc.dtype == np.uint8 and st.dtype == np.uint8
    one_ulp = np.nextafter(LEVELS[100], np.float32(1))
    for off in (one_ulp, np.float32(0.5), np.float32(1) / np.float32(254), np.float32(-1) / np.float32(255), np.float32(256) / np.float32(255),
                np.float32('nan'), np.float32('inf')):
        x = _frames(LEVELS, n=3)
        x[1, 0, 1, 77, 2] = off                                       # one pixel of sequence 1
        assert ds.uint8_levels(x) == (None, 1)
        with pytest.raises(ValueError, match='sequence 11 '):         # named by its number in the set: the chunk starts at 10
            ds.FrameStorage('uint8').encode(x, first=10)
        st = ds.FrameStorage('auto')
        enc = st.encode(x)
        assert st.storage == 'float32' and enc.dtype == np.float32 and np.array_equal(enc, x, equal_nan=True)
        assert ds.FrameStorage('float32').encode(x).dtype == np.float32
    with pytest.raises(ValueError, match='storage'):
        ds.FrameStorage('fp16')


def test_auto_storage_contradicted_by_a_later_chunk_raises():
    st = ds.FrameStorage('auto')
    assert st.storage is None
    st.encode(_frames(LEVELS, n=4), first=0)
    assert st.storage == 'uint8'
    assert st.encode(_frames(LEVELS[::-1], n=4), first=4).dtype == np.uint8
    later = _frames(LEVELS, n=4)
    later[2] += np.float32(1e-3)
    with pytest.raises(ValueError, match=r"sequence 10 .*storage='float32'"):
        st.encode(later, first=8)
    # decided float32 first: anything goes afterwards
    st = ds.FrameStorage('auto')
    st.encode(later)
    assert st.storage == 'float32' and st.encode(_frames(LEVELS)).dtype == np.float32


def test_validation_errors_need_neither_gpu_nor_library(monkeypatch):
    import torch
    from pivp_amd import _lib

    def boom(*a, **k):
        raise AssertionError('validation must come first')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(torch.cuda, 'mem_get_info', boom)
    monkeypatch.setattr(torch.cuda, 'current_stream', boom)
    img, act, sta = np.zeros((4, 3, 8, 8, 3), np.float32), np.zeros((4, 3, 5), np.float32), np.zeros((4, 3, 5), np.float32)
    for bad in ((img[..., :2], act, sta), (img[0], act, sta), (img, act[:3], sta), (img, act, sta[:, :2]), (img, act[..., :4], sta),
                (img[:0], act[:0], sta[:0])):
        with pytest.raises(ValueError):
            ds.DeviceDataset(*bad, device='cuda:0')
    with pytest.raises(ValueError, match='storage'):
        ds.DeviceDataset(img, act, sta, device='cuda:0', storage='int8')
    with pytest.raises(ValueError, match='no CPU path'):
        ds.DeviceDataset(img, act, sta, device='cpu')
    with pytest.raises(ValueError, match='sequence 0 '):               # 'uint8' on frames off the grid: refused before anything is allocated
        ds.DeviceDataset(img + np.float32(0.3), act, sta, device='cuda:0', storage='uint8')
    # indices: gather() validates them first
    dd = ds.DeviceDataset.__new__(ds.DeviceDataset)
    dd.N, dd.T, dd.H, dd.W = 4, 3, 8, 8
    for bad in ([], [4], [-1, 0], [0.0, 1.0], [[0, 1]], [True, False], 2):
        with pytest.raises(ValueError):
            dd.gather(bad)
        with pytest.raises(ValueError):
            ds.check_indices(bad, 4)
    ok = ds.check_indices([3, 0, 3], 4)
    assert ok.dtype == np.int32 and ok.tolist() == [3, 0, 3] and ds.check_indices(np.array([1], np.int64), 4).dtype == np.int32
    assert ds.check_set_shapes(img.shape, act.shape, sta.shape) == (4, 3, 8, 8)


def test_iterator_over_sequence_numbers_draws_the_examples_order():
    """A SerialIterator over range(N) and one over the examples consume the global RNG alike: N = 7, batches of 2, 9 draws across two epoch
    boundaries; and a repeat=False pass."""
    N = 7
    rs = np.random.RandomState(0)
    img, act, sta = rs.rand(N, 2, 4, 4, 3).astype(np.float32), rs.randn(N, 2, 5).astype(np.float32), rs.randn(N, 2, 5).astype(np.float32)
    examples = ds.group_examples(img, act, sta)
    for repeat, draws in ((True, 9), (False, 4)):
        runs = []
        for dataset in (examples, range(N)):
            np.random.seed(21)
            it = ds.SerialIterator(dataset, 2, repeat=repeat, shuffle=True)
            log = []
            for _ in range(draws):
                epoch = it.epoch
                log.append((it.next(), epoch, it.epoch, it.is_new_epoch, it.current_position))
            if not repeat:
                with pytest.raises(StopIteration):
                    it.next()
            runs.append((log, np.random.rand()))                      # ... and the global RNG is left in the same state
        (by_example, ra), (by_number, rb) = runs
        assert ra == rb and sum(l[3] for l in by_number) == (2 if repeat else 1)
        for (xa, *ka), (xb, *kb) in zip(by_example, by_number):
            assert ka == kb and len(xa) == len(xb) and all(0 <= int(j) < N for j in xb)
            assert all(np.array_equal(x[0], img[j]) and np.array_equal(x[1], act[j]) and np.array_equal(x[2], sta[j]) for x, j in zip(xa, xb))
    # the split: two ranges over one set, k as in split_train_val
    tr, va = ds.split_index_ranges(N, 0.7)
    (ti, _, _), (vi, _, _) = ds.split_train_val(img, act, sta, 0.7)
    assert (len(tr), len(va)) == (len(ti), len(vi)) and list(tr) + list(va) == list(range(N))
    assert np.array_equal(img[list(va)], vi)


def test_rank_slices_equal_the_feeders():
    N, B = 8, 4
    rs = np.random.RandomState(1)
    img, act, sta = rs.rand(N, 2, 4, 4, 3).astype(np.float32), rs.randn(N, 2, 5).astype(np.float32), rs.randn(N, 2, 5).astype(np.float32)
    for world in (1, 2, 4):
        for rank in range(world):
            np.random.seed(8)
            feeder = ds.DeviceFeeder(ds.SerialIterator(ds.group_examples(img, act, sta), B, repeat=True, shuffle=True), rank=rank, world=world,
                                     device='cpu')
            fed = []
            for _ in range(5):                                        # 8 sequences, batches of 4: epoch boundaries, reshuffles from the global RNG
                fed.append(feeder.get()[0])
                feeder.prefetch()
            np.random.seed(8)
            numbers = ds.SerialIterator(range(N), B, repeat=True, shuffle=True)
            for x in fed:
                mine = ds.rank_slice(numbers.next(), rank, world)
                assert len(mine) == B // world
                ref = pivp_amd.concat_examples([[img[j], act[j], sta[j]] for j in mine])
                assert all(np.array_equal(t.numpy(), r) for t, r in zip(x, ref))
    with pytest.raises(ValueError, match='not divisible'):
        ds.rank_slice([0, 1, 2], 0, 2)


def test_parsers_have_the_flags_and_default_to_the_host_feed():
    from pivp_amd import train, evaluate
    for parser, argv in ((train.build_parser(), []), (evaluate.build_parser(), ['20170101-000000-CDNA-32', 'training-0'])):
        a = parser.parse_args(argv)
        assert a.device_dataset == 0 and a.device_storage == 'auto'
        b = parser.parse_args(argv + ['--device_dataset', '1', '--device_storage', 'uint8'])
        assert b.device_dataset == 1 and b.device_storage == 'uint8'
        for bad in (['--device_dataset', '2'], ['--device_storage', 'fp16']):
            with pytest.raises(SystemExit):
                parser.parse_args(argv + bad)
    assert pivp_amd.DeviceDataset is ds.DeviceDataset and pivp_amd.DeviceBatcher is ds.DeviceBatcher


def test_data_header_library_and_ctypes_table_agree():
    """The data feed's entry points have a header of their own, include/pivp_data.h, and a table of their own, `_lib.DATA_SIGNATURES`: the model's
    ABI (include/pivp_hip.h against `_lib.SIGNATURES`, tests/test_host.py) stays as it was, version included."""
    import os
    import re
    import subprocess
    import __graft_entry__ as g
    from pivp_amd import _lib, _digest, build
    g.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(root, 'include', 'pivp_data.h')).read()))
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.DATA_SIGNATURES) == {'pivp_gather_batch'} and declared <= exported
    assert not declared & set(_lib.SIGNATURES)
    res, args = _lib.DATA_SIGNATURES['pivp_gather_batch']
    assert res is _lib._i and args == [_lib._vp, _lib._i] + [_lib._vp] * 3 + [_lib._i, _lib._ll] + [_lib._i] * 3 + [_lib._vp] * 4
    lib = _lib.load()
    assert lib.pivp_gather_batch.argtypes == args and lib.pivp_abi_version() == 17
    assert 'batch_gather.hip' in build.SOURCES and 'pivp_data.h' in [os.path.basename(f) for f in _digest.source_files()]
