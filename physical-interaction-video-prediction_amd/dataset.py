"""On-disk dataset of the reference and the host-side feed of its training loop.

Format (written by the reference's src/data/make_dataset.py:130-158, read at train_model.py:813-834 and
predict_model.py:30-51): `<data_dir>/map.csv`, every field quoted, header
`id,img_bitmap_path,img_np_path,action_np_path,state_np_path,img_bitmap_pred_path,img_np_pred_path`, one row per sequence;
columns 2/3/4 name per-sequence `.npy` files relative to data_dir: images (T,H,W,3) float32 in [0,1], actions (T,5),
states (T,5); column 6 the raw uint8 frames used by predict.  The split is by index, no shuffle (train_model.py:836-843).

Two feeds of the training loop: `DeviceFeeder` (the default: the set in host RAM, every batch laid out by `concat_examples` and copied) and, opt-in,
`DeviceDataset` + `DeviceBatcher` (the set in HBM as the files hold it, every batch one pivp_gather_batch launch)."""
import csv
import os

import numpy as np

MAP_HEADER = ['id', 'img_bitmap_path', 'img_np_path', 'action_np_path', 'state_np_path', 'img_bitmap_pred_path', 'img_np_pred_path']


def read_map(data_dir):
    """Rows of map.csv without the header; raises ValueError("No file map found") like predict_model.py:37-38."""
    path = os.path.join(data_dir, 'map.csv')
    with open(path, 'r', newline='') as f:
        rows = [r for r in csv.reader(f)]
    if len(rows) <= 1:
        raise ValueError("No file map found")
    return rows[1:]


def write_map(data_dir, rows):
    """Write map.csv the way make_dataset.py:153-158 does (QUOTE_ALL, same header)."""
    with open(os.path.join(data_dir, 'map.csv'), 'w', newline='') as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(MAP_HEADER)
        for r in rows:
            w.writerow(r)


def load_dataset(data_dir):
    """train_model.py:826-834: every sequence into RAM as float32: images (N,T,H,W,3), actions (N,T,A), states (N,T,S) -- whatever widths
    the files hold (5 / 5 in the push data set)."""
    rows = read_map(data_dir)
    images = np.asarray([np.float32(np.load(os.path.join(data_dir, r[2]))) for r in rows], dtype=np.float32)
    actions = np.asarray([np.float32(np.load(os.path.join(data_dir, r[3]))) for r in rows], dtype=np.float32)
    states = np.asarray([np.float32(np.load(os.path.join(data_dir, r[4]))) for r in rows], dtype=np.float32)
    return images, actions, states


def split_train_val(images, actions, states, train_val_split=0.95):
    """train_model.py:836-843: first floor(split * N) sequences train, the rest validate."""
    k = int(np.floor(train_val_split * len(images)))
    return (images[:k], actions[:k], states[:k]), (images[k:], actions[k:], states[k:])


def group_examples(images, actions, states):
    """train_model.py:899-911: list of [images, actions, states] per sequence (what the iterator serves)."""
    return [[images[i], actions[i], states[i]] for i in range(len(images))]


def get_data_info(data_dir, data_index):
    """predict_model.py:30-51: (image, image_pred, image_bitmap_pred, action, state) of one sequence."""
    rows = read_map(data_dir)
    data_index = int(data_index)
    if data_index > len(rows) - 1:
        raise ValueError("Data index {} is out of range for available data".format(data_index + 1))
    r = rows[data_index]
    image = np.float32(np.load(os.path.join(data_dir, r[2])))
    image_pred = np.float32(np.load(os.path.join(data_dir, r[6])))
    action = np.float32(np.load(os.path.join(data_dir, r[3])))
    state = np.float32(np.load(os.path.join(data_dir, r[4])))
    return image, image_pred, r[5], action, state


class SerialIterator(object):
    """chainer.iterators.SerialIterator (2.0.x) as used at train_model.py:914-915: a permutation drawn from NumPy's global
    RNG at reset, reshuffled in place at every epoch boundary; with repeat=True the last batch of an epoch is completed
    from the start of the next one."""

    def __init__(self, dataset, batch_size, repeat=True, shuffle=True):
        self.dataset = dataset
        self.batch_size = batch_size
        self._repeat = repeat
        self._shuffle = shuffle
        self.reset()

    def reset(self):
        self._order = np.random.permutation(len(self.dataset)) if self._shuffle else None
        self.current_position = 0
        self.epoch = 0
        self.is_new_epoch = False

    def __iter__(self):
        return self

    def __next__(self):
        if not self._repeat and self.epoch > 0:
            raise StopIteration
        i = self.current_position
        i_end = i + self.batch_size
        N = len(self.dataset)
        pick = (lambda a, b: [self.dataset[j] for j in range(a, min(b, N))]) if self._order is None else \
               (lambda a, b: [self.dataset[j] for j in self._order[a:b]])
        batch = pick(i, i_end)
        if i_end >= N:
            if self._repeat:
                rest = i_end - N
                if self._order is not None:
                    np.random.shuffle(self._order)
                if rest > 0:
                    batch.extend(pick(0, rest))
                self.current_position = rest
            else:
                self.current_position = 0
            self.epoch += 1
            self.is_new_epoch = True
        else:
            self.is_new_epoch = False
            self.current_position = i_end
        return batch

    next = __next__


class DeviceFeeder(object):
    """Overlapped host feed of the training loop (the reference's loop, train_model.py:937-950, is synchronous: `concat_examples`
    and the host -> device copy of every batch sit between two `optimizer.update` calls).

    Two slots, each a set of PINNED host buffers and a set of device buffers.  `get()` hands out batch t on the device (the caller's
    stream is made to wait for its copy) together with the iterator's bookkeeping AS IT WAS when batch t was drawn; `prefetch()`,
    called right after the step of batch t has been enqueued, draws batch t + 1 from the iterator, runs `concat_examples` and the
    rank's shard slice into the other slot's pinned buffers and starts the copy on a second stream, so both run under the GPU's work
    on batch t.  The iterator is advanced exactly as a plain `iterator.next()` loop would advance it, one batch early: order of the
    batches, shards, `epoch` and `is_new_epoch` are unchanged (tests/test_dataset_host.py).  With device='cpu' (tests) the slots are
    plain host tensors and the copy is a memcpy.

    Slot reuse: the copy into a slot's DEVICE buffers waits for an event recorded on the caller's stream when the batch AFTER the
    slot's previous occupant was handed out (its step is enqueued before that), the write into its PINNED buffers for the event of
    its previous copy.

    INVARIANT the caller keeps (train.py does): `get()` returns the slot's OWN device buffers -- `Model.__call__` keeps their addresses,
    it does not copy -- and they are overwritten by the copy stream once the `get()` after next has run.  So every kernel that reads
    a batch must have been enqueued on, or joined into, the stream that is current at the following `get()`: `Model.__call__` /
    `Model.backward` / `Adam.update` satisfy that (the plan's side stream is joined into the caller's stream before
    `pivp_rollout_backward` returns, the all-reduce's stream before `update` returns).  A caller that runs the model on ANOTHER stream
    than the one current at `get()`, or that catches a failed `update()` and carries on, must `clone()` the batch (or synchronise the
    device) before it asks for the next but one.  `tests/test_gpu_pipeline.py::test_device_feeder_matches_the_synchronous_loop` runs the
    fed loop against the synchronous one."""

    def __init__(self, iterator, rank=0, world=1, device='cuda:0'):
        import torch
        self._torch = torch
        self.iterator = iterator
        self.rank, self.world = int(rank), int(world)
        self.device = torch.device(device)
        self.cuda = self.device.type == 'cuda'
        self._slots = [None, None]
        self._staged = None           # (slot index, epoch when drawn, is_new_epoch after the draw) of the batch waiting for get()
        self._count = 0
        self._copy_stream = torch.cuda.Stream(device=self.device) if self.cuda else None
        self._exhausted = False

    def _slot(self, k, arrays):
        torch = self._torch
        sl = self._slots[k]
        if sl is None or any(tuple(h.shape) != a.shape for h, a in zip(sl['host'], arrays)):
            host = [torch.empty(a.shape, dtype=torch.float32, pin_memory=self.cuda) for a in arrays]
            dev = [torch.empty(a.shape, dtype=torch.float32, device=self.device) for a in arrays] if self.cuda else host
            sl = self._slots[k] = dict(host=host, dev=dev, copied=None, consumed=None)
        return sl

    def prefetch(self):
        """Draw the next batch and start its journey to the device.  No-op when one is already staged or the iterator has ended."""
        if self._staged is not None or self._exhausted:
            return
        from .data import concat_examples
        torch = self._torch
        epoch = self.iterator.epoch
        try:
            batch = self.iterator.next()
        except StopIteration:
            self._exhausted = True
            return
        new_epoch = self.iterator.is_new_epoch
        img, act, sta = concat_examples(batch)
        B = img.shape[1]
        if B % self.world:
            raise ValueError('batch of %d sequences is not divisible by %d ranks' % (B, self.world))
        per = B // self.world
        lo = self.rank * per
        arrays = [a[:, lo:lo + per] for a in (img, act, sta)]
        k = self._count % 2
        self._count += 1
        sl = self._slot(k, arrays)
        if sl['copied'] is not None:
            sl['copied'].synchronize()              # the previous copy OUT of these pinned buffers has finished (two batches ago)
        for h, a in zip(sl['host'], arrays):
            np.copyto(h.numpy(), a)
        if self.cuda:
            with torch.cuda.stream(self._copy_stream):
                if sl['consumed'] is not None:
                    self._copy_stream.wait_event(sl['consumed'])
                for h, d in zip(sl['host'], sl['dev']):
                    d.copy_(h, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            sl['copied'] = ev
        self._staged = (k, epoch, new_epoch)

    def get(self):
        """-> ([images (T,B/world,3,H,W), actions, states] on the device, epoch at the draw, is_new_epoch after the draw)."""
        torch = self._torch
        if self._staged is None:
            self.prefetch()
        if self._staged is None:
            raise StopIteration
        k, epoch, new_epoch = self._staged
        self._staged = None
        sl = self._slots[k]
        if self.cuda:
            main = torch.cuda.current_stream(self.device)
            main.wait_event(sl['copied'])
            other = self._slots[1 - k]
            if other is not None:                   # everything enqueued so far used the OTHER slot's batch at the latest
                ev = torch.cuda.Event()
                ev.record(main)
                other['consumed'] = ev
            return list(sl['dev']), epoch, new_epoch
        return [t.clone() for t in sl['host']], epoch, new_epoch


# ---- the data set on the device ------------------------------------------------------------------------------------------------------
STORAGES = ('auto', 'float32', 'uint8')


def uint8_levels(images, raw=False):
    """Frames in [0, 1] -> (their uint8 levels k, None) when EVERY pixel x is exactly np.float32(k) / np.float32(255) with k = rint(255 x) in
    0..255 -- the value pivp_gather_batch hands back for level k, so storing k loses nothing --, else (None, index along axis 0 of the first
    entry with a pixel that is not).  raw: the frames ARE levels (predict's raw frames, 0..255): every x must be an integer k in 0..255."""
    x = np.asarray(images, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        k = np.rint(x if raw else x * np.float32(255))
        ok = (k >= 0) & (k <= 255)                                # NaN and +-inf fail here
        k = np.where(ok, k, 0).astype(np.uint8)
        ok &= (k.astype(np.float32) if raw else k.astype(np.float32) / np.float32(255)) == x
    if ok.all():
        return k, None
    return None, int(np.argmin(ok.reshape(len(x), -1).all(axis=1)))


class FrameStorage(object):
    """How a DeviceDataset holds its frames, decided chunk by chunk on the host: 'float32' (always allowed, a copy), 'uint8' (a quarter of the
    bytes; only for frames on the k / 255 grid, see `uint8_levels`) or 'auto' (uint8 if the FIRST chunk allows it; a later chunk that does not
    is an error, the set is half uploaded by then).  raw: see `uint8_levels`."""

    def __init__(self, storage='auto', raw=False):
        if storage not in STORAGES:
            raise ValueError('storage must be one of %s, got %r' % (', '.join(STORAGES), storage))
        self.requested = storage
        self.raw = bool(raw)
        self.storage = None if storage == 'auto' else storage     # None: not decided yet

    @property
    def dtype(self):
        return np.uint8 if self.storage == 'uint8' else np.float32

    def encode(self, images, first=0):
        """One chunk of frames (n, T, H, W, 3), sequence numbers first .. first + n - 1 -> the array to store (uint8 levels or float32)."""
        x = np.asarray(images, dtype=np.float32)
        if self.storage == 'float32':
            return x
        k, bad = uint8_levels(x, self.raw)
        if self.storage is None:
            self.storage = 'uint8' if k is not None else 'float32'
            return k if k is not None else x
        if k is None:
            if self.requested == 'auto':
                raise ValueError("storage='auto' chose uint8 from the first sequences, but sequence %d has pixels that are not k/255 levels: "
                                 "pass storage='float32'" % (first + bad))
            raise ValueError("storage='uint8' needs every pixel to be np.float32(k) / np.float32(255) for an integer k in 0..255; sequence %d "
                             "has others (use storage='float32')" % (first + bad))
        return k


def check_indices(indices, N):
    """Sequence numbers of one batch -> contiguous int32 array; ValueError unless they are B >= 1 integers in [0, N)."""
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.size < 1:
        raise ValueError('a batch is a non-empty 1-d list of sequence numbers, got shape %s' % (idx.shape,))
    if idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError('sequence numbers must be integers, got %s' % idx.dtype)
    if int(idx.min()) < 0 or int(idx.max()) >= N:
        raise ValueError('sequence numbers must lie in [0, %d), got %d .. %d' % (N, int(idx.min()), int(idx.max())))
    return np.ascontiguousarray(idx, dtype=np.int32)


DEVICE_WIDTH = 5      # pivp_gather_batch copies five columns of an action and of a state (include/pivp_data.h)


def check_device_widths(action_dim, state_dim):
    """The device-resident feed serves the reference data's widths alone; every other width goes through the host feed (`load_dataset`,
    `concat_examples`, `DeviceFeeder`), which serves any."""
    if (action_dim, state_dim) != (DEVICE_WIDTH, DEVICE_WIDTH):
        raise ValueError('a DeviceDataset holds actions and states of width 5 (the on-device gather copies five columns), got action_dim=%s, '
                         'state_dim=%s: use the host feed for other widths' % (action_dim, state_dim))


def check_set_shapes(images_shape, actions_shape, states_shape):
    """-> (N, T, H, W) of a data set with images (N,T,H,W,3), actions (N,T,5), states (N,T,5); ValueError otherwise."""
    if len(images_shape) != 5 or images_shape[4] != 3 or min(images_shape) < 1:
        raise ValueError('images must be (N, T, H, W, 3) with N, T, H, W >= 1, got %s' % (tuple(images_shape),))
    N, T, H, W = (int(v) for v in images_shape[:4])
    for name, s in (('actions', actions_shape), ('states', states_shape)):
        if tuple(s) != (N, T, 5):
            raise ValueError('%s must be (%d, %d, 5) like the images, got %s' % (name, N, T, tuple(s)))
    if H * W * 3 >= 2 ** 31:
        raise ValueError('frames of %d x %d are too large' % (H, W))
    return N, T, H, W


def rank_slice(batch, rank, world):
    """A rank's share of the drawn batch: `DeviceFeeder.prefetch`'s slice [rank * B/world, (rank + 1) * B/world)."""
    B = len(batch)
    if B % world:
        raise ValueError('batch of %d sequences is not divisible by %d ranks' % (B, world))
    per = B // world
    return batch[rank * per:(rank + 1) * per]


def split_index_ranges(N, train_val_split=0.95):
    """`split_train_val` as two ranges of sequence numbers over ONE set: [0, k) trains, [k, N) validates."""
    k = int(np.floor(train_val_split * N))
    return range(0, k), range(k, N)


class DeviceDataset(object):
    """The whole data set in HBM, in the layout of the files: frames [N][T][H][W][3] as float32 or as uint8 levels (`FrameStorage`), actions and
    states [N][T][5].  `gather(indices)` sends B sequence numbers to the device and ONE pivp_gather_batch launch writes the time-major planar
    batch that `Model.__call__` takes -- bit for bit what `concat_examples` makes of the same sequences on the host.  Nothing here synchronises
    with the device after the upload; there is no CPU path."""

    def __init__(self, images, actions, states, device='cuda:0', storage='auto', chunk=256):
        sa, ss = np.shape(actions), np.shape(states)
        if len(sa) == 3 and len(ss) == 3:      # (anything else: check_set_shapes' complaint)
            check_device_widths(sa[2], ss[2])
        shape = check_set_shapes(np.shape(images), sa, ss)
        self._begin(shape, device, storage)
        for lo in range(0, self.N, chunk):
            self._put(lo, images[lo:lo + chunk], actions[lo:lo + chunk], states[lo:lo + chunk])

    @classmethod
    def from_dir(cls, data_dir, device='cuda:0', storage='auto', chunk=256, raw=False):
        """Read <data_dir>/map.csv sequence by sequence and upload in chunks of `chunk` sequences through one pinned staging buffer: the host
        never holds more than a chunk.  raw: the frames are predict's raw ones (column 6, levels 0..255, any size) instead of the training
        frames in [0, 1]; see `scale`."""
        rows = read_map(data_dir)
        load = lambda r, col: np.float32(np.load(os.path.join(data_dir, r[col])))
        cols = (6 if raw else 2, 3, 4)
        first = load(rows[0], cols[0])
        if first.ndim != 4:
            raise ValueError('%s must hold (T, H, W, 3) frames, got %s' % (rows[0][cols[0]], first.shape))
        shape = check_set_shapes((len(rows),) + first.shape, (len(rows), first.shape[0], 5), (len(rows), first.shape[0], 5))
        self = cls.__new__(cls)
        self._begin(shape, device, storage, raw)
        for lo in range(0, self.N, chunk):
            part = rows[lo:lo + chunk]
            arrays = [np.stack([load(r, col) for r in part]) for col in cols]
            if arrays[1].ndim == 3 and arrays[2].ndim == 3:
                check_device_widths(arrays[1].shape[2], arrays[2].shape[2])
            check_set_shapes((self.N,) + arrays[0].shape[1:], (self.N,) + arrays[1].shape[1:], (self.N,) + arrays[2].shape[1:])
            if arrays[0].shape[1:] != (self.T, self.H, self.W, 3):
                raise ValueError('sequences %d.. have frames %s, the first one %s' % (lo, arrays[0].shape[1:], (self.T, self.H, self.W, 3)))
            self._put(lo, *arrays)
        return self

    @property
    def scale(self):
        """What is left to multiply gathered frames by to bring them to [0, 1]: 1/255 for raw frames held as float32 (the gather copies the
        levels), else 1 (uint8 storage always hands back k / 255)."""
        return 1.0 / 255.0 if self._policy.raw and self.storage == 'float32' else 1.0

    def _begin(self, shape, device, storage, raw=False):
        import torch
        self._torch = torch
        self.N, self.T, self.H, self.W = shape
        self._policy = FrameStorage(storage, raw)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('a DeviceDataset lives on a GPU (there is no CPU path), got device %s' % (device,))
        self.storage = self._policy.storage       # None until the first chunk has been seen under 'auto'
        self.nbytes = 0
        self.frames = self.actions = self.states = None
        self._stage = None
        self._slots = []                          # index buffers of gather(): [pinned host, device, event after the launch that read it]

    def _allocate(self):
        torch = self._torch
        item = 1 if self.storage == 'uint8' else 4
        need = self.N * self.T * (self.H * self.W * 3 * item + 2 * 5 * 4)
        free, total = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise RuntimeError('the data set needs %.2f GB on %s as %s (%d sequences of %d frames %d x %d), %.2f GB of %.2f are free'
                               % (need / 1e9, self.device, self.storage, self.N, self.T, self.H, self.W, free / 1e9, total / 1e9))
        self.nbytes = need
        self.frames = torch.empty((self.N, self.T, self.H, self.W, 3), dtype=torch.uint8 if item == 1 else torch.float32, device=self.device)
        self.actions = torch.empty((self.N, self.T, 5), dtype=torch.float32, device=self.device)
        self.states = torch.empty((self.N, self.T, 5), dtype=torch.float32, device=self.device)

    def _put(self, lo, images, actions, states):
        """Upload sequences lo .. lo + n - 1.  One pinned staging set, reused: the copies out of it are awaited before the next chunk is laid in."""
        torch = self._torch
        enc = self._policy.encode(images, lo)
        if self.frames is None:
            self.storage = self._policy.storage
            self._allocate()
        parts = [enc, np.asarray(actions, dtype=np.float32), np.asarray(states, dtype=np.float32)]
        n = len(enc)
        if self._stage is None or self._stage[0].shape[0] < n:
            self._stage = [torch.empty((n,) + p.shape[1:], dtype=torch.from_numpy(p[:0]).dtype, pin_memory=True) for p in parts]
        for st, p, dst in zip(self._stage, parts, (self.frames, self.actions, self.states)):
            np.copyto(st.numpy()[:n], p)
            dst[lo:lo + n].copy_(st[:n], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        if lo + n >= self.N:
            self._stage = None

    def _slot(self, B):
        torch = self._torch
        for sl in self._slots:
            if sl[0].numel() >= B and sl[2].query():      # its last launch has read the indices: the pinned words may change
                return sl
        cap = max(B, 64)
        sl = [torch.empty(cap, dtype=torch.int32, pin_memory=True), torch.empty(cap, dtype=torch.int32, device=self.device), torch.cuda.Event()]
        self._slots.append(sl)
        return sl

    def gather(self, indices, out=None):
        """B sequence numbers -> [images (T,B,3,H,W), actions (T,B,5), states (T,B,5)] on the device, written by one launch on the current
        stream; `out`: three such float32 tensors to write into.  The indices are validated on the host, laid into a pinned buffer and copied
        without blocking; the call never synchronises (a pinned buffer is reused only once the launch that read it has finished, otherwise a
        new one is made)."""
        idx = check_indices(indices, self.N)
        B = len(idx)
        shapes = [(self.T, B, 3, self.H, self.W), (self.T, B, 5), (self.T, B, 5)]
        torch = self._torch
        if out is not None:
            if len(out) != 3:
                raise ValueError('out must be [images, actions, states]')
            for o, s in zip(out, shapes):
                if tuple(o.shape) != s or o.dtype != torch.float32 or o.device != self.device or not o.is_contiguous():
                    raise ValueError('out tensors must be contiguous float32 %s on %s' % (shapes, self.device))
        from . import _lib
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if out is None:
                out = [torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes]
            host, dev, event = sl = self._slot(B)
            host.numpy()[:B] = idx
            dev[:B].copy_(host[:B], non_blocking=True)
            stream = torch.cuda.current_stream(self.device)
            _lib.check(lib.pivp_gather_batch(self.frames.data_ptr(), int(self.storage == 'uint8'), self.actions.data_ptr(), self.states.data_ptr(),
                                             dev.data_ptr(), B, self.N, self.T, self.H, self.W, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), stream.cuda_stream), 'pivp_gather_batch')
            event.record(stream)
        return list(out)


class DeviceBatcher(object):
    """`DeviceFeeder`'s interface over a `DeviceDataset`: the iterator -- the same `SerialIterator`, over a list or range of SEQUENCE NUMBERS instead
    of examples, so it draws from NumPy's global RNG exactly as before and order, wrap-around, `epoch` and `is_new_epoch` are unchanged -- yields the
    batch's numbers, the rank keeps its slice of them (`rank_slice`: the feeder's shard) and one gather launch on the caller's stream, inside
    `get()`, writes the batch.  There is nothing to overlap: `prefetch()` does nothing, and the iterator is advanced in `get()`, i.e. at the point
    of the loop where the feeder's `prefetch()` + `get()` pair hands the same batch over (after the previous step's own RNG draws).

    ONE set of output buffers, reused by every `get()` (a new set only when the batch size changes, as for the last batch of a repeat=False
    pass).  `Model.__call__` keeps the batch's addresses, it does not copy, so the next gather overwrites what the previous step read -- safe
    because of stream order alone: the gather is enqueued on the stream current at `get()`, behind everything enqueued there before, and
    `Model.__call__` / `Model.backward` / `Adam.update` leave nothing behind on other streams (the plan's side stream is joined into the caller's
    stream before `pivp_rollout_backward` returns, the all-reduce's stream before `update` returns).  The caller's obligation: every kernel
    that reads a batch is enqueued on, or joined into, the stream that is current at the NEXT `get()`.  A caller that runs the model on another
    stream, keeps a batch across a `get()`, or carries on after a failed `update()` must `clone()` the batch or synchronise first."""

    def __init__(self, device_dataset, iterator, rank=0, world=1):
        self.dataset = device_dataset
        self.iterator = iterator
        self.rank, self.world = int(rank), int(world)
        self._out = None

    def prefetch(self):
        """Nothing to do ahead of time (kept so that the training loop is the same for both feeds)."""

    def get(self):
        """-> ([images (T,B/world,3,H,W), actions, states] on the device, epoch at the draw, is_new_epoch after the draw); StopIteration when a
        repeat=False iterator has ended."""
        epoch = self.iterator.epoch
        batch = self.iterator.next()
        new_epoch = self.iterator.is_new_epoch
        mine = rank_slice(list(batch), self.rank, self.world)
        if self._out is not None and self._out[0].shape[1] != len(mine):
            self._out = None
        self._out = self.dataset.gather(mine, out=self._out)
        return list(self._out), epoch, new_epoch

    def __iter__(self):
        return self

    def __next__(self):
        return self.get()[0]
