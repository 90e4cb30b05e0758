"""Training entry point with the reference's flags (train_model.py:772-791) on the MI355X model.

    python -m pivp_amd.train --data_dir ... --output_dir models --num_iterations 100000 --batch_size 32 ...
    python -m torch.distributed.run --nproc-per-node 8 -m pivp_amd.train ...        # data parallel, one process per GPU

Follows the host loop of train_model.py:792-1049: load every sequence listed in <data_dir>/map.csv, 95/5 split by index,
shuffled repeat iterator, optimizer.update per iteration, per-epoch [mean, std, min, max, median] of loss and PSNR, and a
checkpoint directory `<output_dir>/<YYYYmmdd-HHMMSS>-<TYPE>-<B>/` holding `training-<epoch>` (model npz), `state-<epoch>`
(optimizer npz), `training-global_*.npy` and a `version` file.  Defects of the reference OFF the hot path are not reproduced
(SURVEY.md App. D): validation really runs every `validation_interval` epochs, --pretrained_state is loaded into the
optimizer, validation statistics do not overwrite the PSNR file."""
import argparse
import logging
import os
import subprocess
import time

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')    # before torch: this pool's host driver only supports dmabuf IPC (RCCL across processes needs it)

import numpy as np
import torch

from . import dataset as ds
from .checkpoint import load_npz, load_optimizer_npz, save_npz, save_optimizer_npz
from .data import concat_examples
from .model import Model, using_config
from .optimizer import Adam, GradientClipping
from .parallel import GradAllReduce


def build_parser():
    p = argparse.ArgumentParser(description='Train the model based on the data saved in ../processed')
    p.add_argument('--data_dir', default='data/processed/brain-robotics-data/push/push_train')
    p.add_argument('--output_dir', default='models')
    p.add_argument('--event_log_dir', default='models')                       # accepted, unused (as in the reference)
    p.add_argument('--num_iterations', type=int, default=100000)
    p.add_argument('--pretrained_model', default='')
    p.add_argument('--pretrained_state', default='')
    p.add_argument('--sequence_length', type=int, default=10)                 # accepted, unused: T comes from the data
    p.add_argument('--context_frames', type=int, default=2)
    p.add_argument('--use_state', type=int, default=1)
    p.add_argument('--model_type', default='CDNA')
    p.add_argument('--num_masks', type=int, default=10)
    # the widths of an action and of a robot state in the data (the push data set's 5 / 5; BAIR pushing 4 / 3, RoboNet 4 / 5): Model(action_dim=, state_dim=)
    p.add_argument('--action_dim', type=int, default=5)
    p.add_argument('--state_dim', type=int, default=5)
    p.add_argument('--schedsamp_k', type=float, default=900.0)
    p.add_argument('--train_val_split', type=float, default=0.95)
    p.add_argument('--batch_size', type=int, default=32)
    p.add_argument('--learning_rate', type=float, default=0.001)
    p.add_argument('--gpu', type=int, default=0)
    p.add_argument('--validation_interval', type=int, default=200)
    p.add_argument('--save_interval', type=int, default=50)
    p.add_argument('--debug', type=int, default=0)
    # 1: bit-reproducible training (Model(deterministic=True)) and host RNGs seeded with 0 -- shuffle, scheduled sampling, initial weights --
    # so that two runs over the same data write identical training-N / state-N arrays
    p.add_argument('--deterministic', type=int, default=0, choices=(0, 1))
    # 1: the data set lives on the GPU as the files hold it (dataset.DeviceDataset) and every batch is one gather launch from the drawn sequence
    # numbers (dataset.DeviceBatcher) instead of concat_examples + a host-to-device copy; same batches, same bits.  --device_storage: how the
    # frames are held there, uint8 only for frames on the k/255 grid (auto: decided from the first sequences)
    p.add_argument('--device_dataset', type=int, default=0, choices=(0, 1))
    p.add_argument('--device_storage', default='auto', choices=ds.STORAGES)
    # the guarded Adam step (optimizer.py): --grad_clip t > 0 adds chainer's GradientClipping(t); --skip_nonfinite 1 leaves the parameters alone on a
    # step whose gradient holds a NaN / inf and counts it; --log_grad_norm 1 only records the norm.  Any of them: the per-step global gradient norm
    # stays on the device, is read once per epoch and saved as training-global_grad_norm.npy.  All off: the plain Adam launch, log and files as before
    p.add_argument('--grad_clip', type=float, default=0.0)
    p.add_argument('--skip_nonfinite', type=int, default=0, choices=(0, 1))
    p.add_argument('--log_grad_norm', type=int, default=0, choices=(0, 1))
    # the training objective's image terms (losses.ImageLoss): weights of the MSE, L1, gradient-difference and DSSIM = 1 - SSIM terms.  1 / 0 / 0 / 0 is
    # the reference's objective: nothing new runs and the files are as before.  Anything else: validation scores the same loss, the per-step means
    # of the four terms stay on the device, are read once per epoch and saved as training-global_loss_terms.npy (per-rank means, like the loss)
    p.add_argument('--loss_mse', type=float, default=1.0)
    p.add_argument('--loss_l1', type=float, default=0.0)
    p.add_argument('--loss_gdl', type=float, default=0.0)
    p.add_argument('--loss_dssim', type=float, default=0.0)
    # truncated back-propagation through time: every drawn sequence is cut into N consecutive windows (T divisible by N); each window is one forward,
    # one backward with the state it started from as a constant, and one Adam step, the ConvLSTM state carried from window to window and cleared
    # between sequences (Model(carry_state=True, state_backward=True)).  1, the default: the sequence is one window and nothing new runs
    p.add_argument('--tbptt_windows', type=int, default=1)
    return p


def model_state_flags(args):
    """-> the Model keywords --tbptt_windows adds: none for 1 (the model is built exactly as before)."""
    if args.tbptt_windows < 1:
        raise SystemExit('--tbptt_windows must be >= 1 (1: off)')
    return dict(carry_state=True, state_backward=True) if args.tbptt_windows > 1 else {}


def train_step(optimizer, model, x, itr, windows=1):
    """One drawn batch: optimizer.update on the whole sequence (windows = 1, the path as it always was), or on each of its consecutive windows in
    turn with the state carried across them.  The caller clears the state between sequences.  -> [(loss, psnr_all)] device scalars, one per update."""
    if windows == 1:
        optimizer.update(model, x, itr)
        return [(model.loss, model.psnr_all)]
    from .tbptt import split_windows
    out = []
    for w in split_windows(x, windows):
        optimizer.update(model, w, itr)
        out.append((model.loss, model.psnr_all))
    return out


def image_loss_from_args(args):
    """-> the ImageLoss of --loss_*, or None for the reference's objective."""
    from .losses import ImageLoss
    try:
        spec = ImageLoss(mse=args.loss_mse, l1=args.loss_l1, gdl=args.loss_gdl, dssim=args.loss_dssim)
    except ValueError as e:
        raise SystemExit('--loss_*: %s' % e)
    return None if spec.is_reference() else spec


def grad_norm_stat(norms, stat):
    """[mean, std, min, max, median] of an epoch's per-step gradient norms.  The norm of a step with a NaN / inf gradient is itself non-finite: such
    steps are left out (their number is the skipped-steps count when --skip_nonfinite is on); an epoch without a finite norm gives a row of NaN."""
    finite = [v for v in norms if np.isfinite(v)]
    return stat(finite) if finite else [float('nan')] * 5


def _git_version():
    try:
        ex = lambda a: subprocess.check_output(['git'] + a, stderr=subprocess.DEVNULL).decode().strip()
        return ex(['rev-parse', '--abbrev-ref', 'HEAD']) + '\n' + ex(['rev-parse', 'HEAD'])
    except Exception:
        return 'unknown'


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
    logger = logging.getLogger(__name__)
    world = int(os.environ.get('WORLD_SIZE', '1')); rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(args.gpu)))
    dp = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.cuda.set_device(local_rank)
        dist.init_process_group('nccl', device_id=torch.device('cuda:%d' % local_rank))
        dp = GradAllReduce()
    device = 'cuda:%d' % local_rank

    if args.device_dataset:
        try:
            ds.check_device_widths(args.action_dim, args.state_dim)
        except ValueError as e:
            raise SystemExit('--device_dataset 1: %s' % e)
        dset = ds.DeviceDataset.from_dir(args.data_dir, device, storage=args.device_storage)
        train_set, valid_set = ds.split_index_ranges(dset.N, args.train_val_split)      # sequence numbers: the iterators draw those
        n_all = dset.N
        logger.info('Data set on %s as %s: %.1f MB', device, dset.storage, dset.nbytes / 1e6)
    else:
        images, actions, states = ds.load_dataset(args.data_dir)
        (tr_i, tr_a, tr_s), (va_i, va_a, va_s) = ds.split_train_val(images, actions, states, args.train_val_split)
        train_set, valid_set = ds.group_examples(tr_i, tr_a, tr_s), ds.group_examples(va_i, va_a, va_s)
        n_all = len(images)
    logger.info('Data set contain %d, %d will be use for training and %d will be use for validation', n_all, len(train_set), len(valid_set))
    model = Model(num_masks=args.num_masks, is_cdna=args.model_type == 'CDNA', is_dna=args.model_type == 'DNA',
                  is_stp=args.model_type == 'STP', use_state=args.use_state, scheduled_sampling_k=args.schedsamp_k,
                  num_frame_before_prediction=args.context_frames, prefix='train', device=device, keep_activations=True,
                  deterministic=bool(args.deterministic), image_loss=image_loss_from_args(args), action_dim=args.action_dim, state_dim=args.state_dim,
                  **model_state_flags(args))
    extra_loss = model.image_loss is not None
    if args.grad_clip < 0 or args.grad_clip != args.grad_clip:
        raise SystemExit('--grad_clip must be >= 0 (0: off)')
    guarded = bool(args.grad_clip > 0 or args.skip_nonfinite or args.log_grad_norm)
    if guarded:
        optimizer = Adam(alpha=args.learning_rate, skip_nonfinite=bool(args.skip_nonfinite), track_grad_norm=True).setup(model, data_parallel=dp)
        if args.grad_clip > 0:
            optimizer.add_hook(GradientClipping(args.grad_clip))
    else:
        optimizer = Adam(alpha=args.learning_rate).setup(model, data_parallel=dp)
    if args.pretrained_model:
        load_npz(args.pretrained_model, model)
    per_rank = args.batch_size // world
    if per_rank * world != args.batch_size:
        raise SystemExit('--batch_size must be divisible by the number of ranks')
    np.random.seed(0 if world > 1 or args.deterministic else None)      # identical shuffles on every rank; each takes its shard of the batch
    if world > 1:                                 # ... but its own scheduled-sampling draws (rank-offset stream)
        model.sampling_rng = np.random.RandomState(1 + rank)
    train_iter = ds.SerialIterator(train_set, args.batch_size, repeat=True, shuffle=True)
    valid_iter = ds.SerialIterator(valid_set, args.batch_size, repeat=False, shuffle=True)
    save_dir = os.path.join(args.output_dir, '%s-%s-%d' % (time.strftime('%Y%m%d-%H%M%S'), args.model_type, args.batch_size))
    local_losses, local_psnr, g_loss, g_psnr, g_loss_v, g_psnr_v = [], [], [], [], [], []
    local_terms, g_terms = [], []                     # runs with an image loss: the steps' four term means as device tensors, read at the epoch's end
    local_gnorm, g_gnorm = [], []                     # guarded runs: the steps' gradient norms as device scalars, read at the epoch's end
    stat = lambda a: [float(np.mean(a)), float(np.std(a)), float(np.min(a)), float(np.max(a)), float(np.median(a))]
    state_loaded = False
    itr, start = 0, None
    # Host feed (TM:937-950 is synchronous): batch t + 1 is drawn, laid out (concat_examples), sharded and copied from pinned memory on a
    # second stream while the GPU works on batch t; iterator order, shards and epoch bookkeeping are those of the plain loop
    # --device_dataset 1: nothing to lay out or copy, the batch is gathered on the device inside get() (every rank validates the whole batch, as below)
    if args.device_dataset:
        feeder = ds.DeviceBatcher(dset, train_iter, rank=rank, world=world)
        valid_batches = ds.DeviceBatcher(dset, valid_iter)
    else:
        feeder = ds.DeviceFeeder(train_iter, rank=rank, world=world, device=device)
        valid_batches = None
    while itr < args.num_iterations:
        x, epoch, is_new_epoch = feeder.get()
        start = start or time.time()
        if world > 1 and itr == 0:                  # replicas start identical: rank 0's lazily initialised weights
            with using_config('train', False):
                model(x, 0)
            import torch.distributed as dist
            model.broadcast_params(src=0); model.reset_state()      # (also invalidates the precision modes' weight packs)
        if args.pretrained_state and not state_loaded:
            with using_config('train', False):
                model(x, 0)
            model.reset_state(); load_optimizer_npz(args.pretrained_state, optimizer); state_loaded = True
        steps = train_step(optimizer, model, x, itr, args.tbptt_windows)      # enqueues the whole step; returns while the GPU is still working on it
        if guarded:
            local_gnorm.append(optimizer.grad_norm.clone())      # (a view of a buffer the next step overwrites; no synchronisation)
        if extra_loss:
            local_terms.append(torch.stack([model.loss_terms[k] for k in ('mse', 'l1', 'gdl', 'dssim')]))
        if itr + 1 < args.num_iterations:
            feeder.prefetch()                       # ... so the next batch's host work and copy run underneath it
        stats = torch.stack([model.loss, model.psnr_all]).to(torch.float64)
        if len(steps) > 1:                          # --tbptt_windows: the mean over the sequence's windows (gradient norm and loss terms: the last window's)
            stats = torch.stack([torch.stack(s) for s in steps]).to(torch.float64).mean(dim=0)
        if world > 1:                              # the logged statistics are those of the GLOBAL batch (mean over the ranks' shards)
            dist.all_reduce(stats); stats /= world
        lv, pv = stats.tolist()                     # the step's one host synchronisation
        local_losses.append(lv); local_psnr.append(pv)
        model.reset_state()
        if rank == 0:
            logger.info('%d %s', epoch + 1, local_losses[-1])
        if is_new_epoch:
            g_loss.append(stat(local_losses)); g_psnr.append(stat(local_psnr))
            if extra_loss:                          # one row per epoch: the epoch's mean of each term
                g_terms.append(torch.stack(local_terms).to(torch.float64).mean(dim=0).tolist())
                if rank == 0:
                    logger.info('[TRAIN] Epoch #: %d  loss terms  mse %.6f  l1 %.6f  gdl %.6f  dssim %.6f', epoch + 1, *g_terms[-1])
                local_terms = []
            if guarded:
                g_gnorm.append(grad_norm_stat(torch.stack(local_gnorm).tolist(), stat))
                skipped = optimizer.skipped_steps   # (reads the device counter)
                if rank == 0:
                    logger.info('[TRAIN] Epoch #: %d  elapsed %.2fs  loss %.6f  psnr %.3f  grad norm %.6g  skipped steps %d', epoch + 1,
                                time.time() - start, g_loss[-1][0], g_psnr[-1][0], g_gnorm[-1][0], skipped)
                local_gnorm = []
            elif rank == 0:
                logger.info('[TRAIN] Epoch #: %d  elapsed %.2fs  loss %.6f  psnr %.3f', epoch + 1, time.time() - start, g_loss[-1][0], g_psnr[-1][0])
            local_losses, local_psnr, start = [], [], None
            if (epoch + 1) % args.validation_interval == 0 and len(valid_set) > 0:
                vl, vp = [], []
                for vb in (valid_batches or valid_iter):
                    vx = vb if valid_batches else list(concat_examples(vb))
                    with using_config('train', False):
                        vl.append(float(model(vx, itr))); vp.append(float(model.psnr_all))
                    model.reset_state()
                g_loss_v.append(stat(vl)); g_psnr_v.append(stat(vp))
                valid_iter.reset()
            if epoch % args.save_interval == 0 and rank == 0:
                if not os.path.exists(save_dir):
                    os.makedirs(save_dir)
                    with open(os.path.join(save_dir, 'version'), 'w') as f:
                        f.write(_git_version() + '\n')
                save_npz(os.path.join(save_dir, 'training-' + str(epoch)), model)
                save_optimizer_npz(os.path.join(save_dir, 'state-' + str(epoch)), optimizer, epoch)
                np.save(os.path.join(save_dir, 'training-global_losses'), np.array(g_loss))
                np.save(os.path.join(save_dir, 'training-global_psnr_all'), np.array(g_psnr))
                np.save(os.path.join(save_dir, 'training-global_losses_valid'), np.array(g_loss_v))
                np.save(os.path.join(save_dir, 'training-global_psnr_all_valid'), np.array(g_psnr_v))
                if guarded:
                    np.save(os.path.join(save_dir, 'training-global_grad_norm'), np.array(g_gnorm))
                if extra_loss:
                    np.save(os.path.join(save_dir, 'training-global_loss_terms'), np.array(g_terms))
        itr += 1
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return save_dir


if __name__ == '__main__':
    main()
