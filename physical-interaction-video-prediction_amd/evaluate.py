"""Held-out evaluation of a trained model: per-sample MSE, PSNR and SSIM of every predicted frame, as curves over the prediction step
(Finn et al. 2016, fig. 5 and 6).  No counterpart in the reference, whose only quality number is psnr_all (the PSNR of the batch-mean MSE).

    python -m pivp_amd.evaluate <model_dir> <model_name> [first_sequence] --data_dir <dir> [--batch_size 32] [--max_sequences N]

Takes `predict.py`'s model arguments.  Loads the checkpoint, walks the sequences of <data_dir>/map.csv in order -- the raw frames of predict.py,
resized on the device to the trained size and scaled by 1/255 (`predict.resize_images`) --, runs `Model.evaluate` per batch (one feed-self
rollout and one pivp_frame_metrics launch) and feeds a `metrics.StepCurves`, which stays on the device until the end.  Prints one line per
prediction step and writes `metrics-<model_name>.npz` next to the checkpoint: `<metric>_mean`, `_std`, `_min`, `_max` (metric = mse, psnr, ssim),
each of length T - context_frames, `count`, and `psnr_n_inf` (frames identical to their ground truth: +inf PSNR, kept out of the moments).
Rendering is out of scope."""
import argparse
import os

import numpy as np
import torch

from . import dataset as ds
from .checkpoint import load_npz
from .data import concat_examples
from .metrics import METRICS, StepCurves
from .model import Model


def build_parser():
    p = argparse.ArgumentParser(description='Per-step MSE / PSNR / SSIM of a trained {model} over a data set')
    p.add_argument('model_dir'); p.add_argument('model_name')
    p.add_argument('data_index', type=int, nargs='?', default=0, help='first sequence of map.csv to evaluate (predict.py: the one sequence)')
    p.add_argument('--models_dir', default='models')
    p.add_argument('--data_dir', default='data/processed/brain-robotics-data/push/push_testnovel')
    p.add_argument('--model_type', default='')
    p.add_argument('--schedsamp_k', type=float, default=-1)
    p.add_argument('--context_frames', type=int, default=2)
    p.add_argument('--use_state', type=int, default=1)
    p.add_argument('--num_masks', type=int, default=10)
    # the widths of an action and of a robot state in the data (the push data set's 5 / 5; BAIR pushing 4 / 3, RoboNet 4 / 5): Model(action_dim=, state_dim=)
    p.add_argument('--action_dim', type=int, default=5)
    p.add_argument('--state_dim', type=int, default=5)
    p.add_argument('--image_height', type=int, default=64)
    p.add_argument('--image_width', type=int, default=64)
    p.add_argument('--gpu', type=int, default=0)
    p.add_argument('--out', default='')
    p.add_argument('--batch_size', type=int, default=32)
    p.add_argument('--max_sequences', type=int, default=0, help='0: every sequence from data_index on')
    p.add_argument('--win', type=int, default=11)
    p.add_argument('--sigma', type=float, default=1.5)
    # 1: the raw frames of the whole data set are uploaded once (dataset.DeviceDataset) and every batch is gathered on the device.  As float32
    # the results are those of the host walk bit for bit; as uint8 a level k reaches the resize as k / 255 instead of being scaled after it,
    # which moves a frame by an ulp or so
    p.add_argument('--device_dataset', type=int, default=0, choices=(0, 1))
    p.add_argument('--device_storage', default='auto', choices=ds.STORAGES)
    return p


def model_type_of(args):
    if args.model_type != '':
        return args.model_type
    parts = args.model_dir.split('-')
    if len(parts) != 4:
        raise ValueError("Model {} is not recognized, use --model_type to describe the type".format(args.model_dir))
    return parts[2]


def curves_to_arrays(result):
    """StepCurves.result() -> the flat dict of arrays that goes into the npz."""
    out = {}
    for k in METRICS:
        for f in ('mean', 'std', 'min', 'max'):
            out['%s_%s' % (k, f)] = result[k][f]
    out['count'] = result['mse']['count']
    out['psnr_n_inf'] = result['psnr']['n_inf']
    return out


def evaluate(args):
    """-> (flat dict of per-step arrays, number of sequences evaluated)."""
    from .predict import resize_images
    path = os.path.join(args.models_dir, args.model_dir)
    if not os.path.exists(os.path.join(path, args.model_name)):
        raise ValueError("Directory {} does not exists".format(path))
    if not os.path.exists(args.data_dir):
        raise ValueError("Directory {} does not exists".format(args.data_dir))
    if args.batch_size < 1 or args.max_sequences < 0 or args.data_index < 0:
        raise ValueError('--batch_size must be positive, --max_sequences and the first sequence non-negative')
    total = len(ds.read_map(args.data_dir))
    if args.data_index > total - 1:
        raise ValueError("Data index {} is out of range for available data".format(args.data_index + 1))
    stop = total if args.max_sequences == 0 else min(total, args.data_index + args.max_sequences)
    model_type = model_type_of(args)
    device = 'cuda:%d' % args.gpu
    model = Model(num_masks=args.num_masks, is_cdna=model_type == 'CDNA', is_dna=model_type == 'DNA', is_stp=model_type == 'STP',
                  use_state=args.use_state, scheduled_sampling_k=args.schedsamp_k, num_frame_before_prediction=args.context_frames,
                  prefix='evaluate', device=device, action_dim=args.action_dim, state_dim=args.state_dim)
    load_npz(os.path.join(path, args.model_name), model)
    curves = StepCurves()
    size = (args.image_height, args.image_width)
    if args.device_dataset:
        ds.check_device_widths(args.action_dim, args.state_dim)
        from . import _lib
        lib = _lib.load()
        dset = ds.DeviceDataset.from_dir(args.data_dir, device, storage=args.device_storage, raw=True)
        for lo in range(args.data_index, stop, args.batch_size):
            img, act, sta = dset.gather(list(range(lo, min(lo + args.batch_size, stop))))
            T, B = img.shape[:2]
            resized = torch.empty((T, B, 3) + size, dtype=torch.float32, device=img.device)
            with torch.cuda.device(img.device):
                _lib.check(lib.pivp_resize_images(img.data_ptr(), resized.data_ptr(), T * B * 3, dset.H, dset.W, size[0], size[1], dset.scale,
                                                  torch.cuda.current_stream(img.device).cuda_stream), 'pivp_resize_images')
            curves.add(model.evaluate([resized, act, sta], win=args.win, sigma=args.sigma))
            model.reset_state()
        return curves_to_arrays(curves.result()), stop - args.data_index
    for lo in range(args.data_index, stop, args.batch_size):
        batch = []
        for i in range(lo, min(lo + args.batch_size, stop)):
            _, image_pred, _, action, state = ds.get_data_info(args.data_dir, i)
            batch.append([image_pred, action, state])
        img, act, sta = concat_examples(batch)
        T = img.shape[0]
        resized = torch.stack([resize_images(img[t], (args.image_height, args.image_width), device, 1.0 / 255.0) for t in range(T)])
        curves.add(model.evaluate([resized, act, sta], win=args.win, sigma=args.sigma))
        model.reset_state()
    return curves_to_arrays(curves.result()), stop - args.data_index


def main(argv=None):
    args = build_parser().parse_args(argv)
    arrays, n = evaluate(args)
    out = args.out or os.path.join(args.models_dir, args.model_dir, 'metrics-%s.npz' % args.model_name)
    np.savez(out, **arrays)
    for s in range(len(arrays['count'])):
        print('step %2d  mse %.6f +- %.6f  psnr %.3f +- %.3f dB  ssim %.4f +- %.4f  (%d frames)'
              % (s + 1, arrays['mse_mean'][s], arrays['mse_std'][s], arrays['psnr_mean'][s], arrays['psnr_std'][s], arrays['ssim_mean'][s],
                 arrays['ssim_std'][s], arrays['count'][s]))
    print('%d sequences -> %s' % (n, out))


if __name__ == '__main__':
    main()
