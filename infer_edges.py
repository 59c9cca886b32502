#!/usr/bin/env python3
"""infer_edges.py -- depth inference core of the reference script (/root/reference/infer_edges.py:237-366, rows H3):
image file -> PIL + LANCZOS resize -> [1,3,H,W] in [0,1] -> model_wrapper.depth(image)['inv_depths'][0][0] -> inv2depth ->
``NNNNNNNN_regular.npy`` (float32 metres) + ``NNNNNNNN_regular.png`` (depth / max * 255).

With an ``analysis`` section in the YAML the reference's analysis stage follows (infer_edges.py:129-183), on the device:
``analysis.run_heavy_edge_metrics`` -> the edge benchmark over ``analysis.edge_image_list`` (mindtheedge_amd/utils/edge_benchmark.py) ->
``sfm_analysis/debug_plots/edge_AUC.txt`` and ``mean_frames_bsds_edge_metrics.csv``; ``analysis.run_metrics`` -> the per-frame depth metrics
against ``analysis.gt_image_list`` (utils/depth_analysis.py) -> ``frames_depth_metrics.csv`` and ``mean_frames_depth_metrics.csv``.
``analysis.just_evaluate`` skips the inference and evaluates the ``*_regular.npy`` files already there.  Also read: ``analysis.min_depth``,
``max_depth``, ``gt_crop``, ``eval_mask_image_list``, ``prec_recall_eval_range_min/max`` and ``save.folder`` (where predictions and analysis go
when the analysis stage runs).  With image files in ``gt_image_list`` ``run_metrics`` also writes the D3R ordinal error,
``mean_frames_ord_metrics.txt``.  The plots and the pickle are left out.  Without those keys nothing changes.

``--split`` is the reference's own loop (infer_edges.py:100-123, 237-366): column 0 (image) and column 3 (LiDAR) of every line of
``config.datasets.test.split[0]``; per frame ``NNNNNNNN_regular.npy/.png`` and the log-coloured ``NNNNNNNN_regular_color.png`` (Spectral,
made on the device: utils/depth.py::depth_log_color) and, when ``datasets.test.input_depth_type[0] != ''`` and the network has the sparse
branch, the RGB+LiDAR pass as ``NNNNNNNN_lidar.npy/.png`` and ``_lidar_color.png`` -- upstream computes that prediction, globs for
``*_lidar.npy`` and never writes it; writing it is a deliberate deviation.  Then ``input_list.txt``, ``pred_list.txt`` and
``pred_lidar_list.txt`` (sorted; upstream lists them in glob order) in the output folder, which is ``save.folder`` when that is set."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # see mindtheedge_amd/__init__.py: side stream / RCCL streams need their own hardware queues


def infer_depth(model_wrapper, image):
    """image: fp32 [B,3,H,W] on the GPU, H and W multiples of 32 -> depth [B,1,H,W] fp32 (metres)."""
    import torch
    from mindtheedge_amd.utils.depth import inv2depth
    from mindtheedge_amd import kernels as K
    model_wrapper.eval()
    with torch.no_grad():
        pred_inv_depth = model_wrapper.depth(image, rgb_edge=None)['inv_depths'][0][0]
    depth = inv2depth(pred_inv_depth)
    # The eval forward runs the GroupNorm cluster kernels too (bounded inter-workgroup waits); the optimizer that polls the device error word on the
    # training path never runs here.  The depth goes to the host next (save_depth), so waiting for the stream costs nothing that is not paid anyway.
    torch.cuda.current_stream().synchronize()
    K.check_device_errors()
    return depth


IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.ppm')


def load_frame(path, image_shape=None):
    """One input frame -> float32 [3,H,W] in [0,1] on the host, the way the reference prepares it (infer_edges.py:266-282):
    PIL ``Image.open`` -> ``resize_image`` to the configured (H, W) with LANCZOS (datasets/augmentations.py:16-35; ANTIALIAS is
    LANCZOS) -> ``to_tensor`` (HWC uint8 / 255 -> CHW).  ``.npy`` arrays ([3,H,W] or [H,W,3], [0,1] or uint8) are taken as they are."""
    import numpy as np
    import torch
    if path.lower().endswith(IMAGE_EXT):
        from PIL import Image
        im = Image.open(path).convert('RGB')
        if image_shape is not None and tuple(image_shape) != (im.size[1], im.size[0]):
            im = im.resize((int(image_shape[1]), int(image_shape[0])), Image.LANCZOS)
        a = np.asarray(im, dtype=np.uint8)
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1), dtype=np.float32) / 255.0)
    a = np.load(path).astype(np.float32)
    if a.shape[-1] == 3:
        a = a.transpose(2, 0, 1)
    return torch.from_numpy(np.ascontiguousarray(a) / np.float32(255.0 if a.max() > 1.5 else 1.0))


def save_depth(output_base, depth, png=True, tag='regular', npy=True):
    """``<base>_regular.npy`` (float32 metres) and, as the reference (infer_edges.py:349-353), ``<base>_regular.png`` =
    depth / max * 255 as 8-bit grey (cv2.imwrite of a float array saturates-and-rounds to uint8).  tag: 'regular' or 'lidar'."""
    import numpy as np
    d = depth.detach().float().cpu().numpy()
    if npy:
        np.save(output_base + '_%s.npy' % tag, d)
    if png:
        from PIL import Image
        Image.fromarray(np.clip(np.rint(d / d.max() * 255.0), 0, 255).astype(np.uint8)).save(output_base + '_%s.png' % tag)


def save_depth_color(output_base, depth, tag='regular'):
    """``<base>_<tag>_color.png``: the reference's log colouring (infer_edges.py:355-366) of a CUDA [H,W] depth map, made on the device."""
    from PIL import Image
    from mindtheedge_amd.utils.depth import depth_log_color
    Image.fromarray(depth_log_color(depth).cpu().numpy()).save(output_base + '_%s_color.png' % tag)


def parse_split_columns(line):
    """One line of the test split -> (image path, LiDAR path): columns 0 and 3 of a blank-separated line (infer_edges.py:103-105)."""
    cols = line.split('\n')[0].split(' ')
    if len(cols) < 4:
        raise ValueError("split line {!r}: expected at least 4 blank-separated columns (image, .., .., LiDAR)".format(line))
    return cols[0], cols[3]


def read_split_columns(path):
    with open(path) as f:
        return [parse_split_columns(l) for l in f.readlines() if l.strip()]


def check_split_lidar(path, dataset):
    """A KITTI velodyne ``.bin`` cannot be read the reference's way: infer_edges.py:291-299 allocates np.zeros(original_shape) with PIL's
    (W, H) size and indexes it by [y, x], which either raises or writes a transposed map."""
    if path.rsplit('.', 1)[-1] == 'bin' and dataset == 'KITTI':
        raise ValueError("{}: a KITTI .bin LiDAR file is not supported -- upstream infer_edges.py:291-299 indexes a [W,H] array by [y,x]; "
                         "use the projected .png / .npz / .npy map".format(path))


def load_split_frame(path, image_shape=(), crop_shape=()):
    """infer_edges.py:266-282: PIL open -> LANCZOS resize to image_shape -> with a two-value crop_eval_borders (h, w) the crop centred in x
    and aligned to the bottom -> float32 [3,H,W] in [0,1] on the host (the same PIL pipeline as load_frame)."""
    import numpy as np
    import torch
    from PIL import Image
    im = Image.open(path).convert('RGB')
    if len(image_shape) > 0 and tuple(image_shape) != (im.size[1], im.size[0]):
        im = im.resize((int(image_shape[1]), int(image_shape[0])), Image.LANCZOS)
    if len(crop_shape) == 2:
        start_x = int((im.size[0] - crop_shape[1]) / 2)
        start_y = int(im.size[1] - crop_shape[0])
        im = im.crop((start_x, start_y, start_x + int(crop_shape[1]), start_y + int(crop_shape[0])))
    a = np.asarray(im, dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1), dtype=np.float32) / 255.0)


def load_split_lidar(path, dataset, shape, device):
    """The LiDAR column (infer_edges.py:284-322): the map through lidar_prep.read_lidar_map (negatives to 0), then resize_depth_preserve to
    the network's shape -> float32 [1,1,H,W] on the device."""
    from mindtheedge_amd.datasets.kitti_edges import resize_depth_preserve
    from mindtheedge_amd.datasets.lidar_prep import read_lidar_map
    check_split_lidar(path, dataset)
    m = read_lidar_map(path, device, clamp_negative=True)
    return resize_depth_preserve(m, (int(shape[0]), int(shape[1]))).unsqueeze(0).unsqueeze(0)


def _shape_tuple(v):
    import ast
    if v is None or v == '':
        return ()
    return tuple(ast.literal_eval(v)) if isinstance(v, str) else tuple(v)


def run_split(config, wrapper, folder, png=True):
    """The reference's inference loop over config.datasets.test.split[0] -> the number of frames written."""
    import glob
    import torch
    from mindtheedge_amd.utils.depth import inv2depth
    from mindtheedge_amd.utils.save import save_paths_list
    from mindtheedge_amd import kernels as K
    test = config.datasets.test
    if not test.split:
        raise ValueError("--split needs config.datasets.test.split[0]")
    columns = read_split_columns(test.split[0])
    dataset = (test.dataset or ['KITTI'])[0] if isinstance(test.dataset, (list, tuple)) else test.dataset
    image_shape = _shape_tuple(config.datasets.augmentation.image_shape)
    crop_shape = _shape_tuple(config.datasets.augmentation.crop_eval_borders)
    with_lidar = (test.input_depth_type or [''])[0] != ''
    sparse_branch = bool(getattr(wrapper.model.depth_net, 'with_san', False))
    npy = bool(config.save.depth.npz)
    os.makedirs(folder, exist_ok=True)
    device = torch.device('cuda', torch.cuda.current_device())
    for counter, (image_file, lidar_file) in enumerate(columns):
        base = os.path.join(folder, '%08d' % counter)
        frame = load_split_frame(image_file, image_shape, crop_shape).unsqueeze(0).to(device)
        depth = infer_depth(wrapper, frame)
        save_depth(base, depth[0, 0], png=png, npy=npy)
        save_depth_color(base, depth[0, 0])
        if with_lidar and sparse_branch:
            lidar = load_split_lidar(lidar_file, dataset, frame.shape[-2:], device)
            with torch.no_grad():
                depth_rgbd = inv2depth(wrapper.depth(frame, lidar, rgb_edge=None)['inv_depths'][0][0])
            torch.cuda.current_stream().synchronize()
            K.check_device_errors()
            save_depth(base, depth_rgbd[0, 0], png=png, tag='lidar', npy=npy)
            save_depth_color(base, depth_rgbd[0, 0], tag='lidar')
    save_paths_list([c[0] for c in columns], folder, "input_list.txt")
    save_paths_list(sorted(glob.glob(os.path.join(folder, '*_regular.npy'))), folder, "pred_list.txt")
    save_paths_list(sorted(glob.glob(os.path.join(folder, '*_lidar.npy'))), folder, "pred_lidar_list.txt")
    return len(columns)


def _read_list(path):
    with open(path) as f:
        return [l.strip() for l in f.read().splitlines() if l.strip()]


def run_analysis(config, folder):
    """The reference's analysis stage (infer_edges.py:129-183) over the ``*_regular.npy`` predictions in ``folder``."""
    import csv
    import glob
    import numpy as np
    an = config.analysis
    plots = os.path.join(folder, 'sfm_analysis', 'debug_plots')
    os.makedirs(plots, exist_ok=True)
    preds = sorted(glob.glob(os.path.join(folder, '*_regular.npy')))
    lo = 0.0 if an.min_depth is None else float(an.min_depth)
    hi = 80.0 if an.max_depth is None else float(an.max_depth)
    crop = [44, 1197, 153, 371] if an.gt_crop is None else [int(v) for v in an.gt_crop]
    if an.run_heavy_edge_metrics:
        from mindtheedge_amd.utils.edge_benchmark import evaluate_lists
        rmin = 0.12 if an.prec_recall_eval_range_min is None else float(an.prec_recall_eval_range_min)
        rmax = 0.65 if an.prec_recall_eval_range_max is None else float(an.prec_recall_eval_range_max)
        precision_vec, recall_vec, f1, f2 = evaluate_lists(preds, _read_list(an.edge_image_list), rmin, rmax,
                                                           gt_crop=crop, min_depth=lo, max_depth=hi)
        with open(os.path.join(plots, 'mean_frames_bsds_edge_metrics.csv'), 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['', 'Precision', 'Recall'])
            for i, (p, r) in enumerate(zip(precision_vec, recall_vec)):
                w.writerow([i, p, r])
        print('AUC over all range: ' + str(f1))
        print('AUC over partial range: ' + str(f2))
        with open(os.path.join(plots, 'edge_AUC.txt'), 'w') as f:
            f.write('AUC over all range: ' + str(f1) + '\n')
            f.write('AUC over partial range: ' + str(f2) + '\n')
    if an.run_metrics:
        from mindtheedge_amd.utils.depth_analysis import run_depth_metrics
        masks = _read_list(an.eval_mask_image_list) if an.eval_mask_image_list else None
        gts = _read_list(an.gt_image_list)
        run_depth_metrics(gts, preds, plots, lo, hi, gt_crop=crop, mask_list=masks)
        from mindtheedge_amd.utils.depth_analysis import ORD_IMAGE_EXT, run_ord_metrics
        if gts and all(g.lower().endswith(ORD_IMAGE_EXT) for g in gts):            # upstream reads them with cv2.imread: image files only
            ord_error = run_ord_metrics(gts, preds)
            with open(os.path.join(plots, 'mean_frames_ord_metrics.txt'), 'w') as f:
                f.writelines(str(ord_error.mean()))


def main():
    ap = argparse.ArgumentParser(description='PackNet-SAN depth inference on MI355X')
    ap.add_argument('--config', type=str, required=True, help='YAML (model.depth_net.checkpoint_path may name a .ckpt)')
    ap.add_argument('--input', type=str, nargs='*', default=[], help='image files (png / jpg: resized to the configured shape with LANCZOS, as the '
                    'reference) or .npy arrays [3,H,W] / [H,W,3] in [0,1] (or uint8)')
    ap.add_argument('--no-png', action='store_true', help='write only the .npy depth maps')
    ap.add_argument('--output', type=str, default='results')
    ap.add_argument('--synthetic', type=int, default=0, help='number of synthetic frames of the configured shape')
    ap.add_argument('--split', action='store_true', help="the reference's loop: image and LiDAR columns of config.datasets.test.split[0], "
                    'the RGB and the RGB+LiDAR pass, colour maps and the three list files')
    ap.add_argument('--graph', action='store_true', help='replay the forward from a HIP graph (single frames are launch-bound)')
    ap.add_argument('--ema', action='store_true', help="load the checkpoints' averaged weights ('state_dict_ema', written by a run with "
                    'model.optimizer.ema_decay > 0) instead of the raw ones; a file without them is an error')
    args = ap.parse_args()
    import numpy as np
    import torch
    from mindtheedge_amd.utils.config import load_config
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    config = load_config(args.config)
    if args.ema:
        config.model.checkpoint_ema = config.model.depth_net.checkpoint_ema = True
    an = config.analysis or {}
    analyse = bool(an.get('run_heavy_edge_metrics') or an.get('run_metrics'))
    if analyse and (config.save or {}).get('folder'):
        args.output = config.save.folder
    if analyse and an.get('just_evaluate'):
        run_analysis(config, args.output)
        return
    if not os.path.exists(config.model.depth_net.checkpoint_path or ''):
        config.model.depth_net.checkpoint_path = ''
    wrapper = ModelWrapper(config).cuda()
    if args.split:
        if config.save.folder:
            args.output = config.save.folder
        n = run_split(config, wrapper, args.output, png=not args.no_png)
        print('wrote %d depth maps to %s' % (n, args.output))
        if analyse:
            run_analysis(config, args.output)
        return
    os.makedirs(args.output, exist_ok=True)
    shape = config.datasets.augmentation.image_shape
    import ast
    H, W = ast.literal_eval(shape) if isinstance(shape, str) else tuple(shape)
    images = [load_frame(p, (H, W)) for p in args.input]
    g = torch.Generator().manual_seed(0)
    images += [torch.rand(3, H, W, generator=g) for _ in range(args.synthetic)]
    graphed = None
    for ctr, img in enumerate(images):
        frame = img.unsqueeze(0).cuda()
        if args.graph:
            from mindtheedge_amd.utils.depth import inv2depth
            from mindtheedge_amd.utils.graph import GraphedDepth
            if graphed is None or tuple(graphed.rgb.shape) != tuple(frame.shape):
                wrapper.eval()
                graphed = GraphedDepth(wrapper.depth_net, frame)
            depth = inv2depth(graphed(frame)['inv_depths'][0][0])
        else:
            depth = infer_depth(wrapper, frame)
        save_depth(os.path.join(args.output, '%08d' % ctr), depth[0, 0], png=not args.no_png)
    print('wrote %d depth maps to %s' % (len(images), args.output))
    if analyse:
        run_analysis(config, args.output)


if __name__ == '__main__':
    main()
