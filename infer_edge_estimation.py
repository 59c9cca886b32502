#!/usr/bin/env python3
"""infer_edge_estimation.py -- compute core of the reference's depth-edge annotation driver
(/root/reference/infer_edge_estimation.py:119-259) on the MI355X: for one frame

    pred = model_wrapper.depth(image [, lidar / 200])['inv_depths'][0]            (:181-183, :216, :232)
    for every scale: probability = pred[scale] / 2 -> uint8 normals -> NMS -> hysteresis   (:186-206, :234-256)

with the network (RGB-only pass and, with a LiDAR map, the RGB+LiDAR pass through the sparse SAN branch) and the whole
post-processing on the device.  ``--split FILE --save DIR`` is the reference's driver loop (:79-117): column 0 (frame) and column 3
(LiDAR map: .png / .bin / .npy, mindtheedge_amd/datasets/lidar_prep.py) of every split line are read, ``DIR/NNNNNNNN_{regular,lidar}_00S.png``
(edges * 255) and ``DIR/normals/...`` are written and, at the end, the 8-column ``rgb_lidar_edges_split.txt`` that the training reader
takes.  ``annotate_frame`` returns device tensors; ``--synthetic`` runs it on synthetic frames and prints what would be written.  The RGB+LiDAR pass uses the parity-unpinned SAN branch
(DESIGN.md 4.12); the post-processing is the pinned / Sobel-unpinned row f-2.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # see mindtheedge_amd/__init__.py


def annotate_frame(model_wrapper, image, lidar_image=None, multiscale=True, nms=True, hysteresis=True, normals=True,
                   infer_rgb=True):
    """image: fp32 [1,3,H,W] in [0,1] on the GPU; lidar_image: fp32 [1,1,H,W] metres (zeros = no return) or None.
    -> {'regular': [(edges, normals), ...per scale], 'lidar': [...]}: edges float32 [1,H_s,W_s] (the reference writes
    edges * 255 as PNG), normals uint8 [1,H_s,W_s] or None.  Keys follow the reference's '_regular_00N' / '_lidar_00N' files."""
    import torch
    from mindtheedge_amd.utils.tools import annotate_edges
    scales = 4 if multiscale else 1
    model_wrapper.eval()
    out = {}
    with torch.no_grad():
        if infer_rgb:
            pred = model_wrapper.depth(image, rgb_edge=None)['inv_depths'][0]
            out['regular'] = annotate_edges(pred, nms=nms, hysteresis_=hysteresis, normals=normals, scales=scales)
        if lidar_image is not None:
            pred = model_wrapper.depth(image, lidar_image / 200.0, rgb_edge=None)['inv_depths'][0]      # reference :216 ("why 200???")
            out['lidar'] = annotate_edges(pred, nms=nms, hysteresis_=hysteresis, normals=normals, scales=scales)
    return out


def save_split_list(rgb_files, lidar_files, save_folder_edges, save_folder_normals):
    """``<edges folder>/rgb_lidar_edges_split.txt``, one line per annotated frame in the training reader's eight columns (reference
    :108-117): rgb, lidar (as depth), the scale-0 '_lidar' edge map, lidar, three absent columns, the scale-0 '_lidar' normal map."""
    with open(os.path.join(save_folder_edges, 'rgb_lidar_edges_split.txt'), 'w') as f:
        for ctr, (rgb, lidar) in enumerate(zip(rgb_files, lidar_files)):
            name = '%08d_lidar_000.png' % ctr
            f.write(' '.join([rgb, lidar, save_folder_edges + '/' + name, lidar, 'None', 'None', 'None', save_folder_normals + '/' + name]) + '\n')


def save_edges(path, edges):
    """edges * 255 as an 8-bit grey PNG, rounded and saturated (what cv2.imwrite does with a float array; infer_edges.save_depth's rule)"""
    import numpy as np
    from PIL import Image
    e = edges.detach().float().cpu().numpy().reshape(edges.shape[-2:])
    Image.fromarray(np.clip(np.rint(e * 255.0), 0, 255).astype(np.uint8)).save(path)


def annotate_split(model_wrapper, config, split_file, save_dir, image_shape):
    """The reference's loop over a split file (:79-103) -> number of frames.  datasets.test.is_infer_rgb / is_infer_lidar /
    input_depth_type select the passes as upstream (:183, :209)."""
    import torch
    from PIL import Image
    from infer_edges import load_frame
    from mindtheedge_amd.datasets.kitti_edges import resize_depth_preserve
    from mindtheedge_amd.datasets.lidar_prep import read_lidar_map
    test = config.datasets.test
    types = test.input_depth_type if isinstance(test.input_depth_type, (list, tuple)) else [test.input_depth_type]
    with_lidar = bool(types) and types[0] not in ('', None) and bool(test.is_infer_lidar)
    with open(split_file, 'r') as f:
        lines = [x.split('\n')[0].split(' ') for x in f.readlines() if x.strip()]
    files, lidar_files = [x[0] for x in lines], [x[3] for x in lines]
    normals_dir = save_dir + '/normals'
    os.makedirs(normals_dir, exist_ok=True)
    dev = torch.device('cuda', torch.cuda.current_device())
    for ctr, (fn, lidar_fn) in enumerate(zip(files, lidar_files)):
        image = load_frame(fn, image_shape).unsqueeze(0).to(dev)
        lidar = None
        if with_lidar:
            lidar = read_lidar_map(lidar_fn, dev, clamp_negative=True)                      # :211-220
            if tuple(lidar.shape) != tuple(image_shape):
                lidar = resize_depth_preserve(lidar, image_shape)
            lidar = lidar.unsqueeze(0).unsqueeze(0)
        out = annotate_frame(model_wrapper, image, lidar, infer_rgb=bool(test.is_infer_rgb))
        for key, per_scale in out.items():
            for s, (e, n) in enumerate(per_scale):
                name = '%08d_%s_%03d.png' % (ctr, key, s)
                save_edges(os.path.join(save_dir, name), e)
                if n is not None:
                    Image.fromarray(n.detach().cpu().numpy().reshape(n.shape[-2:])).save(os.path.join(normals_dir, name))
        print('Processed image ' + str(ctr + 1))
    save_split_list(files, lidar_files, save_dir, normals_dir)
    return len(files)


def main(argv=None):
    ap = argparse.ArgumentParser(description='depth-edge annotation (DEE inference + post-processing) on MI355X')
    ap.add_argument('--config', type=str, required=True, help='Input file (.yaml)')
    ap.add_argument('--synthetic', type=int, default=0, help='annotate N synthetic frames')
    ap.add_argument('--split', type=str, default='', help='annotate the frames (column 0) and LiDAR maps (column 3) of this split file')
    ap.add_argument('--save', type=str, default='', help='folder for the annotations of --split')
    ap.add_argument('--no-lidar', action='store_true')
    args = ap.parse_args(argv)
    assert args.config.endswith('.yaml'), 'You need to provide a .yaml file'
    import time
    import torch
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.utils.config import load_config
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    config = load_config(args.config, {'model': {'depth_net': {'with_san': not args.no_lidar}}})
    config.model.depth_net.checkpoint_path = config.model.depth_net.checkpoint_path if os.path.exists(
        config.model.depth_net.checkpoint_path or '') else ''
    K.set_compute_dtype('bf16')
    wrapper = ModelWrapper(config).cuda().eval()
    H, W = tuple(config.datasets.augmentation.image_shape) if not isinstance(config.datasets.augmentation.image_shape, str) \
        else eval(config.datasets.augmentation.image_shape)
    if args.split:
        assert args.save, '--split needs --save DIR'
        n = annotate_split(wrapper, config, args.split, args.save, (H, W))
        print('annotated %d frames into %s' % (n, args.save))
        return
    assert args.synthetic > 0, 'file readers are not part of this build: pass --synthetic N or call annotate_frame() on your tensors'
    g = torch.Generator(device='cuda').manual_seed(0)
    t0 = None
    for i in range(args.synthetic + 1):
        if i == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        image = torch.rand(1, 3, H, W, generator=g, device='cuda')
        lidar = None if args.no_lidar else (torch.rand(1, 1, H, W, generator=g, device='cuda') < 0.05).float() * \
            (2 + 70 * torch.rand(1, 1, H, W, generator=g, device='cuda'))
        out = annotate_frame(wrapper, image, lidar)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(args.synthetic, 1)
    for key, per_scale in out.items():
        for s, (e, n) in enumerate(per_scale):
            print('%08d_%s_%03d.png  edges %s kept %d   normals %s' % (args.synthetic - 1, key, s, tuple(e.shape), int((e > 0).sum()),
                                                                      None if n is None else tuple(n.shape)))
    print('%.2f ms per frame (%s passes, 4 scales, post-processing on device)' % (dt * 1e3, ' + '.join(out.keys())))


if __name__ == '__main__':
    main()
