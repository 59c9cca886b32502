"""save_depth / save_paths_list of the reference (packnet_sfm/utils/save.py): per test sample
``<save.folder>/depth/<dataset prefix>/<basename of save.pretrained>/<filename>_{depth.npz,depth.png,rgb.png,viz.png}``.

The colour image is made on the device (utils/depth.py::viz_inv_depth, csrc/depth_viz.hip) and crosses to the host as uint8; the RGB
frame is rounded to uint8 on the device as well.  Both PNGs are what cv2.imwrite writes for the reference's float images (round half to
even, saturating; parity-unpinned against OpenCV) and are stored in RGB order, as the reference's channel flip in front of cv2 leaves them."""
import os

import numpy as np
import torch

from .depth import inv2depth, viz_inv_depth, write_depth


def save_paths_list(paths, out_path, file_name):
    assert file_name is not None
    out_file_name = os.path.join(out_path, file_name)
    print(out_file_name)
    with open(out_file_name, 'w') as f:
        for item in paths:
            f.write("%s\n" % item)


def prepare_dataset_prefix(config, dataset_idx):
    """utils/logging.py:35-63: the path's stem, then -<split stem>, -<depth_type> and -<camera> where given."""
    prefix = '{}'.format(os.path.splitext(config.path[dataset_idx].split('/')[-1])[0])
    if config.split[dataset_idx] != '' and '{' not in config.split[dataset_idx]:
        prefix += '-{}'.format(os.path.splitext(os.path.basename(config.split[dataset_idx]))[0])
    if config.depth_type[dataset_idx] != '':
        prefix += '-{}'.format(config.depth_type[dataset_idx])
    if len(config.cameras[dataset_idx]) == 1:
        prefix += '-{}'.format(config.cameras[dataset_idx][0])
    return prefix


def write_image_u8(filename, image_u8):
    """uint8 [H,W,3] RGB (device or host tensor, or array) -> PNG"""
    from PIL import Image
    a = image_u8.detach().cpu().numpy() if hasattr(image_u8, 'detach') else np.asarray(image_u8)
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).save(filename)


def save_depth(batch, output, args, dataset, save):
    """batch: the collated test batch ('rgb' [B,3,H,W] in [0,1], 'filename' a list, optionally 'intrinsics'); output: evaluate_depth's
    ('inv_depth' [B,1,H,W]); args: the step arguments (args[1] = dataset index); dataset: config.datasets.test; save: config.save."""
    if not save or save.folder == '' or save.folder is None:
        return
    flags = save.depth
    if not (flags.rgb or flags.viz or flags.npz or flags.png):
        return
    rgb = batch['rgb']
    pred_inv_depth = output['inv_depth']
    filename = batch['filename']
    if isinstance(filename, str):
        filename = [filename]
    dataset_idx = 0 if args is None or len(args) < 2 or args[1] is None else int(args[1])
    save_path = os.path.join(save.folder, 'depth', prepare_dataset_prefix(dataset, dataset_idx),
                             os.path.basename(save.pretrained or '').split('.')[0])
    os.makedirs(save_path, exist_ok=True)
    for i in range(rgb.shape[0]):
        if flags.npz:
            write_depth('{}/{}_depth.npz'.format(save_path, filename[i]), depth=inv2depth(pred_inv_depth[i]),
                        intrinsics=batch['intrinsics'][i] if 'intrinsics' in batch else None)
        if flags.png:
            write_depth('{}/{}_depth.png'.format(save_path, filename[i]), depth=inv2depth(pred_inv_depth[i]))
        if flags.rgb:
            rgb_i = (rgb[i].detach().float().permute(1, 2, 0) * 255).round().clamp(0, 255).to(torch.uint8)
            write_image_u8('{}/{}_rgb.png'.format(save_path, filename[i]), rgb_i)
        if flags.viz:
            write_image_u8('{}/{}_viz.png'.format(save_path, filename[i]), viz_inv_depth(pred_inv_depth[i]))
