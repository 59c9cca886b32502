"""Data formats of the depth-edge training set (data half) -- the pieces of the reference's
packnet_sfm/datasets/gta_dataset.py and augmentations.py that define WHAT the training batch contains:

  * the 8-column split file (gta_dataset.py:184-211): image, depth, edge, lidar, seg, rgb_edge, rgb_edge_for_loss, normal
  * multi-scale annotation naming (gta_dataset.py:366-369,414-418): ``..._000.png`` plus ``_001`` .. ``_003`` for the
    half / quarter / eighth resolution edge and normal maps
  * target preparation, on the device: edges / 255, normals de-quantised from uint8 to radians, sparse maps resized with
    ``resize_depth_preserve`` (augmentations.py:58-100,159-217)

File decoding (PNG / .npy readers) stays on the host with PIL / numpy, as upstream; everything arithmetic runs in the
HIP library (csrc/data_prep.hip) on CUDA tensors -- host tensors raise MteError.
"""
import os

import torch

SPLIT_COLUMNS = ('rgb', 'depth', 'edge', 'lidar', 'seg', 'rgb_edge', 'rgb_edge_for_loss', 'normal')


def parse_split_line(line):
    """One line of the split file -> {column: path or None} following gta_dataset.py:184-211 (space separated, a trailing
    newline column is dropped, the literal 'None' marks an absent seg / rgb_edge / normal file)."""
    names = line.split(' ')
    if names[-1] == '\n':
        names = names[:-1]
    rec = {}
    for col, name in zip(SPLIT_COLUMNS, names):
        path = name.split('\n')[0]
        rec[col] = None if path in ('None', '') else path
    return rec


def read_split(path):
    with open(path, 'r') as f:
        return [parse_split_line(line) for line in f.readlines() if line.strip()]


def multiscale_paths(path_000, require_existing=True):
    """[scale 0, 1, 2, 3] file names of an edge / normal annotation (gta_dataset.py:366-369: the stem before '_000' plus
    '_00N.png'); with require_existing only scale 0 is returned when '_001.png' is not on disk, like the reference."""
    stem = path_000.split('_000')[0]
    if require_existing and not os.path.exists(stem + '_001.png'):
        return [path_000]
    return [path_000] + [stem + '_00' + str(i) + '.png' for i in range(1, 4)]


def _u8(t):
    from .. import kernels as K
    K._require_gpu(t)
    if t.dtype != torch.uint8:
        raise ValueError("expected the uint8 map read from the PNG, got {}".format(t.dtype))
    return t.contiguous()


def edge_target(edge_u8):
    """uint8 edge annotation -> float32 target: /255 when the map is on the 0..255 scale (max > 1), unchanged otherwise
    (augmentations.py:186-188).  One host read (the maximum) per map, as upstream."""
    from .. import kernels as K
    src = _u8(edge_u8)
    if not bool(src.max() > 1):
        return src.float()
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    K.lib.mte_edge_target_from_u8(src.data_ptr(), out.data_ptr(), src.numel(), K._stream())
    return out


def normal_target(normal_u8):
    """uint8 normal annotation -> radians: (360 * (v / 255) - 180) * pi / 180 (gta_dataset.py:407-409), float64 inside."""
    from .. import kernels as K
    src = _u8(normal_u8)
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    K.lib.mte_normal_target_from_u8(src.data_ptr(), out.data_ptr(), src.numel(), K._stream())
    return out


def resize_depth_preserve(depth, shape):
    """augmentations.py:58-100 for float maps [h,w] / [B,h,w] on the device -> [H,W] / [B,H,W]: every valid (> 0) pixel
    moves to (int(y*H/h), int(x*W/w)); the last one in raster order wins a shared target; zeros elsewhere."""
    from .. import kernels as K
    K._require_gpu(depth)
    squeeze = depth.dim() == 2
    src = (depth.unsqueeze(0) if squeeze else depth).detach().float().contiguous()
    if src.dim() != 3:
        raise ValueError("expected [h,w] or [B,h,w], got {}".format(tuple(depth.shape)))
    if not isinstance(shape, (tuple, list)):
        shape = tuple(int(s * shape) for s in src.shape[-2:])               # a single number is a resize ratio (:78-79)
    B, h, w = src.shape
    H, W = int(shape[0]), int(shape[1])
    out = torch.empty((B, H, W), dtype=torch.float32, device=src.device)
    ws = torch.empty((B, H, W), dtype=torch.int32, device=src.device)
    K.lib.mte_resize_depth_preserve(src.data_ptr(), B, h, w, out.data_ptr(), H, W, ws.data_ptr(), K._stream())
    return out[0] if squeeze else out


def prepare_edge_sample(edge_maps_u8, normal_maps_u8, shape):
    """The edge / normal part of resize_sample (augmentations.py:178-211) for one sample: lists of uint8 maps for scales
    0..3 (CUDA tensors [h_s,w_s]) -> {'edge', 'edge_1'.., 'normal', 'normal_1'..} float32 [1,H_s,W_s] with H_s = H >> s.
    Normals keep their size when it already is the target size; otherwise they are resized bilinearly like cv2.resize
    (parity-unpinned restatement, utils/edge.py::resize_linear)."""
    from ..utils.edge import resize_linear
    H, W = int(shape[0]), int(shape[1])
    out = {}
    for s, e in enumerate(edge_maps_u8):
        key = 'edge' if s == 0 else 'edge_%d' % s
        tgt = (int(H / (2 ** s)), int(W / (2 ** s)))
        resized = resize_depth_preserve(_u8(e).float(), tgt)
        out[key] = (resized / 255.0 if bool(resized.max() > 1) else resized).unsqueeze(0)
    for s, n in enumerate(normal_maps_u8):
        key = 'normal' if s == 0 else 'normal_%d' % s
        tgt = (int(H / (2 ** s)), int(W / (2 ** s)))
        rad = normal_target(n)
        out[key] = (rad if tuple(rad.shape) == tgt else resize_linear(rad, tgt)).unsqueeze(0)
    return out


# ---- a reader on top of the formats above -------------------------------------------------------------------------------
# File decoding is host I/O (PIL / numpy, the reference uses PIL and cv2.imread); everything after it -- the crop, the LANCZOS
# resize of the frame, colour jitter and ToTensor (image_prep.py), sparse resizes, target scaling, de-quantisation -- runs on the
# device, and so do the LiDAR column's projection and perturbation (lidar_prep.py).  Not rebuilt: the colour matrix, context frames.

def _read_gray_u8(path):
    """cv2.imread(path)[:, :, 0] of the reference for the 8-bit single-channel annotation PNGs."""
    import numpy as np
    from PIL import Image
    if path.endswith('.npy'):
        return np.load(path)
    a = np.array(Image.open(path))
    return a if a.ndim == 2 else a[:, :, -1 if a.shape[2] >= 3 else 0]      # OpenCV channel 0 is blue = PIL's channel 2


def read_png_depth(path):
    """KITTI 16-bit depth PNG -> float32 metres, -1 where there is no return (reference kitti_dataset.py:40-46)."""
    import numpy as np
    from PIL import Image
    if path.endswith('.npy'):
        return np.load(path).astype(np.float32)
    png = np.array(Image.open(path), dtype=int)
    assert png.max() > 255, 'Wrong .png depth file'
    depth = png.astype(np.float32) / 256.
    depth[png == 0] = -1.
    return depth


class KittiEdgeSplitDataset:
    """One sample per split-file line: rgb (cropped, LANCZOS-resized to ``image_shape`` like the reference's resize_image, colour
    jittered, /255 -- on the device, image_prep.py), depth (resize_depth_preserve), edge / edge_1..3 and normal / normal_1..3 targets.
    ``__getitem__`` returns device tensors shaped like the reference's collated sample with batch size 1 removed: rgb [3,H,W],
    depth [1,H,W], ...

    jittering = (brightness, contrast, saturation, hue) draws the reference's colour jitter per sample from Python's ``random``
    (the sample then also carries the un-jittered ``rgb_original``); crop_train_borders crops rgb, depth, edge and normal
    before the resize like crop_sample.  Both default to () = off.

    input_depth_type (None, '' or [''] = off) switches the split's LiDAR column on (.png / .npy / velodyne .bin, lidar_prep.py): cropped
    and resized like the depth map it becomes ``lidar`` and ``input_depth``; with lidar_scale and lidar_add both non-empty (2 x 3 ranges,
    reference augment_depth_values) the ``input_depth`` copy is perturbed with lidar_drop_rate, drawing from ``np.random``.

    mode 'validation' / 'test' (default 'train') returns the reference's validation_transforms / test_transforms sample instead
    (datasets/eval_prep.py): crop_eval_borders crops rgb, input_depth and rgb_edge only, validation takes its size from the frame, test
    resizes to image_shape when one is given (() = not at all); depth keeps its native size; no jitter, no perturbation, no normals.
    with_filename (the config-driven loaders set it) adds the reference's ``filename = '<split stem>_%010d' % idx`` to these samples."""

    def __init__(self, split_file, image_shape, device='cuda', root='', jittering=(), crop_train_borders=(), input_depth_type=None,
                 lidar_scale=(), lidar_add=(), lidar_drop_rate=0.0, mode='train', crop_eval_borders=(), with_filename=False):
        if mode not in ('train', 'validation', 'test'):
            raise ValueError("Unknown mode {}".format(mode))
        self.mode = mode
        self.crop_eval_borders = tuple(crop_eval_borders or ())
        self.records = read_split(split_file)
        self.split = split_file.split('/')[-1].split('.')[0]               # gta_dataset.py:149, the stem of the evaluation samples' 'filename'
        self.with_filename = bool(with_filename)
        # the evaluation modes take their size from the frame (validation) or resize only when a shape is given (test)
        self.shape = (int(image_shape[0]), int(image_shape[1])) if image_shape is not None and len(image_shape) > 0 else ()
        self.device = torch.device(device)
        self.root = root
        self.jittering = tuple(jittering or ())
        self.crop_train_borders = tuple(crop_train_borders or ())
        types = [input_depth_type] if isinstance(input_depth_type, str) else list(input_depth_type or [])
        self.with_input_depth = any(t not in (None, '') for t in types)
        self.lidar_scale, self.lidar_add = tuple(lidar_scale or ()), tuple(lidar_add or ())
        self.lidar_drop_rate = float(lidar_drop_rate)

    def __len__(self):
        return len(self.records)

    def _p(self, path):
        return path if os.path.isabs(path) or not self.root else os.path.join(self.root, path)

    def _u8_map(self, path, borders):
        import numpy as np
        a = _read_gray_u8(path)
        if borders is not None:
            a = a[borders[1]:borders[3], borders[0]:borders[2]]               # crop_depth, augmentations.py:425-444
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(self.device)

    def _map(self, path):
        """an annotation map as its file holds it: uint8 (PNG) or float32 (.npy), on the device"""
        import numpy as np
        a = _read_gray_u8(path)
        a = a.astype(np.uint8) if a.dtype.kind in 'ub' else a.astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _eval_item(self, idx):
        """mode 'validation' / 'test': the files decoded on the host as in training, then eval_prep.validation_sample / test_sample on the
        device (the reference's validation_transforms / test_transforms, datasets/transforms.py:53-125)."""
        import numpy as np
        from PIL import Image
        from . import eval_prep as ep
        rec = self.records[idx]
        img = Image.open(self._p(rec['rgb'])).convert('RGB')
        sample = {'idx': idx, 'rgb': torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).to(self.device)}
        if self.with_filename:
            sample['filename'] = '%s_%010d' % (self.split, idx)            # gta_dataset.py:339: what save_depth names its files after
        d_full = None
        if rec.get('depth'):
            d_full = read_png_depth(self._p(rec['depth']))
            sample['depth'] = torch.from_numpy(d_full).to(self.device)
        if self.with_input_depth and rec.get('lidar'):
            from . import lidar_prep as lp
            sample['input_depth'] = lp.read_lidar_map(self._p(rec['lidar']), self.device, depth_map=d_full)
        if rec.get('edge'):
            for s, p in enumerate(multiscale_paths(self._p(rec['edge']))):
                sample['edge' if s == 0 else 'edge_%d' % s] = self._map(p)
        if rec.get('rgb_edge'):
            sample['rgb_edge'] = self._map(self._p(rec['rgb_edge']))
        if self.mode == 'validation':
            return ep.validation_sample(sample, self.crop_eval_borders)
        return ep.test_sample(sample, self.shape, self.crop_eval_borders)

    def __getitem__(self, idx):
        if self.mode != 'train':
            return self._eval_item(idx)
        import numpy as np
        from PIL import Image
        from . import image_prep as ip
        rec = self.records[idx]
        H, W = self.shape
        img = Image.open(self._p(rec['rgb'])).convert('RGB')
        borders = ip.parse_crop_borders(self.crop_train_borders, img.size[::-1]) if self.crop_train_borders else None
        frame = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).to(self.device)
        if borders is not None or img.size != (W, H):
            frame = ip.resize_image_u8(frame, (H, W), crop=borders)          # crop_image + transforms.Resize(shape, ANTIALIAS), augmentations.py:16-35
        params = ip.draw_color_jitter(self.jittering)
        sample = {'idx': idx}
        if self.jittering:
            rgb, original = ip.color_jitter_to_tensor(frame.unsqueeze(0), [params], want_original=True)
            sample['rgb'], sample['rgb_original'] = rgb[0], original[0]
        else:
            sample['rgb'] = ip.color_jitter_to_tensor(frame.unsqueeze(0))[0]
        d = None
        if rec.get('depth'):
            d = d_full = read_png_depth(self._p(rec['depth']))
            if borders is not None:
                d = np.ascontiguousarray(d[borders[1]:borders[3], borders[0]:borders[2]])
            sample['depth'] = resize_depth_preserve(torch.from_numpy(d).to(self.device), self.shape).unsqueeze(0)
        if self.with_input_depth and rec.get('lidar'):
            from . import lidar_prep as lp
            lidar = lp.read_lidar_map(self._p(rec['lidar']), self.device, depth_map=d_full if d is not None else None)   # gta_dataset.py:368-382
            if borders is not None:
                lidar = lidar[borders[1]:borders[3], borders[0]:borders[2]].contiguous()
            lidar = resize_depth_preserve(lidar, self.shape)
            sample['lidar'] = lidar.unsqueeze(0)
            if len(self.lidar_scale) > 0 and len(self.lidar_add) > 0:        # transforms.py:46-48: only the network's input is perturbed
                sample['input_depth'] = lp.augment_depth_values(lidar, self.lidar_scale, self.lidar_add, self.lidar_drop_rate).unsqueeze(0)
            else:
                sample['input_depth'] = lidar.clone().unsqueeze(0)
        edges, normals = [], []
        # crop_sample crops 'edge' and 'normal' only: the coarser scales keep their frame (augmentations.py:512-518)
        if rec.get('edge'):
            edges = [self._u8_map(p, borders if s == 0 else None) for s, p in enumerate(multiscale_paths(self._p(rec['edge'])))]
        if rec.get('normal'):
            normals = [self._u8_map(p, borders if s == 0 else None) for s, p in enumerate(multiscale_paths(self._p(rec['normal'])))]
        sample.update(prepare_edge_sample(edges, normals, self.shape))
        return sample


def collate(samples):
    out = {}
    for k in samples[0]:
        vals = [s[k] for s in samples]
        out[k] = torch.stack(vals) if torch.is_tensor(vals[0]) else vals
    return out


class SplitLoader:
    """Minimal epoch iterator: rank-strided, fixed order or shuffled per epoch (``set_epoch``), drops the ragged tail."""

    def __init__(self, dataset, batch_size, rank=0, world=1, shuffle=True, seed=0):
        self.ds, self.bs, self.rank, self.world, self.shuffle, self.seed, self.epoch = dataset, batch_size, rank, world, shuffle, seed, 0
        self.sampler = self                                           # Trainer.fit calls loader.sampler.set_epoch(epoch)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.ds) // self.world // self.bs

    def __iter__(self):
        order = torch.randperm(len(self.ds), generator=torch.Generator().manual_seed(self.seed + self.epoch)).tolist() \
            if self.shuffle else list(range(len(self.ds)))
        mine = order[self.rank::self.world]
        for i in range(len(self)):
            yield collate([self.ds[j] for j in mine[i * self.bs:(i + 1) * self.bs]])


def _as_tuple(v):
    """a YAML list, a tuple or the reference's string form '(0.2, 0.2, 0.2, 0.05)' -> tuple; None / '' -> ()"""
    if v is None or v == '':
        return ()
    return tuple(eval(v)) if isinstance(v, str) else tuple(v)


def make_loader(config, rank, world):
    """``train_edges.py --data mindtheedge_amd.datasets.kitti_edges:make_loader``: config.datasets.train.split[0] is the
    8-column split file, config.datasets.train.path[0] (optional) the root folder of its relative paths;
    config.datasets.augmentation.jittering / .crop_train_borders as in the reference (default (): off);
    config.datasets.train.input_depth_type and config.datasets.augmentation.lidar_scale / lidar_add / lidar_drop_rate for the LiDAR column.
    config.datasets.train.num_workers (default 0) > 0 returns the prefetching loader (datasets/prefetch.py: same batches, decoded on that
    many threads config.datasets.train.prefetch batches ahead) instead of SplitLoader."""
    tr = config.datasets.train
    shape = config.datasets.augmentation.image_shape
    shape = eval(shape) if isinstance(shape, str) else tuple(shape)
    root = (tr.get('path') or [''])[0] if isinstance(tr.get('path'), (list, tuple)) else (tr.get('path') or '')
    split = tr['split'][0] if isinstance(tr['split'], (list, tuple)) else tr['split']
    aug = config.datasets.augmentation
    ds = KittiEdgeSplitDataset(split, shape, device=torch.device('cuda', torch.cuda.current_device()), root=root,
                               jittering=_as_tuple(aug.get('jittering')), crop_train_borders=_as_tuple(aug.get('crop_train_borders')),
                               input_depth_type=tr.get('input_depth_type'), lidar_scale=_as_tuple(aug.get('lidar_scale')),
                               lidar_add=_as_tuple(aug.get('lidar_add')), lidar_drop_rate=float(aug.get('lidar_drop_rate') or 0.0))
    from .prefetch import PrefetchSplitLoader, choose_loader
    if choose_loader(tr.get('num_workers')) == 'prefetch':
        return PrefetchSplitLoader(ds, int(tr.batch_size), rank, world, num_workers=int(tr.get('num_workers')),
                                   prefetch=int(tr.get('prefetch') or 2))
    return SplitLoader(ds, int(tr.batch_size), rank, world)


# ---- evaluation loaders (reference setup_dataset / setup_dataloader, models/model_wrapper.py:675-790) ---------------------------------

def shard_indices(n, rank, world):
    """The frames of rank ``rank``: r, r + world, ... in file order, nothing padded.  The reference's DistributedSampler repeats frames to
    even the ranks out and all_reduce_metrics removes the repeats by 'idx'; here every frame is seen exactly once and
    ModelWrapper.validation_epoch_end divides the summed metrics by the summed count."""
    return list(range(int(n)))[int(rank)::int(world)]


class EvalLoader:
    """File order, rank-strided (shard_indices), keeps the ragged tail.  Frames of one batch must share their sizes."""

    def __init__(self, dataset, batch_size=1, rank=0, world=1):
        self.ds, self.bs, self.rank, self.world = dataset, max(int(batch_size), 1), rank, world

    def indices(self):
        return shard_indices(len(self.ds), self.rank, self.world)

    def __len__(self):
        return (len(self.indices()) + self.bs - 1) // self.bs

    def __iter__(self):
        mine = self.indices()
        for i in range(0, len(mine), self.bs):
            samples = [self.ds[j] for j in mine[i:i + self.bs]]
            for s in samples[1:]:
                for k, v in s.items():
                    if torch.is_tensor(v) and tuple(v.shape) != tuple(samples[0][k].shape):
                        raise ValueError("batch_size {} needs frames of one size: '{}' is {} in frame {} and {} in frame {}".format(
                            self.bs, k, tuple(samples[0][k].shape), samples[0]['idx'], tuple(v.shape), s['idx']))
            yield collate(samples)


def _at(values, i, default=''):
    """entry i of a per-dataset list of the config; a scalar or a one-entry list counts for every dataset (default_config.py: [''])"""
    if not isinstance(values, (list, tuple)):
        return default if values is None else values
    if len(values) == 0:
        return default
    return values[i] if i < len(values) else values[-1]


def _make_eval_loaders(config, mode, rank, world):
    section = config.datasets[mode]
    splits = section.get('split') or []
    splits = [splits] if isinstance(splits, str) else list(splits)
    aug = config.datasets.augmentation
    shape = aug.get('image_shape')
    shape = _as_tuple(shape)
    loaders = []
    for i, split in enumerate(splits):
        name = _at(section.get('dataset'), i, 'KITTI')
        if name not in ('KITTI', 'GTA'):                                  # both are the 8-column split reader (model_wrapper.py:700-735)
            raise ValueError("Unknown dataset {} (KITTI and GTA read the 8-column split file)".format(name))
        root = _at(section.get('path'), i, '')
        split_file = split if os.path.isabs(split) or os.path.exists(split) or not root else os.path.join(root, split)
        ds = KittiEdgeSplitDataset(split_file, shape, device=torch.device('cuda', torch.cuda.current_device()), root=root,
                                   input_depth_type=_at(section.get('input_depth_type'), i, ''), mode=mode,
                                   crop_eval_borders=_as_tuple(aug.get('crop_eval_borders')), with_filename=True)
        loaders.append(EvalLoader(ds, int(section.get('batch_size') or 1), rank, world))
    return loaders


def make_val_loaders(config, rank=0, world=1):
    """One EvalLoader per entry of config.datasets.validation.split ([] without one); path / depth_type / input_depth_type per index."""
    return _make_eval_loaders(config, 'validation', rank, world)


def make_test_loaders(config, rank=0, world=1):
    return _make_eval_loaders(config, 'test', rank, world)
