"""The pieces under the prefetching training loader (datasets/prefetch.py):

  * ``decode_train_record``   host stage: the files of one split record as numpy arrays, nothing else.  It runs on worker threads and
                              touches neither ``torch.cuda`` nor the kernel library: all device work is the consumer thread's.
                              With the LiDAR column it also reads that file, raw, and counts the returns of the resized map.
  * ``plan_targets``          the descriptor rows (csrc/batch_prep.hip) and the output layout of a batch's depth / LiDAR / edge / normal targets
  * ``HostArena`` / ``pack_arena``   the raw arrays of a batch and the descriptor table in ONE buffer at 16-byte-aligned offsets, so that
                              a batch is one upload
  * ``prepare_targets``       device stage: ``mte_batch_prep`` over the uploaded arena -> {'depth', 'edge', .., 'normal', ..} float32
                              [B,1,H_s,W_s], written in place (no torch.stack), without a host read

File conventions are those of kitti_edges.py (``_read_gray_u8``, ``read_png_depth``, ``multiscale_paths``); the arithmetic is that of
``prepare_edge_sample`` / ``resize_depth_preserve``, bit for bit.
"""
import os

import numpy as np

EDGE_U8, SPARSE_U16, SPARSE_F32, NORMAL_U8 = 0, 1, 2, 3                  # MTE_PREP_* of include/mte_kernels.h
ROW_WORDS = 12                                                           # MTE_BATCH_PREP_ROW_WORDS
ALIGN = 16
_KIND_DTYPE = {EDGE_U8: np.uint8, SPARSE_U16: np.uint16, SPARSE_F32: np.float32, NORMAL_U8: np.uint8}


def scale_key(name, s):
    return name if s == 0 else '%s_%d' % (name, s)


def _read_depth_raw(path):
    """read_png_depth without its arithmetic: a 16-bit PNG stays uint16 (0 = no return; the device divides by 256), a .npy is float32.
    A PNG whose values do not fit 16 bits is converted here as read_png_depth does (rare: PIL mode 'I' files)."""
    from PIL import Image
    if path.endswith('.npy'):
        return np.load(path).astype(np.float32)
    png = np.asarray(Image.open(path))
    assert png.max() > 255, 'Wrong .png depth file'
    if png.dtype == np.uint16:
        return png
    if png.dtype.kind in 'ui' and png.min() >= 0 and png.max() <= 65535:
        return png.astype(np.uint16)
    depth = png.astype(int).astype(np.float32) / 256.
    depth[png == 0] = -1.
    return depth


def decode_train_record(rec, root='', with_lidar=False, lidar_raw=True, crop_borders=(), shape=None):
    """One record of the split file (kitti_edges.parse_split_line) -> {'rgb': uint8 [h,w,3], 'depth': uint16 [h,w] (.png) / float32 (.npy) /
    None, 'edge': [uint8 [h_s,w_s] per scale], 'normal': [...]}.  with_lidar adds 'lidar_path' (resolved) and 'lidar': the file's map, raw
    (lidar_prep.read_lidar_raw: uint16 for a 16-bit .png, float32 for .npy / .npz) -- or None for a velodyne .bin, whose batch goes through
    the per-sample functions at hand-over (lidar_batchable), and with lidar_raw=False (the per-sample path for every batch).  With shape
    (the dataset's (H, W); crop_borders its crop_train_borders) it also adds 'lidar_cells': the returns of the cropped and resized map
    (lidar_prep.resized_cells), so that the count the draws depend on is known before the batch is handed over.  Pure file decoding and
    numpy; safe on any thread."""
    from PIL import Image
    from .kitti_edges import _read_gray_u8, multiscale_paths

    def p(path):
        return path if os.path.isabs(path) or not root else os.path.join(root, path)

    out = {'rgb': np.asarray(Image.open(p(rec['rgb'])).convert('RGB'), dtype=np.uint8), 'depth': None, 'edge': [], 'normal': []}
    if rec.get('depth'):
        out['depth'] = np.ascontiguousarray(_read_depth_raw(p(rec['depth'])))
    for name in ('edge', 'normal'):
        if rec.get(name):
            out[name] = [np.ascontiguousarray(_read_gray_u8(q).astype(np.uint8)) for q in multiscale_paths(p(rec[name]))]
    if with_lidar:
        out['lidar_path'] = p(rec['lidar']) if rec.get('lidar') else None
        out['lidar'] = out['lidar_cells'] = None
        if out['lidar_path'] and lidar_raw:
            from . import lidar_prep as lp
            out['lidar'] = lp.read_lidar_raw(out['lidar_path'])
            if out['lidar'] is not None and shape is not None:
                out['lidar_cells'] = lp.resized_cells(out['lidar'], lidar_window(out, crop_borders), shape)
    return out


def lidar_window(smp, crop_borders):
    """the crop window of a sample's LiDAR map: crop_train_borders are resolved against the frame, as for every other map of the sample"""
    from .image_prep import parse_crop_borders
    borders = parse_crop_borders(crop_borders, smp['rgb'].shape[:2]) if crop_borders else None
    return crop_window(borders, *smp['lidar'].shape)


def lidar_batchable(samples):
    """True where the LiDAR column of this batch goes through the batched pass: every sample carries a decoded map.  One velodyne .bin
    (its return count depends on the device projection) sends the whole batch through the per-sample functions."""
    return all(s.get('lidar') is not None for s in samples)


def crop_window(borders, h, w):
    """(x, y, height, width) of ``a[top:bottom, left:right]`` on an h x w map (numpy's slicing clamps to the map); None = the whole map"""
    if borders is None:
        return 0, 0, h, w
    left, top, right, bottom = (int(v) for v in borders)
    x0, x1, y0, y1 = min(left, w), min(right, w), min(top, h), min(bottom, h)
    if x1 <= x0 or y1 <= y0:
        raise ValueError("crop window {} leaves nothing of a {} x {} map".format(tuple(borders), h, w))
    return x0, y0, y1 - y0, x1 - x0


def plan_targets(samples, borders, shape, lidar=False):
    """samples: decode_train_record results of one batch; borders: per sample (left, top, right, bottom) or None; shape: (H, W).
    -> (arrays, rows, keys, fallbacks, winner_elems, out_elems):
      arrays        the source maps, in row order (the arena packs them)
      rows          int64 [n, ROW_WORDS] with src_off still 0 (pack_arena fills it in)
      keys          [(key, (H_s, W_s), first element in the output arena)] in the order of the collated sample; every key is
                    [B,1,H_s,W_s]; preserve-resized keys come first in the arena (their winner words share the offsets)
      fallbacks     [(key, b, index into arrays, crop window)]: normal maps that are not at their target size (mte_resize_linear path)
    lidar: also lay out the decoded LiDAR maps (lidar_batchable) as the key 'lidar' behind 'depth': sparse rows with the scale-0 crop window,
    like the depth map.  Every sample of a batch must carry the same maps (as kitti_edges.collate requires)."""
    H, W = int(shape[0]), int(shape[1])
    B = len(samples)
    first = samples[0]
    layout = []                                                          # (key, kind group, tgt)
    if first['depth'] is not None:
        layout.append(('depth', 'depth', 0, (H, W)))
    if lidar:
        if not lidar_batchable(samples):
            raise KeyError("the LiDAR maps of this batch are not all decoded: it takes the per-sample path")
        layout.append(('lidar', 'lidar', 0, (H, W)))
    for name in ('edge', 'normal'):
        for s in range(len(first[name])):
            layout.append((scale_key(name, s), name, s, (int(H / (2 ** s)), int(W / (2 ** s)))))
    for smp in samples[1:]:
        if (smp['depth'] is None) != (first['depth'] is None) or len(smp['edge']) != len(first['edge']) or len(smp['normal']) != len(first['normal']):
            raise KeyError("the records of one batch carry different maps (depth / edge scales / normal scales)")
    offsets, cursor = {}, 0
    for resized in (True, False):                                        # normals last: no winner words for them
        for key, name, s, tgt in layout:
            if (name != 'normal') == resized:
                offsets[key] = cursor
                cursor += -(-B * tgt[0] * tgt[1] // 4) * 4              # keys start on 16 bytes
        if resized:
            winner_elems = cursor
    out_elems = max(cursor, 1)
    arrays, rows, fallbacks = [], [], []
    for key, name, s, tgt in layout:
        for b, smp in enumerate(samples):
            a = smp[name] if name in ('depth', 'lidar') else smp[name][s]
            if a.ndim != 2:
                raise ValueError("'{}' of sample {} is a {} array, expected [h,w]".format(key, b, a.shape))
            h, w = a.shape
            x0, y0, ch, cw = crop_window(borders[b] if s == 0 else None, h, w)      # crop_sample crops scale 0 only
            if name in ('depth', 'lidar'):
                kind = SPARSE_U16 if a.dtype == np.uint16 else SPARSE_F32
            else:
                kind = EDGE_U8 if name == 'edge' else NORMAL_U8
            if kind == NORMAL_U8 and (ch, cw) != tgt:
                fallbacks.append((key, b, len(arrays), (x0, y0, ch, cw)))
                arrays.append(a)
                rows.append(None)
                continue
            arrays.append(a.astype(_KIND_DTYPE[kind], copy=False))
            rows.append([kind, 0, h, w, x0, y0, ch, cw, offsets[key] + b * tgt[0] * tgt[1], tgt[0], tgt[1], 0])
    keys = [(key, tgt, offsets[key]) for key, _, _, tgt in layout]
    return arrays, rows, keys, fallbacks, winner_elems, out_elems


def _up(n):
    return -(-int(n) // ALIGN) * ALIGN


def arena_layout(arrays, n_rows):
    """-> (table offset, [array offsets], total bytes): the table first, every array on a 16-byte boundary"""
    cursor = _up(n_rows * ROW_WORDS * 8)
    offs = []
    for a in arrays:
        offs.append(cursor)
        cursor = _up(cursor + a.nbytes)
    return 0, offs, max(cursor, ALIGN)


class HostArena:
    """A growing uint8 host buffer (pinned when ``pin``: the source of a non-blocking upload) with a numpy view on it."""

    def __init__(self, pin=False):
        self.pin, self.tensor, self.view = bool(pin), None, None

    @property
    def capacity(self):
        return 0 if self.tensor is None else int(self.tensor.numel())

    def reserve(self, nbytes):
        """room for nbytes; growing drops the old buffer (the caller has made sure nothing reads it any more) -> True if it grew"""
        if nbytes <= self.capacity:
            return False
        import torch
        self.tensor = torch.empty(_up(nbytes + nbytes // 4), dtype=torch.uint8, pin_memory=self.pin)      # head-room: KITTI's frame sizes differ by a few %
        self.view = self.tensor.numpy()
        return True


def pack_arena(arena, arrays, rows):
    """Copies the arrays and the descriptor table into ``arena`` (a HostArena with enough room: arena_layout) -> (table offset, array
    offsets, bytes used, indices of the rows in the table).  rows[i] is None for arrays that have no row (the normal fallback)."""
    live = [i for i, r in enumerate(rows) if r is not None]
    t_off, offs, total = arena_layout(arrays, len(live))
    if total > arena.capacity:
        raise ValueError("the arena holds {} bytes, the batch needs {}".format(arena.capacity, total))
    table = np.zeros((len(live), ROW_WORDS), dtype=np.int64)
    for j, i in enumerate(live):
        table[j] = rows[i]
        table[j, 1] = offs[i]
    arena.view[t_off:t_off + table.nbytes] = table.reshape(-1).view(np.uint8)
    for a, off in zip(arrays, offs):
        arena.view[off:off + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return t_off, offs, total, live


def unpack_arena(view, n_rows, t_off=0):
    """the table and the source maps back out of a packed arena (tests, debugging) -> (int64 [n, ROW_WORDS], [arrays])"""
    table = np.frombuffer(bytes(view[t_off:t_off + n_rows * ROW_WORDS * 8]), dtype=np.int64).reshape(n_rows, ROW_WORDS).copy()
    maps = []
    for kind, off, h, w in table[:, :4]:
        dt = np.dtype(_KIND_DTYPE[int(kind)])
        maps.append(np.frombuffer(bytes(view[off:off + h * w * dt.itemsize]), dtype=dt).reshape(h, w))
    return table, maps


def prepare_targets(arena_dev, arena_host, t_off, n_rows, keys, B, winner_elems, out_elems):
    """The device stage over an uploaded arena: arena_dev (uint8 CUDA tensor) holds what arena_host (the HostArena's tensor) held when the
    upload was queued, the table of n_rows rows at t_off.  -> {key: float32 [B,1,H_s,W_s]}, views of one output arena.  One fill and three
    kernels for the whole batch; nothing is read back."""
    import torch
    from .. import kernels as K
    K._require_gpu(arena_dev)
    if arena_dev.dtype != torch.uint8 or arena_host.dtype != torch.uint8 or arena_host.is_cuda:
        raise ValueError("expected a uint8 device arena and its uint8 host copy")
    out = torch.empty(out_elems, dtype=torch.float32, device=arena_dev.device)
    if n_rows:
        work = torch.empty(winner_elems + n_rows, dtype=torch.int32, device=arena_dev.device)
        K.lib.mte_batch_prep(arena_dev.data_ptr(), min(int(arena_dev.numel()), int(arena_host.numel())), arena_host.data_ptr() + t_off,
                             arena_dev.data_ptr() + t_off, n_rows, out.data_ptr(), out_elems, work.data_ptr(), winner_elems, K._stream())
    return {key: out[off:off + B * tgt[0] * tgt[1]].view(B, 1, tgt[0], tgt[1]) for key, tgt, off in keys}
