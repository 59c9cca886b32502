"""The LiDAR half of the reference's data path on the device (csrc/lidar_prep.hip):

  * ``augment_depth_values``     utils/depth.py:366-438, wired in datasets/transforms.py:46-48: perturb the pixel position and
                                 the value of every LiDAR return, resolve collisions, drop a random share of the survivors
  * ``draw_lidar_perturbation`` / ``draw_lidar_keep``   its random draws, from numpy's stream in the reference's order, so that
                                 ``np.random.seed(k)`` reproduces the reference's sample (as ``draw_color_jitter`` does for ``random``)
  * ``read_lidar``               velodyne ``.bin`` -> [3,N] points in camera axes (datasets/gta_dataset.py:58-80); host I/O
  * ``project_lidar``            process_lidar (gta_dataset.py:85-104): the cloud -> a sparse [H,W] map
  * ``read_lidar_map``           the LiDAR column of a split file in its three formats (gta_dataset.py:368-382,
                                 infer_edge_estimation.py:209-220) -> a sparse map on the device

  * ``resized_cells`` / ``count_survivors``   the two counts the draws depend on -- the returns n of the cropped and resized map and
                                 the survivors n' of the perturbation -- computed on the host, exactly, from the raw file contents and
                                 the drawn offsets (pure numpy; the rules of csrc/lidar_prep.hip and of the preserve-resize in integers)
  * ``draw_batch`` / ``pack_batch_rows`` / ``perturb_batch`` / ``augment_depth_values_batch``   the perturbation of a whole [B,H,W]
                                 batch: the draws per sample in batch order, one descriptor table, nine launches whatever B is
                                 (``mte_batch_lidar_perturb``), no host read; ``check_status`` compares the device's counts afterwards

The draws depend on the number of returns and on the number of survivors.  ``augment_depth_values`` asks the device for them: two
4-byte host reads per perturbed map.  The batched form takes them from the host functions above and leaves the device's own counts in a
status array (the prefetching loader compares them when the batch's slot comes round again, datasets/prefetch.py).  Tensors handed to
these functions are CUDA tensors -- host tensors raise MteError.

Departures from the reference: points that land in one cell are resolved by "lowest ordinal survives" (the reference's unstable
``np.argsort`` leaves the choice to the numpy build; this is the reference under ``kind='stable'``); an empty map returns zeros (the
reference raises an IndexError); the projected depth is stored as float32 (the reference carries float64 to the end).
"""
import numpy as np
import torch

GTA_INTRINSICS = ((960.0, 0.0, 960.0), (0.0, 960.0, 540.0), (0.0, 0.0, 1.0))       # gta_dataset.py / infer_edge_estimation.py:92


def _column_draws(scale_lo, scale_hi, add_lo, add_hi, n, signed):
    """One column (i, j or d) of the perturbation: (per-point scale or None, per-point offset), consuming numpy's stream as
    rand_values_for_depth_augmentation does (utils/depth.py:440-467)."""
    rand = np.random.rand
    scale = None
    if scale_lo is not None and scale_hi is not None:
        invert = rand(n) < 0.5                                                        # drawn first, applied last
        scale = scale_lo + rand(n) * (scale_hi - scale_lo) if scale_lo != scale_hi else np.ones(n)
        scale[invert] = 1 / scale[invert]
    add = np.zeros(n)
    if add_lo is not None and add_hi is not None:
        if add_lo != add_hi:
            add = add_lo + rand(n) * (add_hi - add_lo)
        if signed:
            negative = rand(n) < 0.5
            add[negative] = -add[negative]
    return scale, add


def draw_lidar_perturbation(n, scale_range, add_range):
    """scale_range / add_range: 2 x 3 = (min row, max row) x (i, j, d) columns -> (scale_d0, add_i, add_j, add_d): the global value
    scale (the first of the d column's per-point scales, as upstream) and float64 [n] offsets; only the i and j offsets draw a sign.
    The per-point scales of i and j are drawn and discarded, as upstream.  A None in the d column of the scale range raises (upstream
    indexes the integer 1 there)."""
    scale_range, add_range = np.array(scale_range), np.array(add_range)
    if scale_range.shape != (2, 3) or add_range.shape != (2, 3):
        raise ValueError("expected 2 x 3 ranges, got {} and {}".format(scale_range.shape, add_range.shape))
    n = int(n)
    _, add_i = _column_draws(scale_range[0, 0], scale_range[1, 0], add_range[0, 0], add_range[1, 0], n, True)
    _, add_j = _column_draws(scale_range[0, 1], scale_range[1, 1], add_range[0, 1], add_range[1, 1], n, True)
    scale_d, add_d = _column_draws(scale_range[0, 2], scale_range[1, 2], add_range[0, 2], add_range[1, 2], n, False)
    if scale_d is None:
        raise TypeError("the depth column of lidar_scale holds None: the reference cannot take its global scale either")
    return float(scale_d[0]), add_i.astype(np.float64), add_j.astype(np.float64), add_d.astype(np.float64)


def draw_lidar_keep(n_survivors, drop_rate):
    """uint8 [n']: 1 for the survivors (by rank) that stay -- the first n' - int(round(n' * drop_rate)) entries of one
    np.random.permutation(n'), utils/depth.py:421-424."""
    n = int(n_survivors)
    drop = int(round(n * drop_rate))
    perm = np.random.permutation(n)
    keep = np.zeros(n, dtype=np.uint8)
    keep[perm[:n - drop]] = 1
    return keep


def augment_depth_values(depth, scale_range, add_range, drop_rate=0.1, draws=None):
    """float [H,W] CUDA tensor (0 = no return) -> float32 [H,W]; None passes through.  draws (tests): a dict with 'scale_d0', 'add_i',
    'add_j', 'add_d' (float64 [n]) and optionally 'keep' (uint8 [n']) used instead of numpy's stream."""
    if depth is None:
        return None
    from .. import kernels as K
    K._require_gpu(depth)
    if depth.dim() != 2:
        raise ValueError("expected an [H,W] map, got {}".format(tuple(depth.shape)))
    src = depth.detach().float().contiguous()
    H, W = int(src.shape[0]), int(src.shape[1])
    dev = src.device
    work = torch.empty((K.lib.mte_lidar_perturb_work_bytes(H, W) + 7) // 8, dtype=torch.int64, device=dev)
    counts = work[:1].view(torch.int32)                                                # [n, n']
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    K.lib.mte_lidar_index(src.data_ptr(), H, W, work.data_ptr(), K._stream())
    n = int(counts[0].item())                                                          # host read 1
    if n == 0:
        K.lib.mte_lidar_scatter(H, W, 0, None, 0, out.data_ptr(), None, K._stream())
        return out
    if draws is None:
        scale_d0, add_i, add_j, add_d = draw_lidar_perturbation(n, scale_range, add_range)
    else:
        scale_d0 = float(draws['scale_d0'])
        add_i, add_j, add_d = (np.asarray(draws[k], dtype=np.float64) for k in ('add_i', 'add_j', 'add_d'))
    if not (add_i.shape == add_j.shape == add_d.shape == (n,)):
        raise ValueError("the map has {} returns, the draws are for {}".format(n, (add_i.shape, add_j.shape, add_d.shape)))
    adds = torch.from_numpy(np.stack([add_i, add_j, add_d])).to(dev)
    K.lib.mte_lidar_perturb(src.data_ptr(), H, W, n, scale_d0, adds[0].data_ptr(), adds[1].data_ptr(), adds[2].data_ptr(),
                            work.data_ptr(), K._stream())
    survivors = int(counts[1].item())                                                  # host read 2
    if draws is not None and draws.get('keep') is not None:
        keep = np.ascontiguousarray(np.asarray(draws['keep']).astype(np.uint8))
    else:
        keep = draw_lidar_keep(survivors, drop_rate)
    if keep.shape != (survivors,):
        raise ValueError("{} points survive, the keep mask is for {}".format(survivors, keep.shape))
    keep_dev = torch.from_numpy(keep).to(dev) if survivors else None
    K.lib.mte_lidar_scatter(H, W, n, keep_dev.data_ptr() if survivors else None, survivors, out.data_ptr(), work.data_ptr(), K._stream())
    return out


LIDAR_BATCH_ROW_WORDS = 8                                                            # MTE_LIDAR_BATCH_ROW_WORDS of include/mte_kernels.h


def read_lidar_raw(path):
    """A map file of the LiDAR column as the decode threads keep it (host only): a 16-bit ``.png`` stays uint16 (0 = no return; the
    device divides by 256), a ``.npy`` / the ``velodyne_depth`` of a ``.npz`` become float32 -- what read_lidar_map uploads, before its
    arithmetic.  A ``.bin`` (a cloud, not a map) gives None: it goes through project_lidar."""
    from .batch_prep import _read_depth_raw
    ext = path.rsplit('.', 1)[-1]
    if ext == 'bin':
        return None
    if ext == 'png':
        m = _read_depth_raw(path)                                                      # uint16, or float32 for the rare non-16-bit file
    elif ext == 'npy':
        m = np.load(path).astype(np.float32)                                           # whatever its type: read_lidar_map uploads its values as float32
    elif ext == 'npz':
        with np.load(path) as z:
            m = z['velodyne_depth'].astype(np.float32)
    else:
        raise ValueError("LiDAR file {}: expected .png, .bin, .npy or .npz".format(path))
    if m.ndim != 2:
        raise ValueError("LiDAR file {} holds a {} array, expected [h,w]".format(path, m.shape))
    return np.ascontiguousarray(m)


def resized_cells(raw, window, shape):
    """The returns of the cropped and preserve-resized map, on the host: raw [h,w] (uint16 or float, > 0 = a return, so neither the 0 of a
    PNG nor read_png_depth's -1 counts), window (x, y, height, width) of the crop (batch_prep.crop_window), shape (H, W) -> sorted int64
    flat indices ty * W + tx of the distinct target cells (int(y * (H / h)), int(x * (W / w))) in double, as bp_scatter_kernel and
    rdp_scatter_kernel compute them; cells outside the target are dropped.  len() is n; the order is the raster order in which
    mte_lidar_index / np.where number the returns.  A map already at the target size goes through the same rule (the per-sample path
    resizes it too: that is what removes the -1)."""
    H, W = int(shape[0]), int(shape[1])
    x0, y0, ch, cw = (int(v) for v in window)
    if ch <= 0 or cw <= 0:
        raise ValueError("crop window {} leaves nothing of a {} map".format(tuple(window), np.asarray(raw).shape))
    ys, xs = np.nonzero(np.asarray(raw)[y0:y0 + ch, x0:x0 + cw] > 0)
    ty = (ys.astype(np.float64) * (float(H) / float(ch))).astype(np.int64)
    tx = (xs.astype(np.float64) * (float(W) / float(cw))).astype(np.int64)
    inside = (ty < H) & (tx < W)
    hit = np.zeros(H * W, dtype=bool)
    hit[ty[inside] * W + tx[inside]] = True
    return np.flatnonzero(hit)


def count_survivors(cells, shape, add_i, add_j):
    """n' on the host: cells (resized_cells: the positions, in ordinal order), the drawn float64 [n] offsets -> the number of distinct
    keys with 0 <= jj < cols other than the map's smallest key (header of csrc/lidar_prep.hip): key = rint(i + add_i) + rows * (rint(j +
    add_j) - 1), ii = key mod rows (non-negative), jj = (key - ii) / rows + 1.  A key with jj in range and a cell determine each other,
    so the distinct keys are counted on a bitmap of the map."""
    rows, cols = int(shape[0]), int(shape[1])
    cells = np.asarray(cells, dtype=np.int64)
    n = len(cells)
    if n == 0:
        return 0
    add_i, add_j = np.asarray(add_i, dtype=np.float64), np.asarray(add_j, dtype=np.float64)
    if add_i.shape != (n,) or add_j.shape != (n,):
        raise ValueError("the map has {} returns, the draws are for {}".format(n, (add_i.shape, add_j.shape)))
    i, j = cells // cols, cells % cols
    ip = np.rint(np.clip(i + add_i, -1e15, 1e15)).astype(np.int64)                     # lp_round_index; np.rint = half to even
    jp = np.rint(np.clip(j + add_j, -1e15, 1e15)).astype(np.int64)
    key = ip + rows * (jp - 1)
    ii = key % rows
    jj = (key - ii) // rows + 1
    inside = (jj >= 0) & (jj < cols)
    hit = np.zeros(rows * cols, dtype=bool)
    hit[ii[inside] * cols + jj[inside]] = True
    lowest = int(np.argmin(key))
    return int(hit.sum()) - int(inside[lowest])                                        # every point with the smallest key is discarded


def draw_batch(cells, shape, scale_range, add_range, drop_rate=0.1, draws=None):
    """The draws of a batch, per sample in batch order, the perturbation first and the keep permutation after it -- numpy's stream is
    consumed exactly as B calls of augment_depth_values consume it (an empty map draws nothing).  cells: per sample resized_cells.
    draws (tests): per sample None or the dict augment_depth_values takes.  -> per sample {'n', 'survivors', 'scale_d0', 'adds' float64
    [3,n], 'keep' uint8 [n']}."""
    out = []
    for b, c in enumerate(cells):
        n = len(c)
        given = draws[b] if draws is not None else None
        if n == 0:
            out.append({'n': 0, 'survivors': 0, 'scale_d0': 1.0, 'adds': np.zeros((3, 0)), 'keep': np.zeros(0, dtype=np.uint8)})
            continue
        if given is None:
            scale_d0, add_i, add_j, add_d = draw_lidar_perturbation(n, scale_range, add_range)
        else:
            scale_d0 = float(given['scale_d0'])
            add_i, add_j, add_d = (np.asarray(given[k], dtype=np.float64) for k in ('add_i', 'add_j', 'add_d'))
        if not (add_i.shape == add_j.shape == add_d.shape == (n,)):
            raise ValueError("map {} has {} returns, the draws are for {}".format(b, n, (add_i.shape, add_j.shape, add_d.shape)))
        survivors = count_survivors(c, shape, add_i, add_j)
        if given is not None and given.get('keep') is not None:
            keep = np.ascontiguousarray(np.asarray(given['keep']).astype(np.uint8))
        else:
            keep = draw_lidar_keep(survivors, drop_rate)
        if keep.shape != (survivors,):
            raise ValueError("{} points of map {} survive, the keep mask is for {}".format(survivors, b, keep.shape))
        out.append({'n': n, 'survivors': survivors, 'scale_d0': float(scale_d0), 'adds': np.stack([add_i, add_j, add_d]), 'keep': keep})
    return out


def batch_arrays(drawn):
    """the arrays of draw_batch's result that go into the upload arena, two per sample: float64 [3,n], uint8 [n']"""
    arrays = []
    for d in drawn:
        arrays += [np.ascontiguousarray(d['adds'], dtype=np.float64), np.ascontiguousarray(d['keep'], dtype=np.uint8)]
    return arrays


def pack_batch_rows(drawn, offsets):
    """The descriptor table of mte_batch_lidar_perturb: offsets = the arena's byte offsets of batch_arrays(drawn), in its order -> int64
    [B, LIDAR_BATCH_ROW_WORDS] = (n, n', bits of scale_d0, add_i, add_j, add_d, keep offsets, 0)."""
    table = np.zeros((len(drawn), LIDAR_BATCH_ROW_WORDS), dtype=np.int64)
    for b, d in enumerate(drawn):
        adds, keep, n = int(offsets[2 * b]), int(offsets[2 * b + 1]), int(d['n'])
        if adds % 8:
            raise ValueError("the float64 draws of map {} start at byte {}: not on 8 bytes".format(b, adds))
        table[b] = (n, int(d['survivors']), np.float64(d['scale_d0']).view(np.int64), adds, adds + 8 * n, adds + 16 * n, keep, 0)
    return table


def perturb_batch(lidar, arena_dev, arena_host, table_off, status=None):
    """Device stage: lidar float32 [B,H,W] / [B,1,H,W] CUDA tensor; arena_dev (uint8 CUDA tensor) holds what arena_host (uint8 host tensor)
    held when the upload was queued, the table of B rows (pack_batch_rows) at byte table_off.  -> (float32 tensor of lidar's shape, status
    int32 [B,4] on the device: n and n' of the table beside the device's own, see check_status).  Nine launches, nothing read back."""
    from .. import kernels as K
    K._require_gpu(lidar)
    K._require_gpu(arena_dev)
    if lidar.dtype != torch.float32 or not lidar.is_contiguous() or lidar.dim() not in (3, 4) or (lidar.dim() == 4 and lidar.shape[1] != 1):
        raise ValueError("expected a contiguous float32 [B,H,W] or [B,1,H,W] tensor, got {} {}".format(lidar.dtype, tuple(lidar.shape)))
    if arena_dev.dtype != torch.uint8 or arena_host.dtype != torch.uint8 or arena_host.is_cuda:
        raise ValueError("expected a uint8 device arena and its uint8 host copy")
    B, H, W = int(lidar.shape[0]), int(lidar.shape[-2]), int(lidar.shape[-1])
    nbytes = min(int(arena_dev.numel()), int(arena_host.numel()))
    if table_off < 0 or table_off % 8 or table_off + B * LIDAR_BATCH_ROW_WORDS * 8 > nbytes:
        raise ValueError("the table of {} rows at byte {} is not inside an arena of {} bytes".format(B, table_off, nbytes))
    work_bytes = K.lib.mte_batch_lidar_perturb_work_bytes(B, H, W)
    if work_bytes <= 0:
        raise K.MteError("mte_batch_lidar_perturb does not take a batch of {} maps of {} x {}".format(B, H, W))
    work = torch.empty(work_bytes // 8, dtype=torch.int64, device=lidar.device)
    out = torch.empty_like(lidar)
    if status is None:
        status = torch.empty((B, 4), dtype=torch.int32, device=lidar.device)
    K.lib.mte_batch_lidar_perturb(lidar.data_ptr(), B, H, W, arena_dev.data_ptr(), nbytes, arena_host.data_ptr() + table_off,
                                  arena_dev.data_ptr() + table_off, out.data_ptr(), work.data_ptr(), status.data_ptr(), K._stream())
    return out, status


def check_status(status, what=''):
    """status: int [B,4] on the host (n of the host, n of the device, n' of the host, n' of the device) once the pass has completed.
    Raises MteError naming the samples whose counts differ: their draws were sized for another map, the batch is not the reference's."""
    from .._lib import MteError
    st = np.asarray(status).reshape(-1, 4)
    bad = np.flatnonzero((st[:, 0] != st[:, 1]) | (st[:, 2] != st[:, 3]))
    if len(bad):
        raise MteError("LiDAR perturbation{}: the host counted (n, n') = {} but the device {} for sample(s) {}".format(
            ' of ' + what if what else '', [(int(st[b, 0]), int(st[b, 2])) for b in bad], [(int(st[b, 1]), int(st[b, 3])) for b in bad],
            [int(b) for b in bad]))


def augment_depth_values_batch(lidar, cells, scale_range, add_range, drop_rate=0.1, draws=None):
    """augment_depth_values for a [B,H,W] CUDA batch in one pass.  cells: per sample the sorted flat indices of its returns (resized_cells;
    for a map that is on the host anyway, np.flatnonzero(map > 0)).  draws (tests): per sample None or the dict augment_depth_values
    takes.  -> (float32 tensor of lidar's shape, status): nothing is read back here; check_status(status.cpu()) afterwards."""
    from . import batch_prep as bp
    drawn = draw_batch(cells, tuple(lidar.shape[-2:]), scale_range, add_range, drop_rate, draws)
    arrays = batch_arrays(drawn)
    _, offs, total = bp.arena_layout(arrays, 0)
    t_off = total
    table = pack_batch_rows(drawn, offs)
    host = bp.HostArena()
    host.reserve(t_off + table.nbytes)
    bp.pack_arena(host, arrays, [None] * len(arrays))
    host.view[t_off:t_off + table.nbytes] = table.reshape(-1).view(np.uint8)
    return perturb_batch(lidar, host.tensor.to(lidar.device), host.tensor, t_off)


def read_lidar(path):
    """velodyne .bin (float32 x, y, z, intensity per point) -> float32 [3,N] = (-y, -z, x), rows with a NaN removed."""
    xyzi = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
    points = np.stack([-xyzi[:, 1], -xyzi[:, 2], xyzi[:, 0]], axis=1)
    return points[~np.isnan(points).any(axis=1)].T


def project_lidar(points, K, shape=(1080, 1920), depth_map=None):
    """points [3,N] (numpy or tensor), K 3 x 3 intrinsics, depth_map None or an [H,W] map (numpy or CUDA tensor) -> float32 [H,W] CUDA
    tensor: the depth p[2] of the last point that falls into each pixel, 0 elsewhere; with depth_map, returns that differ from it by more
    than 0.1 are removed."""
    from .. import kernels as Kn
    H, W = int(shape[0]), int(shape[1])
    dev = torch.device('cuda', torch.cuda.current_device())
    if torch.is_tensor(depth_map):
        Kn._require_gpu(depth_map)
        dev = depth_map.device
    if torch.is_tensor(points):
        pts = points.detach().to(device=dev, dtype=torch.float64).contiguous()
    else:
        pts = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float64))).to(dev)
    if pts.dim() != 2 or pts.shape[0] != 3:
        raise ValueError("expected [3,N] points, got {}".format(tuple(pts.shape)))
    Kn._require_gpu(pts)
    kmat = torch.from_numpy(np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))).to(dev)
    dm = None
    if depth_map is not None:
        dm = (depth_map.detach() if torch.is_tensor(depth_map) else torch.from_numpy(np.ascontiguousarray(depth_map)).to(dev)).float().contiguous()
        if tuple(dm.shape) != (H, W):
            raise ValueError("depth_map is {}, the output {}".format(tuple(dm.shape), (H, W)))
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    ws = torch.empty((H, W), dtype=torch.int32, device=dev)
    N = int(pts.shape[1])
    Kn.lib.mte_lidar_project(pts.data_ptr() if N else None, N, kmat.data_ptr(), dm.data_ptr() if dm is not None else None, out.data_ptr(),
                             H, W, ws.data_ptr(), Kn._stream())
    return out


def read_lidar_map(path, device, depth_map=None, clamp_negative=False):
    """One file of the split's LiDAR column -> float32 [h,w] on `device`: a 16-bit ``.png`` through read_png_depth (-1 = no return;
    clamp_negative turns those into 0, as the annotation driver does), a ``.npy`` as it is, the ``velodyne_depth`` array of a ``.npz``
    (infer_edges.py's split mode; clamped like the png), a velodyne ``.bin`` projected with the GTA
    intrinsics into the shape of depth_map (which then also removes returns that are off by more than 10 cm) or, without one, into the
    reference's 1080 x 1920."""
    from .kitti_edges import read_png_depth
    ext = path.rsplit('.', 1)[-1]
    if ext == 'bin':
        shape = (1080, 1920) if depth_map is None else tuple(depth_map.shape[-2:])
        if depth_map is not None and not torch.is_tensor(depth_map):
            depth_map = torch.from_numpy(np.ascontiguousarray(depth_map, dtype=np.float32)).to(device)
        with torch.cuda.device(device):
            return project_lidar(read_lidar(path), GTA_INTRINSICS, shape, depth_map)
    if ext == 'png':
        m = read_png_depth(path)
        if clamp_negative:
            m[m < 0.0] = 0.0
    elif ext == 'npy':
        m = np.load(path)
    elif ext == 'npz':                                                                 # read_npz_depth(file, 'velodyne'), kitti_dataset.py:35-38
        with np.load(path) as z:
            m = z['velodyne_depth'].astype(np.float32)
        if clamp_negative:
            m[m < 0.0] = 0.0
    else:
        raise ValueError("LiDAR file {}: expected .png, .bin, .npy or .npz".format(path))
    if m.ndim != 2:
        raise ValueError("LiDAR file {} holds a {} array, expected [h,w]".format(path, m.shape))
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(device)
