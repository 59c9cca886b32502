"""The LiDAR half of the reference's data path on the device (csrc/lidar_prep.hip):

  * ``augment_depth_values``     utils/depth.py:366-438, wired in datasets/transforms.py:46-48: perturb the pixel position and
                                 the value of every LiDAR return, resolve collisions, drop a random share of the survivors
  * ``draw_lidar_perturbation`` / ``draw_lidar_keep``   its random draws, from numpy's stream in the reference's order, so that
                                 ``np.random.seed(k)`` reproduces the reference's sample (as ``draw_color_jitter`` does for ``random``)
  * ``read_lidar``               velodyne ``.bin`` -> [3,N] points in camera axes (datasets/gta_dataset.py:58-80); host I/O
  * ``project_lidar``            process_lidar (gta_dataset.py:85-104): the cloud -> a sparse [H,W] map
  * ``read_lidar_map``           the LiDAR column of a split file in its three formats (gta_dataset.py:368-382,
                                 infer_edge_estimation.py:209-220) -> a sparse map on the device

The draws depend on the number of returns and on the number of survivors, which only the device knows: two 4-byte host reads
per perturbed map.  Tensors handed to these functions are CUDA tensors -- host tensors raise MteError.

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
