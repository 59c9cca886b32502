"""A numpy restatement of the rules of csrc/lidar_prep.hip -- not the reference's code: the perturbation is
written from the rules (cells, smallest key, lowest ordinal), without a sort, so that it can be compared with the reference's
sort / diff formulation in tests/golden/lidar_prep.npz and with the kernels."""
import numpy as np


def perturb_points(depth, scale_d0, add_i, add_j, add_d):
    """stages 1 and 2 -> dict of per-point arrays (ordinal order): 'dprime' float64, 'ii', 'jj' int64 target cell, 'key',
    'survivor' bool (owns its cell, key is not the smallest, jj in range), and 'n'."""
    depth = np.asarray(depth)
    rows, cols = depth.shape
    i, j = np.where(depth > 0)                                        # raster order
    n = len(i)
    d = depth[i, j].astype(np.float64)
    dprime = np.asarray(add_d, dtype=np.float64)[:n] + d * float(scale_d0)
    ip = np.rint(i + np.asarray(add_i, dtype=np.float64)[:n]).astype(np.int64)      # np.round = half to even
    jp = np.rint(j + np.asarray(add_j, dtype=np.float64)[:n]).astype(np.int64)
    key = ip + rows * (jp - 1)
    ii = key % rows                                                   # non-negative modulo
    jj = (key - ii) // rows + 1
    survivor = np.zeros(n, dtype=bool)
    if n:
        smallest = key.min()
        seen = set()
        for k in range(n):                                            # ordinal order: the first point of a key owns it
            if key[k] in seen:
                continue
            seen.add(key[k])
            survivor[k] = key[k] != smallest and 0 <= jj[k] < cols
    return {'n': n, 'dprime': dprime, 'ii': ii, 'jj': jj, 'key': key, 'survivor': survivor}


def augment_depth_values(depth, scale_d0, add_i, add_j, add_d, keep):
    """the three stages with explicit draws -> float64 [H,W] (the kernel stores float32 of it).  keep: uint8 / bool [n'] by survivor rank."""
    depth = np.asarray(depth)
    out = np.zeros(depth.shape)
    if not (depth > 0).any():
        return out
    p = perturb_points(depth, scale_d0, add_i, add_j, add_d)
    s = np.where(p['survivor'])[0]                                    # rank m = position in s
    keep = np.asarray(keep).astype(bool)
    assert len(keep) == len(s), (len(keep), len(s))
    s = s[keep]
    out[p['ii'][s], p['jj'][s]] = p['dprime'][s]
    return out


def count_survivors(depth, scale_d0, add_i, add_j, add_d):
    if not (np.asarray(depth) > 0).any():
        return 0
    return int(perturb_points(depth, scale_d0, add_i, add_j, add_d)['survivor'].sum())


def project_lidar(points, K, shape=(1080, 1920), depth_map=None):
    """process_lidar's rules for an (H, W) output -> float64 [H,W] (the kernel stores float32 of it)."""
    H, W = shape
    points = np.asarray(points, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    out = np.zeros((H, W))
    with np.errstate(all='ignore'):
        for idx in range(points.shape[1]):                            # a later point overwrites an earlier one
            X, Y, Z = points[:, idx]
            p0, p1, p2 = (K[r, 0] * X + K[r, 1] * Y + K[r, 2] * Z for r in range(3))
            u, v = p0 / p2, p1 / p2
            if u >= 0 and u < W and v >= 0 and v < H:
                out[int(v), int(u)] = p2
        if depth_map is not None:
            err = np.sqrt((out - np.asarray(depth_map)) ** 2)
            out[(err > 0.1) & (out > 0)] = 0
    return out


# ---- tests/golden/lidar_prep.npz (make_golden_lidar.py): sparse maps are stored as (flat index, value) pairs

def dense(z, prefix, shape, dtype=np.float64):
    out = np.zeros(int(shape[0]) * int(shape[1]), dtype=dtype)
    out[z[prefix + "_idx"]] = z[prefix + "_val"]
    return out.reshape(int(shape[0]), int(shape[1]))


def aug_case(z, name):
    """-> dict: 'depth' float32 [H,W], 'draws' (what augment_depth_values(draws=...) takes), 'stable' float64 [H,W], 'asis' or None,
    'seed', 'drop', 'scale', 'add'"""
    pre = "aug_%s" % name
    shape = tuple(int(v) for v in z[pre + "_shape"])
    draws = {'scale_d0': float(z[pre + "_scale_d0"]), 'add_i': z[pre + "_add_i"], 'add_j': z[pre + "_add_j"], 'add_d': z[pre + "_add_d"],
             'keep': z[pre + "_keep"]}
    return {'depth': dense(z, pre + "_in", shape, np.float32), 'draws': draws, 'stable': dense(z, pre + "_stable", shape),
            'asis': dense(z, pre + "_asis", shape) if pre + "_asis_idx" in z.files else None, 'seed': int(z[pre + "_seed"]),
            'drop': float(z[pre + "_drop"]), 'scale': ((1, 1, 1), (1, 1, 1.1)), 'add': tuple(map(tuple, z[pre + "_add"]))}


def proj_case(z, name):
    pre = "proj_%s" % name
    shape = tuple(int(v) for v in z[pre + "_shape"])
    return {'points': z[pre + "_points"], 'K': z[pre + "_K"], 'shape': shape, 'out': dense(z, pre, shape),
            'depth_map': dense(z, pre + "_map", shape, np.float32) if pre + "_map_idx" in z.files else None}
