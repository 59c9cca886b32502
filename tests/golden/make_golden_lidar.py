"""Generates tests/golden/lidar_prep.npz from the upstream reference (development container only): ``augment_depth_values`` and
``rand_values_for_depth_augmentation`` (packnet_code/packnet_sfm/utils/depth.py:366-467) and ``process_lidar``
(packnet_code/packnet_sfm/datasets/gta_dataset.py:85-104), run as they are.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lidar.py

Perturbation cases ``aug_<name>_*``: the input map, the draws (regenerated with the reference's own draw function under the case's
seed and checked against the permutation the reference drew), the reference's output with ``np.argsort`` made stable for the
duration of the call (``_stable``) and, for drop rate 0, its output as it is (``_asis``).  Projection cases ``proj_<name>_*``.
Sparse maps are stored as (flat index, value) pairs.  The generator checks what the fixtures are meant to exercise: collisions in
every case that can have them, row indices that wrap on both sides, target columns out of range on both sides, repeated pixels,
and no projected coordinate within 1e-9 of an integer (so that the summation order of K P cannot move a pixel)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import                                   # noqa: E402

SCALE = ((1, 1, 1), (1, 1, 1.1))
GTA_K = np.array([960, 0, 960, 0, 960, 540, 0, 0, 1], dtype=np.float64).reshape(3, 3)
#            name        shape      density  a    drop
AUG_CASES = [("kitti8", (48, 160), 0.05, 1.5, 0.1), ("dense", (24, 80), 0.3, 2.0, 0.25), ("wide", (96, 320), 0.05, 1.5, 0.1),
             ("far", (16, 24), 0.4, 3.0, 0.5), ("crowd", (12, 40), 0.6, 1.0, 0.1), ("keepall", (13, 21), 0.5, 1.0, 0.0),
             ("dropall", (13, 21), 0.5, 1.0, 1.0), ("noshift", (16, 24), 0.3, 0.0, 0.1), ("single", (9, 11), None, 1.5, 0.1)]


def sparse(a):
    flat = np.asarray(a).reshape(-1)
    idx = np.flatnonzero(flat)
    return idx.astype(np.int32), flat[idx]


def make_map(shape, density, seed):
    """float32-representable values, handed to the reference as float64 so that no numpy version computes in float32"""
    rs = np.random.RandomState(seed)
    if density is None:
        d = np.zeros(shape, dtype=np.float32)
        d[shape[0] // 2, shape[1] // 2] = np.float32(17.25)
        return d
    return ((rs.rand(*shape) < density) * (1.0 + 79.0 * rs.rand(*shape))).astype(np.float32)


class stable_argsort:
    def __enter__(self):
        self.orig = np.argsort
        np.argsort = lambda a, *args, **kw: self.orig(a, kind='stable')

    def __exit__(self, *exc):
        np.argsort = self.orig


class recorded_permutation:
    def __enter__(self):
        self.orig, self.calls = np.random.permutation, []

        def record(n):
            p = self.orig(n)
            self.calls.append(np.array(p))
            return p
        np.random.permutation = record
        return self

    def __exit__(self, *exc):
        np.random.permutation = self.orig


def aug_case(rd, name, shape, density, a, drop, seed):
    """-> (fixture entries, statistics) or None when the case holds no collision although it should"""
    add = ((0, 0, 0), (a, a, 0.5))
    depth = make_map(shape, density, seed)
    rows, cols = shape
    ii, jj = np.where(depth > 0)
    n = len(ii)
    np.random.seed(seed)
    raises = False
    with stable_argsort(), recorded_permutation() as rec:
        try:
            stable = rd.augment_depth_values(depth.astype(np.float64), SCALE, add, drop)[:, :, 0]
        except IndexError:
            # no point survives: the reference has drawn its (empty) permutation and then fails on its empty float index arrays, as it
            # does on an empty map.  The fixture records that and holds the all-zero map the rules give.
            raises, stable = True, np.zeros(shape)
    (perm,) = rec.calls
    assert raises == (len(perm) == 0), name
    # the draws, by the reference's own function in augment_depth_values' order
    np.random.seed(seed)
    sr, ar = np.array(SCALE), np.array(add)
    _, add_i = rd.rand_values_for_depth_augmentation(sr[:, 0], ar[:, 0], n, is_add_neg_allowed=True)
    _, add_j = rd.rand_values_for_depth_augmentation(sr[:, 1], ar[:, 1], n, is_add_neg_allowed=True)
    scale_d, add_d = rd.rand_values_for_depth_augmentation(sr[:, 2], ar[:, 2], n, is_add_neg_allowed=False)
    again = np.random.permutation(len(perm))
    assert np.array_equal(again, perm), name
    keep = np.zeros(len(perm), dtype=np.uint8)
    keep[perm[:len(perm) - int(round(len(perm) * drop))]] = 1
    ip, jp = np.round(ii + add_i).astype('int'), np.round(jj + add_j).astype('int')
    key = ip + rows * (jp - 1)
    tj = (key - key % rows) // rows + 1
    stats = {'n': n, 'survivors': len(perm), 'collisions': n - len(np.unique(key)), 'wrap_low': int((ip < 0).sum()),
             'wrap_high': int((ip >= rows).sum()), 'col_low': int((tj < 0).sum()), 'col_high': int((tj >= cols).sum())}
    if a > 0 and n > 1 and stats['collisions'] == 0:
        return None
    pre = "aug_%s_" % name
    out = {pre + "shape": np.array(shape), pre + "seed": np.array(seed), pre + "drop": np.array(drop), pre + "add": np.array(add, dtype=np.float64),
           pre + "scale_d0": np.array(scale_d[0]), pre + "add_i": add_i, pre + "add_j": add_j, pre + "add_d": add_d, pre + "keep": keep,
           pre + "reference_raises": np.array(raises)}
    out[pre + "in_idx"], out[pre + "in_val"] = sparse(depth)
    out[pre + "stable_idx"], out[pre + "stable_val"] = sparse(stable)
    if drop == 0:
        np.random.seed(seed)
        asis = rd.augment_depth_values(depth.astype(np.float64), SCALE, add, drop)[:, :, 0]
        out[pre + "asis_idx"], out[pre + "asis_val"] = sparse(asis)
    return out, stats


def clear_of_integers(points, K):
    """the points whose projected coordinates stay 1e-9 away from every integer (non-finite quotients pass: they are dropped anyway)"""
    with np.errstate(all='ignore'):
        p = np.matmul(K, points)
        uv = (p / p[2, :])[:2]
        near = np.abs(uv - np.round(uv)) < 1e-9
    return points[:, ~np.any(near & np.isfinite(uv), axis=0)]


def proj_cases(gd):
    out, stats = {}, {}
    rs = np.random.RandomState(7)
    pts = np.stack([rs.uniform(-30, 30, 5000), rs.uniform(-8, 8, 5000), rs.uniform(0.5, 80, 5000)])
    pts = clear_of_integers(pts, GTA_K)
    ref = gd.process_lidar(pts, GTA_K)
    out["proj_big_points"], out["proj_big_K"], out["proj_big_shape"] = pts, GTA_K, np.array(ref.shape)
    out["proj_big_idx"], out["proj_big_val"] = sparse(ref)
    stats['big'] = int((ref != 0).sum())
    # the same cloud against a depth map that is off by more than 10 cm on about half of the returns
    off = np.where(rs.rand(*ref.shape) < 0.5, 0.5, 0.01) * np.where(rs.rand(*ref.shape) < 0.5, -1.0, 1.0)
    depth = np.where(ref != 0, ref + off, 0.0).astype(np.float32)
    masked = gd.process_lidar(pts, GTA_K, depth)
    out["proj_depth_points"], out["proj_depth_K"], out["proj_depth_shape"] = pts, GTA_K, np.array(ref.shape)
    out["proj_depth_map_idx"], out["proj_depth_map_val"] = sparse(depth)
    out["proj_depth_idx"], out["proj_depth_val"] = sparse(masked)
    stats['depth'] = (int((masked != 0).sum()), int((ref != 0).sum()))
    assert 0.3 < stats['depth'][0] / stats['depth'][1] < 0.7
    # 200 points into 24 x 40: 150 pixels drawn at random and 50 more returns on pixels already taken; the reference's canvas is
    # 1080 x 1920 whatever the camera, its top-left 24 x 40 corner is the map of that size (cells do not influence each other)
    Ks = np.array([20, 0, 20, 0, 20, 12, 0, 0, 1], dtype=np.float64).reshape(3, 3)
    u = np.concatenate([rs.uniform(-4, 46, 150), np.zeros(50)])
    v = np.concatenate([rs.uniform(-3, 28, 150), np.zeros(50)])
    inside = np.flatnonzero((u[:150] >= 0) & (u[:150] < 40) & (v[:150] >= 0) & (v[:150] < 24))
    again = rs.choice(inside, 50)
    u[150:], v[150:] = np.floor(u[again]) + rs.uniform(0.05, 0.95, 50), np.floor(v[again]) + rs.uniform(0.05, 0.95, 50)
    z = rs.uniform(1, 60, 200)
    small = clear_of_integers(np.stack([(u - 20) * z / 20, (v - 12) * z / 20, z]), Ks)
    ref = gd.process_lidar(small, Ks)[:24, :40]
    with np.errstate(all='ignore'):
        p = np.matmul(Ks, small)
        pn = p / p[2]
    ok = (pn[0] >= 0) & (pn[0] < 40) & (pn[1] >= 0) & (pn[1] < 24)
    cells = pn[1, ok].astype(int) * 40 + pn[0, ok].astype(int)
    stats['small_repeats'] = int(ok.sum() - len(np.unique(cells)))
    assert stats['small_repeats'] >= 20 and (~ok).sum() > 0
    out["proj_small_points"], out["proj_small_K"], out["proj_small_shape"] = small, Ks, np.array([24, 40])
    out["proj_small_idx"], out["proj_small_val"] = sparse(ref)
    # points behind the camera and on its plane (z = 0: non-finite quotients)
    back = np.stack([rs.uniform(-30, 30, 300), rs.uniform(-8, 8, 300), rs.uniform(-40, 40, 300)])
    back[2, ::15] = 0.0
    back[0, 0] = 0.0                                                  # 0 / 0
    back = clear_of_integers(back, GTA_K)
    with np.errstate(all='ignore'):
        ref = gd.process_lidar(back, GTA_K)
    stats['behind'] = (int((ref < 0).sum()), int((ref > 0).sum()), int((back[2] == 0).sum()))
    assert stats['behind'][0] > 5 and stats['behind'][1] > 5 and stats['behind'][2] > 5
    out["proj_behind_points"], out["proj_behind_K"], out["proj_behind_shape"] = back, GTA_K, np.array(ref.shape)
    out["proj_behind_idx"], out["proj_behind_val"] = sparse(ref)
    return out, stats


def main():
    assert ref_import.reference_available()
    ref_import.install_stubs()
    from packnet_code.packnet_sfm.utils import depth as rd
    from packnet_code.packnet_sfm.datasets import gta_dataset as gd
    out, totals = {}, {}
    names = []
    for c, (name, shape, density, a, drop) in enumerate(AUG_CASES):
        seed = 100 * (c + 1)
        got = aug_case(rd, name, shape, density, a, drop, seed)
        while got is None:                                            # no collision: try the next seed
            seed += 1
            got = aug_case(rd, name, shape, density, a, drop, seed)
        entries, stats = got
        out.update(entries)
        names.append(name)
        print(name, seed, stats)
        for k, v in stats.items():
            totals[k] = totals.get(k, 0) + v
    for k in ('wrap_low', 'wrap_high', 'col_low', 'col_high'):        # over the set: both wraps, both out-of-range sides
        assert totals[k] > 0, (k, totals)
    out["aug_names"] = np.array(names)
    p_out, p_stats = proj_cases(gd)
    out.update(p_out)
    out["proj_names"] = np.array(["big", "depth", "small", "behind"])
    print(p_stats)
    path = os.path.join(HERE, "lidar_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
