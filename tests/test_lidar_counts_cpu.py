"""CPU: the two counts the LiDAR draws depend on, computed on the host (mindtheedge_amd/datasets/lidar_prep.py: resized_cells,
count_survivors, draw_batch), against the restated rules of tests/lidar_ref.py (perturbation) and oracle/data_oracle.py (preserve-resize)
on crafted maps.  Every comparison is exact: n, n' and the ordinal order."""
import numpy as np
import pytest

import lidar_ref as R
from oracle import data_oracle as do

from mindtheedge_amd.datasets import batch_prep as bp
from mindtheedge_amd.datasets import lidar_prep as lp


def _as_read(raw):
    """what the per-sample path hands to resize_depth_preserve: read_png_depth's arithmetic for a 16-bit map, the floats as they are"""
    if raw.dtype != np.uint16:
        return raw.astype(np.float32)
    out = raw.astype(np.float32) / np.float32(256.)
    out[raw == 0] = -1.
    return out


def _resized(raw, borders, shape):
    m = _as_read(raw)
    if borders is not None:
        m = m[borders[1]:borders[3], borders[0]:borders[2]]
    return do.resize_depth_preserve(m, shape)


def _maps():
    g = np.random.default_rng(7)
    u16 = ((g.random((37, 70)) < 0.3) * g.integers(1, 65536, (37, 70))).astype(np.uint16)       # zeros = no return
    u16[0, :3] = (0, 1, 65535)
    f32 = ((g.random((40, 66)) < 0.4) * (g.random((40, 66)) * 80)).astype(np.float32)
    f32[g.random((40, 66)) < 0.3] = -1.                                                          # read_png_depth's "no return"
    small = ((g.random((9, 14)) < 0.5) * (1 + g.random((9, 14)))).astype(np.float32)
    at_size = _as_read(((g.random((32, 64)) < 0.2) * g.integers(1, 9000, (32, 64))).astype(np.uint16))      # -1 where the file had 0
    return {"u16_larger": u16, "f32_larger_with_minus_one": f32, "f32_smaller": small, "f32_at_target_size": at_size,
            "empty": np.zeros((37, 70), dtype=np.uint16), "single": np.pad(np.ones((1, 1), dtype=np.float32), ((5, 20), (9, 30)))}


@pytest.mark.parametrize("name", sorted(_maps()))
@pytest.mark.parametrize("borders", [None, (2, 3, 60, 33)])
def test_returns_of_the_resized_map(name, borders):
    raw = _maps()[name]
    want = _resized(raw, borders, (32, 64))
    cells = lp.resized_cells(raw, bp.crop_window(borders, *raw.shape), (32, 64))
    assert cells.dtype == np.int64 and cells.ndim == 1
    np.testing.assert_array_equal(cells, np.flatnonzero(want.reshape(-1) > 0))                  # n and the ordinal (raster) order
    assert (want >= 0).all()                                                                    # the -1 of a map at target size is gone too
    if name == "empty":
        assert len(cells) == 0
    if name == "single":
        assert len(cells) == 1
    if name.endswith("larger") and borders is None:
        assert len(cells) < int((raw > 0).sum())                                                # collisions: several sources share a target


def test_resize_collisions_and_upscale_by_hand():
    raw = np.zeros((4, 4), dtype=np.uint16)
    raw[0, 0] = raw[0, 1] = raw[1, 1] = 7                                                       # all three land in target (0, 0)
    raw[3, 3] = 9
    assert list(lp.resized_cells(raw, (0, 0, 4, 4), (2, 2))) == [0, 3]
    assert list(lp.resized_cells(raw, (1, 1, 3, 3), (3, 3))) == [0, 8]                          # the window moves the origin
    assert list(lp.resized_cells(raw, (0, 0, 4, 4), (8, 8))) == [0, 2, 18, 54]                  # upscale: one cell each, (y*2, x*2)
    assert list(lp.resized_cells(np.float32([[0, -1], [np.nan, 2]]), (0, 0, 2, 2), (2, 2))) == [3]


def _cells(depth):
    return np.flatnonzero(np.asarray(depth).reshape(-1) > 0)


def _check(depth, add_i, add_j):
    """n' and (through draw_batch with injected draws) the keep length against lidar_ref"""
    depth = np.asarray(depth, dtype=np.float32)
    n = int((depth > 0).sum())
    add_i, add_j = np.asarray(add_i, dtype=np.float64), np.asarray(add_j, dtype=np.float64)
    want = R.count_survivors(depth, 1.0, add_i, add_j, np.zeros(n))
    got = lp.count_survivors(_cells(depth), depth.shape, add_i, add_j)
    assert got == want, (got, want)
    return got


def test_empty_map_and_single_return():
    assert _check(np.zeros((5, 7)), [], []) == 0
    one = np.zeros((5, 7))
    one[2, 3] = 4.0
    for di, dj in ((0, 0), (1.4, -2.0), (-9, 30)):
        assert _check(one, [di], [dj]) == 0                                                     # the smallest key is always discarded


def test_several_points_share_the_smallest_key():
    d = np.zeros((6, 8))
    d[1, 1] = d[1, 2] = d[2, 1] = d[4, 5] = d[5, 7] = 1.0                                       # ordinals 0..4
    # the first three are moved into cell (1, 1): key 1 + 6 * 0 is the smallest of the map, all three go; two others stay
    assert _check(d, [0, 0, -1, 0, 0], [0, -1, 0, 0, 0]) == 2
    # everything into one cell: one key, the smallest: nothing survives
    assert _check(d, [0, 0, -1, -3, -4], [0, -1, 0, -4, -6]) == 0
    # two points share a key that is not the smallest: one survivor for the cell
    assert _check(d, [0, 0, 0, 0, -1], [0, 0, 0, 0, -2]) == 3


def test_jj_out_of_range_on_both_sides_and_rows_that_wrap():
    d = np.zeros((6, 8))
    d[0, 0] = d[2, 3] = d[3, 7] = d[5, 7] = d[5, 0] = 1.0                                       # ordinals: (0,0) (2,3) (3,7) (5,0) (5,7)
    add_i = [0, 0, 0, 0, 0]
    assert _check(d, add_i, [-2, 0, 0, 0, 0]) == 4                                              # jj = -2: left of the map (and the smallest key)
    assert _check(d, add_i, [0, 0, 1, 0, 3]) == 2                                               # jj = 8 and 10: right of the map; (0,0) holds the smallest key
    # a negative row wraps through the modulo into the column to the left: (2,3) - 3 rows -> key -1 + 6 * 2 = 11 -> ii 5, jj 2
    p = R.perturb_points(d.astype(np.float32), 1.0, [0, -3, 0, 0, 0], [0, 0, 0, 0, 0], np.zeros(5))
    assert (p['ii'][1], p['jj'][1]) == (5, 2)
    assert _check(d, [0, -3, 0, 0, 0], [0, 0, 0, 0, 0]) == 4
    # (0,0) - 1 row -> key -1 - 6 = -7 -> ii 5, jj -1: out of range on the left after the wrap
    assert _check(d, [-1, 0, 0, 0, 0], [0, 0, 0, 0, 0]) == 4
    # a row past the bottom wraps into the column to the right; from the last column it leaves the map
    assert _check(d, [0, 0, 0, 0, 2], [0, 0, 0, 0, 0]) == 3
    # a whole map height up: (5,0) - 6 rows -> key -7 -> (5, -1), outside and now the smallest key, so (0,0) stays; (5,7) - 6 -> key 35 -> (5, 6)
    assert _check(d, [0, 0, 0, -6, -6], [0, 0, 0, 0, 0]) == 4
    # .. and when the wrapped point lands on (3,7)'s cell (key 3 + 6 * 6 = 39 = 9 + 6 * 5: (3,6) + 6 rows), the cell keeps one survivor
    d[3, 6] = 1.0                                                                               # ordinals: (0,0) (2,3) (3,6) (3,7) (5,0) (5,7)
    assert _check(d, [0, 0, 6, 0, 0, 0], [0, 0, 0, 0, 0, 0]) == 4


def test_half_integer_offsets_round_half_to_even():
    d = np.zeros((8, 8))
    d[2, 2] = d[3, 2] = d[4, 4] = d[6, 6] = 1.0
    # 2 + 0.5 -> 2, 3 + 0.5 -> 4 (half to even): with half-up, (2,2) and (3,2) would sit in rows 3 and 4 instead
    p = R.perturb_points(d.astype(np.float32), 1.0, [0.5, 0.5, -0.5, 0], [0, 0, 0.5, 0], np.zeros(4))
    assert list(p['ii']) == [2, 4, 4, 6] and list(p['jj']) == [2, 2, 4, 6]
    assert _check(d, [0.5, 0.5, -0.5, 0], [0, 0, 0.5, 0]) == 3
    # 2.5 -> 2 and 1.5 -> 2 collide: (2,2) + 0.5 and (3,2) - 1.5... rows 2 and 2 -> one cell, which holds the smallest key
    assert _check(d, [0.5, -1.5, 0, 0], [0, 0, 0, 0]) == 2
    assert _check(d, [0, 0, 0.5, 0], [0, 0, 0.5, -1.5]) == 3                                    # 4.5 -> 4, 4.5 -> 4, 6 - 1.5 -> 4 (column)


@pytest.mark.parametrize("seed", range(6))
def test_random_maps_and_offsets_against_the_restated_rules(seed):
    g = np.random.default_rng(seed)
    H, W = ((12, 20), (32, 64), (5, 9))[seed % 3]
    d = ((g.random((H, W)) < (0.1, 0.5, 0.9)[seed % 3]) * (1 + g.random((H, W)))).astype(np.float32)
    n = int((d > 0).sum())
    spread = (1.5, 6.0, 40.0)[seed // 2]                                                        # up to far outside the map
    add_i = np.round(g.uniform(-spread, spread, n) * 2) / 2                                     # halves included
    add_j = np.round(g.uniform(-spread, spread, n) * 2) / 2
    _check(d, add_i, add_j)


def test_draw_batch_consumes_numpys_stream_like_the_per_sample_path():
    """different n per sample, an empty map among them: the perturbation for n, then the permutation for n', sample after sample"""
    g = np.random.default_rng(3)
    scale, add = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5))
    maps = [((g.random((12, 20)) < p) * (1 + g.random((12, 20)))).astype(np.float32) for p in (0.3, 0.0, 0.05, 0.7)]
    np.random.seed(21)
    want = []
    for m in maps:                                                                              # augment_depth_values's sequence, counts from lidar_ref
        n = int((m > 0).sum())
        if n == 0:
            want.append(None)
            continue
        s, ai, aj, ad = lp.draw_lidar_perturbation(n, scale, add)
        keep = lp.draw_lidar_keep(R.count_survivors(m, s, ai, aj, ad), 0.2)
        want.append((s, ai, aj, ad, keep))
    tail = np.random.rand()
    np.random.seed(21)
    got = lp.draw_batch([_cells(m) for m in maps], (12, 20), scale, add, 0.2)
    assert np.random.rand() == tail
    assert [d['n'] for d in got] == [int((m > 0).sum()) for m in maps] and got[1]['n'] == 0 and got[1]['survivors'] == 0
    for d, w in zip(got, want):
        if w is None:
            assert d['adds'].shape == (3, 0) and d['keep'].shape == (0,)
            continue
        assert d['scale_d0'] == w[0] and d['adds'].dtype == np.float64 and d['keep'].dtype == np.uint8
        np.testing.assert_array_equal(d['adds'], np.stack(w[1:4]))
        np.testing.assert_array_equal(d['keep'], w[4])
        assert d['survivors'] == len(w[4])
    # injected draws: sizes are checked against the host's counts
    with pytest.raises(ValueError):
        lp.draw_batch([_cells(maps[0])], (12, 20), scale, add, 0.2, draws=[{'scale_d0': 1.0, 'add_i': np.zeros(3), 'add_j': np.zeros(3), 'add_d': np.zeros(3)}])
    n0 = got[0]['n']
    with pytest.raises(ValueError):
        lp.draw_batch([_cells(maps[0])], (12, 20), scale, add, 0.2,
                      draws=[{'scale_d0': 1.0, 'add_i': np.zeros(n0), 'add_j': np.zeros(n0), 'add_d': np.zeros(n0), 'keep': np.ones(n0, dtype=np.uint8)}])
