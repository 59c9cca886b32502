"""CPU: the host side of the LiDAR column in the prefetching training loader (mindtheedge_amd/datasets/batch_prep.py, lidar_prep.py,
prefetch.py): the workers read the file, the rows and the arena carry the maps and the draws, the draw sequence is the per-sample
path's.  The device stage is replaced by a stand-in; no GPU is touched."""
import inspect
import os
import threading

import numpy as np
import pytest
from PIL import Image

import lidar_ref as R
from oracle import data_oracle as do

from mindtheedge_amd.datasets import batch_prep as bp
from mindtheedge_amd.datasets import lidar_prep as lp
from mindtheedge_amd.datasets.kitti_edges import parse_split_line, read_png_depth
from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader

SCALE, ADD = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5))
SHAPE = (12, 20)


def _write(tmp):
    """three records: a 16-bit .png, a float64 .npy and a .npz with -1, each with another number of returns; and the line of a .bin"""
    g = np.random.default_rng(8)
    maps = {}
    for i, (h, w, p) in enumerate(((15, 26, 0.3), (12, 20, 0.1), (9, 14, 0.6))):
        Image.fromarray(g.integers(0, 256, (15, 26, 3), dtype=np.uint8)).save(os.path.join(tmp, "rgb%d.png" % i))
        raw = ((g.random((h, w)) < p) * g.integers(256, 60 * 256, (h, w))).astype(np.uint16)
        raw[h - 1, w - 1] = 999
        maps[i] = raw
    Image.fromarray(maps[0]).save(os.path.join(tmp, "lidar0.png"))
    np.save(os.path.join(tmp, "lidar1.npy"), maps[1] / 256.0)                                   # float64 on disk
    np.savez(os.path.join(tmp, "lidar2.npz"), velodyne_depth=np.where(maps[2] == 0, -1.0, maps[2] / 256.0), other=np.zeros(3))
    lines = ["rgb%d.png None None lidar%d.%s None None None None\n" % (i, i, ext) for i, ext in enumerate(("png", "npy", "npz"))]
    return maps, [parse_split_line(l) for l in lines] + [parse_split_line("rgb0.png None None cloud.bin None None None None\n")]


def test_the_worker_reads_the_file_and_counts_the_returns(tmp_path):
    tmp = str(tmp_path)
    maps, recs = _write(tmp)
    borders = (1, 10, 2, 20)                                              # (y, height, x, width) -> left 2, top 1, right 22, bottom 11
    got = [bp.decode_train_record(r, tmp, with_lidar=True, crop_borders=borders, shape=SHAPE) for r in recs]
    assert got[0]['lidar'].dtype == np.uint16 and got[1]['lidar'].dtype == np.float32 and got[2]['lidar'].dtype == np.float32
    np.testing.assert_array_equal(got[0]['lidar'], maps[0])
    np.testing.assert_array_equal(got[1]['lidar'], (maps[1] / 256.0).astype(np.float32))
    np.testing.assert_array_equal(got[2]['lidar'], np.where(maps[2] == 0, -1.0, maps[2] / 256.0).astype(np.float32))
    assert got[3]['lidar'] is None and got[3]['lidar_cells'] is None and got[3]['lidar_path'].endswith("cloud.bin")      # never opened: there is no such file
    assert bp.lidar_batchable(got[:3]) and not bp.lidar_batchable(got) and not bp.lidar_batchable([got[3]])              # the .bin fall-back is per batch
    # the same PNG assertion and arithmetic as the per-sample reader
    as_read = got[0]['lidar'].astype(np.float32) / 256
    as_read[got[0]['lidar'] == 0] = -1
    np.testing.assert_array_equal(as_read, read_png_depth(os.path.join(tmp, "lidar0.png")))
    Image.fromarray(np.full((5, 6), 255, dtype=np.uint16)).save(os.path.join(tmp, "low.png"))
    with pytest.raises(AssertionError):
        bp.decode_train_record(parse_split_line("rgb0.png None None low.png None None None None\n"), tmp, with_lidar=True)
    # n, counted on the worker with the frame's crop borders, against the resize of the cropped map
    for i in range(3):
        m = np.where(maps[i] == 0, -1.0, maps[i] / 256.0).astype(np.float32)[1:11, 2:22]
        want = do.resize_depth_preserve(m, SHAPE)
        np.testing.assert_array_equal(got[i]['lidar_cells'], np.flatnonzero(want.reshape(-1) > 0))
    assert len({len(g['lidar_cells']) for g in got[:3]}) == 3
    # a .npy is float32 of its values whatever type it was saved with: only a 16-bit PNG means 1/256 m
    for name, dt in (("u16.npy", np.uint16), ("i32.npy", np.int32), ("i64.npy", np.int64)):
        np.save(os.path.join(tmp, name), (maps[1] // 256).astype(dt))
        d = bp.decode_train_record(parse_split_line("rgb1.png None None %s None None None None\n" % name), tmp, with_lidar=True, shape=SHAPE)
        assert d['lidar'].dtype == np.float32, name
        np.testing.assert_array_equal(d['lidar'], (maps[1] // 256).astype(np.float32))
        np.testing.assert_array_equal(d['lidar'], np.ascontiguousarray(np.load(os.path.join(tmp, name)), dtype=np.float32))      # read_lidar_map's cast
        assert bp.plan_targets([d], [None], SHAPE, lidar=True)[1][0][0] == bp.SPARSE_F32
    # lidar_raw=False is the per-sample column: the path only; without shape nothing is counted; without with_lidar no key at all
    old = bp.decode_train_record(recs[0], tmp, with_lidar=True, lidar_raw=False, shape=SHAPE)
    assert old['lidar'] is None and old['lidar_cells'] is None and old['lidar_path'] == os.path.join(tmp, "lidar0.png")
    assert bp.decode_train_record(recs[0], tmp, with_lidar=True)['lidar_cells'] is None
    assert 'lidar' not in bp.decode_train_record(recs[0], tmp)
    # after decode the files can go: planning needs the samples only
    for name in ("lidar0.png", "lidar1.npy", "lidar2.npz"):
        os.remove(os.path.join(tmp, name))
    arrays, rows, keys, fallbacks, winner_elems, out_elems = bp.plan_targets(got[:3], [(2, 1, 22, 11)] * 3, SHAPE, lidar=True)
    assert [k for k, _, _ in keys] == ['lidar'] and len(arrays) == 3 and not fallbacks
    with pytest.raises(KeyError):
        bp.plan_targets(got, [None] * 4, SHAPE, lidar=True)               # a batch with a .bin record has no 'lidar' rows


def test_nothing_on_a_worker_reaches_for_the_device():
    for fn in (bp.decode_train_record, bp.lidar_window, lp.read_lidar_raw, lp.resized_cells, lp.count_survivors, lp.draw_batch, lp.batch_arrays,
               lp.pack_batch_rows):
        src = inspect.getsource(fn).split('"""')[-1]
        assert "torch" not in src and "kernels" not in src and "lib." not in src, fn.__name__


def _samples():
    g = np.random.default_rng(5)
    out = []
    for (h, w), dt in (((37, 70), np.uint16), ((40, 66), np.float32)):
        lidar = ((g.random((h, w)) < 0.2) * g.integers(1, 65536, (h, w))).astype(dt)
        out.append({'rgb': g.integers(0, 256, (h, w, 3), dtype=np.uint8), 'depth': g.integers(0, 65536, (h, w)).astype(np.uint16),
                    'edge': [g.integers(0, 2, (h, w), dtype=np.uint8)], 'normal': [], 'lidar': lidar, 'lidar_path': 'x'})
    return out


def test_rows_offsets_and_the_arena_round_trip_with_the_draws():
    samples = _samples()
    borders = [(2, 1, 66, 33), None]
    arrays, rows, keys, fallbacks, winner_elems, out_elems = bp.plan_targets(samples, borders, (32, 64), lidar=True)
    assert [k for k, _, _ in keys] == ['depth', 'lidar', 'edge'] and [t for _, t, _ in keys] == [(32, 64)] * 3
    dst = {k: off for k, _, off in keys}
    assert dst == {'depth': 0, 'lidar': 2 * 2048, 'edge': 4 * 2048} and winner_elems == out_elems == 6 * 2048
    assert [r[0] for r in rows] == [bp.SPARSE_U16, bp.SPARSE_U16, bp.SPARSE_U16, bp.SPARSE_F32, bp.EDGE_U8, bp.EDGE_U8]
    assert rows[2][2:11] == [37, 70, 2, 1, 32, 64, dst['lidar'], 32, 64] and rows[3][2:11] == [40, 66, 0, 0, 40, 66, dst['lidar'] + 2048, 32, 64]
    assert arrays[2] is samples[0]['lidar'] and arrays[3] is samples[1]['lidar']
    # without the flag the plan is the one of a batch without the column
    assert [k for k, _, _ in bp.plan_targets(samples, borders, (32, 64))[2]] == ['depth', 'edge']
    # the draws of both samples and the perturbation's table behind the maps and the frames, as DeviceStage packs them
    cells = [lp.resized_cells(s['lidar'], bp.crop_window(b, *s['lidar'].shape), (32, 64)) for s, b in zip(samples, borders)]
    np.random.seed(4)
    drawn = lp.draw_batch(cells, (32, 64), SCALE, ADD, 0.2)
    extra = lp.batch_arrays(drawn)
    assert [a.dtype for a in extra] == [np.float64, np.uint8] * 2 and [a.shape for a in extra] == [(3, d['n']) if i % 2 == 0 else (d['survivors'],)
                                                                                                  for d in drawn for i in (0, 1)]
    packed = arrays + [s['rgb'] for s in samples] + extra
    _, ahead, _ = bp.arena_layout(packed, len(rows))
    table = lp.pack_batch_rows(drawn, ahead[len(arrays) + 2:])
    packed.append(table.reshape(-1))
    arena = bp.HostArena()
    arena.reserve(bp.arena_layout(packed, len(rows))[2])
    arena.view[:] = 0xAB
    t_off, offs, total, live = bp.pack_arena(arena, packed, rows + [None] * (len(packed) - len(arrays)))
    assert offs[:len(ahead)] == ahead and all(o % 16 == 0 for o in offs) and len(live) == 6
    back = np.frombuffer(bytes(arena.view[offs[-1]:offs[-1] + table.nbytes]), dtype=np.int64).reshape(2, lp.LIDAR_BATCH_ROW_WORDS)
    np.testing.assert_array_equal(back, table)
    for b, d in enumerate(drawn):
        n, m, bits, o_i, o_j, o_d, o_k, zero = (int(v) for v in back[b])
        assert (n, m, zero) == (d['n'], d['survivors'], 0) and n == len(cells[b]) and 0 < m < n
        assert np.int64(bits).view(np.float64) == d['scale_d0'] and 1 / 1.1 <= d['scale_d0'] <= 1.1        # (drawn in 1 .. 1.1, inverted for half of the draws)
        assert o_i % 8 == 0 and o_j % 8 == 0 and o_d % 8 == 0 and (o_j - o_i, o_d - o_j) == (8 * n, 8 * n)      # float64 on 8 bytes
        for row, off in enumerate((o_i, o_j, o_d)):
            np.testing.assert_array_equal(np.frombuffer(bytes(arena.view[off:off + 8 * n]), dtype=np.float64), d['adds'][row])
        np.testing.assert_array_equal(arena.view[o_k:o_k + m], d['keep'])
        assert o_d + 8 * n <= o_k and o_k + m <= offs[-1] <= total
    # the maps are where their rows say, in the kinds' types
    tab, maps = bp.unpack_arena(arena.view, 6)
    np.testing.assert_array_equal(maps[2], samples[0]['lidar'])
    np.testing.assert_array_equal(maps[3], samples[1]['lidar'])
    assert maps[3].dtype == np.float32 and tab[3, 1] == offs[3]
    with pytest.raises(ValueError):
        lp.pack_batch_rows(drawn, [4, 0, 8, 0])                           # float64 draws off their boundary


JITTER = (0.2, 0.2, 0.2, 0.05)


class _Stage:
    """stands in for DeviceStage: runs its draw loop (prefetch.draw_handover) at hand-over, on the consumer thread, and keeps the draws"""

    def __init__(self, maps):
        self.maps, self.seen, self.jitter = maps, [], []

    def decode(self, j):                                                  # odd records come from a decoder that did not count
        m = self.maps[j]
        return {'j': j, 'lidar': m, 'lidar_cells': np.flatnonzero(m.reshape(-1) > 0) if j % 2 == 0 else None}

    def __call__(self, samples, idxs):
        from mindtheedge_amd.datasets.prefetch import draw_handover
        assert threading.current_thread() is threading.main_thread()
        params, drawn = draw_handover(samples, [None] * len(samples), SHAPE, JITTER, (SCALE, ADD, 0.25))
        self.jitter += params
        self.seen.append(drawn)
        return {'idx': list(idxs)}


def test_draw_sequence_is_the_per_sample_paths_for_a_batch_with_different_n():
    """the stage's own draw loop against what ds[j] draws, sample after sample: the colour jitter from `random`, then the perturbation for
    n and the permutation for n' from np.random (an empty map: nothing); one random.random() between batches, as the model's flip draw"""
    import random
    from mindtheedge_amd.datasets import image_prep as ip
    from mindtheedge_amd.datasets.prefetch import draw_handover
    g = np.random.default_rng(2)
    maps = [((g.random(SHAPE) < p) * (1 + g.random(SHAPE))).astype(np.float32) for p in (0.4, 0.1, 0.0, 0.7, 0.25, 0.05)]
    np.random.seed(77)
    random.seed(78)
    want, want_jitter = [], []
    for k, m in enumerate(maps):
        want_jitter.append(ip.draw_color_jitter(JITTER))
        n = int((m > 0).sum())
        if n:
            s, ai, aj, ad = lp.draw_lidar_perturbation(n, SCALE, ADD)
            want.append((n, s, ai, aj, ad, lp.draw_lidar_keep(R.count_survivors(m, s, ai, aj, ad), 0.25)))
        else:
            want.append((0,))
        if k % 3 == 2:
            random.random()
    tails = (np.random.rand(), random.random())
    stage = _Stage(maps)
    np.random.seed(77)
    random.seed(78)
    loader = PrefetchSplitLoader(list(range(6)), 3, shuffle=False, num_workers=3, device_stage=stage, decode=stage.decode)
    got_idx = []
    for b in loader:
        got_idx.append(b['idx'])
        random.random()
    assert got_idx == [[0, 1, 2], [3, 4, 5]]
    assert (np.random.rand(), random.random()) == tails
    assert repr(stage.jitter) == repr(want_jitter)
    got = [d for batch in stage.seen for d in batch]
    assert len({d['n'] for d in got}) == 6
    for d, w in zip(got, want):
        assert d['n'] == w[0]
        if w[0]:
            assert d['scale_d0'] == w[1] and d['survivors'] == len(w[5])
            np.testing.assert_array_equal(d['adds'], np.stack(w[2:5]))
            np.testing.assert_array_equal(d['keep'], w[5])
    # without the column (or with it unperturbed / on the per-sample path) only the jitter is drawn
    state = np.random.get_state()[1].copy()
    params, drawn = draw_handover([stage.decode(0), stage.decode(1)], [None, None], SHAPE, JITTER, None)
    assert len(params) == 2 and drawn == [] and (np.random.get_state()[1] == state).all()
    # a crop window that leaves nothing of a map is an error with the window in it, not a division by zero
    with pytest.raises(ValueError, match="leaves nothing"):
        lp.resized_cells(maps[0], (0, 0, 0, 5), SHAPE)


def test_status_check_names_the_samples():
    from mindtheedge_amd._lib import MteError
    lp.check_status(np.array([[5, 5, 3, 3], [0, 0, 0, 0]]))
    with pytest.raises(MteError, match=r"records \[8, 9\].*\(7, 2\).*\(6, 2\).*sample\(s\) \[1\]"):
        lp.check_status(np.array([[5, 5, 3, 3], [7, 6, 2, 2]]), "the batch of records [8, 9]")
    with pytest.raises(MteError, match=r"sample\(s\) \[0, 2\]"):
        lp.check_status(np.array([[5, 5, 3, 4], [1, 1, 0, 0], [2, 3, 1, 1]]))
