"""CPU: the host side of the prefetching training loader (mindtheedge_amd/datasets/batch_prep.py, prefetch.py) -- the pure decoder
against the per-sample readers, the arena / descriptor-table packing, the index and batch order against SplitLoader, worker failures and
thread shutdown, and the configuration key.  The device stage is replaced by a stand-in; no GPU is touched."""
import os
import threading
import time

import numpy as np
import pytest
import torch
from PIL import Image

from mindtheedge_amd.datasets import batch_prep as bp
from mindtheedge_amd.datasets.kitti_edges import SplitLoader, _read_gray_u8, parse_split_line, read_png_depth
from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader, choose_loader, epoch_batches


def _write_record(tmp, with_scales=True):
    g = np.random.default_rng(3)
    Image.fromarray(g.integers(0, 256, (11, 17, 3), dtype=np.uint8)).save(os.path.join(tmp, "rgb.png"))
    raw = ((g.random((11, 17)) < 0.3) * g.integers(1, 65536, (11, 17))).astype(np.uint16)
    raw[0, 0], raw[0, 1], raw[0, 2] = 0, 1, 65535
    Image.fromarray(raw).save(os.path.join(tmp, "depth.png"))
    np.save(os.path.join(tmp, "depth.npy"), (raw / 256.0).astype(np.float64))
    os.makedirs(os.path.join(tmp, "normals"), exist_ok=True)
    for s in range(4 if with_scales else 1):
        Image.fromarray(((g.random((12 >> s, 16 >> s)) < 0.2) * 255).astype(np.uint8)).save(os.path.join(tmp, "e_00%d.png" % s))        # grey
        Image.fromarray(g.integers(0, 256, (12 >> s, 16 >> s, 3), dtype=np.uint8)).save(os.path.join(tmp, "normals", "e_00%d.png" % s))   # 3-channel
    return raw


def test_decode_equals_the_per_sample_readers(tmp_path):
    tmp = str(tmp_path)
    raw = _write_record(tmp)
    rec = parse_split_line("rgb.png depth.png e_000.png lidar.bin None None None normals/e_000.png\n")
    d = bp.decode_train_record(rec, tmp, with_lidar=True)
    assert d['rgb'].dtype == np.uint8 and d['rgb'].shape == (11, 17, 3)
    np.testing.assert_array_equal(d['rgb'], np.asarray(Image.open(os.path.join(tmp, "rgb.png")).convert('RGB')))
    assert d['depth'].dtype == np.uint16
    np.testing.assert_array_equal(d['depth'], raw)
    as_float = d['depth'].astype(np.float32) / 256
    as_float[d['depth'] == 0] = -1
    want = read_png_depth(os.path.join(tmp, "depth.png"))
    assert want.dtype == as_float.dtype
    np.testing.assert_array_equal(as_float, want)
    assert len(d['edge']) == 4 and len(d['normal']) == 4
    for s in range(4):
        for name, path in (('edge', "e_00%d.png" % s), ('normal', "normals/e_00%d.png" % s)):
            assert d[name][s].dtype == np.uint8 and d[name][s].ndim == 2
            np.testing.assert_array_equal(d[name][s], _read_gray_u8(os.path.join(tmp, path)))
    assert d['lidar_path'] == os.path.join(tmp, "lidar.bin") and 'lidar_path' not in bp.decode_train_record(rec, tmp)
    # a .npy depth map is float32 as read_png_depth returns it; absent columns stay absent
    d = bp.decode_train_record(parse_split_line("rgb.png depth.npy None None None None None None\n"), tmp)
    assert d['depth'].dtype == np.float32 and d['edge'] == [] and d['normal'] == []
    np.testing.assert_array_equal(d['depth'], read_png_depth(os.path.join(tmp, "depth.npy")))
    assert bp.decode_train_record(parse_split_line("rgb.png None None None None None None None\n"), tmp)['depth'] is None


def test_decode_follows_multiscale_paths_and_rejects_an_8_bit_depth_file(tmp_path):
    tmp = str(tmp_path)
    _write_record(tmp, with_scales=False)                                 # no _001: scale 0 only, like the reference
    d = bp.decode_train_record(parse_split_line("rgb.png depth.png e_000.png None None None None normals/e_000.png\n"), tmp)
    assert len(d['edge']) == 1 and len(d['normal']) == 1
    Image.fromarray(np.full((5, 6), 255, dtype=np.uint16)).save(os.path.join(tmp, "low.png"))
    with pytest.raises(AssertionError):
        read_png_depth(os.path.join(tmp, "low.png"))
    with pytest.raises(AssertionError):
        bp.decode_train_record(parse_split_line("rgb.png low.png None None None None None None\n"), tmp)


def test_the_decoder_does_not_touch_the_device_modules():
    """the worker threads run decode_train_record: nothing in its module may reach for the runtime"""
    import inspect
    for fn in (bp.decode_train_record, bp._read_depth_raw):
        src = inspect.getsource(fn).split('"""')[-1]
        assert "torch" not in src and "kernels" not in src and "lib." not in src


def _samples():
    g = np.random.default_rng(5)
    out = []
    for h, w in ((37, 70), (40, 66)):
        out.append({'rgb': g.integers(0, 256, (h, w, 3), dtype=np.uint8), 'depth': g.integers(0, 65536, (h, w)).astype(np.uint16),
                    'edge': [g.integers(0, 2, (h, w), dtype=np.uint8)] + [g.integers(0, 256, (32 >> s, 64 >> s), dtype=np.uint8) for s in (1, 2, 3)],
                    'normal': [g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h, w), dtype=np.uint8)]})
    return out


def test_arena_and_descriptor_table_round_trip():
    samples = _samples()
    borders = [(2, 1, 66, 33), None]                                      # sample 0 is cropped to 32 x 64: its normal map is at the target size then
    arrays, rows, keys, fallbacks, winner_elems, out_elems = bp.plan_targets(samples, borders, (32, 64))
    assert [k for k, _, _ in keys] == ['depth', 'edge', 'edge_1', 'edge_2', 'edge_3', 'normal', 'normal_1']
    assert [tgt for _, tgt, _ in keys] == [(32, 64), (32, 64), (16, 32), (8, 16), (4, 8), (32, 64), (16, 32)]
    # normal of sample 1 (40 x 66 uncropped) and normal_1 of both (frame size, not 16 x 32) go through the per-map path
    assert [(k, b) for k, b, _, _ in fallbacks] == [('normal', 1), ('normal_1', 0), ('normal_1', 1)]
    assert sum(r is None for r in rows) == 3 and len(arrays) == len(rows) == 14
    # outputs: each key contiguous [B,1,H,W], 16-byte aligned, the preserve-resized ones first, nothing overlapping
    spans = sorted((off, off + 2 * t[0] * t[1], k) for k, t, off in keys)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= out_elems and all(s[0] % 4 == 0 for s in spans)
    assert winner_elems == min(off for k, _, off in keys if k.startswith('normal')) and winner_elems == 2 * (2 * 2048 + 512 + 128 + 32)
    extra = [s['rgb'] for s in samples]
    t_off, offs, total = bp.arena_layout(arrays + extra, 11)
    arena = bp.HostArena()
    assert arena.capacity == 0 and arena.reserve(total) and arena.capacity >= total and not arena.reserve(total // 2)
    arena.view[:] = 0xAB
    t_off2, offs2, total2, live = bp.pack_arena(arena, arrays + extra, rows + [None, None])
    assert (t_off2, offs2, total2) == (t_off, offs, total) and len(live) == 11
    assert all(o % 16 == 0 for o in offs) and t_off % 16 == 0 and offs[0] >= 11 * bp.ROW_WORDS * 8
    ends = [o + a.nbytes for o, a in zip(offs, arrays + extra)]
    assert all(e <= o for e, o in zip(ends, offs[1:])) and ends[-1] <= total
    table, maps = bp.unpack_arena(arena.view, 11)
    for j, i in enumerate(live):
        np.testing.assert_array_equal(maps[j], arrays[i])
        assert maps[j].dtype == arrays[i].dtype
        assert table[j, 1] == offs[i] and list(table[j, 2:4]) == list(arrays[i].shape) and table[j, 11] == 0
    kinds = [int(k) for k in table[:, 0]]
    assert kinds == [bp.SPARSE_U16] * 2 + [bp.EDGE_U8] * 8 + [bp.NORMAL_U8]
    assert list(table[0, 4:8]) == [2, 1, 32, 64] and list(table[1, 4:8]) == [0, 0, 40, 66]       # crop window (x, y, h, w); scale 0 only
    assert list(table[4, 4:8]) == [0, 0, 16, 32]
    dst = {k: off for k, _, off in keys}
    assert table[1, 8] == dst['depth'] + 32 * 64 and list(table[9, 8:11]) == [dst['edge_3'] + 32, 4, 8]
    for b in range(2):                                                    # the frames ride in the same arena
        o = offs[14 + b]
        np.testing.assert_array_equal(arena.view[o:o + extra[b].size].reshape(extra[b].shape), extra[b])
    # growth: a larger batch does not fit, reserve() makes room and the packing is the same
    big = arrays + extra + [np.zeros(3 * arena.capacity, dtype=np.uint8)]
    with pytest.raises(ValueError):
        bp.pack_arena(arena, big, rows + [None] * 3)
    before = arena.capacity
    assert arena.reserve(bp.arena_layout(big, 11)[2]) and arena.capacity > 3 * before
    assert bp.pack_arena(arena, big, rows + [None] * 3)[1][:16] == offs
    np.testing.assert_array_equal(bp.unpack_arena(arena.view, 11)[0], table)
    # batches whose records carry different maps are refused like collate refuses them
    odd = _samples()
    odd[1]['edge'] = odd[1]['edge'][:1]
    with pytest.raises(KeyError):
        bp.plan_targets(odd, [None, None], (32, 64))
    with pytest.raises(ValueError):
        bp.crop_window((70, 0, 80, 10), 37, 70)
    assert bp.crop_window((8, 8, 120, 56), 80, 160) == (8, 8, 48, 112) and bp.crop_window((8, 8, 120, 56), 40, 100) == (8, 8, 32, 92)


class _Stub:
    """a dataset of n records and a device stage that only collates what the workers returned"""

    def __init__(self, n, slow=(), missing=()):
        self.n, self.slow, self.missing = n, set(slow), set(missing)
        self.staged = []

    def __len__(self):
        return self.n

    def __getitem__(self, j):                                             # SplitLoader's side
        return {'idx': j, 'x': torch.tensor([float(j)])}

    def decode(self, j):                                                  # a worker's side
        if j in self.slow:
            time.sleep(0.05)
        if j in self.missing:
            open("/nonexistent/frame_%d.png" % j)
        return {'j': j, 'thread': threading.current_thread().name}

    def stage(self, samples, idxs):
        assert threading.current_thread() is threading.main_thread()      # device work is the consumer's
        assert [s['j'] for s in samples] == list(idxs)
        self.staged.append(list(idxs))
        return {'idx': list(idxs), 'x': torch.tensor([[float(j)] for j in idxs])}


def _loader(stub, bs, **kw):
    return PrefetchSplitLoader(stub, bs, device_stage=stub.stage, decode=stub.decode, **kw)


@pytest.mark.parametrize("shuffle", [False, True])
def test_index_order_is_split_loaders(shuffle):
    stub = _Stub(23)                                                      # 23 records, world 2, batch 3: 3 batches per rank, ragged tail dropped
    for rank in (0, 1):
        ref = SplitLoader(stub, 3, rank, 2, shuffle=shuffle, seed=7)
        new = _loader(stub, 3, rank=rank, world=2, shuffle=shuffle, seed=7, num_workers=2)
        assert len(new) == len(ref) == 3 and new.sampler is new and new.shuffle == shuffle
        seen = []
        for epoch in (0, 1):
            ref.sampler.set_epoch(epoch)
            new.sampler.set_epoch(epoch)
            a, b = list(ref), list(new)
            assert [x['idx'] for x in a] == [x['idx'] for x in b] and len(b) == 3
            assert all(torch.equal(x['x'], y['x']) for x, y in zip(a, b))
            seen.append([x['idx'] for x in b])
        assert (seen[0] != seen[1]) == shuffle
    assert epoch_batches(7, 2, 0, 1, False, 0, 0) == [[0, 1], [2, 3], [4, 5]]
    # the attribute the LiDAR test flips after construction works here too
    new = _loader(stub, 4)
    new.shuffle = False
    assert [b['idx'] for b in new][:2] == [[0, 1, 2, 3], [4, 5, 6, 7]]


@pytest.mark.parametrize("workers", [1, 2, 4])
def test_batch_order_with_slow_records(workers):
    start = threading.active_count()
    stub = _Stub(12, slow=(0, 5, 6))
    loader = _loader(stub, 2, shuffle=False, num_workers=workers, prefetch=2)
    got = [b['idx'] for b in loader]
    assert got == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]] == stub.staged
    assert threading.active_count() == start                              # exhausted: the pool is gone
    assert [b['idx'] for b in loader] == got                              # a second iter() works
    assert threading.active_count() == start


def test_worker_failure_surfaces_at_its_batch_and_threads_are_joined():
    start = threading.active_count()
    stub = _Stub(12, missing=(7,))
    loader = _loader(stub, 2, shuffle=False, num_workers=4, prefetch=2)
    it = iter(loader)
    assert [next(it)['idx'] for _ in range(3)] == [[0, 1], [2, 3], [4, 5]]      # batch 3 (records 6, 7) is decoded by now: nothing raised yet
    with pytest.raises(FileNotFoundError):
        next(it)
    assert threading.active_count() == start
    with pytest.raises(StopIteration):
        next(it)
    # early break
    for b in _loader(_Stub(40, slow=range(40)), 2, shuffle=False, num_workers=4, prefetch=2):
        break
    assert threading.active_count() == start
    # close() on a running iterator; a new iter() also ends the previous one
    loader = _loader(_Stub(40), 2, shuffle=False, num_workers=3)
    it = iter(loader)
    next(it)
    assert threading.active_count() > start
    loader.close()
    assert threading.active_count() == start
    with pytest.raises(StopIteration):
        next(it)
    it = iter(loader)
    next(it)
    it2 = iter(loader)
    assert next(it2)['idx'] == [0, 1]
    with pytest.raises(StopIteration):
        next(it)
    loader.close()
    assert threading.active_count() == start
    assert _loader(_Stub(4), 2, num_workers=64).num_workers == 16
    with pytest.raises(ValueError):
        _loader(_Stub(4), 2, num_workers=0)


def test_configuration_key_and_loader_choice():
    from mindtheedge_amd.utils.config import load_config
    cfg = load_config(None)
    assert cfg.datasets.train.num_workers == 0 and cfg.datasets.train.prefetch == 2
    assert choose_loader(cfg.datasets.train.num_workers) == 'split'
    assert choose_loader(None) == 'split' and choose_loader(0) == 'split'
    assert choose_loader(1) == 'prefetch' and choose_loader(16) == 'prefetch'
    with pytest.raises(ValueError):
        choose_loader(-1)
    assert load_config(None, {"datasets": {"train": {"num_workers": 8}}}).datasets.train.num_workers == 8
