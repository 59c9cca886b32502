"""GPU (-m gpu): the LiDAR column of the prefetching training loader -- decoded ahead, resized in mte_batch_prep, perturbed by
mte_batch_lidar_perturb (csrc/lidar_prep.hip) -- against SplitLoader and against augment_depth_values per map.  Every comparison is bit
equality.  Maps are tiny (32 x 64 targets; 48 x 96 where a map has to span three scan chunks)."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import lidar_ref as R
from guard_band import Flat

pytestmark = pytest.mark.gpu
SCALE, ADD = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5))
JITTER = (0.2, 0.2, 0.2, 0.05)
# (frame size, LiDAR file, LiDAR map size): larger than, equal to and smaller than the 32 x 64 target; record 5 has no return at all
RECORDS = (((37, 70), "png", (37, 70)), ((40, 66), "npy", (40, 66)), ((37, 70), "npz", (37, 70)),
           ((37, 70), "png", (32, 64)), ((37, 70), "npy", (20, 40)), ((40, 66), "npy", (40, 66)))


INT_RECORDS = (((37, 70), "npy_u16", (37, 70)), ((40, 66), "npy_i32", (40, 66)), ((37, 70), "bin", (37, 70)))


def _write_bin(path, raw):
    """a velodyne cloud whose GTA projection hits returns of the depth map `raw` (uint16, /256) exactly, plus points that miss"""
    h, w = raw.shape
    ys, xs = np.nonzero(raw)
    ys, xs = ys[::3], xs[::3]
    z = raw[ys, xs].astype(np.float64) / 256.0
    X, Y = (xs + 0.5 - 960.0) / 960.0 * z, (ys + 0.5 - 540.0) / 960.0 * z
    pts = np.stack([z, -X, -Y, np.ones_like(z)], axis=1)                  # camera axes are (-y, -z, x) of the file
    pts = np.concatenate([pts, [[5.0, 0.0, 0.0, 1.0], [np.nan, 1.0, 1.0, 1.0]]]).astype(np.float32)
    pts.tofile(path)


def _write_split(tmp, shape=(32, 64), records=RECORDS, lines=None, name="split"):
    H, W = shape
    g = np.random.default_rng(4)
    os.makedirs(os.path.join(tmp, "normals"), exist_ok=True)
    rows = []
    for i, ((h, w), kind, (lh, lw)) in enumerate(records):
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(tmp, "rgb%d.png" % i))
        raw = ((g.random((h, w)) < 0.15) * (256 + g.integers(0, 70 * 256, (h, w)))).astype(np.uint16)
        raw[0, 0] = 300
        Image.fromarray(raw).save(os.path.join(tmp, "depth%d.png" % i))
        sparse = ((g.random((lh, lw)) < 0.12) * (256 + g.integers(0, 60 * 256, (lh, lw)))).astype(np.uint16)
        sparse[lh - 1, lw - 1] = 700
        lidar = "lidar%d.%s" % (i, kind.split("_")[0])
        if kind in ("npy_u16", "npy_i32"):                                # metres as integers: a .npy is taken as it is, whatever its type
            np.save(os.path.join(tmp, lidar), (sparse // 256).astype(np.uint16 if kind == "npy_u16" else np.int32))
        elif kind == "png":
            Image.fromarray(sparse).save(os.path.join(tmp, lidar))
        elif kind == "npy":
            np.save(os.path.join(tmp, lidar), np.zeros((lh, lw), dtype=np.float32) if i == 5 else (sparse / 256.0).astype(np.float32))
        elif kind == "npz":
            np.savez(os.path.join(tmp, lidar), velodyne_depth=np.where(sparse == 0, -1.0, sparse / 256.0))      # float64 with -1, cast on reading
        else:
            _write_bin(os.path.join(tmp, lidar), raw)
        for s in range(4):
            Image.fromarray(((g.random((H >> s, W >> s)) < 0.2) * 255).astype(np.uint8)).save(os.path.join(tmp, "%08d_e_00%d.png" % (i, s)))
            Image.fromarray(g.integers(0, 256, (H >> s, W >> s), dtype=np.uint8)).save(os.path.join(tmp, "normals", "%08d_e_00%d.png" % (i, s)))
        rows.append("rgb%d.png depth%d.png %08d_e_000.png %s None None None normals/%08d_e_000.png\n" % (i, i, i, lidar, i))
    split = os.path.join(tmp, "%s.txt" % name)
    with open(split, "w") as f:
        f.writelines(rows[j] for j in (lines if lines is not None else range(len(records))))
    return split


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("prefetch_lidar"))
    bin_tmp = str(tmp_path_factory.mktemp("prefetch_lidar_bin"))
    int_tmp = str(tmp_path_factory.mktemp("prefetch_lidar_int"))
    return {"root": tmp, "split": _write_split(tmp), "cycled": _write_split(tmp, lines=[j % 6 for j in range(24)], name="cycled"),
            "bin_root": bin_tmp, "bin": _write_split(bin_tmp, records=(RECORDS[0], ((37, 70), "bin", (37, 70)), RECORDS[1])),
            "int_root": int_tmp, "int": _write_split(int_tmp, records=INT_RECORDS),
            "int_bin": _write_split(int_tmp, records=INT_RECORDS, lines=[0, 2, 1], name="int_bin")}


def _dataset(files, split="split", perturbed=True, drop=0.2, **kw):
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset
    if perturbed:
        kw.update(lidar_scale=SCALE, lidar_add=ADD, lidar_drop_rate=drop)
    return KittiEdgeSplitDataset(files[split], (32, 64), root=files[{"bin": "bin_root", "int": "int_root", "int_bin": "int_root"}.get(split, "root")], input_depth_type=["velodyne"], **kw)


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.is_tensor(b[k]) and a[k].dtype == b[k].dtype == torch.float32 and a[k].shape == b[k].shape and a[k].device == b[k].device, k
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
        else:
            assert a[k] == b[k], k


def _both(ds, bs, seeds, **kw):
    """an epoch of SplitLoader and of the prefetching loader, both random streams seeded before each -> (batches, batches, tails, loader)"""
    from mindtheedge_amd.datasets.kitti_edges import SplitLoader
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    out, tails = [], []
    new = PrefetchSplitLoader(ds, bs, shuffle=False, num_workers=2, **kw)
    for loader in (SplitLoader(ds, bs, shuffle=False), new):
        random.seed(seeds)
        np.random.seed(seeds)
        got = []
        for batch in loader:
            got.append(batch)
            random.random()
        tails.append((random.random(), float(np.random.rand())))
        out.append(got)
    return out[0], out[1], tails, new


@pytest.mark.parametrize("perturbed,drop,bs,crop", [(True, 0.2, 3, False), (True, 0.0, 1, False), (True, 1.0, 3, True), (True, 0.2, 1, True),
                                                    (False, 0.0, 3, True), (False, 0.0, 1, False)])
def test_batches_bit_equal_with_split_loader(files, perturbed, drop, bs, crop):
    kw = {"crop_train_borders": (2, 33, 3, 60)} if crop else {}
    ds = _dataset(files, perturbed=perturbed, drop=drop, jittering=JITTER, **kw)
    ref, new, tails, loader = _both(ds, bs, seeds=13)
    assert len(ref) == len(new) == 6 // bs and {"rgb_original", "depth", "lidar", "input_depth", "edge_3", "normal_3"} <= set(ref[0])
    for a, b in zip(ref, new):
        _same(a, b)
    assert tails[0] == tails[1]                                           # both random streams stand where SplitLoader leaves them
    assert all(bool(b["lidar"].any()) for b in new if b["idx"] != [5])
    first = new[0]
    assert torch.equal(first["lidar"], first["input_depth"]) == (not perturbed)
    if perturbed:
        assert bool(first["input_depth"].any()) == (drop < 1.0)
        assert all(s.status is not None and s.check is None for s in loader._stage.slots[:min(4, 6 // bs)])      # the batched pass ran, every check was made
        empty = new[-1]["input_depth"][-1]                                # record 5: no return, nothing drawn, zeros
        assert not bool(empty.any())
    else:
        assert all(s.status is None for s in loader._stage.slots)


def test_a_batch_with_a_bin_record_takes_the_per_sample_path(files):
    from mindtheedge_amd.datasets import batch_prep as bp
    ds = _dataset(files, "bin")
    ref, new, tails, loader = _both(ds, 3, seeds=2)
    assert len(new) == 1
    _same(ref[0], new[0])
    assert tails[0] == tails[1]
    assert bool(new[0]["lidar"][1].any())                                 # the projected cloud left returns
    samples = [loader._stage.decode(j) for j in range(3)]
    assert [s["lidar"] is None for s in samples] == [False, True, False] and not bp.lidar_batchable(samples)
    assert all(s.status is None for s in loader._stage.slots)             # the batched pass did not run


@pytest.mark.parametrize("split,bs", [("int", 2), ("int_bin", 3)])
def test_integer_npy_maps_are_not_taken_for_16_bit_pngs(files, split, bs):
    """a uint16 and an int32 .npy hold metres, not 1/256 m: float32 of the values as SplitLoader reads them -- in the batched pass (the
    first two records) and when a .bin record sends the decoded maps through the per-sample functions"""
    ds = _dataset(files, split)
    ref, new, tails, loader = _both(ds, bs, seeds=5)
    assert len(new) == 1 and tails[0] == tails[1]
    _same(ref[0], new[0])
    samples = [loader._stage.decode(j) for j in range(bs)]
    assert all(s["lidar"].dtype == np.float32 for s in samples if s["lidar"] is not None)
    for b in (0, bs - 1):                                                 # the integer records: whole metres, up to 60, not 60 / 256
        values = new[0]["lidar"][b][new[0]["lidar"][b] > 0]
        assert bool((values == values.round()).all()) and float(values.max()) > 30
    assert all((s.status is not None) == (split == "int") for s in loader._stage.slots[:1])


def test_no_host_read_with_the_perturbed_column(files):
    """three next() calls under torch's synchronisation debug mode; the per-sample stage raises under it (the guard is live, and this is
    what the column cost before)"""
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    ds = _dataset(files, "cycled")
    old = PrefetchSplitLoader(ds, 2, shuffle=False, num_workers=2, prefetch=2, batched_lidar=False)
    loader = PrefetchSplitLoader(ds, 2, shuffle=False, num_workers=2, prefetch=2)
    assert not old._stage.batched_lidar and loader._stage.batched_lidar
    it_old, it = iter(old), iter(loader)
    next(it_old), next(it_old)
    got = [next(it), next(it)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            next(it_old)                                                  # counts[0].item() of augment_depth_values
        for _ in range(3):
            got.append(next(it))                                          # the fifth batch reuses the first slot: its count check runs here too
    finally:
        torch.cuda.set_sync_debug_mode("default")
        old.close()
        loader.close()
    assert [b["idx"] for b in got] == [[2 * i, 2 * i + 1] for i in range(5)]
    assert bool(got[4]["input_depth"].any()) and not torch.equal(got[4]["input_depth"], got[4]["lidar"])
    for k in ("lidar", "depth", "edge"):                                  # the records cycle: batch 3 is batch 0 again (the draws differ, the maps do not)
        assert torch.equal(got[0][k], got[3][k])


# ---- the kernel, one call for a batch of crafted maps -----------------------------------------------------------------------------------------------
H, W = 48, 96                                                             # 4608 elements: three scan chunks of 2048


def _crafted():
    """-> (maps float32 [B,H,W], draws per map).  0 empty; 1 a single return; 2 every return moved into one cell; 3 everything dropped;
    4 ~60 % density (n > one scan chunk); 5 ~5 %; 6 ~30 %: neighbouring samples differ in n."""
    from mindtheedge_amd.datasets import lidar_prep as lp
    g = np.random.default_rng(11)
    maps = np.zeros((7, H, W), dtype=np.float32)
    maps[1, 20, 33] = 7.5
    for y, x in ((3, 4), (10, 50), (40, 90), (47, 95), (0, 0)):
        maps[2, y, x] = 1.0 + y
    for b, p in ((3, 0.2), (4, 0.6), (5, 0.05), (6, 0.3)):
        maps[b] = (g.random((H, W)) < p) * (1 + 60 * g.random((H, W)))
    draws = []
    for b in range(7):
        i, j = np.nonzero(maps[b] > 0)
        n = len(i)
        if b == 2:
            add_i, add_j = 7.0 - i, 9.0 - j                               # all into (7, 9)
        else:
            add_i, add_j = np.round(g.uniform(-1.5, 1.5, n) * 2) / 2, np.round(g.uniform(-1.5, 1.5, n) * 2) / 2      # halves included
        d = {'scale_d0': 1.0 + 0.01 * b, 'add_i': add_i.astype(np.float64), 'add_j': add_j.astype(np.float64), 'add_d': g.uniform(0, 0.5, n)}
        survivors = lp.count_survivors(np.flatnonzero(maps[b].reshape(-1) > 0), (H, W), d['add_i'], d['add_j']) if n else 0
        d['keep'] = np.zeros(survivors, dtype=np.uint8) if b == 3 else (g.random(survivors) < 0.8).astype(np.uint8)
        draws.append(d)
    return maps, draws


def _pack(maps, draws, edit=None):
    """arena (host tensor) with the draws and the table -> (host tensor, table offset, table view); edit(table) changes rows before the upload"""
    from mindtheedge_amd.datasets import batch_prep as bp
    from mindtheedge_amd.datasets import lidar_prep as lp
    cells = [np.flatnonzero(m.reshape(-1) > 0) for m in maps]
    drawn = lp.draw_batch(cells, (H, W), SCALE, ADD, 0.2, draws)
    arrays = lp.batch_arrays(drawn)
    _, offs, total = bp.arena_layout(arrays, 0)
    table = lp.pack_batch_rows(drawn, offs)
    if edit is not None:
        edit(table)
    host = bp.HostArena()
    host.reserve(total + table.nbytes + 64)
    host.view[:] = 0
    bp.pack_arena(host, arrays, [None] * len(arrays))
    host.view[total:total + table.nbytes] = table.reshape(-1).view(np.uint8)
    return host.tensor, total, table, drawn


def _call(maps, host, t_off):
    """one raw call with guard bands around the output, the workspace and the status -> (out Flat, work Flat, status Flat)"""
    from mindtheedge_amd import kernels as K
    B = len(maps)
    src = torch.from_numpy(maps).cuda()
    dev = host.cuda()
    work_bytes = K.lib.mte_batch_lidar_perturb_work_bytes(B, H, W)
    assert work_bytes > 0 and work_bytes % 8 == 0
    out, work, status = Flat(B * H * W), Flat(work_bytes // 8, torch.float64), Flat(4 * B)
    K.lib.mte_batch_lidar_perturb(src.data_ptr(), B, H, W, dev.data_ptr(), int(dev.numel()), host.data_ptr() + t_off, dev.data_ptr() + t_off,
                                  out.ptr, work.ptr, status.ptr, K._stream())
    torch.cuda.synchronize()
    return out, work, status


def _status(flat, B):
    return flat.get().view(torch.int32).view(B, 4).numpy()


@pytest.fixture(scope="module")
def crafted():
    maps, draws = _crafted()
    host, t_off, table, drawn = _pack(maps, draws)
    want = np.stack([R.augment_depth_values(m, d['scale_d0'], d['add_i'], d['add_j'], d['add_d'], d['keep']).astype(np.float32) for m, d in zip(maps, draws)])
    return {"maps": maps, "draws": draws, "host": host, "t_off": t_off, "table": table, "drawn": drawn, "want": want}


def test_batched_kernel_against_augment_depth_values_per_map(crafted):
    from mindtheedge_amd.datasets import lidar_prep as lp
    maps, draws, drawn = crafted["maps"], crafted["draws"], crafted["drawn"]
    n = [d['n'] for d in drawn]
    assert n[0] == 0 and n[1] == 1 and n[2] == 5 and n[4] > 2048 and len(set(n)) == 7
    assert [d['survivors'] for d in drawn][:3] == [0, 0, 0] and drawn[4]['survivors'] > 0
    assert [d['survivors'] for d in drawn] == [R.count_survivors(m, 1.0, d['add_i'], d['add_j'], d['add_d']) for m, d in zip(maps, draws)]
    out, work, status = _call(maps, crafted["host"], crafted["t_off"])
    assert out.guard_ok() and work.guard_ok() and status.guard_ok()
    got = out.get().view(7, H, W)
    st = _status(status, 7)
    np.testing.assert_array_equal(st, [[d['n'], d['n'], d['survivors'], d['survivors']] for d in drawn])
    lp.check_status(st)
    for b in range(7):
        per_map = lp.augment_depth_values(torch.from_numpy(maps[b]).cuda(), SCALE, ADD, 0.2, draws=draws[b]).cpu()
        assert torch.equal(got[b].view(torch.int32), per_map.view(torch.int32)), b
        np.testing.assert_array_equal(got[b].numpy().view(np.int32), crafted["want"][b].view(np.int32))       # and the restated rules
    assert not got[:4].any() and bool(got[4].any()) and bool(got[5].any())
    # the Python entry: the same batch through augment_depth_values_batch
    again, st2 = lp.augment_depth_values_batch(torch.from_numpy(maps).cuda(), [np.flatnonzero(m.reshape(-1) > 0) for m in maps], SCALE, ADD, 0.2, draws=draws)
    assert torch.equal(again.cpu().view(torch.int32), got.view(torch.int32))
    lp.check_status(st2.cpu().numpy())


def test_the_same_call_twice_is_bit_equal(crafted):
    a = _call(crafted["maps"], crafted["host"], crafted["t_off"])[0].get()
    b = _call(crafted["maps"], crafted["host"], crafted["t_off"])[0].get()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("column,delta", [(0, 1), (0, -1), (1, 1), (1, -1)], ids=["n+1", "n-1", "survivors+1", "survivors-1"])
def test_a_wrong_host_count_is_reported_not_followed(crafted, column, delta):
    """the table claims one return / one survivor more or less than the map has (samples 4 and 6): every loop stops at the smaller of the
    two counts, the call succeeds, nothing outside the buffers is written, the status names the samples"""
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.datasets import lidar_prep as lp
    maps, draws, drawn = crafted["maps"], crafted["draws"], crafted["drawn"]

    def edit(table):
        table[4, column] += delta
        table[6, column] += delta

    host, t_off, table, _ = _pack(maps, draws, edit)
    out, work, status = _call(maps, host, t_off)                          # MTE_OK: the wrapper did not raise
    assert out.guard_ok() and work.guard_ok() and status.guard_ok()
    st = _status(status, 7)
    bad = [b for b in range(7) if st[b, 0] != st[b, 1] or st[b, 2] != st[b, 3]]
    assert bad == [4, 6]
    assert [int(st[b, 1]) for b in range(7)] == [d['n'] for d in drawn]   # the device's own n is the map's
    assert all(int(st[b, column * 2]) == (drawn[b]['n'], drawn[b]['survivors'])[column] + delta for b in (4, 6))
    with pytest.raises(MteError, match=r"sample\(s\) \[4, 6\]"):
        lp.check_status(st, "a test batch")
    got = out.get().view(7, H, W)
    for b in (0, 1, 2, 3, 5):                                             # the other samples are untouched by their neighbours' rows
        np.testing.assert_array_equal(got[b].numpy().view(np.int32), crafted["want"][b].view(np.int32))
    assert bool(torch.isfinite(got).all())


def test_a_row_outside_the_arena_is_refused_before_any_launch(crafted):
    from mindtheedge_amd import kernels as K
    maps, draws = crafted["maps"], crafted["draws"]
    B = len(maps)
    src = torch.from_numpy(maps).cuda()
    work_bytes = K.lib.mte_batch_lidar_perturb_work_bytes(B, H, W)
    host, t_off, table, _ = _pack(maps, draws)
    nbytes = int(host.numel())
    for row, col, bad in ((4, 3, nbytes), (4, 4, -8), (5, 5, nbytes - 8), (6, 6, nbytes + 1), (4, 3, int(table[4, 3]) + 4), (4, 0, H * W + 1), (4, 1, int(table[4, 0]) + 1),
                          (5, 0, -1)):
        def edit(t):
            t[row, col] = bad
        broken, off, _, _ = _pack(maps, draws, edit)
        dev = broken.cuda()
        out, work, status = Flat(B * H * W), Flat(work_bytes // 8, torch.float64), Flat(4 * B)
        with pytest.raises(K.MteError):
            K.lib.mte_batch_lidar_perturb(src.data_ptr(), B, H, W, dev.data_ptr(), nbytes, broken.data_ptr() + off, dev.data_ptr() + off,
                                          out.ptr, work.ptr, status.ptr, K._stream())
        torch.cuda.synchronize()
        assert out.untouched() and work.untouched() and status.untouched(), (row, col)
    assert K.lib.mte_batch_lidar_perturb_work_bytes(0, H, W) == 0 and K.lib.mte_batch_lidar_perturb_work_bytes(70000, H, W) == 0


# ---- the loader's count check -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,delta", [("n", 1), ("n", -1), ("survivors", 1), ("survivors", -1)])
def test_loader_raises_at_the_next_reuse_of_the_slot(files, monkeypatch, which, delta):
    """the host count of record 1 (batch 0) is made wrong by one: the batch is handed out (nobody has looked yet), the four batches after
    it too, and the next() that takes batch 0's slot again raises, naming the batch"""
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.datasets import lidar_prep as lp
    from mindtheedge_amd.datasets.prefetch import DeviceStage, PrefetchSplitLoader
    ds = _dataset(files, "cycled")
    stage = DeviceStage(ds, 4)
    decode = stage.decode
    if which == "n":
        def decode(j):
            smp = stage.decode(j)
            if j == 1:
                cells = smp['lidar_cells']
                spare = np.setdiff1d(np.arange(32 * 64), cells)[:1]
                smp['lidar_cells'] = np.sort(np.concatenate([cells, spare])) if delta > 0 else cells[:-1]
            return smp
    else:
        true_count, calls = lp.count_survivors, []

        def wrong(cells, shape, add_i, add_j):
            calls.append(1)
            return true_count(cells, shape, add_i, add_j) + (delta if len(calls) == 2 else 0)      # the second sample of the first batch
        monkeypatch.setattr(lp, "count_survivors", wrong)
    np.random.seed(1)
    loader = PrefetchSplitLoader(ds, 2, shuffle=False, num_workers=2, prefetch=2, device_stage=stage, decode=decode)
    it = iter(loader)
    try:
        for _ in range(4):
            next(it)                                                      # four slots: nothing is reused yet
        with pytest.raises(MteError, match=r"records \[0, 1\].*sample\(s\) \[1\]"):
            next(it)
    finally:
        loader.close()
        torch.cuda.synchronize()


def test_loader_checks_the_last_batches_when_the_epoch_ends(files, monkeypatch):
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.datasets import lidar_prep as lp
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    true_count, calls = lp.count_survivors, []

    def wrong(cells, shape, add_i, add_j):
        calls.append(1)
        return true_count(cells, shape, add_i, add_j) + (1 if len(calls) == 4 else 0)              # batch 1, its first sample (record 3)
    monkeypatch.setattr(lp, "count_survivors", wrong)
    loader = PrefetchSplitLoader(_dataset(files), 3, shuffle=False, num_workers=2)
    it = iter(loader)
    assert next(it)["idx"] == [0, 1, 2] and next(it)["idx"] == [3, 4, 5]
    with pytest.raises(MteError, match=r"records \[3, 4, 5\].*sample\(s\) \[0\]"):
        next(it)                                                          # no third batch: the outstanding checks are made instead
    torch.cuda.synchronize()


# ---- a training step --------------------------------------------------------------------------------------------------------------------------------
def test_one_completion_step_on_a_batch_of_each_stage(tmp_path):
    """The batches of the two stages are bit-equal (every key); one training step of the completion model on each must then give bit-equal
    losses.  The second half holds as far as the model repeats itself: the training path of the sparse branch takes its batch-norm
    statistics with floating-point atomics (csrc/san.hip: fold_channel_sums), whose order of addition is the scheduler's, so the last bits
    of the loss can differ between two steps on the same batch."""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.models.SemiSupEdgeCompletionModel import SemiSupEdgeCompletionModel
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    shape = (64, 128)
    split = _write_split(str(tmp_path), shape, records=(((69, 134), "png", (69, 134)), ((72, 130), "npy", (72, 130))))
    ds = KittiEdgeSplitDataset(split, shape, root=str(tmp_path), input_depth_type=["velodyne"], lidar_scale=SCALE, lidar_add=ADD, lidar_drop_rate=0.2)
    batches = []
    for batched in (False, True):
        np.random.seed(6)
        (b,) = list(PrefetchSplitLoader(ds, 2, shuffle=False, num_workers=2, batched_lidar=batched))
        batches.append(b)
    _same(*batches)
    assert not torch.equal(batches[1]["lidar"], batches[1]["input_depth"])
    K.set_compute_dtype("fp32")
    try:
        torch.manual_seed(42)
        net = PackNetSAN01(dropout=None, version="1A", with_san=True)
        model = SemiSupEdgeCompletionModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog",
                                           supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.0)
        model.add_depth_net(net.cuda())
        model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
        model.train()
        losses = []
        for batch in batches:
            model.zero_grad()
            out = model(dict(batch))
            out["loss"].sum().backward()
            losses.append(out["loss"].detach().float().cpu())
        assert torch.isfinite(losses[0]).all() and float(losses[0].abs().sum()) > 0
        assert torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32))
    finally:
        K.set_compute_dtype("bf16")
