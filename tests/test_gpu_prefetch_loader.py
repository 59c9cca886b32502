"""GPU (-m gpu): the prefetching training loader (mindtheedge_amd/datasets/prefetch.py) and the batched target preparation under it
(csrc/batch_prep.hip) against SplitLoader / the per-map functions.  Every comparison is bit equality."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
SIZES = ((37, 70), (40, 66))                                             # two source frame sizes in every batch of 2
JITTER = (0.2, 0.2, 0.2, 0.05)
SCALE, ADD = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5))


def _write_split(tmp, shape, records=6, lines=None):
    """records alternate between the two frame sizes; even records carry their edge / normal maps at the target sizes (shape >> s), odd ones
    at frame size for every scale (scale 3 then shrinks 37 x 70 -> 4 x 8); edge maps alternate between the 0/255 and the 0/1 scale; the depth
    map of record 2 is a .npy.  lines: the records the split file lists, in order (default: each once)."""
    H, W = shape
    g = np.random.default_rng(1)
    os.makedirs(os.path.join(tmp, "normals"), exist_ok=True)
    rows = []
    for i in range(records):
        h, w = SIZES[i % 2] if shape == (32, 64) else (shape[0] + 5 + 3 * (i % 2), shape[1] + 6 - 4 * (i % 2))
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(tmp, "rgb%d.png" % i))
        raw = ((g.random((h, w)) < 0.15) * (256 + g.integers(0, 70 * 256, (h, w)))).astype(np.uint16)
        raw[0, 0] = 300
        depth = "depth%d.png" % i
        Image.fromarray(raw).save(os.path.join(tmp, depth))
        np.save(os.path.join(tmp, "lidar%d.npy" % i), ((g.random((h, w)) < 0.1) * (1 + 60 * g.random((h, w)))).astype(np.float32))
        if i == 2:
            depth = "depth2.npy"
            np.save(os.path.join(tmp, depth), raw.astype(np.float32) / 256.0)
        for s in range(4):
            eh, ew = (H >> s, W >> s) if i % 2 == 0 else (h, w)
            top = 255 if i % 4 < 2 else 1
            Image.fromarray(((g.random((eh, ew)) < 0.2) * top).astype(np.uint8)).save(os.path.join(tmp, "%08d_e_00%d.png" % (i, s)))
            Image.fromarray(g.integers(0, 256, (eh, ew), dtype=np.uint8)).save(os.path.join(tmp, "normals", "%08d_e_00%d.png" % (i, s)))
        lidar = "depth%d.png" % i if i % 2 else "lidar%d.npy" % i
        rows.append("rgb%d.png %s %08d_e_000.png %s None None None normals/%08d_e_000.png\n" % (i, depth, i, lidar, i))
    split = os.path.join(tmp, "split_%d.txt" % len(lines or rows))
    with open(split, "w") as f:
        f.writelines(rows[j] for j in (lines if lines is not None else range(records)))
    return split


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("prefetch"))
    return {"root": tmp, "split": _write_split(tmp, (32, 64)), "cycled": _write_split(tmp, (32, 64), lines=[j % 6 for j in range(24)])}


def _dataset(files, split="split", **kw):
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset
    return KittiEdgeSplitDataset(files[split], (32, 64), root=files["root"], **kw)


def _same(a, b, skip=()):
    """every key (and their order), shape, dtype and bit"""
    assert list(a) == list(b)
    for k in a:
        if k in skip:
            continue
        if torch.is_tensor(a[k]):
            assert torch.is_tensor(b[k]) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
            assert a[k].dtype == torch.float32
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
        else:
            assert a[k] == b[k], k


def _both(ds, bs=2, seeds=None, **kw):
    """an epoch of SplitLoader and of the prefetching loader over one dataset -> (batches, batches, draws after each loop); with seeds, both
    random streams are seeded before each loop and one random.random() is consumed between batches, as the model's flip draw does"""
    from mindtheedge_amd.datasets.kitti_edges import SplitLoader
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    shuffle, seed = kw.pop("shuffle", False), kw.pop("seed", 0)
    out, tails = [], []
    for loader in (SplitLoader(ds, bs, shuffle=shuffle, seed=seed), PrefetchSplitLoader(ds, bs, shuffle=shuffle, seed=seed, **kw)):
        if seeds is not None:
            random.seed(seeds)
            np.random.seed(seeds)
        got = []
        for batch in loader:
            got.append(batch)
            random.random()
        tails.append((random.random(), float(np.random.rand())))
        out.append(got)
    return out[0], out[1], tails


@pytest.mark.parametrize("shuffle", [False, True])
def test_targets_bit_equal_with_split_loader(files, shuffle):
    ref, new, _ = _both(_dataset(files), shuffle=shuffle, seed=3, num_workers=2)
    assert len(ref) == len(new) == 3
    assert list(ref[0]) == ["idx", "rgb", "depth", "edge", "edge_1", "edge_2", "edge_3", "normal", "normal_1", "normal_2", "normal_3"]
    for a, b in zip(ref, new):
        _same(a, b)
    assert ref[0]["edge_3"].shape == (2, 1, 4, 8) and ref[0]["normal_1"].shape == (2, 1, 16, 32)
    assert all(bool(b[k].any()) for b in new for k in b if k != "idx")
    if shuffle:
        assert [b["idx"] for b in new] != [[0, 1], [2, 3], [4, 5]]


def test_jittering_and_draw_order(files):
    ref, new, tails = _both(_dataset(files, jittering=JITTER), seeds=11, num_workers=4)
    assert "rgb_original" in ref[0] and len(new) == 3
    for a, b in zip(ref, new):
        _same(a, b)
    assert not torch.equal(new[0]["rgb"], new[0]["rgb_original"])
    assert tails[0] == tails[1]                                           # the global draw sequence is the same after the loop


def test_crop_train_borders(files):
    ref, new, _ = _both(_dataset(files, crop_train_borders=(2, 33, 3, 60), jittering=JITTER), seeds=5, num_workers=2)
    for a, b in zip(ref, new):
        _same(a, b)
    plain = _both(_dataset(files), num_workers=1)[1]
    assert not torch.equal(plain[0]["depth"], new[0]["depth"]) and not torch.equal(plain[0]["edge"], new[0]["edge"])


@pytest.mark.parametrize("perturbed", [False, True])
def test_lidar_column(files, perturbed):
    kw = {"lidar_scale": SCALE, "lidar_add": ADD, "lidar_drop_rate": 0.2} if perturbed else {}
    ref, new, tails = _both(_dataset(files, input_depth_type=["velodyne"], **kw), seeds=9, num_workers=2)
    assert list(ref[0])[:5] == ["idx", "rgb", "depth", "lidar", "input_depth"]
    for a, b in zip(ref, new):
        _same(a, b)
    assert torch.equal(new[0]["lidar"], new[0]["input_depth"]) != perturbed and tails[0] == tails[1]


@pytest.mark.parametrize("prefetch", [1, 2])
def test_slot_reuse_over_twelve_batches(files, prefetch):
    ref, new, _ = _both(_dataset(files, "cycled"), num_workers=2, prefetch=prefetch)
    assert len(new) == 12
    for a, b in zip(ref, new):
        _same(a, b)
    _same(new[0], new[3], skip=('idx',))                                                 # the records cycle: batch 3 is batch 0 again, from another slot


def _case_maps():
    from mindtheedge_amd.datasets import batch_prep as bp
    g = np.random.default_rng(2)
    ones = np.ones((12, 20), dtype=np.uint8)
    lost, kept = ones.copy(), ones.copy()
    lost[0, 0] = 200                                                      # (0,0), (0,1), (1,0), (1,1) share target (0,0): the 1 at (1,1) wins
    kept[1, 1] = 200
    u16 = ((g.random((9, 14)) < 0.4) * g.integers(1, 65536, (9, 14))).astype(np.uint16)
    u16[0, :3] = (0, 1, 65535)
    u16[8, 13] = 65535
    return [("binary", bp.EDGE_U8, ((g.random((37, 70)) < 0.3) * 1).astype(np.uint8), (4, 8), False),
            ("bytes", bp.EDGE_U8, ((g.random((37, 70)) < 0.3) * g.integers(1, 256, (37, 70))).astype(np.uint8), (16, 32), True),
            ("large_value_lost", bp.EDGE_U8, lost, (6, 10), False), ("large_value_kept", bp.EDGE_U8, kept, (6, 10), True),
            ("zeros", bp.EDGE_U8, np.zeros((7, 9), dtype=np.uint8), (3, 5), False), ("u16", bp.SPARSE_U16, u16, (5, 6), None),
            ("upscale", bp.EDGE_U8, g.integers(0, 256, (5, 7), dtype=np.uint8), (8, 12), True),
            ("f32", bp.SPARSE_F32, ((g.random((11, 300)) < 0.5) * (g.random((11, 300)) * 80 - 5)).astype(np.float32), (8, 200), None),
            ("normal", bp.NORMAL_U8, g.integers(0, 256, (6, 10), dtype=np.uint8), (6, 10), None),
            ("many_blocks", bp.EDGE_U8, ((g.random((300, 400)) < 0.05) * 255).astype(np.uint8), (270, 301), True)]


def test_reference_behaviour_of_the_collision_case_on_the_cpu():
    """the 12 x 20 -> 6 x 10 case before it is used: the oracle's resize loses the single 200 to a later 1, or keeps it"""
    cases = {name: a for name, _, a, _, _ in _case_maps()}
    lost = do.resize_depth_preserve(cases["large_value_lost"].astype(np.float32), (6, 10))
    kept = do.resize_depth_preserve(cases["large_value_kept"].astype(np.float32), (6, 10))
    assert lost.max() == 1 and lost.min() == 1 and kept.max() == 200 and kept[0, 0] == 200 and (kept == 1).sum() == 59


def test_batched_kernel_decides_per_map():
    """all maps in ONE call; each against the per-map functions"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets import batch_prep as bp
    from mindtheedge_amd.datasets.kitti_edges import normal_target, prepare_edge_sample, resize_depth_preserve
    cases = _case_maps()
    arrays = [a for _, _, a, _, _ in cases]
    rows, cursor = [], 0
    for _, kind, a, (H, W), _ in sorted(cases, key=lambda c: c[1] == bp.NORMAL_U8):      # the normal map last: no winner words
        rows.append((kind, cursor, H, W))
        cursor += -(-H * W // 4) * 4
        if kind != bp.NORMAL_U8:
            winner_elems = cursor
    order = {id(c[2]): r for c, r in zip(sorted(cases, key=lambda c: c[1] == bp.NORMAL_U8), rows)}
    table = [[order[id(a)][0], 0, a.shape[0], a.shape[1], 0, 0, a.shape[0], a.shape[1], order[id(a)][1], order[id(a)][2], order[id(a)][3], 0] for a in arrays]
    host = bp.HostArena()
    host.reserve(bp.arena_layout(arrays, len(arrays))[2])
    t_off, offs, total, live = bp.pack_arena(host, arrays, table)
    dev = host.tensor.cuda()
    results = []
    for fill in (0x00, 0x7f):                                             # nothing relies on a cleared output or workspace
        out = torch.full((cursor,), fill, dtype=torch.uint8, device="cuda").repeat_interleave(4).view(torch.float32)
        work = torch.full((winner_elems + len(arrays),), fill, dtype=torch.uint8, device="cuda").repeat_interleave(4).view(torch.int32)
        K.lib.mte_batch_prep(dev.data_ptr(), total, host.tensor.data_ptr() + t_off, dev.data_ptr() + t_off, len(arrays), out.data_ptr(), cursor,
                             work.data_ptr(), winner_elems, K._stream())
        results.append(out.cpu())
    for (name, kind, a, (H, W), divided) in cases:
        off = order[id(a)][1]
        got = results[0][off:off + H * W].view(H, W)
        src = torch.from_numpy(a).cuda()
        if kind == bp.EDGE_U8:
            want = prepare_edge_sample([src], [], (H, W))["edge"][0]
            resized = resize_depth_preserve(src.float(), (H, W))
            assert bool(resized.max() > 1) == divided, name
            assert torch.equal(want, resized / 255.0 if divided else resized), name
            np.testing.assert_array_equal(resized.cpu().numpy(), do.resize_depth_preserve(a.astype(np.float32), (H, W)).astype(np.float32))
        elif kind == bp.SPARSE_U16:
            as_read = a.astype(np.float32) / 256.
            as_read[a == 0] = -1.
            want = resize_depth_preserve(torch.from_numpy(as_read).cuda(), (H, W))
            assert float(want.max()) == 65535 / 256 and float(want[want > 0].min()) > 0
        elif kind == bp.SPARSE_F32:
            want = resize_depth_preserve(src, (H, W))
            assert bool((src < 0).any()) and bool((want >= 0).all())
        else:
            want = normal_target(src)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got.view(torch.int32), want.cpu().view(torch.int32)), name
        assert torch.equal(results[1][off:off + H * W].view(torch.int32), got.reshape(-1).view(torch.int32)), name      # (the gaps between maps are not written)
    # the entry point checks the table before it launches anything
    normal_row = [i for i, c in enumerate(cases) if c[1] == bp.NORMAL_U8][0]
    for r, col, bad in ((0, 0, 4), (0, 1, total), (1, 1, -16), (0, 4, 1), (0, 6, 0), (0, 8, cursor), (0, 9, 1 << 31), (5, 1, offs[5] + 1),
                        (normal_row, 9, 5)):                              # (.., a normal map is never resized)
        broken = bp.HostArena()
        broken.reserve(total)
        bp.pack_arena(broken, arrays, table)
        rows_view = broken.view[t_off:t_off + len(arrays) * bp.ROW_WORDS * 8].view(np.int64).reshape(len(arrays), bp.ROW_WORDS)
        rows_view[r, col] = bad
        with pytest.raises(K.MteError):
            K.lib.mte_batch_prep(dev.data_ptr(), total, broken.tensor.data_ptr() + t_off, dev.data_ptr() + t_off, len(arrays), out.data_ptr(), cursor,
                                 work.data_ptr(), winner_elems, K._stream())
    torch.cuda.synchronize()


def test_no_host_read_in_steady_state(files):
    """torch's synchronisation debug mode (live on this runtime: the self-check below) around three next() calls after two warm-up batches"""
    from mindtheedge_amd.datasets.kitti_edges import prepare_edge_sample
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    edge = torch.from_numpy(((np.random.default_rng(0).random((32, 64)) < 0.2) * 255).astype(np.uint8)).cuda()
    loader = PrefetchSplitLoader(_dataset(files, "cycled"), 2, shuffle=False, num_workers=2, prefetch=2)
    it = iter(loader)
    got = [next(it), next(it)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            prepare_edge_sample([edge], [], (32, 64))                     # the per-sample path reads the maximum on the host: the guard is live
        for _ in range(3):
            got.append(next(it))
    finally:
        torch.cuda.set_sync_debug_mode("default")
        loader.close()
    _same(got[0], got[3], skip=('idx',))                                                 # and what was queued under the guard is the usual batch
    _same(got[1], got[4], skip=('idx',))


def test_one_training_step_on_a_batch_of_each_loader(tmp_path):
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, SplitLoader
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    H, W = 64, 128
    split = _write_split(str(tmp_path), (H, W), records=2)
    ds = KittiEdgeSplitDataset(split, (H, W), root=str(tmp_path))
    (a,), (b,) = list(SplitLoader(ds, 2, shuffle=False)), list(PrefetchSplitLoader(ds, 2, shuffle=False, num_workers=2))
    _same(a, b)
    K.set_compute_dtype("fp32")
    try:
        torch.manual_seed(42)
        net = PackNetSAN01(dropout=None, version="1A")
        model = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog",
                                 supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.0)
        model.add_depth_net(net.cuda())
        model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
        model.train()
        losses = []
        for batch in (a, b):
            model.zero_grad()
            out = model(dict(batch))
            out["loss"].sum().backward()
            losses.append(out["loss"].detach().float().cpu())
        assert torch.isfinite(losses[0]).all() and float(losses[0].abs().sum()) > 0
        assert torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32))
    finally:
        K.set_compute_dtype("bf16")
