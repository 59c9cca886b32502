"""GPU (-m gpu): csrc/depth_viz.hip and the layers above it against tests/viz_ref.py (itself held against the reference's recorded
outputs on the CPU, test_viz_ref_cpu.py): order statistics exactly equal to np.sort picks, viz_inv_depth and the log colouring as uint8
images, the D3R count as an integer, save_depth through ModelWrapper.test_step and infer_edges.py --split."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viz_ref                                               # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "viz.npz"))
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 24 * 80, 96 * 320]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def picks(values, ks, positive_only=False):
    from mindtheedge_amd.utils.depth import order_stats
    out, cnt = order_stats(dev(values), ks, positive_only)
    return out.cpu().numpy(), cnt.cpu().numpy()


def check_picks(values, ks, positive_only=False):
    got, cnt = picks(values, ks, positive_only)
    for row, c, k in zip(got, cnt, ks):
        a, b, n = viz_ref.sort_pick(values, k, positive_only)
        assert c == n and row[0] == a and row[1] == b, (len(values), k, row, (a, b), c, n)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_order_stats_equal_sort_picks(n):
    from mindtheedge_amd.utils.depth import percentile_position
    rs = np.random.RandomState(n)
    ks = [0, n - 2, percentile_position(n, 95)[0]]             # n = 1: rank -1 is clamped to 0, rank n is clamped to n - 1
    check_picks((rs.rand(n) * 3).astype(np.float32), ks)
    check_picks(rs.randn(n).astype(np.float32) * np.float32(40), ks + [n - 1, n // 2])
    mixed = rs.randn(n).astype(np.float32)
    mixed[rs.rand(n) < 0.3] = 0
    mixed[rs.rand(n) < 0.1] = -0.0
    npos = int((mixed > 0).sum())
    check_picks(mixed, [0, npos - 2, max(npos - 1, 0) * 95 // 100, npos], positive_only=True)
    check_picks(mixed, ks)


@pytest.mark.parametrize("n", [65, 4097])
def test_order_stats_degenerate_inputs(n):
    rs = np.random.RandomState(5)
    ks = [0, 1, n // 2, n - 2, n - 1]
    check_picks(np.full(n, 0.37, dtype=np.float32), ks)
    check_picks(np.where(rs.rand(n) < 0.5, np.float32(0.25), np.float32(7.5)).astype(np.float32), ks)
    # ties that share the upper digits of the key: a handful of neighbouring floats, each many times
    base = np.float32(1.2345678)
    near = np.array([np.nextafter(base, np.float32(2), dtype=np.float32)] * 3 + [base] * 2 + [np.float32(base + 3e-7 * i) for i in range(8)], dtype=np.float32)
    check_picks(near[rs.randint(len(near), size=n)], ks)
    check_picks(np.zeros(n, dtype=np.float32), [0, n - 1], positive_only=True)     # nothing takes part: (0, 0), count 0


def test_order_stats_batch_of_three_and_repeatable():
    from mindtheedge_amd.utils.depth import order_stats
    rs = np.random.RandomState(9)
    x = rs.randn(3, 24 * 80).astype(np.float32)
    x[0, rs.rand(1920) < 0.9] = 0
    x[1, rs.rand(1920) < 0.2] = -1
    x[2] = np.abs(x[2]) + 1
    counts = [(r > 0).sum() for r in x]
    ks = [int((c - 1) * 0.95) for c in counts]
    assert len(set(counts)) == 3
    xd = dev(x)
    out, cnt = order_stats(xd, ks, True)
    again, cnt2 = order_stats(xd, ks, True)
    assert torch.equal(out, again) and torch.equal(cnt, cnt2)
    for b in range(3):
        a, c, n = viz_ref.sort_pick(x[b], ks[b], True)
        assert (out[b, 0].item(), out[b, 1].item(), cnt[b].item()) == (a, c, n)
    plain, _ = order_stats(xd.reshape(3, 24, 80), 100)
    for b in range(3):
        assert tuple(plain[b].tolist()) == viz_ref.sort_pick(x[b], 100)[:2]


def test_percentile_equals_np_percentile():
    from mindtheedge_amd.utils.depth import percentile_f32
    rs = np.random.RandomState(11)
    for shape, q in (((24, 80), 95), ((5, 7), 95), ((96, 320), 95), ((24, 80), 50), ((1, 1), 95), ((24, 80), 100), ((24, 80), 0)):
        a = (rs.rand(*shape) * 0.3).astype(np.float32)
        a[rs.rand(*shape) < 0.2] = 0
        a[0, 0] = 0.2
        assert percentile_f32(dev(a), q).tobytes() == np.percentile(a, q).tobytes()
        assert percentile_f32(dev(a), q, positive_only=True).tobytes() == np.percentile(a[a > 0], q).tobytes()


def viz_input(shape, d, seed):
    rs = np.random.RandomState(seed)
    x = (rs.rand(*shape) * 1.2 * d).astype(np.float32)
    flat = x.reshape(-1)
    special = [np.float32(-0.1), np.float32(0), np.float32(d), np.float32(2 * d), np.float32(np.float32(0.999999) * d)]
    special += [np.float32(np.float32(k) / np.float32(256) * d) for k in (1, 2, 3, 127, 128, 129, 254, 255, 256)]
    flat[:len(special)] = special
    flat[rs.rand(flat.size) < 0.1] = 0
    flat[len(special):len(special) + 3] = [0, -1, 0]
    return x


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 24, 80)])
@pytest.mark.parametrize("colormap", ["plasma", "Spectral"])
def test_viz_inv_depth_equals_the_statement(shape, colormap):
    from mindtheedge_amd.utils.depth import color_table, colormap_u8, viz_divisor, viz_inv_depth
    x = viz_input(shape, np.float32(0.3 + 1e-6), shape[1])
    for b in range(shape[0]):
        for kw in ({}, {"normalizer": 0.3}, {"filter_zeros": True}, {"percentile": 50}):
            got = viz_inv_depth(dev(x[b:b + 1]), colormap=colormap, **kw)
            ref_kw = {("q" if k == "percentile" else k): v for k, v in kw.items()}
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == shape[1:] + (3,)
            assert np.array_equal(got.cpu().numpy(), viz_ref.viz_inv_depth(x[b], colormap=colormap, **ref_kw)), (b, kw)
    assert np.array_equal(viz_inv_depth(dev(x[0])).cpu().numpy(), viz_ref.viz_inv_depth(x[0]))             # [H,W] as well as [1,H,W]
    # the whole batch in one launch, a divisor per image
    norms = [0.3, 0.11][:shape[0]]
    d = dev(np.array([viz_divisor(v) for v in norms], dtype=np.float32))
    got = colormap_u8(dev(x), color_table(colormap, "rint", "cuda"), divisor=d).cpu().numpy()
    for b, v in enumerate(norms):
        assert np.array_equal(got[b], viz_ref.viz_inv_depth(x[b], normalizer=v, colormap=colormap))


def test_viz_inv_depth_equals_the_recorded_reference():
    from mindtheedge_amd.utils.depth import viz_inv_depth
    for frame in ("a", "b"):
        for case, kw in (("default", {}), ("norm", {"normalizer": 0.3}), ("fz", {"filter_zeros": True}), ("spectral", {"colormap": "Spectral"})):
            want = np.clip(np.rint(Z["viz_%s_%s" % (frame, case)] * 255), 0, 255).astype(np.uint8)
            assert np.array_equal(viz_inv_depth(dev(Z["viz_%s_inv" % frame]).unsqueeze(0), **kw).cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(24, 80), (17, 31)])
def test_log_colouring_outside_the_guard_band(shape):
    """The kernel takes log(v) in double and rounds it to float32 once, as the statement does; numpy's own float32 log -- the reference --
    and a device log may each be off by one unit in the last place of log(v).  With L the float32 log, x = (L - lo) / hi: an error of one ulp
    in L, plus half an ulp of the difference and half an ulp of the quotient (both no larger than an ulp of the largest |L| of the frame once
    scaled back), is at most three ulps of L at the largest |log v| of the frame; in units of the index x * 256 that is
        band = 3 * ulp_f32(max |log v|) * 256 / hi.
    A pixel whose float64 value of x * 256 lies at least the band away from every integer must have exactly the statement's colour; inside the
    band the index may differ by one.  Depths are log-uniform in [1, 80]: band ~ 3 * 4.8e-7 * 256 / 4.4 ~ 8e-5, so about 0.02 % of the pixels
    (and the minimum and the maximum, which sit on 0 and 256 by construction) fall inside; at most 1 % may."""
    from mindtheedge_amd.utils.depth import depth_log_color
    rs = np.random.RandomState(shape[0])
    depth = np.exp(rs.rand(*shape) * np.log(80.0)).astype(np.float32)
    want, exact, idx = viz_ref.log_color(depth)
    logs = np.log(depth.astype(np.float64))
    band = 3 * float(np.spacing(np.float32(np.abs(logs).max()))) * 256 / (logs.max() - logs.min())
    near = np.abs(exact - np.rint(exact)) < band
    print("band", band, "inside", int(near.sum()), "of", near.size)
    assert band < 2e-4 and near.mean() <= 0.01
    got = depth_log_color(dev(depth))
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,)
    got = got.cpu().numpy()
    assert np.array_equal(got[~near], want[~near])
    assert viz_ref.within_one_index(got, idx, viz_ref.table("Spectral", "trunc"))[near].all()
    assert np.array_equal(depth_log_color(dev(depth)).cpu().numpy(), got)                         # run to run


def test_log_colouring_equals_the_recorded_reference_outside_the_band():
    from mindtheedge_amd.utils.depth import depth_log_color
    depth = Z["log_a_depth"]
    _, exact, idx = viz_ref.log_color(depth)
    logs = np.log(depth.astype(np.float64))
    near = np.abs(exact - np.rint(exact)) < 3 * float(np.spacing(np.float32(np.abs(logs).max()))) * 256 / (logs.max() - logs.min())
    got = depth_log_color(dev(depth)).cpu().numpy()
    assert near.mean() <= 0.01 and np.array_equal(got[~near], Z["log_a_color"][~near])


def test_d3r_count_fixture_and_random_pairs():
    from mindtheedge_amd.utils.depth_analysis import d3r_count
    gt, pred = dev(Z["d3r_gt"]).float(), dev(Z["d3r_pred"])
    assert d3r_count(gt, pred, Z["d3r_pairs"]) == int(Z["d3r_agree"].sum())
    rs = np.random.RandomState(4)
    g = ((rs.rand(24, 80) < 0.7) * rs.randint(1, 256, size=(24, 80))).astype(np.uint8)
    p = (g * (1 + 0.05 * rs.randn(24, 80)) + rs.rand(24, 80)).astype(np.float32)
    p[3, 5] = 0                                                                               # a zero prediction: inf / nan ratios agree with nothing
    n = int((g > 0).sum())
    for P in (1, 100, 2500):
        pairs = rs.randint(0, n, size=(P, 2))
        want = viz_ref.d3r_count(g, p, pairs)
        assert d3r_count(dev(g).float(), dev(p), pairs) == want
        assert d3r_count(dev(g).float(), dev(p), pairs) == want
    assert 0 < want < 2500
    with pytest.raises(ValueError):
        d3r_count(dev(g).float(), dev(p), [[0, n]])


@pytest.mark.parametrize("valid,pairs", [(12000, 5000), (6000, 2500), (3000, 1000), (1500, 500), (300, 100)])
def test_ordinal_error_takes_each_rung_of_the_ladder(valid, pairs):
    from mindtheedge_amd.utils.depth_analysis import frame_ord_error
    rs = np.random.RandomState(valid)
    shape = (96, 320)
    g = np.zeros(shape[0] * shape[1], dtype=np.uint8)
    g[rs.permutation(g.size)[:valid]] = rs.randint(1, 256, size=valid)
    g = g.reshape(shape)
    p = (g * (1 + 0.1 * rs.randn(*shape)) + 1 + rs.rand(*shape)).astype(np.float32)
    np.random.seed(21)
    got = frame_ord_error(g, p)
    np.random.seed(21)
    perm = np.random.permutation(valid)[:2 * pairs].reshape(pairs, 2)
    assert got == 1 - viz_ref.d3r_count(g, p, perm) / pairs and 0 < got < 1


def test_ordinal_error_refuses_fewer_than_200_valid_pixels():
    from mindtheedge_amd.utils.depth_analysis import frame_ord_error
    g = np.zeros((24, 80), dtype=np.uint8)
    g.reshape(-1)[:199] = 9
    with pytest.raises(ValueError):
        frame_ord_error(g, np.ones((24, 80), dtype=np.float32))


def test_run_ord_metrics_equals_the_recorded_reference(tmp_path):
    from PIL import Image
    from mindtheedge_amd.utils.depth_analysis import run_ord_metrics
    gts, preds = [], []
    for i in range(2):
        gts.append(os.path.join(tmp_path, "gt_%d.png" % i))
        preds.append(os.path.join(tmp_path, "pred_%d.npy" % i))
        Image.fromarray(Z["ord_gt_%d" % i]).save(gts[-1])
        np.save(preds[-1], Z["ord_pred_%d" % i])
    for name, paths in (("gt.txt", gts), ("pred.txt", preds)):
        with open(os.path.join(tmp_path, name), "w") as f:
            f.write("".join(p + "\n" for p in paths))
    np.random.seed(int(Z["ord_seed"]))
    got = run_ord_metrics(os.path.join(tmp_path, "gt.txt"), os.path.join(tmp_path, "pred.txt"))
    assert got.dtype == np.float64 and np.array_equal(got, Z["ord_error"])
    np.random.seed(int(Z["ord_seed"]))
    assert np.array_equal(run_ord_metrics(gts, preds), Z["ord_error"])


# ---- save_depth through test_step

def _wrapper(overrides, seed=3):
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    K.set_compute_dtype("bf16")
    cfg = load_config(None, overrides)
    torch.manual_seed(seed)
    return ModelWrapper(cfg).cuda().eval()


def test_save_depth_through_test_step(tmp_path):
    from PIL import Image
    from mindtheedge_amd.utils.depth import inv2depth
    folder = os.path.join(tmp_path, "out")
    test = {"path": ["/data/KITTI_tiny"], "split": ["splits/test_files.txt"], "depth_type": ["groundtruth"], "cameras": [[]]}
    base = {"model": {"loss": {"supervised_loss_weight": 1.0}}, "datasets": {"augmentation": {"image_shape": (64, 96)}, "test": test}}
    saving = _wrapper({**base, "save": {"folder": folder, "pretrained": "/ckpt/run7/epoch=3.ckpt"}})
    silent = _wrapper(base)
    rs = np.random.RandomState(6)
    rgb = dev(rs.rand(1, 3, 64, 96).astype(np.float32))
    depth = dev(((rs.rand(1, 1, 64, 96) < 0.4) * (1 + 60 * rs.rand(1, 1, 64, 96))).astype(np.float32))
    batch = {"idx": [0], "filename": ["test_files_0000000000"], "rgb": rgb, "depth": depth}
    out = saving.test_step(dict(batch), 0, 0)
    inv_pp = saving.evaluate_depth(dict(batch), (0, 0))["inv_depth"]
    where = os.path.join(folder, "depth", "KITTI_tiny-test_files-groundtruth", "epoch=3")
    stem = os.path.join(where, "test_files_0000000000")
    assert sorted(os.listdir(where)) == [os.path.basename(stem) + s for s in ("_depth.npz", "_depth.png", "_rgb.png", "_viz.png")]
    d = inv2depth(inv_pp[0]).squeeze().cpu()
    with np.load(stem + "_depth.npz", allow_pickle=True) as z:
        assert np.array_equal(z["depth"], d.numpy())
    assert np.array_equal(np.array(Image.open(stem + "_depth.png")), (d * 256).int().numpy())
    assert np.array_equal(np.array(Image.open(stem + "_viz.png")), viz_ref.viz_inv_depth(inv_pp[0, 0].float().cpu().numpy()))
    assert np.array_equal(np.array(Image.open(stem + "_rgb.png")),
                          np.rint(rgb[0].permute(1, 2, 0).cpu().numpy() * np.float32(255)).astype(np.uint8))
    # folder '': nothing is written and the metrics are those of a wrapper without the key
    before = sorted(os.listdir(tmp_path))
    quiet = silent.test_step(dict(batch), 0, 0)
    assert sorted(os.listdir(tmp_path)) == before
    assert set(quiet) == set(out)
    for k in out:
        if torch.is_tensor(out[k]):
            assert torch.equal(out[k], quiet[k]), k


def test_test_loader_samples_are_named_and_saved_under_their_names(tmp_path):
    import eval_prep_ref as R
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, make_test_loaders
    folder = os.path.join(str(tmp_path), "KITTI_tiny")
    split = R.write_split(folder, n=2)
    out = os.path.join(tmp_path, "saved")
    section = {"dataset": ["KITTI"], "path": [folder], "split": [split], "depth_type": ["groundtruth"]}
    wrap = _wrapper({"model": {"loss": {"supervised_loss_weight": 1.0}}, "datasets": {"augmentation": {"image_shape": (64, 128)}, "test": section},
                     "save": {"folder": out, "depth": {"npz": False, "png": False}}})
    stem = os.path.splitext(os.path.basename(split))[0]
    (loader,) = make_test_loaders(wrap.config, 0, 1)
    for i, batch in enumerate(loader):
        assert batch["filename"] == ["%s_%010d" % (stem, i)]
        wrap.test_step(batch, i, 0)
    where = os.path.join(out, "depth", "KITTI_tiny-%s-groundtruth" % stem, "")
    assert sorted(os.listdir(where)) == sorted("%s_%010d_%s.png" % (stem, i, kind) for i in range(2) for kind in ("rgb", "viz"))
    assert "filename" not in KittiEdgeSplitDataset(split, (64, 128), root=folder, mode="test")[0]      # only when asked for


# ---- infer_edges.py --split

def _split_inputs(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(8)
    lines = []
    for i in range(2):
        img, lidar = os.path.join(tmp_path, "img_%d.png" % i), os.path.join(tmp_path, "lidar_%d.png" % i)
        Image.fromarray(rs.randint(0, 256, size=(64, 96, 3)).astype(np.uint8)).save(img)
        Image.fromarray(((rs.rand(64, 96) < 0.2) * rs.randint(300, 20000, size=(64, 96))).astype(np.uint16)).save(lidar)
        lines.append("%s d e %s n re\n" % (img, lidar))
    split = os.path.join(tmp_path, "test_files.txt")
    with open(split, "w") as f:
        f.write("".join(lines))
    return split


def _split_yaml(tmp_path, name, split, folder, with_san, input_depth_type):
    from test_gpu_entry_points import _yaml
    with open(_yaml(tmp_path, 64, 96)) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["depth_net"]["with_san"] = with_san
    cfg["datasets"]["test"] = {"dataset": ["KITTI"], "path": [str(tmp_path)], "split": [split], "input_depth_type": [input_depth_type]}
    cfg["save"] = {"folder": folder}
    path = os.path.join(tmp_path, name)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def _read_lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_infer_edges_split_mode(tmp_path):
    from test_gpu_entry_points import _run_main
    split = _split_inputs(tmp_path)
    rgb_dir, both_dir, plain_dir = (os.path.join(tmp_path, d) for d in ("rgb_only", "both", "plain"))
    _run_main("infer_edges", ["infer_edges.py", "--config", _split_yaml(tmp_path, "a.yaml", split, rgb_dir, False, ""), "--split"])
    names = ["%08d_regular%s" % (i, s) for i in range(2) for s in (".npy", ".png", "_color.png")]
    assert sorted(os.listdir(rgb_dir)) == sorted(names + ["input_list.txt", "pred_list.txt", "pred_lidar_list.txt"])
    assert _read_lines(os.path.join(rgb_dir, "pred_lidar_list.txt")) == []
    assert _read_lines(os.path.join(rgb_dir, "pred_list.txt")) == [os.path.join(rgb_dir, "%08d_regular.npy" % i) for i in range(2)]
    assert _read_lines(os.path.join(rgb_dir, "input_list.txt")) == [os.path.join(tmp_path, "img_%d.png" % i) for i in range(2)]
    from PIL import Image
    color = np.array(Image.open(os.path.join(rgb_dir, "00000001_regular_color.png")))
    depth = np.load(os.path.join(rgb_dir, "00000001_regular.npy"))
    want, exact, idx = viz_ref.log_color(depth)
    assert color.shape == (64, 96, 3) and (color == want).all(axis=-1).mean() >= 0.99
    assert viz_ref.within_one_index(color, idx, viz_ref.table("Spectral", "trunc")).all()
    # the --input path on the same frame
    cfg_plain = _split_yaml(tmp_path, "p.yaml", split, "", False, "")
    _run_main("infer_edges", ["infer_edges.py", "--config", cfg_plain, "--input", os.path.join(tmp_path, "img_0.png"), "--output", plain_dir])
    assert sorted(os.listdir(plain_dir)) == ["00000000_regular.npy", "00000000_regular.png"]
    assert np.array_equal(np.load(os.path.join(plain_dir, "00000000_regular.npy")), np.load(os.path.join(rgb_dir, "00000000_regular.npy")))
    # with the sparse branch and a LiDAR type: the second pass is written too
    _run_main("infer_edges", ["infer_edges.py", "--config", _split_yaml(tmp_path, "b.yaml", split, both_dir, True, "png"), "--split"])
    lidar_names = ["%08d_lidar%s" % (i, s) for i in range(2) for s in (".npy", ".png", "_color.png")]
    assert sorted(os.listdir(both_dir)) == sorted(names + lidar_names + ["input_list.txt", "pred_list.txt", "pred_lidar_list.txt"])
    assert _read_lines(os.path.join(both_dir, "pred_lidar_list.txt")) == [os.path.join(both_dir, "%08d_lidar.npy" % i) for i in range(2)]
    for i in range(2):
        reg, lid = (np.load(os.path.join(both_dir, "%08d_%s.npy" % (i, t))) for t in ("regular", "lidar"))
        assert reg.shape == lid.shape == (64, 96) and np.isfinite(lid).all() and not np.array_equal(reg, lid)
        assert not np.array_equal(np.array(Image.open(os.path.join(both_dir, "%08d_regular_color.png" % i))),
                                  np.array(Image.open(os.path.join(both_dir, "%08d_lidar_color.png" % i))))
