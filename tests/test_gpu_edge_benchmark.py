"""GPU (-m gpu): the edge benchmark on the device -- the matcher (mte_edge_match) against the exact solver of
tests/edge_benchmark_ref.py (counts compared with ==, every returned partner map checked), the fixed-scale Canny against
oracle/canny_oracle.py, the per-frame depth metrics against the golden values of the reference's own code, and the pipeline
end to end.  PARITY UNPINNED against py-bsds500 and OpenCV (neither is available): see DESIGN.md."""
import os

import numpy as np
import pytest
import torch

import edge_benchmark_ref as ebr
from conftest import GOLDEN
from oracle import canny_oracle as co
from test_edge_benchmark_cpu import FRAME_CASES, RANDOM_GRID, golden_npz, random_48x64, tiny_pairs

pytestmark = pytest.mark.gpu


def _match(pred, gt, r2, gt_of=None, init_mate=None):
    """numpy in -> (result [B,4], mates [B,H,W]) numpy"""
    from mindtheedge_amd.utils.edge_benchmark import edge_match
    im = None if init_mate is None else torch.from_numpy(np.ascontiguousarray(init_mate, dtype=np.int32)).cuda()
    res, mates = edge_match(torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).cuda(), r2, gt_of=gt_of, init_mate=im,
                            return_mates=True)
    return res.cpu().numpy(), mates.cpu().numpy()


def _check(pred, gt, r2, res, mates, want):
    assert res[3] == 0
    assert res[1] == (pred > 127.5).sum() and res[2] == (gt > 127.5).sum()
    assert res[0] == want
    ebr.check_mates(pred, gt, r2, mates, res[0])


@pytest.mark.parametrize("r2", [1, 2])
def test_tiny_maps_in_one_call(r2):
    pred, gt = tiny_pairs()
    perm = np.random.default_rng(r2).permutation(len(gt))           # gt is stored shuffled: gt_of leads each instance to its own
    stored = np.empty_like(gt)
    stored[perm] = gt
    res, mates = _match(pred, stored, r2, gt_of=perm.astype(np.int32))
    for b in range(len(pred)):
        _check(pred[b], gt[b], r2, res[b], mates[b], ebr.max_matching_size(pred[b], gt[b], r2))


@pytest.mark.parametrize("density,r2", RANDOM_GRID)
def test_random_48x64(density, r2):
    pred, gt = random_48x64(density, r2)
    res, mates = _match(pred, gt, r2)
    _check(pred[0], gt[0], r2, res[0], mates[0], ebr.max_matching_size(pred[0], gt[0], r2))


def _chain(n, H, W, row, sym=0):
    """ground truth at x = 0, 2, .., 2n-2 and predictions at x = 1, 3, .., 2n-1 of one row; every prediction starts paired with its
    RIGHT neighbour, which leaves the last prediction and the first annotation free: one augmenting path of 2n-1 edges.
    sym: one of the eight flips / transposes."""
    def tf(y, x):
        if sym & 1:
            y = H - 1 - y
        if sym & 2:
            x = W - 1 - x
        return (x, y) if sym & 4 else (y, x)
    h, w = (W, H) if sym & 4 else (H, W)
    pred, gt, init = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), -np.ones((h, w), np.int32)
    for k in range(n):
        gy, gx = tf(row, 2 * k)
        py, px = tf(row, 2 * k + 1)
        gt[gy, gx] = 255.0
        pred[py, px] = 255.0
        if k < n - 1:
            my, mx = tf(row, 2 * k + 2)
            init[py, px] = my * w + mx
    return pred, gt, init


@pytest.mark.parametrize("sym", range(8))
def test_long_augmenting_path_all_symmetries(sym):
    pred, gt, init = _chain(40, 5, 81, 2, sym)
    res, mates = _match(pred[None], gt[None], 1, init_mate=init[None])
    _check(pred, gt, 1, res[0], mates[0], 40)
    res, mates = _match(pred[None], gt[None], 1)                    # and from the kernel's own initialisation
    _check(pred, gt, 1, res[0], mates[0], 40)


def test_long_augmenting_path_600():
    pred, gt, init = _chain(600, 3, 1201, 1)
    res, mates = _match(pred[None], gt[None], 1, init_mate=init[None])
    _check(pred, gt, 1, res[0], mates[0], 600)


def test_invalid_init_mate_is_reported_not_trusted():
    pred, gt, init = _chain(40, 5, 81, 2)
    W = 81
    p0 = 2 * W + 1                                                  # the first prediction, (2, 1)
    bad = []
    for value in (5 * W + 7, -7, 1 << 29):                          # partner outside the image
        b = init.copy(); b.reshape(-1)[p0] = value; bad.append(b)
    b = init.copy(); b.reshape(-1)[p0] = 2 * W + 4; bad.append(b)   # the partner of the NEXT prediction: claimed twice
    b = init.copy(); b.reshape(-1)[p0] = 2 * W + 1; bad.append(b)   # not a ground-truth pixel
    b = init.copy(); b.reshape(-1)[p0] = 2 * W + 0; bad.append(b)   # fine (left neighbour, free) -- the control
    b = init.copy(); b.reshape(-1)[p0] = 2 * W + 6; b.reshape(-1)[p0 + 4] = -1; bad.append(b)   # a free annotation, but outside r2
    b = init.copy(); b.reshape(-1)[0] = 2 * W + 0; bad.append(b)    # an entry on a pixel that is no predicted edge
    init_all = np.stack(bad)
    n = len(bad)
    res, mates = _match(np.repeat(pred[None], n, 0), gt[None], 1, gt_of=np.zeros(n, np.int32), init_mate=init_all)
    for i in range(n):
        if i == 5:
            _check(pred, gt, 1, res[i], mates[i], 40)
        else:
            assert res[i, 3] != 0 and res[i, 0] == 0 and np.all(mates[i] == -1), i


def test_degenerate_cases():
    from mindtheedge_amd._lib import MteError
    g = np.random.default_rng(5)
    H, W = 9, 13
    some = (g.random((H, W)) < 0.3).astype(np.float32) * 255.0
    zero = np.zeros((H, W), np.float32)
    for pred, gt in ((zero, some), (some, zero), (zero, zero)):
        res, mates = _match(pred[None], gt[None], 5)
        _check(pred, gt, 5, res[0], mates[0], 0)
    # one predicted pixel in each corner; annotations only where a matcher without bounds checks would look (wrapped rows)
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        pred, gt = zero.copy(), zero.copy()
        pred[y, x] = 255.0
        gt[(y + 1) % H if x == W - 1 else (y - 1) % H, W - 1 - x] = 255.0     # the linear neighbour across the row end
        gt[H - 1 - y, x] = 255.0                                              # the opposite row
        res, mates = _match(pred[None], gt[None], 2)
        _check(pred, gt, 2, res[0], mates[0], ebr.max_matching_size(pred, gt, 2))
        assert res[0, 0] == 0
    pred, gt = ebr.random_maps(1, 20, 24, 0.3, seed=9)
    res, mates = _match(pred, gt, 0)                                          # r2 = 0: the intersection
    _check(pred[0], gt[0], 0, res[0], mates[0], int(((pred[0] > 0) & (gt[0] > 0)).sum()))
    pred, gt = ebr.random_maps(1, 20, 24, 0.1, seed=10)
    res, mates = _match(pred, gt, 64)                                         # r2 at the limit
    _check(pred[0], gt[0], 64, res[0], mates[0], ebr.max_matching_size(pred[0], gt[0], 64))
    with pytest.raises(MteError, match="UNSUPPORTED"):
        _match(pred, gt, 65)
    res, _ = _match(pred, gt, 1, gt_of=np.array([3], np.int32))               # gt_of outside [0, Bg)
    assert res[0, 3] != 0


def _annotation(name="kitti_de_000114_10.png"):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name)), dtype=np.uint8).astype(np.float32) * 255.0


def test_benchmark_shape_twelve_predictions_share_one_annotation():
    gt = np.ascontiguousarray(_annotation()[153:371, 44:1197])
    assert gt.shape == (218, 1153)
    r2 = ebr.radius2(gt.shape, 0.002)
    assert r2 == 5
    preds = []
    for seed in range(12):
        g = np.random.default_rng(seed)
        p = np.zeros(gt.shape, bool)
        p[1:, 2:] = gt[:-1, :-2] > 0
        p &= g.random(gt.shape) >= 0.10
        p |= g.random(gt.shape) < 0.01
        preds.append(p.astype(np.float32) * 255.0)
    preds = np.stack(preds)
    res, mates = _match(preds, gt[None], r2, gt_of=np.zeros(12, np.int32))
    for b in range(12):
        _check(preds[b], gt, r2, res[b], mates[b], ebr.max_matching_size(preds[b], gt, r2))
    from mindtheedge_amd.utils.edge_benchmark import correspond_pixels_count
    got = correspond_pixels_count(torch.from_numpy(preds).cuda(), torch.from_numpy(gt).cuda(), max_dist=0.002, gt_of=[0] * 12)
    assert np.array_equal(got, res[:, :3])


@pytest.mark.parametrize("case", FRAME_CASES)
def test_frame_metrics_golden(case):
    from mindtheedge_amd.utils.depth_analysis import frame_depth_metrics
    z = golden_npz()
    lo, hi = z[case + "_limits"]
    mask = torch.from_numpy(z[case + "_mask"]).cuda() if case + "_mask" in z.files else None
    r = frame_depth_metrics(torch.from_numpy(z[case + "_gt"]).cuda(), torch.from_numpy(z[case + "_pred"]).cuda(), lo, hi,
                            gt_crop=z[case + "_crop"].tolist(), mask=mask)
    want = z[case + "_vals"]
    got = np.array([r["mean_rel_err"], r["std_rel_err"], r["abs_rel_err"], r["accuracy_1p1"], r["accuracy_1p25"]])
    print(case, got, want)
    assert [r["valid"], r["count_1p1"], r["count_1p25"]] == z[case + "_counts"].tolist()
    if case == "frame_empty":
        assert np.isnan(got).all()
    else:
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


def test_frame_metrics_full_size_against_numpy():
    from mindtheedge_amd.utils.depth_analysis import frame_depth_metrics
    g = np.random.default_rng(11)
    H, W = 384, 1280
    gt = np.floor(g.random((2, H, W)) * 90 * 256) / 256.0
    gt[g.random((2, H, W)) < 0.7] = 0.0
    pred = (gt * (1 + 0.2 * g.standard_normal((2, H, W))) + g.random((2, H, W)) + 0.5).astype(np.float32)
    crop = [44, 1197, 153, 371]
    r = frame_depth_metrics(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), 0.0, 80.0, gt_crop=crop)
    for b in range(2):
        w = ebr.frame_depth_metrics(gt[b], pred[b], 0.0, 80.0, gt_crop=crop)
        assert [r[k][b] for k in ("valid", "count_1p1", "count_1p25")] == [w[k] for k in ("valid", "count_1p1", "count_1p25")]
        for k in ("mean_rel_err", "std_rel_err", "abs_rel_err", "accuracy_1p1", "accuracy_1p25"):
            print(k, r[k][b], w[k])
            assert abs(r[k][b] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), k


def _scene(H, W, seed, top=70.0):
    """steps plus a ramp (metres)"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    d = 4.0 + (top - 4.0) * (1.0 - y / H) + 0.004 * x
    for _ in range(14):
        cx, cy, r, z = g.random() * W, g.random() * H, 5 + g.random() * 0.12 * W, 3 + g.random() * (top - 10)
        m = ((x - cx) / r) ** 2 + ((y - cy) / (0.6 * r)) ** 2 < 1
        d = np.where(m, np.minimum(d, z), d)
    return d.astype(np.float32)


@pytest.mark.parametrize("H,W", [(24, 40), (48, 160)])
def test_fixed_scale_canny_matches_restatement(H, W):
    from mindtheedge_amd.utils.edge import canny_from_depth
    from mindtheedge_amd.utils.edge_benchmark import canny_fixed_scale, edge_from_depth
    d = _scene(H, W, seed=H, top=95.0)                            # some depths beyond max_depth: the clamp is exercised
    d[0, 0] = -3.0                                                # and one below min_depth
    pairs = [(t // 2, t) for t in range(20, 241, 20)]
    edges, vis = canny_fixed_scale(torch.from_numpy(d).cuda(), 0.0, 80.0, pairs, return_vis=True)
    q = ebr.quantise_fixed(d, 0.0, 80.0)
    np.testing.assert_array_equal(vis.cpu().numpy(), q)
    for p, (lo, hi) in enumerate(pairs):
        np.testing.assert_array_equal(edges[p].cpu().numpy(), co.canny(q, lo, hi).astype(np.float32))
    one = edge_from_depth(torch.from_numpy(d).cuda(), (W, H), thresh_1=20, thresh_2=40)
    np.testing.assert_array_equal(one.cpu().numpy(), co.canny(q, 20, 40).astype(np.float32))
    # a map whose maximum is below max_depth: the fixed scale differs from the per-image scale of canny_from_depth
    low = _scene(H, W, seed=H + 1, top=30.0)
    fixed = canny_fixed_scale(torch.from_numpy(low).cuda(), 0.0, 80.0, [(10, 20)])[0].cpu().numpy()
    np.testing.assert_array_equal(fixed, co.canny(ebr.quantise_fixed(low, 0.0, 80.0), 10, 20).astype(np.float32))
    own = canny_from_depth(torch.from_numpy(low).cuda(), thresholds=((10, 20),))[0].cpu().numpy()
    assert not np.array_equal(fixed, own)


@pytest.fixture(scope="module")
def two_frames():
    gts = [_annotation("kitti_de_000114_10.png"), _annotation("kitti_de_000076_10.png")]
    depths = [_scene(384, 1280, seed=21), _scene(384, 1280, seed=22)]
    return depths, gts


def test_pr_evaluation_equals_the_cpu_pipeline(two_frames):
    from mindtheedge_amd.utils import edge_benchmark as eb
    depths, gts = two_frames
    prec, rec = eb.pr_evaluation([torch.from_numpy(d).cuda() for d in depths], [torch.from_numpy(g).cuda() for g in gts])
    wp, wr = ebr.pr_evaluation_ref(depths, gts)
    assert len(prec) == 12 and prec == wp and rec == wr
    pr, wpr = np.vstack((prec, rec)).T, np.vstack((wp, wr)).T
    assert eb.mean_recall_at_precision_range(pr) == ebr.mean_recall_at_precision_range(wpr)
    assert eb.mean_recall_at_precision_range(pr, 0.12, 0.65) == ebr.mean_recall_at_precision_range(wpr, 0.12, 0.65)
    assert sum(rec) > 0                                            # the scenes do produce matched edges


def test_entry_points_write_the_analysis_files(two_frames, tmp_path, capsys):
    import shutil
    import yaml
    from test_gpu_entry_points import _run_main, _yaml
    depths, gts = two_frames
    pred_dir = os.path.join(tmp_path, "pred")
    os.makedirs(pred_dir)
    for i, d in enumerate(depths):
        np.save(os.path.join(pred_dir, "%08d_regular.npy" % i), d)
    with open(os.path.join(tmp_path, "pred.txt"), "w") as f:
        f.write("a/00000000_regular.npy\nb/00000001_regular.npy\n")
    with open(os.path.join(tmp_path, "gt.txt"), "w") as f:
        f.write("x/kitti_de_000114_10.png\nx/kitti_de_000076_10.png\n")
    _run_main("eval_depth_edges", ["eval_depth_edges.py", "--depth_pred_list_path", os.path.join(tmp_path, "pred.txt"), "--depth_pred_dir_path", pred_dir,
                                   "--depth_edge_gt_list_path", os.path.join(tmp_path, "gt.txt"), "--depth_edge_gt_dir_path", GOLDEN])
    out = capsys.readouterr().out
    assert "AUC over all range: " in out and "AUC over partial range: " in out
    # infer_edges.py: without analysis keys exactly today's files ...
    cfg = _yaml(tmp_path, 96, 160)
    plain = os.path.join(tmp_path, "plain")
    _run_main("infer_edges", ["infer_edges.py", "--config", cfg, "--synthetic", "2", "--output", plain])
    assert sorted(os.listdir(plain)) == ["00000000_regular.npy", "00000000_regular.png", "00000001_regular.npy", "00000001_regular.png"]
    # ... and with them the analysis files beside the predictions
    edge_list, gt_list = os.path.join(tmp_path, "edges.txt"), os.path.join(tmp_path, "depth_gt.txt")
    rng = np.random.default_rng(0)
    with open(edge_list, "w") as fe, open(gt_list, "w") as fg:
        for i in range(2):
            from PIL import Image
            e = (rng.random((96, 160)) < 0.05).astype(np.uint8) * 255
            Image.fromarray(e).save(os.path.join(tmp_path, "edge_%d.png" % i))
            np.save(os.path.join(tmp_path, "gt_%d.npy" % i), np.floor(rng.random((96, 160)) * 60 * 256) / 256.0)
            fe.write(os.path.join(tmp_path, "edge_%d.png\n" % i))
            fg.write(os.path.join(tmp_path, "gt_%d.npy\n" % i))
    with open(cfg) as f:
        c = yaml.safe_load(f)
    folder = os.path.join(tmp_path, "analysed")
    c["analysis"] = {"run_heavy_edge_metrics": True, "run_metrics": True, "edge_image_list": edge_list, "gt_image_list": gt_list,
                     "min_depth": 0.0, "max_depth": 80.0, "gt_crop": [4, 150, 10, 90], "eval_mask_image_list": "",
                     "prec_recall_eval_range_min": 0.12, "prec_recall_eval_range_max": 0.65, "just_evaluate": False}
    c["save"] = {"folder": folder}
    with open(cfg, "w") as f:
        yaml.safe_dump(c, f)
    _run_main("infer_edges", ["infer_edges.py", "--config", cfg, "--synthetic", "2"])
    plots = os.path.join(folder, "sfm_analysis", "debug_plots")
    assert sorted(os.listdir(plots)) == ["edge_AUC.txt", "frames_depth_metrics.csv", "mean_frames_bsds_edge_metrics.csv", "mean_frames_depth_metrics.csv"]
    assert np.array_equal(np.load(os.path.join(folder, "00000001_regular.npy")), np.load(os.path.join(plain, "00000001_regular.npy")))
    with open(os.path.join(plots, "edge_AUC.txt")) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("AUC over all range: ") and lines[1].startswith("AUC over partial range: ")
    with open(os.path.join(plots, "frames_depth_metrics.csv")) as f:
        rows = f.read().splitlines()
    assert rows[0] == ",frm_idx,mean_rel_err,std_rel_err,abs_rel_err,accuracy_1p1,accuracy_1p25,median_scale_factor" and len(rows) == 3
    with open(os.path.join(plots, "mean_frames_bsds_edge_metrics.csv")) as f:
        assert f.readline().strip() == ",Precision,Recall" and len(f.read().splitlines()) == 12
    # just_evaluate: the stage again over the predictions already there, no inference
    c["analysis"]["just_evaluate"] = True
    with open(cfg, "w") as f:
        yaml.safe_dump(c, f)
    before = open(os.path.join(plots, "frames_depth_metrics.csv")).read()
    shutil.rmtree(os.path.join(folder, "sfm_analysis"))
    _run_main("infer_edges", ["infer_edges.py", "--config", cfg])
    assert open(os.path.join(plots, "frames_depth_metrics.csv")).read() == before
