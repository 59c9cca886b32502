"""GPU (-m gpu): the evaluation path on real files.  The two resize kernels of csrc/eval_prep.hip bit for bit against the NumPy statement
(tests/eval_prep_ref.py; both restate OpenCV and are parity-unpinned), one validation and one test sample of KittiEdgeSplitDataset against
the reference's outputs (tests/golden/eval_prep.npz), the probability edge metrics and gt_crop against the chamfer oracle, Trainer.validate
over make_val_loaders against oracle/metrics_oracle.py, and train_edges.py with the validation section and the checkpoint policy."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_prep_ref as R                                     # noqa: E402
from oracle import canny_oracle as co                         # noqa: E402
from oracle import edge_oracle as eo                          # noqa: E402
from oracle import metrics_oracle as mo                       # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_prep.npz")
#          source      target
SHAPES = [((7, 5), (3, 9)),             # up in one axis, down in the other
          ((70, 150), (64, 128)),       # the validation frame; 32 blocks
          ((64, 128), (32, 64)),        # exactly 2x in both axes: the area branch of the uint8 kernel
          ((33, 64), (16, 32)),         # 2x in width only: the general branch
          ((1, 1), (3, 5)), ((9, 1), (4, 3)), ((1, 9), (3, 4)),
          ((35, 75), (32, 64)), ((5, 7), (5, 7))]
CROP = (2, 66, 5, 140)


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_linear_u8_bit_equal(src, dst, B):
    from mindtheedge_amd.datasets.eval_prep import resize_linear_u8
    g = np.random.default_rng(src[0] * 1000 + src[1] + B)
    for kind in ("bytes", "binary"):
        a = g.integers(0, 256, (B,) + src, dtype=np.uint8) if kind == "bytes" else ((g.random((B,) + src) < 0.3) * 255).astype(np.uint8)
        got = resize_linear_u8(torch.from_numpy(a).cuda(), dst).cpu().numpy()
        want = R.resize_linear_u8(a, dst)
        assert got.shape == (B,) + dst and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)                                # every pixel of every map
    one = resize_linear_u8(torch.from_numpy(a[0]).cuda(), dst)                  # the [h,w] form
    np.testing.assert_array_equal(one.cpu().numpy(), want[0])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_nearest_f32_bit_equal(src, dst, B):
    from mindtheedge_amd.datasets.eval_prep import resize_nearest_f32
    g = np.random.default_rng(src[0] * 1000 + src[1] + B)
    a = ((g.random((B,) + src) < 0.4) * (1 + 79 * g.random((B,) + src))).astype(np.float32)
    a[:, 0, 0] = -1.0
    got = resize_nearest_f32(torch.from_numpy(a).cuda(), dst).cpu().numpy()
    assert got.shape == (B,) + dst
    np.testing.assert_array_equal(got.view(np.uint32), R.resize_nearest_f32(a, dst).view(np.uint32))


def test_resize_kernels_refuse_bad_arguments():
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.eval_prep import resize_linear_u8, resize_nearest_f32
    u = torch.zeros((2, 4, 4), dtype=torch.uint8, device="cuda")
    f = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    out = torch.full((2, 4, 4), 7, dtype=torch.uint8, device="cuda")
    for args in [(0, 0, 4, 4, 0, 4, 4), (u.data_ptr(), 2, 4, 4, 0, 4, 4), (u.data_ptr(), 0, 4, 4, out.data_ptr(), 4, 4),
                 (u.data_ptr(), 2, 0, 4, out.data_ptr(), 4, 4), (u.data_ptr(), 2, 4, 4, out.data_ptr(), 4, 0), (u.data_ptr(), 2, 4, -1, out.data_ptr(), 4, 4)]:
        with pytest.raises(K.MteError):
            K.lib.mte_resize_linear_u8(*args, K._stream())
        with pytest.raises(K.MteError):
            K.lib.mte_resize_nearest_f32(*args, K._stream())
    assert bool((out == 7).all())                                               # nothing was launched
    with pytest.raises(ValueError):
        resize_linear_u8(f, (2, 2))
    with pytest.raises(ValueError):
        resize_nearest_f32(u, (2, 2))
    with pytest.raises(K.MteError):
        resize_linear_u8(u.cpu(), (2, 2))                                       # host tensors: no fallback


def _dataset(tmp_path, fx, mode, crop, image_shape=()):
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset
    split = R.write_split(str(tmp_path), n=1, rgb=fx["rgb"], input_depth=fx["input_depth"], rgb_edge=fx["rgb_edge"])
    return KittiEdgeSplitDataset(split, image_shape, root=str(tmp_path), input_depth_type=["npy"], mode=mode, crop_eval_borders=crop)


def _files(tmp_path):
    from PIL import Image
    png = np.array(Image.open(os.path.join(tmp_path, "depth0.png")), dtype=int)
    depth = np.where(png == 0, -1.0, png / 256.0).astype(np.float32)
    edges = [np.array(Image.open(os.path.join(tmp_path, "edges", "00000000_lidar_00%d.png" % s))) for s in range(4)]
    return depth, edges


@pytest.mark.parametrize("case", ["nocrop", "crop"])
def test_validation_sample_matches_the_reference(tmp_path, fx, case):
    crop = CROP if case == "crop" else ()
    assert tuple(int(v) for v in fx[case + "_crop"]) == crop
    s = _dataset(tmp_path, fx, "validation", crop)[0]
    depth, edges = _files(tmp_path)
    assert s["idx"] == 0 and all(v.is_cuda for v in s.values() if torch.is_tensor(v))
    np.testing.assert_array_equal(s["rgb"].cpu().numpy(), fx[case + "_rgb_out"].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    np.testing.assert_array_equal(s["input_depth"].cpu().numpy(), fx[case + "_input_depth_out"][None])
    assert s["depth"].shape == (1, 70, 150)                                     # native size, not cropped
    np.testing.assert_array_equal(s["depth"][0].cpu().numpy(), depth)
    for key, e, shape in [("edge", edges[0], (64, 128)), ("edge_1", edges[1], (32, 64)), ("edge_2", edges[2], (16, 32)), ("edge_3", edges[3], (8, 16))]:
        want = R.resize_linear_u8(e, shape).astype(np.float32) / np.float32(255)       # the whole map: supervision is not cropped
        np.testing.assert_array_equal(s[key].cpu().numpy(), want[None])
    b = [int(v) for v in fx[case + "_borders"]]
    re_ = np.ascontiguousarray(fx["rgb_edge"][b[1]:b[3], b[0]:b[2]])
    np.testing.assert_array_equal(s["rgb_edge"][0].cpu().numpy(), R.resize_linear_u8(re_, (64, 128)).astype(np.float32) / np.float32(255))
    ref = R.validation_sample({"rgb": fx["rgb"], "input_depth": fx["input_depth"], "rgb_edge": fx["rgb_edge"], "depth": depth, "edge": edges[0],
                               "edge_1": edges[1], "edge_2": edges[2], "edge_3": edges[3]}, crop)
    assert sorted(k for k in s if k != "idx") == sorted(ref)
    for k, v in ref.items():
        np.testing.assert_array_equal(s[k].cpu().numpy(), v)


def test_test_sample_matches_the_reference(tmp_path, fx):
    s = _dataset(tmp_path, fx, "test", CROP, image_shape=(64, 128))[0]
    depth, edges = _files(tmp_path)
    np.testing.assert_array_equal(s["rgb"].cpu().numpy(), fx["crop_rgb_out"].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    b = [int(v) for v in fx["crop_borders"]]
    lid = np.ascontiguousarray(fx["input_depth"][b[1]:b[3], b[0]:b[2]])
    np.testing.assert_array_equal(s["input_depth"][0].cpu().numpy(), R.resize_nearest_f32(lid, (64, 128)))
    np.testing.assert_array_equal(s["depth"][0].cpu().numpy(), depth)
    np.testing.assert_array_equal(s["edge"][0].cpu().numpy(), edges[0].astype(np.float32) / np.float32(255))
    # without an image_shape nothing is resized: the crop only
    s0 = _dataset(tmp_path, fx, "test", CROP)[0]
    want = fx["rgb"][b[1]:b[3], b[0]:b[2]].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    np.testing.assert_array_equal(s0["rgb"].cpu().numpy(), want)
    np.testing.assert_array_equal(s0["input_depth"][0].cpu().numpy(), lid)


def _smooth_probability(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    p = 0.5 + 0.5 * np.sin(x / (2.0 + 3 * g.random()) + y / (3.0 + 2 * g.random()) + 6 * g.random())
    return (0.8 * p + 0.2 * g.random((h, w))).astype(np.float32)


def _want_probability_metrics(prob, gt, crop=None):
    if prob.shape != gt.shape:
        prob = co.resize_linear(prob, gt.shape[1], gt.shape[0])
    want = []
    for t in (0.5, 0.75, 0.9):
        e = (prob > t).astype(np.uint8) * 255
        g_ = gt
        if crop is not None:
            e, g_ = e[crop[2]:crop[3], crop[0]:crop[1]], gt[crop[2]:crop[3], crop[0]:crop[1]]
        want.extend(eo.precision_recall_f1(e, g_))
    return np.array(want, np.float64)


@pytest.mark.parametrize("shape", [(61, 120), (32, 64)])
def test_edge_metrics_from_probability_and_gt_crop(shape):
    from mindtheedge_amd.utils.edge import compute_edge_metrics_from_probability
    prob = _smooth_probability(32, 64, 3)
    g = np.random.default_rng(9)
    gt = ((g.random(shape) < 0.08) * 255).astype(np.float32)
    got = compute_edge_metrics_from_probability(torch.from_numpy(prob).cuda(), torch.from_numpy(gt).cuda())
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (9,)
    want = _want_probability_metrics(prob, gt)
    assert np.isfinite(want).all() and len(set(np.round(want, 6))) > 3          # the three thresholds give different images
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, equal_nan=True)
    # gt_crop = [start_x, end_x, start_y, end_y]: the cropped evaluation equals the evaluation of pre-cropped inputs
    crop = [5, shape[1] - 9, 3, shape[0] - 6]
    cropped = compute_edge_metrics_from_probability(torch.from_numpy(prob).cuda(), torch.from_numpy(gt).cuda(), gt_crop=crop)
    np.testing.assert_allclose(cropped.cpu().numpy(), _want_probability_metrics(prob, gt, crop), rtol=1e-12, equal_nan=True)
    if prob.shape == gt.shape:
        pre = compute_edge_metrics_from_probability(torch.from_numpy(np.ascontiguousarray(prob[crop[2]:crop[3], crop[0]:crop[1]])).cuda(),
                                                    torch.from_numpy(np.ascontiguousarray(gt[crop[2]:crop[3], crop[0]:crop[1]])).cuda())
        assert torch.equal(cropped, pre)
    assert not torch.equal(cropped, got)


MODEL = {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                  "edges_depth_edge_loss_all_scales": True}, "params": {"crop": "garg"}}


def _val_config(folder, split, **validation):
    from mindtheedge_amd.utils.config import load_config
    return load_config(None, {"model": MODEL, "datasets": {"validation": {"dataset": ["KITTI"], "path": [os.path.join(folder, "KITTI_tiny")],
                                                                           "split": [split], "depth_type": ["groundtruth"], **validation}}})


def test_trainer_validate_over_val_loaders_matches_the_oracle(tmp_path):
    """three 70 x 150 frames -> 64 x 128 network input; metrics against the 70 x 150 ground truth, averaged over the frames; gt_crop"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.kitti_edges import make_val_loaders
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.trainers.trainer import Trainer
    from mindtheedge_amd.utils.edge import canny_from_depth, compute_edge_metrics
    from PIL import Image
    K.set_compute_dtype("bf16")
    folder = os.path.join(str(tmp_path), "KITTI_tiny")
    split = R.write_split(folder, n=3)
    cfg = _val_config(str(tmp_path), split)
    loaders = make_val_loaders(cfg, 0, 1)
    assert len(loaders) == 1 and len(loaders[0]) == 3
    torch.manual_seed(3)
    wrap = ModelWrapper(cfg).cuda()
    wrap.train()
    seen = []
    hook = wrap.model.register_forward_hook(lambda mod, args, res: seen.append(res["inv_depths"][0][0][:, 0:1].float().cpu().numpy()))
    (res,) = Trainer(max_epochs=1).validate(loaders, wrap)
    hook.remove()
    assert wrap.training and len(seen) == 6
    prefix = "KITTI_tiny-val_files-groundtruth"
    assert wrap.dataset_prefix("validation", 0) == prefix
    assert len(res) == 28 + 9 and all(k.startswith(prefix + "-") for k in res)
    assert prefix + "-precision_0" in res and prefix + "-f1_2" in res
    keys = ("abs_rel", "sqr_rel", "rmse", "rmse_log", "a1", "a2", "a3")
    want = {m: [] for m in ("", "_pp", "_gt", "_pp_gt")}
    for i in range(3):
        png = np.array(Image.open(os.path.join(folder, "depth%d.png" % i)), dtype=int)
        gt = np.where(png == 0, -1.0, png / 256.0).astype(np.float32)[None, None]
        inv, invf = seen[2 * i], seen[2 * i + 1]
        assert inv.shape == (1, 1, 64, 128)
        pp = mo.post_process_inv_depth(inv, invf, "mean")
        depth, depth_pp = 1.0 / np.maximum(inv, np.float32(1e-6)), 1.0 / np.maximum(pp, np.float32(1e-6))
        for mode in want:
            want[mode].append(mo.compute_depth_metrics(gt, depth_pp if "pp" in mode else depth, crop="garg", use_gt_scale="gt" in mode))
    for mode, rows in want.items():
        mean = np.mean(np.stack(rows).astype(np.float64), axis=0)
        got = np.array([res["%s-%s%s" % (prefix, k, mode)] for k in keys])
        print(mode, got, mean)
        np.testing.assert_allclose(got, mean, rtol=5e-5, atol=1e-7)
    # gt_crop: evaluate_depth scores the window of the whole-map Canny images against the window of the ground truth
    cfgc = _val_config(str(tmp_path), split, gt_crop=[[8, 100, 4, 60]])
    wrap.config = cfgc
    wrap.eval()
    batch = next(iter(make_val_loaders(cfgc, 0, 1)[0]))
    seen.clear()
    hook = wrap.model.register_forward_hook(lambda mod, args, res: seen.append(res["inv_depths"][0][0][:, 0:1].clone()))
    got = wrap.evaluate_depth(batch, (0, 0))["metrics"]["edges"]
    hook.remove()
    from mindtheedge_amd.utils.depth import inv2depth
    depth = inv2depth(seen[0])
    edges = canny_from_depth(depth[0, 0])
    gt_edge = batch["edge"][0, 0] * 255
    pre = compute_edge_metrics([edges[p][4:60, 8:100].contiguous() for p in range(3)], gt_edge[4:60, 8:100].contiguous())
    assert torch.equal(got, pre)
    whole = compute_edge_metrics([edges[p] for p in range(3)], gt_edge)
    assert not torch.equal(got, whole)


def test_estimator_validation_thresholds_the_network_output_and_test_loaders(tmp_path):
    """a depth-edge estimator validates by thresholding its network's RGB (and RGB+LiDAR) output; test_step / test_epoch_end over
    make_test_loaders give the depth metrics only, under the test section's prefix"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.kitti_edges import make_test_loaders, make_val_loaders
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    from mindtheedge_amd.utils.edge import compute_edge_metrics_from_probability
    K.set_compute_dtype("bf16")
    folder = os.path.join(str(tmp_path), "KITTI_tiny")
    split = R.write_split(folder, n=2)
    section = {"dataset": ["GTA"], "path": [folder], "split": [split], "depth_type": ["groundtruth"], "input_depth_type": ["npy"]}
    cfg = load_config(None, {"model": {**MODEL, "name": "EdgeEstimationLIDARModel"},
                             "datasets": {"augmentation": {"image_shape": (64, 128)}, "validation": section, "test": section}})
    wrap = ModelWrapper(cfg).cuda().eval()
    assert wrap.model.depth_net.with_san
    batch = next(iter(make_val_loaders(cfg, 0, 1)[0]))
    assert batch["input_depth"].shape == (1, 1, 64, 128) and batch["depth"].shape == (1, 1, 70, 150)
    seen = []
    hook = wrap.model.depth_net.register_forward_hook(lambda mod, args, res: seen.append((len(args), res["inv_depths"][0][0][:, 0:1].clone())))
    metrics = wrap.evaluate_depth(batch, (0, 0))["metrics"]
    hook.remove()
    assert len(seen) == 4                                            # plain, mirrored, the network's RGB output, its RGB+LiDAR output
    gt_edge = batch["edge"][0, 0] * 255
    assert torch.equal(metrics["edges"], compute_edge_metrics_from_probability(seen[2][1][0, 0], gt_edge))
    assert torch.equal(metrics["edges_input"], compute_edge_metrics_from_probability(seen[3][1][0, 0], gt_edge))
    assert metrics["edges"].shape == (9,) and set(metrics) == {"depth", "depth_pp", "depth_gt", "depth_pp_gt", "edges", "edges_input"}
    # test loaders: image_shape is honoured, input_depth through the nearest resize, depth metrics only
    loaders = make_test_loaders(cfg, 0, 1)
    assert len(loaders) == 1 and len(loaders[0]) == 2
    outs = []
    for i, b in enumerate(loaders[0]):
        assert b["rgb"].shape == (1, 3, 64, 128) and b["input_depth"].shape == (1, 1, 64, 128) and b["depth"].shape == (1, 1, 70, 150)
        outs.append(wrap.test_step(b, i, 0))
    assert all("edges" not in o and "depth_pp_gt" in o for o in outs)
    res = wrap.test_epoch_end(outs, 0)
    prefix = "KITTI_tiny-val_files-groundtruth"
    assert len(res) == 28 and all(k.startswith(prefix + "-") for k in res) and all(np.isfinite(v) for v in res.values())
    want = torch.stack([o["depth_pp_gt"] for o in outs]).sum(0) / 2
    assert abs(res[prefix + "-abs_rel_pp_gt"] - float(want[0])) <= 1e-6 * abs(float(want[0]))


def _yaml(tmp_path, split, folder, validation=True, save_top_k=1):
    with open(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_val.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["datasets"]["augmentation"].update(image_shape=[64, 128], jittering=[])
    cfg["datasets"]["train"].update(batch_size=1, path=[folder], split=[split])
    if validation:
        cfg["datasets"]["validation"].update(path=[folder], split=[split])
    else:
        del cfg["datasets"]["validation"]
    cfg["checkpoint"].update(filepath="", save_top_k=save_top_k)
    path = os.path.join(tmp_path, "cfg_%d.yaml" % int(validation))
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def _run_train(argv):
    import importlib
    old = sys.argv
    sys.argv = argv
    try:
        importlib.import_module("train_edges").main()
    finally:
        sys.argv = old
        from mindtheedge_amd import kernels as K
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


def test_train_edges_validates_and_keeps_the_best_checkpoint(tmp_path, capsys):
    folder = os.path.join(str(tmp_path), "KITTI_tiny")
    split = R.write_split(folder, n=2, frame=(64, 128))
    data = "mindtheedge_amd.datasets.kitti_edges:make_loader"
    save = os.path.join(str(tmp_path), "run")
    _run_train(["train_edges.py", _yaml(str(tmp_path), split, folder), "--data", data, "--epochs", "1", "--save", save])
    out = capsys.readouterr().out
    hist = eval(out.strip().splitlines()[-1])
    assert len(hist) == 1 and hist[0]["steps"] == 2 and len(hist[0]["validation"]) == 1
    val = hist[0]["validation"][0]
    prefix = "KITTI_tiny-val_files-groundtruth"
    assert np.isfinite(val[prefix + "-abs_rel_pp_gt"]) and len([k for k in val if "abs_rel" in k]) == 4
    assert len([l for l in out.splitlines() if l.startswith("validation epoch 0 | " + prefix)]) == 1
    assert os.listdir(save) == ["epoch=0_abs_rel_pp_gt=%.3f.ckpt" % val[prefix + "-abs_rel_pp_gt"]]
    # without the validation section: one file per epoch under the plain name
    save2 = os.path.join(str(tmp_path), "run2")
    _run_train(["train_edges.py", _yaml(str(tmp_path), split, folder, validation=False), "--data", data, "--epochs", "1", "--save", save2])
    out = capsys.readouterr().out
    hist = eval(out.strip().splitlines()[-1])
    assert "validation" not in hist[0] and os.listdir(save2) == ["epoch=0.ckpt"]
