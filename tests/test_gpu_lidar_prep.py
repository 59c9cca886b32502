"""GPU (-m gpu): the LiDAR input path on the device (csrc/lidar_prep.hip, mindtheedge_amd/datasets/lidar_prep.py) against the
fixtures the reference produced (tests/golden/make_golden_lidar.py) and the numpy restatement of the rules (tests/lidar_ref.py,
pinned to those fixtures by tests/test_lidar_ref_cpu.py).  Every comparison of maps is bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

import lidar_ref as R
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "lidar_prep.npz"))
AUG = [str(n) for n in Z["aug_names"]]
PROJ = [str(n) for n in Z["proj_names"]]
SCALE = ((1, 1, 1), (1, 1, 1.1))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", AUG)
def test_fixture_with_stored_draws(name):
    from mindtheedge_amd.datasets.lidar_prep import augment_depth_values
    c = R.aug_case(Z, name)
    got = augment_depth_values(_cuda(c['depth']), c['scale'], c['add'], c['drop'], draws=c['draws'])
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), c['stable'].astype(np.float32))


@pytest.mark.parametrize("name", AUG)
def test_fixture_through_the_seed(name):
    from mindtheedge_amd.datasets.lidar_prep import augment_depth_values
    c = R.aug_case(Z, name)
    np.random.seed(c['seed'])
    got = augment_depth_values(_cuda(c['depth']), c['scale'], c['add'], c['drop'])
    np.testing.assert_array_equal(got.cpu().numpy(), c['stable'].astype(np.float32))


def _random_map(shape, density, seed):
    g = np.random.RandomState(seed)
    return ((g.rand(*shape) < density) * (1.0 + 79.0 * g.rand(*shape))).astype(np.float32)


def _only(shape, i, j):
    d = np.zeros(shape, dtype=np.float32)
    d[i, j] = 12.5
    return d


def _explicit_draws(depth, a, drop, seed):
    """draws from a generator of the test's own: shifts up to +-a pixels, value offsets up to 0.5, a share `drop` dropped"""
    g = np.random.RandomState(seed)
    n = int((depth > 0).sum())
    draws = {'scale_d0': 1.0 + 0.1 * g.rand(), 'add_i': g.uniform(-a, a, n), 'add_j': g.uniform(-a, a, n), 'add_d': g.uniform(0, 0.5, n)}
    survivors = R.count_survivors(depth, draws['scale_d0'], draws['add_i'], draws['add_j'], draws['add_d'])
    draws['keep'] = (g.rand(survivors) >= drop).astype(np.uint8)
    return draws


# one wave, one workgroup of the scan, ragged tails, many workgroups, extreme maps, the workload's size (240 workgroup counts go
# through the second-level scan in one round) and the GTA canvas (1013 counts: four rounds with a carry)
SCAN_CASES = {
    "wave_8x8": lambda: _random_map((8, 8), 0.5, 1), "workgroup_16x16": lambda: _random_map((16, 16), 0.5, 2),
    "ragged_13x21": lambda: _random_map((13, 21), 0.5, 3), "ragged_17x129": lambda: _random_map((17, 129), 0.3, 4),
    "many_96x320": lambda: _random_map((96, 320), 0.05, 5), "full_40x56": lambda: _random_map((40, 56), 2.0, 6),
    "last_pixel": lambda: _only((33, 65), 32, 64), "first_pixel": lambda: _only((33, 65), 0, 0),
    "workload_384x1280": lambda: _random_map((384, 1280), 0.05, 7), "canvas_1080x1920": lambda: _random_map((1080, 1920), 0.01, 8),
}


@pytest.mark.parametrize("name", list(SCAN_CASES))
def test_scan_geometry_against_the_restatement(name):
    from mindtheedge_amd.datasets.lidar_prep import augment_depth_values
    depth = SCAN_CASES[name]()
    if name.startswith("full"):
        assert (depth > 0).all()
    d = _explicit_draws(depth, 1.5, 0.2, 11)
    want = R.augment_depth_values(depth, d['scale_d0'], d['add_i'], d['add_j'], d['add_d'], d['keep']).astype(np.float32)
    got = augment_depth_values(_cuda(depth), None, None, draws=d)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if name in ("last_pixel", "first_pixel"):
        assert not want.any()                                          # a lone point carries the smallest key
    else:
        assert want.any()


def test_empty_map_and_argument_errors():
    from mindtheedge_amd.datasets.lidar_prep import augment_depth_values
    from mindtheedge_amd.kernels import MteError
    assert augment_depth_values(None, SCALE, ((0, 0, 0), (1, 1, 0.5))) is None
    state = np.random.get_state()[1].copy()
    out = augment_depth_values(torch.zeros(9, 14).cuda() - 1.0, SCALE, ((0, 0, 0), (1, 1, 0.5)))      # -1 = no return, as read_png_depth marks it
    assert out.shape == (9, 14) and not out.any()
    assert np.array_equal(np.random.get_state()[1], state)            # nothing was drawn
    with pytest.raises(MteError):
        augment_depth_values(torch.zeros(4, 4), SCALE, ((0, 0, 0), (1, 1, 0.5)))
    with pytest.raises(ValueError):
        augment_depth_values(torch.ones(4, 4).cuda(), None, None, draws={'scale_d0': 1.0, 'add_i': np.zeros(3), 'add_j': np.zeros(3), 'add_d': np.zeros(3)})


def _stages_through_the_c_abi(depth, d, fill):
    """the three stages called directly, every output and workspace buffer pre-filled with `fill` bytes -> (n, n', out)"""
    from mindtheedge_amd import kernels as K
    H, W = depth.shape
    src = _cuda(depth)
    nbytes = K.lib.mte_lidar_perturb_work_bytes(H, W)
    assert nbytes > 0 and K.lib.mte_lidar_perturb_work_bytes(1 << 15, 1 << 15) == 0
    work = torch.full(((nbytes + 7) // 8 * 8,), fill, dtype=torch.uint8, device="cuda")
    out = torch.full((H, W), fill, dtype=torch.uint8, device="cuda").repeat_interleave(4, dim=1).view(torch.float32)
    assert out.shape == (H, W) and work.data_ptr() % 8 == 0
    counts = work[:8].view(torch.int32)
    st = K._stream()
    K.lib.mte_lidar_index(src.data_ptr(), H, W, work.data_ptr(), st)
    n = int(counts[0])
    adds = _cuda(np.stack([d['add_i'], d['add_j'], d['add_d']]))
    K.lib.mte_lidar_perturb(src.data_ptr(), H, W, n, float(d['scale_d0']), adds[0].data_ptr(), adds[1].data_ptr(), adds[2].data_ptr(), work.data_ptr(), st)
    survivors = int(counts[1])
    keep = _cuda(d['keep'])
    K.lib.mte_lidar_scatter(H, W, n, keep.data_ptr(), survivors, out.data_ptr(), work.data_ptr(), st)
    torch.cuda.synchronize()
    return n, survivors, out.cpu().numpy()


@pytest.mark.parametrize("fill", [0x7f, 0xff])                          # 0x7f7f7f7f = 3.4e38 / a huge count, 0xff.. = NaN / -1
def test_no_entry_point_relies_on_a_cleared_buffer(fill):
    from mindtheedge_amd import kernels as K
    depth = _random_map((37, 150), 0.2, 21)
    d = _explicit_draws(depth, 2.0, 0.3, 22)
    want = R.augment_depth_values(depth, d['scale_d0'], d['add_i'], d['add_j'], d['add_d'], d['keep']).astype(np.float32)
    runs = [_stages_through_the_c_abi(depth, d, fill) for _ in range(2)]
    for n, survivors, out in runs:
        assert n == int((depth > 0).sum()) and survivors == len(d['keep'])
        assert np.isfinite(out).all() and out.max() < 100.0
        np.testing.assert_array_equal(out, want)
    assert runs[0][2].tobytes() == runs[1][2].tobytes()
    # an empty map: zeros, the workspace is not needed
    out = torch.full((5, 7), float("nan"), device="cuda")
    K.lib.mte_lidar_scatter(5, 7, 0, None, 0, out.data_ptr(), None, K._stream())
    assert not out.cpu().numpy().any()
    # the projection
    c = R.proj_case(Z, "small")
    H, W = c['shape']
    pts, kmat = _cuda(c['points']), _cuda(c['K'].reshape(9))
    results = []
    for _ in range(2):
        out = torch.full((H, W), fill, dtype=torch.uint8, device="cuda").repeat_interleave(4, dim=1).view(torch.float32)
        ws = torch.full((H, W * 4), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        K.lib.mte_lidar_project(pts.data_ptr(), pts.shape[1], kmat.data_ptr(), None, out.data_ptr(), H, W, ws.data_ptr(), K._stream())
        results.append(out.cpu().numpy())
        np.testing.assert_array_equal(results[-1], c['out'].astype(np.float32))
    assert results[0].tobytes() == results[1].tobytes()


@pytest.mark.parametrize("name", PROJ)
def test_projection_fixture(name):
    from mindtheedge_amd.datasets.lidar_prep import project_lidar
    c = R.proj_case(Z, name)
    dm = None if c['depth_map'] is None else _cuda(c['depth_map'])
    got = project_lidar(c['points'], c['K'], c['shape'], dm)
    assert got.dtype == torch.float32 and tuple(got.shape) == c['shape']
    np.testing.assert_array_equal(got.cpu().numpy(), c['out'].astype(np.float32))
    if name == "big":                                                  # the default shape is the reference's canvas; an empty cloud gives zeros
        assert tuple(project_lidar(c['points'][:, :10], c['K']).shape) == (1080, 1920)
        assert not project_lidar(np.zeros((3, 0)), c['K'], (8, 8)).any()


# ---- the dataset and the annotation driver on files

H, W = 64, 128
LH, LW = 80, 160                                                        # the depth / LiDAR files' size: resized to the frame's
ADD = ((0, 0, 0), (1.5, 1.5, 0.5))
LOSS = {"loss": {"supervised_loss_weight": 1.0}}                       # as the shipped YAML: the photometric term is not built


def _write_split(tmp_path, frames, lidar_ext):
    """rgb, depth (= the LiDAR map), edge and normal annotations at four scales, and the LiDAR map as .png, .npy and velodyne .bin"""
    from PIL import Image
    g = np.random.default_rng(0)
    lines = []
    os.makedirs(os.path.join(tmp_path, "normals"), exist_ok=True)
    for i in range(frames):
        Image.fromarray((g.random((H, W, 3)) * 255).astype(np.uint8)).save(os.path.join(tmp_path, "rgb%d.png" % i))
        raw = ((g.random((LH, LW)) < 0.1) * (256 + g.integers(0, 70 * 256, (LH, LW)))).astype(np.uint16)      # >= 1 m, multiples of 1/256
        raw[0, 0] = 300
        Image.fromarray(raw).save(os.path.join(tmp_path, "lidar%d.png" % i))
        metres = raw.astype(np.float32) / 256.0
        np.save(os.path.join(tmp_path, "lidar%d.npy" % i), metres)
        v, u = np.nonzero(raw)
        z = metres[v, u].astype(np.float64)
        cam = np.stack([(u + 0.5 - 960.0) * z / 960.0, (v + 0.5 - 540.0) * z / 960.0, z], axis=1)       # pixel centres under the GTA intrinsics
        order = g.permutation(len(z))
        cloud = np.stack([cam[order, 2], -cam[order, 0], -cam[order, 1], np.ones(len(z))], axis=1).astype(np.float32)      # (-y, -z, x) = cam
        cloud = np.concatenate([cloud, np.array([[np.nan, 0, 0, 1]], dtype=np.float32)])
        cloud.tofile(os.path.join(tmp_path, "lidar%d.bin" % i))
        for s in range(4):
            Image.fromarray(((g.random((H >> s, W >> s)) < 0.05) * 255).astype(np.uint8)).save(os.path.join(tmp_path, "%08d_lidar_00%d.png" % (i, s)))
            Image.fromarray(g.integers(0, 256, (H >> s, W >> s), dtype=np.uint8)).save(os.path.join(tmp_path, "normals", "%08d_lidar_00%d.png" % (i, s)))
        lines.append("rgb%d.png lidar%d.png %08d_lidar_000.png lidar%d.%s None None None normals/%08d_lidar_000.png\n" % (i, i, i, i, lidar_ext, i))
    split = os.path.join(tmp_path, "split_%s.txt" % lidar_ext)
    with open(split, "w") as f:
        f.writelines(lines)
    return split


def test_dataset_lidar_column(tmp_path):
    from PIL import Image
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, SplitLoader, make_loader
    from mindtheedge_amd.datasets.lidar_prep import draw_lidar_keep, draw_lidar_perturbation
    from mindtheedge_amd.utils.config import load_config
    split = _write_split(tmp_path, 2, "png")
    root = str(tmp_path)
    plain = KittiEdgeSplitDataset(split, (H, W), root=root)[0]
    assert set(plain) == {"idx", "rgb", "depth", "edge", "edge_1", "edge_2", "edge_3", "normal", "normal_1", "normal_2", "normal_3"}
    for off in ("", [""], None):
        assert set(KittiEdgeSplitDataset(split, (H, W), root=root, input_depth_type=off, lidar_scale=SCALE, lidar_add=ADD)[0]) == set(plain)
    # the column as it is
    s = KittiEdgeSplitDataset(split, (H, W), root=root, input_depth_type=["velodyne"])[0]
    assert set(s) == set(plain) | {"lidar", "input_depth"}
    raw = np.array(Image.open(os.path.join(root, "lidar0.png")), dtype=int)
    want = do.resize_depth_preserve(np.where(raw == 0, -1.0, raw / 256.0).astype(np.float32), (H, W)).astype(np.float32)
    assert s["lidar"].shape == (1, H, W) and s["input_depth"].shape == (1, H, W)
    np.testing.assert_array_equal(s["lidar"][0].cpu().numpy(), want)
    np.testing.assert_array_equal(s["input_depth"][0].cpu().numpy(), want)
    for k in plain:
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], s[k]), k
    # the three formats
    for ext in ("npy", "bin"):
        other = KittiEdgeSplitDataset(_write_split(tmp_path, 2, ext), (H, W), root=root, input_depth_type=["velodyne"])[0]
        np.testing.assert_array_equal(other["lidar"][0].cpu().numpy(), np.maximum(want, 0.0) if ext == "bin" else want)
    # perturbed: only the network's input
    ds = KittiEdgeSplitDataset(split, (H, W), root=root, input_depth_type=["velodyne"], lidar_scale=SCALE, lidar_add=ADD, lidar_drop_rate=0.2)
    np.random.seed(5)
    p = ds[0]
    np.testing.assert_array_equal(p["lidar"][0].cpu().numpy(), want)
    np.random.seed(5)
    scale_d0, add_i, add_j, add_d = draw_lidar_perturbation(int((want > 0).sum()), SCALE, ADD)
    keep = draw_lidar_keep(R.count_survivors(want, scale_d0, add_i, add_j, add_d), 0.2)
    perturbed = R.augment_depth_values(want, scale_d0, add_i, add_j, add_d, keep).astype(np.float32)
    np.testing.assert_array_equal(p["input_depth"][0].cpu().numpy(), perturbed)
    assert (perturbed != np.maximum(want, 0.0)).any() and 0 < (perturbed > 0).sum() < (want > 0).sum()
    # crop borders crop the LiDAR map like the depth map
    cropped = KittiEdgeSplitDataset(split, (H, W), root=root, input_depth_type=["velodyne"], crop_train_borders=(8, 8))[0]
    assert torch.equal(cropped["lidar"], cropped["depth"])
    # make_loader reads the keys from the configuration; one DEE training step with the SAN branch on such a batch
    cfg = load_config(None, {"model": {"name": "EdgeEstimationLIDARModel", "loss": {"edges_depth_edge_loss_all_scales": True}},
                             "edges": {"train_depth_edges": True},
                             "datasets": {"augmentation": {"image_shape": (H, W), "lidar_scale": SCALE, "lidar_add": ADD, "lidar_drop_rate": 0.1},
                                          "train": {"batch_size": 2, "split": [split], "path": [root], "input_depth_type": ["velodyne"]}}})
    assert load_config(None).datasets.train.input_depth_type == [""] and load_config(None).datasets.augmentation.lidar_drop_rate == 0.0
    loader = make_loader(cfg, 0, 1)
    loader.shuffle = False
    (batch,) = list(loader)
    assert batch["input_depth"].shape == (2, 1, H, W) and batch["lidar"].shape == (2, 1, H, W)
    assert not torch.equal(batch["input_depth"], batch["lidar"])
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    K.set_compute_dtype("fp32")
    wrap = ModelWrapper(cfg).cuda().train()
    assert wrap.depth_net.with_san
    out = wrap.model(dict(batch))
    assert torch.isfinite(out["loss"]).all() and "edge_lidar_loss" in out["metrics"]
    assert isinstance(loader, SplitLoader)


def test_annotation_driver_on_a_split(tmp_path):
    import yaml
    from PIL import Image
    sys.path.insert(0, ROOT)
    import infer_edge_estimation as iee
    from infer_edges import load_frame
    from mindtheedge_amd.datasets.kitti_edges import read_split, resize_depth_preserve
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    src = os.path.join(tmp_path, "in")
    os.makedirs(src)
    split = _write_split(src, 2, "png")
    lines = [l.split(" ") for l in open(split).read().splitlines()]
    absolute = os.path.join(tmp_path, "abs_split.txt")
    with open(absolute, "w") as f:
        f.writelines(" ".join(c if c == "None" else os.path.join(src, c) for c in l) + "\n" for l in lines)
    cfg_path = os.path.join(tmp_path, "cfg.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"model": LOSS, "datasets": {"augmentation": {"image_shape": [H, W]}, "test": {"input_depth_type": ["velodyne"]}}}, f)
    save = os.path.join(tmp_path, "out")
    iee.main(["--config", cfg_path, "--split", absolute, "--save", save])
    for ctr in range(2):
        for key in ("regular", "lidar"):
            for s in range(4):
                name = "%08d_%s_%03d.png" % (ctr, key, s)
                for folder in (save, os.path.join(save, "normals")):
                    im = np.asarray(Image.open(os.path.join(folder, name)))
                    assert im.dtype == np.uint8 and im.shape == (H >> s, W >> s), (folder, name)
    recs = read_split(os.path.join(save, "rgb_lidar_edges_split.txt"))
    assert len(recs) == 2
    assert recs[1]["rgb"] == os.path.join(src, "rgb1.png") and recs[1]["lidar"] == recs[1]["depth"] == os.path.join(src, "lidar1.png")
    assert recs[1]["edge"] == save + "/00000001_lidar_000.png" and recs[1]["normal"] == save + "/normals/00000001_lidar_000.png"
    assert recs[1]["seg"] is None and os.path.exists(recs[1]["edge"]) and os.path.exists(recs[1]["normal"])
    # the same model (the wrapper seeds its initialisation from the configuration) on the same inputs
    config = load_config(cfg_path, {"model": {"depth_net": {"with_san": True}}})
    config.model.depth_net.checkpoint_path = ""
    wrapper = ModelWrapper(config).cuda().eval()
    image = load_frame(os.path.join(src, "rgb0.png"), (H, W)).unsqueeze(0).cuda()
    raw = np.array(Image.open(os.path.join(src, "lidar0.png")), dtype=np.float32) / 256.0          # no return: 0 (the driver clamps the -1)
    lidar = resize_depth_preserve(torch.from_numpy(raw).cuda(), (H, W))
    edges = iee.annotate_frame(wrapper, image, lidar[None, None])["lidar"][0][0]
    want = np.clip(np.rint(edges.float().cpu().numpy().reshape(H, W) * 255.0), 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(save, "00000000_lidar_000.png"))), want)
    # the passes follow the configuration: without an input depth type only the RGB pass runs
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"model": LOSS, "datasets": {"augmentation": {"image_shape": [H, W]}}}, f)
    rgb_only = os.path.join(tmp_path, "rgb_only")
    iee.main(["--config", cfg_path, "--split", absolute, "--save", rgb_only])
    names = sorted(n for n in os.listdir(rgb_only) if n.endswith(".png"))
    assert names == ["%08d_regular_%03d.png" % (c, s) for c in range(2) for s in range(4)]
