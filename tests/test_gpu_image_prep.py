"""GPU (-m gpu): training-image preparation on device (csrc/image_prep.hip) -- crop + LANCZOS resample, colour jitter + ToTensor --
against the fixtures produced by the reference (tests/golden/make_golden_image_prep.py), against PIL at test time and against the numpy
restatement (tests/image_prep_ref.py, pinned to PIL by tests/test_image_prep_cpu.py).  Every comparison is bit equality."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import image_prep_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.npz")
KITTI_SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241), (370, 1224)]


def _resize(img, shape, crop=None, two_pass=False):
    from mindtheedge_amd.datasets.image_prep import resize_image_u8
    return resize_image_u8(torch.from_numpy(img).cuda(), shape, crop=crop, two_pass=two_pass).cpu().numpy()


def _pil(img, shape, crop=None):
    p = Image.fromarray(img)
    if crop is not None:
        p = p.crop(crop)
    return np.asarray(p.resize((shape[1], shape[0]), Image.LANCZOS))


def _jitter(batch, params, want_original=False):
    from mindtheedge_amd.datasets.image_prep import color_jitter_to_tensor
    out = color_jitter_to_tensor(torch.from_numpy(batch).cuda(), params, want_original=want_original)
    return tuple(t.cpu().numpy() for t in out) if want_original else out.cpu().numpy()


def _want(img, p):
    return R.to_tensor(img if p is None else R.color_jitter(img, p["factors"], p["order"]))


def test_fixtures_through_the_c_abi():
    z = np.load(GOLDEN)
    for name in ("rand", "smooth", "mixed", "skip"):
        shape = tuple(int(v) for v in z["resize_%s_shape" % name])
        for two_pass in (False, True):
            np.testing.assert_array_equal(_resize(z["resize_%s_in" % name], shape, two_pass=two_pass), z["resize_%s_out" % name])
    for i in range(3):
        b = tuple(int(v) for v in z["crop%d_borders" % i])
        np.testing.assert_array_equal(_resize(z["resize_rand_in"], (64, 192), crop=b), z["crop%d_rgb_resized" % i])
    for i, k in enumerate(int(v) for v in z["jitter_seeds"]):
        p = {"factors": tuple(z["jitter_factors"][i]), "order": tuple(int(v) for v in z["jitter_orders"][i])}
        for name in ("rand", "smooth"):
            got = _jitter(z["jitter_%s_in" % name][None], [p])
            np.testing.assert_array_equal(got[0], R.to_tensor(z["jitter_%s_seed%d" % (name, k)]))
        if k < 4:
            np.testing.assert_array_equal(_jitter(z["jitter_rand_in"][None], [p])[0], z["jitter_rand_seed%d_tensor" % k])
    for name in ("rand", "smooth"):
        np.testing.assert_array_equal(_jitter(z["jitter_%s_in" % name][None], None)[0], z["jitter_%s_tensor" % name])


@pytest.mark.parametrize("size", KITTI_SIZES)
def test_kitti_sizes_against_pil(size):
    img = np.random.default_rng(size[1]).integers(0, 256, size + (3,), dtype=np.uint8)
    img[100:200, 300:600] = (np.arange(300)[None, :, None] * 255 // 299 + np.arange(100)[:, None, None]) % 256      # a smooth patch
    for shape in ((384, 1280), (192, 640)):
        np.testing.assert_array_equal(_resize(img, shape), _pil(img, shape))


def test_downscales_fused_and_two_launch_forms_against_pil():
    from mindtheedge_amd import kernels as K
    img = np.random.default_rng(1).integers(0, 256, (384, 1280, 3), dtype=np.uint8)
    want = _pil(img, (192, 640))
    assert K.lib.mte_image_resample_work_bytes(384, 1280, 192, 640, 0) == 0                  # 2x fits the LDS budget: one launch ...
    np.testing.assert_array_equal(_resize(img, (192, 640)), want)
    assert K.lib.mte_image_resample_work_bytes(384, 1280, 192, 640, 1) == 384 * 640 * 3
    np.testing.assert_array_equal(_resize(img, (192, 640), two_pass=True), want)              # ... and the two-launch form gives the same bytes
    # 12x: the tap span of a tile no longer fits, the library takes the two-launch form by itself
    assert K.lib.mte_image_resample_work_bytes(384, 1280, 32, 106, 0) == 384 * 106 * 3
    np.testing.assert_array_equal(_resize(img, (32, 106)), _pil(img, (32, 106)))
    # 6x down: still one launch, with the staged rows split into several chunks
    assert K.lib.mte_image_resample_work_bytes(384, 1280, 64, 213, 0) == 0
    np.testing.assert_array_equal(_resize(img, (64, 213)), _pil(img, (64, 213)))
    # up-scaling 3x
    small = img[:50, :70].copy()
    np.testing.assert_array_equal(_resize(small, (150, 210)), _pil(small, (150, 210)))


def test_crop_window_and_ragged_shapes_against_pil():
    g = np.random.default_rng(2)
    img = g.integers(0, 256, (375, 1242, 3), dtype=np.uint8)
    for crop in ((13, 23, 1229, 375), (1, 0, 1242, 352), (601, 100, 700, 163)):
        for two_pass in (False, True):
            np.testing.assert_array_equal(_resize(img, (384, 1280), crop=crop, two_pass=two_pass), _pil(img, (384, 1280), crop))
    np.testing.assert_array_equal(_resize(img, (375, 1242), crop=(5, 7, 1005, 307)), _pil(img, (375, 1242), (5, 7, 1005, 307)))
    for src, dst in [((1, 1), (5, 4)), ((1, 1), (1, 1)), ((40, 7), (13, 3)), ((9, 7), (17, 65)), ((33, 130), (17, 67)), ((64, 64), (64, 100)),
                     ((64, 64), (100, 64)), ((3, 500), (16, 129))]:
        a = g.integers(0, 256, src + (3,), dtype=np.uint8)
        for two_pass in (False, True):
            np.testing.assert_array_equal(_resize(a, dst, two_pass=two_pass), _pil(a, dst))
    with pytest.raises(ValueError):
        _resize(img, (384, 1280), crop=(0, 0, 1243, 375))


def _eight_params():
    orders = [(0, 1, 2, 3), (1, 0, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1), (0, 2, 3, 1), (3, 1, 0, 2), (2, 0, 1, 3), (1, 3, 2, 0)]
    rng = random.Random(11)
    return [{"factors": (rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.05, 0.05)), "order": o}
            for o in orders]


def _frames(B, H, W, seed):
    g = np.random.default_rng(seed)
    batch = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[:H, :W]
    for b in range(0, B, 2):                                                  # every other frame is smooth (saturated and dark regions)
        for c in range(3):
            batch[b, :, :, c] = np.clip(140 + 130 * np.sin(x / (20.0 + 7 * c + b) + y / (11.0 + 3 * b)), 0, 255)
    return batch


def test_jitter_batch_of_eight_at_kitti_size():
    batch, params = _frames(8, 384, 1280, 5), _eight_params()
    got, orig = _jitter(batch, params, want_original=True)
    for b in range(8):
        np.testing.assert_array_equal(got[b], _want(batch[b], params[b]))
        np.testing.assert_array_equal(orig[b], R.to_tensor(batch[b]))
    # determinism, and independence of the position in the batch
    again = _jitter(batch, params)
    np.testing.assert_array_equal(again, got)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    moved = _jitter(batch[perm], [params[i] for i in perm])
    np.testing.assert_array_equal(moved, got[perm])
    single = _jitter(batch[3:4], [params[3]])
    np.testing.assert_array_equal(single[0], got[3])
    # samples that are left alone beside jittered ones; no parameters at all = plain ToTensor
    mixed = _jitter(batch[:3], [params[0], None, params[2]])
    np.testing.assert_array_equal(mixed[1], R.to_tensor(batch[1]))
    np.testing.assert_array_equal(mixed[2], got[2])
    np.testing.assert_array_equal(_jitter(batch[:2], None), np.stack([R.to_tensor(batch[0]), R.to_tensor(batch[1])]))


def test_jitter_range_ends_constant_and_black_images():
    batch = _frames(2, 96, 320, 6)
    cases = []
    for f in (0.8, 1.2, 1.0, 0.0, 1.7):
        for hue in (0.0, 0.05, -0.05, 0.5, -0.5):
            cases.append({"factors": (f, f, f, hue), "order": (0, 1, 2, 3)})
            cases.append({"factors": (f, 2.0 - f if f <= 2 else 1.0, f, hue), "order": (3, 2, 1, 0)})
    for p in cases:
        got = _jitter(batch, [p, p])
        for b in range(2):
            np.testing.assert_array_equal(got[b], _want(batch[b], p), err_msg=str(p))
    special = np.zeros((3, 61, 67, 3), dtype=np.uint8)                         # all black (maxc == 0), constant grey, constant colour; odd pixel count
    special[1] = 77
    special[2] = (200, 10, 90)
    for p in _eight_params():
        got = _jitter(special, [p] * 3)
        for b in range(3):
            np.testing.assert_array_equal(got[b], _want(special[b], p), err_msg=str(p))
    # single operations and partial orders
    for order in ((1,), (3,), (2, 1), ()):
        p = {"factors": (1.13, 0.87, 1.19, -0.031), "order": order}
        np.testing.assert_array_equal(_jitter(batch[:1], [p])[0], _want(batch[0], p))
    with pytest.raises(ValueError):
        _jitter(batch[:1], [{"factors": (1, 1, 1, 0), "order": (1, 1)}])


def _write_split(tmp_path, H, W, n=3):
    g = np.random.default_rng(0)
    lines = []
    for i in range(n):
        Image.fromarray((g.random((H + 10, W + 20, 3)) * 255).astype(np.uint8)).save(os.path.join(tmp_path, "rgb%d.png" % i))
        depth = ((g.random((H + 10, W + 20)) < 0.1) * (1 + 79 * g.random((H + 10, W + 20))) * 256).astype(np.uint16)
        depth[0, 0] = 600
        Image.fromarray(depth).save(os.path.join(tmp_path, "depth%d.png" % i))
        os.makedirs(os.path.join(tmp_path, "normals"), exist_ok=True)
        for s in range(4):
            hs, ws = ((H + 10, W + 20) if s == 0 else (H >> s, W >> s))
            Image.fromarray(((g.random((hs, ws)) < 0.05) * 255).astype(np.uint8)).save(os.path.join(tmp_path, "%08d_lidar_00%d.png" % (i, s)))
            Image.fromarray(g.integers(0, 256, (hs, ws), dtype=np.uint8)).save(os.path.join(tmp_path, "normals", "%08d_lidar_00%d.png" % (i, s)))
        lines.append("rgb%d.png depth%d.png %08d_lidar_000.png depth%d.png None None None normals/%08d_lidar_000.png\n" % (i, i, i, i, i))
    split = os.path.join(tmp_path, "split.txt")
    open(split, "w").writelines(lines)
    return split


def test_split_dataset_defaults_jitter_and_crop(tmp_path):
    from oracle import data_oracle as do
    from mindtheedge_amd.datasets.image_prep import draw_color_jitter, parse_crop_borders
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, SplitLoader, make_loader
    H, W = 64, 128
    split = _write_split(tmp_path, H, W)
    frame = lambda i: Image.open(os.path.join(tmp_path, "rgb%d.png" % i)).convert("RGB")
    # defaults: the PIL path
    ds = KittiEdgeSplitDataset(split, (H, W), root=str(tmp_path))
    for i in range(3):
        s = ds[i]
        want = (np.asarray(frame(i).resize((W, H), Image.LANCZOS)) / 255).astype(np.float32).transpose(2, 0, 1)
        np.testing.assert_array_equal(s["rgb"].cpu().numpy(), want)
        assert "rgb_original" not in s and s["rgb"].is_contiguous()
    # jitter: the PIL pipeline with the same draws
    dsj = KittiEdgeSplitDataset(split, (H, W), root=str(tmp_path), jittering=(0.2, 0.2, 0.2, 0.05))
    for k in (0, 3, 8):
        random.seed(k)
        got = [dsj[i] for i in range(3)]
        random.seed(k)
        for i in range(3):
            p = draw_color_jitter((0.2, 0.2, 0.2, 0.05))
            resized = np.asarray(frame(i).resize((W, H), Image.LANCZOS))
            np.testing.assert_array_equal(got[i]["rgb"].cpu().numpy(), R.to_tensor(R.color_jitter(resized, p["factors"], p["order"])))
            np.testing.assert_array_equal(got[i]["rgb_original"].cpu().numpy(), R.to_tensor(resized))
    # crop: crop_sample (rgb through PIL's crop, maps by slicing) + the resizes
    crop = (4, 60, -110, 0)
    dsc = KittiEdgeSplitDataset(split, (H, W), root=str(tmp_path), crop_train_borders=crop)
    b = parse_crop_borders(crop, (H + 10, W + 20))
    assert b == (W + 20 - 110, 4, W + 20, 64)
    s = dsc[1]
    want = (np.asarray(frame(1).crop(b).resize((W, H), Image.LANCZOS)) / 255).astype(np.float32).transpose(2, 0, 1)
    np.testing.assert_array_equal(s["rgb"].cpu().numpy(), want)
    d_png = np.array(Image.open(os.path.join(tmp_path, "depth1.png")), dtype=int)
    d = np.where(d_png == 0, -1.0, d_png / 256.0).astype(np.float32)[b[1]:b[3], b[0]:b[2]]
    np.testing.assert_array_equal(s["depth"][0].cpu().numpy(), do.resize_depth_preserve(d, (H, W)).astype(np.float32))
    e = np.array(Image.open(os.path.join(tmp_path, "00000001_lidar_000.png")))[b[1]:b[3], b[0]:b[2]]
    want_e = do.resize_depth_preserve(e.astype(np.float32), (H, W))
    np.testing.assert_array_equal(s["edge"][0].cpu().numpy(), (want_e / 255.0 if want_e.max() > 1 else want_e).astype(np.float32))
    e1 = np.array(Image.open(os.path.join(tmp_path, "00000001_lidar_001.png")))           # coarser scales are not cropped by crop_sample
    np.testing.assert_array_equal(s["edge_1"][0].cpu().numpy(), (e1 / 255.0).astype(np.float32))
    # normal: sliced like crop_depth, de-quantised, then the (existing, parity-unpinned) bilinear device resize to the target shape
    from mindtheedge_amd.datasets.kitti_edges import normal_target
    from mindtheedge_amd.utils.edge import resize_linear
    n_png = np.array(Image.open(os.path.join(tmp_path, "normals", "00000001_lidar_000.png")))
    assert n_png.shape == (H + 10, W + 20)
    n_crop = np.ascontiguousarray(n_png[b[1]:b[3], b[0]:b[2]])
    assert n_crop.shape == (b[3] - b[1], b[2] - b[0]) == (60, 110)
    want_n = resize_linear(normal_target(torch.from_numpy(n_crop).cuda()), (H, W))
    np.testing.assert_array_equal(s["normal"][0].cpu().numpy(), want_n.cpu().numpy())
    assert s["normal_1"].shape == (1, H // 2, W // 2)
    # a window of exactly the target size: no resize anywhere, every map is the slice itself
    crop2 = (4, H, 10, W)
    b2 = parse_crop_borders(crop2, (H + 10, W + 20))
    assert b2 == (10, 4, 10 + W, 4 + H)
    s2 = KittiEdgeSplitDataset(split, (H, W), root=str(tmp_path), crop_train_borders=crop2)[2]
    np.testing.assert_array_equal(s2["rgb"].cpu().numpy(), R.to_tensor(np.asarray(frame(2).crop(b2))))
    n2 = np.array(Image.open(os.path.join(tmp_path, "normals", "00000002_lidar_000.png")))[b2[1]:b2[3], b2[0]:b2[2]]
    np.testing.assert_array_equal(s2["normal"][0].cpu().numpy(), do.normal_from_u8(n2).astype(np.float32))
    e2 = np.array(Image.open(os.path.join(tmp_path, "00000002_lidar_000.png")))[b2[1]:b2[3], b2[0]:b2[2]]
    np.testing.assert_array_equal(s2["edge"][0].cpu().numpy(), (e2 / 255.0).astype(np.float32))
    # make_loader honours the two config keys; a training step on a jittered batch is finite
    from mindtheedge_amd.utils.config import load_config
    cfg = load_config(None, {"datasets": {"augmentation": {"image_shape": (H, W), "jittering": [0.2, 0.2, 0.2, 0.05], "crop_train_borders": list(crop)},
                                          "train": {"batch_size": 2, "split": [split], "path": [str(tmp_path)]}}})
    loader = make_loader(cfg, 0, 1)
    assert loader.ds.jittering == (0.2, 0.2, 0.2, 0.05) and loader.ds.crop_train_borders == crop
    off = make_loader(load_config(None, {"datasets": {"augmentation": {"image_shape": (H, W)},
                                                      "train": {"batch_size": 2, "split": [split], "path": [str(tmp_path)]}}}), 0, 1)
    assert off.ds.jittering == () and off.ds.crop_train_borders == ()
    loader.shuffle = False
    random.seed(1)
    batch = next(iter(loader))
    assert batch["rgb"].shape == (2, 3, H, W) and batch["rgb_original"].shape == (2, 3, H, W)
    assert not torch.equal(batch["rgb"], batch["rgb_original"])
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    K.set_compute_dtype("bf16")
    mcfg = load_config(None, {"model": {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                                                   "edges_depth_edge_loss_all_scales": True, "flip_lr_prob": 0.0}}})
    wrap = ModelWrapper(mcfg).cuda().train()
    out = wrap.training_step(batch)
    assert torch.isfinite(out["loss"]).all()
    out["loss"].sum().backward()
