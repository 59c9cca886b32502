"""CPU: the NumPy statement of the evaluation transforms (tests/eval_prep_ref.py) against the reference's own outputs
(tests/golden/eval_prep.npz, made by tests/golden/make_golden_eval_prep.py) and against hand-computed cases of the uint8 bilinear rule;
the evaluation loaders' sharding, the checkpoint policy and the configuration defaults (plain Python, no device)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_prep_ref as R                                     # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_prep.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", ["nocrop", "crop"])
def test_reference_statement_matches_the_reference(fx, case):
    """70 x 150 frame -> 64 x 128: borders, the cropped keys, LANCZOS rgb and resize_depth_preserve as the reference computed them"""
    from mindtheedge_amd.datasets.image_prep import parse_crop_borders
    crop = tuple(int(v) for v in fx[case + "_crop"])
    borders = tuple(int(v) for v in fx[case + "_borders"])
    assert fx["rgb"].shape == (70, 150, 3)
    assert tuple(R.parse_crop_borders_int(crop, (70, 150))) == borders
    assert tuple(parse_crop_borders(crop, (70, 150))) == borders
    assert (len(crop) > 0) == (case == "crop")
    sample = {"rgb": fx["rgb"], "input_depth": fx["input_depth"], "rgb_edge": fx["rgb_edge"],
              "depth": fx["input_depth"] * 2, "edge": fx["rgb_edge"][::-1].copy()}
    cropped = R._crop(sample, crop)
    assert tuple(cropped["rgb_edge"].shape) == tuple(fx[case + "_rgb_edge_cropped_shape"])
    assert int(cropped["rgb_edge"].astype(np.int64).sum()) == int(fx[case + "_rgb_edge_cropped_sum"])
    assert cropped["depth"].shape == (70, 150) and cropped["edge"].shape == (70, 150)       # supervision keeps its frame
    got = R.validation_sample(sample, crop)
    assert R.eval_shape(cropped["rgb"].shape[:2]) == (64, 128)
    np.testing.assert_array_equal(got["rgb"], fx[case + "_rgb_out"].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    np.testing.assert_array_equal(got["input_depth"][0], fx[case + "_input_depth_out"])
    np.testing.assert_array_equal(got["depth"][0], sample["depth"])
    assert got["edge"].shape == (1, 64, 128) and got["rgb_edge"].shape == (1, 64, 128)
    t = R.test_sample(sample, (64, 128), crop)
    np.testing.assert_array_equal(t["rgb"], got["rgb"])
    assert t["input_depth"].shape == (1, 64, 128) and t["depth"].shape == (1, 70, 150)
    t0 = R.test_sample(sample, (), crop)
    assert t0["rgb"].shape[1:] == cropped["rgb"].shape[:2] and t0["input_depth"].shape[1:] == cropped["rgb"].shape[:2]


def test_dataset_prefix_matches_the_reference(fx):
    cases = json.loads(str(fx["prefix_cases"]))
    assert len(cases) >= 3
    for c in cases:
        s = c["section"]
        for i, want in enumerate(c["prefix"]):
            assert R.dataset_prefix(s["path"][i], s["split"][i], s["depth_type"][i], s["cameras"][i]) == want


def test_wrapper_prefix_matches_the_reference(fx):
    """ModelWrapper.dataset_prefix without building a model"""
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    for c in json.loads(str(fx["prefix_cases"])):
        fake = type("W", (), {"config": load_config(None, {"datasets": {"validation": c["section"]}})})()
        for i, want in enumerate(c["prefix"]):
            assert ModelWrapper.dataset_prefix(fake, "validation", i) == want
    fake = type("W", (), {"config": load_config(None)})()
    assert ModelWrapper.dataset_prefix(fake, "validation", 0) is None and ModelWrapper.dataset_prefix(fake, "test", 0) is None


def test_u8_to_unit_float_is_totensor_for_every_byte():
    v = np.arange(256)
    np.testing.assert_array_equal((v.astype(np.float64) / 255.0).astype(np.float32), v.astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("shape", [(1, 1), (3, 9), (64, 128), (5, 7), (35, 75), (140, 300), (2, 300)])
def test_u8_bilinear_keeps_a_constant_255_map(shape):
    for src in [(70, 150), (7, 5), (1, 1), (1, 9), (9, 1)]:
        out = R.resize_linear_u8(np.full(src, 255, np.uint8), shape)
        assert out.shape == shape and out.dtype == np.uint8 and (out == 255).all(), (src, shape)


def test_u8_bilinear_hand_computed_cases():
    # a 1 x 1 source: every target pixel is that value
    for v in (0, 1, 77, 254):
        assert (R.resize_linear_u8(np.full((1, 1), v, np.uint8), (3, 5)) == v).all()
    # 2 x 2 -> 1 x 1 is exactly 2x in both axes: the area average (1 + 2 + 3 + 5 + 2) >> 2 = 3 (bilinear would give (1+2+3+5)/4 = 2.75 -> 3
    # as well, so a second map separates the two: (0 + 0 + 0 + 255 + 2) >> 2 = 64, bilinear rounds 63.75 through its own shifts)
    assert R.resize_linear_u8(np.array([[1, 2], [3, 5]], np.uint8), (1, 1)).tolist() == [[3]]
    assert R.resize_linear_u8(np.array([[0, 0], [0, 255]], np.uint8), (1, 1)).tolist() == [[64]]
    assert R.resize_linear_u8(np.array([[10, 20, 30, 40], [50, 60, 70, 80]], np.uint8), (1, 2)).tolist() == [[35, 55]]
    # 1 x 2 -> 1 x 4, by hand: fx = -0.25 (clamped), 0.25, 0.75, 1.25 (clamped) -> a1 = 0, 512, 1536, 0 with sx = 0, 0, 0, 1; b0 = 2048
    #   R = 0, 255*512 = 130560, 255*1536 = 391680, 255*2048 = 522240;  ((2048 * (R >> 4)) >> 16) = 0, 255, 765, 1020;  (+2) >> 2
    assert R.resize_linear_u8(np.array([[0, 255]], np.uint8), (1, 4)).tolist() == [[0, 64, 191, 255]]
    # 4 x 2 -> 2 x 2 is 2x in height only: the general branch, rows sampled at fy = 0.5 and 2.5 -> plain means of rows (0,1) and (2,3)
    src = np.array([[0, 8], [16, 24], [100, 108], [116, 124]], np.uint8)
    assert R.resize_linear_u8(src, (2, 2)).tolist() == [[8, 16], [108, 116]]


def test_nearest_hand_computed_cases():
    src = np.arange(12, dtype=np.float32).reshape(3, 4)
    np.testing.assert_array_equal(R.resize_nearest_f32(src, (3, 4)), src)
    np.testing.assert_array_equal(R.resize_nearest_f32(src, (6, 8)), np.repeat(np.repeat(src, 2, 0), 2, 1))
    np.testing.assert_array_equal(R.resize_nearest_f32(src, (1, 2)), np.array([[0, 2]], np.float32))       # floor(dx * 2)
    np.testing.assert_array_equal(R.resize_nearest_f32(src, (2, 3)), src[[0, 1]][:, [0, 1, 2]])             # floor(d * 1.5), floor(d * 4/3)


@pytest.mark.parametrize("n", [0, 1, 3, 8])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharding_sees_every_frame_once_in_order(n, world):
    from mindtheedge_amd.datasets.kitti_edges import EvalLoader, shard_indices
    shares = [shard_indices(n, r, world) for r in range(world)]
    assert sorted(i for s in shares for i in s) == list(range(n))                      # every frame exactly once, nothing padded
    assert all(s == sorted(s) for s in shares)
    assert shares == [R.shard(n, r, world) for r in range(world)]

    class Frames:
        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"idx": i}
    for bs in (1, 2):
        seen = [[i for b in EvalLoader(Frames(), bs, r, world) for i in b["idx"]] for r in range(world)]
        assert seen == shares                                                            # file order, ragged tail kept
        assert [len(EvalLoader(Frames(), bs, r, world)) for r in range(world)] == [(len(s) + bs - 1) // bs for s in shares]


def test_eval_loader_names_the_two_shapes_of_a_mixed_batch():
    import torch
    from mindtheedge_amd.datasets.kitti_edges import EvalLoader

    class Frames:
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return {"idx": i, "rgb": torch.zeros(3, 64, 128 + 32 * i)}
    assert len(list(EvalLoader(Frames(), 1))) == 2
    with pytest.raises(ValueError) as e:
        list(EvalLoader(Frames(), 2))
    assert "(3, 64, 128)" in str(e.value) and "(3, 64, 160)" in str(e.value)


def test_make_eval_loaders_without_a_split_are_empty():
    from mindtheedge_amd.datasets.kitti_edges import make_test_loaders, make_val_loaders
    from mindtheedge_amd.utils.config import load_config
    cfg = load_config(None)
    assert make_val_loaders(cfg, 0, 1) == [] and make_test_loaders(cfg, 0, 1) == []


def test_config_defaults():
    from mindtheedge_amd.utils.config import default_config, load_config
    for cfg in (default_config(), load_config(None)):
        for mode in ("validation", "test"):
            sec = cfg.datasets[mode]
            assert sec.batch_size == 1 and sec.dataset == [] and sec.path == [] and sec.split == []
            assert sec.depth_type == [""] and sec.input_depth_type == [""] and sec.cameras == [[]]
        assert cfg.datasets.validation.gt_crop == []
        assert tuple(cfg.datasets.augmentation.crop_eval_borders) == ()
        assert cfg.checkpoint.monitor == "loss" and cfg.checkpoint.monitor_index == 0 and cfg.checkpoint.mode == "auto"
        assert cfg.checkpoint.save_top_k == -1 and cfg.checkpoint.filepath == ""
        assert cfg.datasets.test.is_infer_rgb is True and cfg.datasets.train.batch_size == 8 and cfg.arch.validate_first is False
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    val = load_config(os.path.join(root, "configs", "train_packnet_san_kitti_with_edges_val.yaml"))
    assert len(val.datasets.validation.split) == 1 and val.checkpoint.monitor == "abs_rel_pp_gt" and val.checkpoint.save_top_k != -1


# ---- checkpoint policy -----------------------------------------------------------------------------------------------------------------

class _FakeWrapper:
    def __init__(self, prefix="KITTI_raw-val-groundtruth"):
        self.current_epoch, self.prefix = 0, prefix

    def dataset_prefix(self, mode, idx=0):
        return self.prefix


def _run_policy(tmp_path, monkeypatch, values, monitor="abs_rel_pp_gt", **kw):
    from mindtheedge_amd.models import model_checkpoint as mc

    def fake_save(path, wrapper):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").close()
        return path
    monkeypatch.setattr(mc, "save_checkpoint", fake_save)
    run = os.path.join(str(tmp_path), "run")
    policy = mc.CheckpointPolicy(run, monitor=monitor, **kw)
    w = _FakeWrapper()
    for epoch, v in enumerate(values):
        w.current_epoch = epoch
        policy.save(w, None if v is None else [{"%s-%s" % (w.prefix, monitor): v, "%s-rmse" % w.prefix: 1.0}])
    return sorted(os.listdir(run)), policy


VALUES = [0.30, 0.10, 0.20, 0.05, 0.40]


def test_policy_auto_rule():
    from mindtheedge_amd.models.model_checkpoint import monitor_mode
    assert monitor_mode("abs_rel_pp_gt") == "min" and monitor_mode("a1_pp_gt") == "max" and monitor_mode("acc") == "max"
    assert monitor_mode("fmeasure_x") == "max" and monitor_mode("loss") == "min" and monitor_mode("rmse", "auto") == "min"
    assert monitor_mode("a1_pp_gt", "min") == "min" and monitor_mode("abs_rel_pp_gt", "max") == "max"
    with pytest.raises(ValueError):
        monitor_mode("loss", "best")


def test_policy_minus_one_and_no_metrics_write_one_file_per_epoch(tmp_path, monkeypatch):
    every = ["epoch=%d.ckpt" % i for i in range(5)]
    files, _ = _run_policy(tmp_path / "a", monkeypatch, VALUES, save_top_k=-1)
    assert files == every
    files, _ = _run_policy(tmp_path / "b", monkeypatch, [None] * 5, save_top_k=2)          # no validation: as without a policy
    assert files == every


@pytest.mark.parametrize("mode", ["min", "max", "auto"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_policy_keeps_the_best_k(tmp_path, monkeypatch, k, mode):
    files, policy = _run_policy(tmp_path, monkeypatch, VALUES, save_top_k=k, mode=mode)
    name = lambda e: "epoch=%d_abs_rel_pp_gt=%.3f.ckpt" % (e, VALUES[e])
    smaller_is_better = mode in ("min", "auto")                                              # auto on abs_rel_pp_gt is min
    assert policy.mode == ("min" if smaller_is_better else "max")
    order = sorted(range(5), key=lambda e: VALUES[e], reverse=not smaller_is_better)
    want = sorted(name(e) for e in (range(5) if k == 0 else order[:k]))
    assert files == want
    assert sorted(os.path.basename(p) for p in policy.best_k) == want


def test_policy_auto_is_max_for_a1(tmp_path, monkeypatch):
    files, policy = _run_policy(tmp_path, monkeypatch, [0.5, 0.9, 0.7], monitor="a1_pp_gt", save_top_k=1, mode="auto")
    assert policy.mode == "max" and files == ["epoch=1_a1_pp_gt=0.900.ckpt"]


def test_policy_unknown_monitor_is_an_error(tmp_path, monkeypatch):
    from mindtheedge_amd.models import model_checkpoint as mc
    policy = mc.CheckpointPolicy(str(tmp_path), monitor="nope", save_top_k=1)
    with pytest.raises(KeyError):
        policy.save(_FakeWrapper(), [{"KITTI_raw-val-groundtruth-abs_rel": 0.1}])
