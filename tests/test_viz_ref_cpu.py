"""CPU: tests/viz_ref.py (the numpy statements the kernels of csrc/depth_viz.hip are held against) and the host arithmetic of
mindtheedge_amd/utils/depth.py against what the reference recorded (tests/golden/viz.npz, make_golden_viz.py), against np.percentile
itself and against matplotlib's tables; the C ABI of the new entry points, the ``save`` defaults and the split-line parsing of
infer_edges.py --split."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viz_ref                                      # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "viz.npz"))
VIZ_ENTRY_POINTS = {"mte_order_stats_work_bytes", "mte_order_stats_f32", "mte_colormap_u8", "mte_d3r_count"}
VIZ_KW = {"default": {}, "norm": {"normalizer": 0.3}, "fz": {"filter_zeros": True}, "spectral": {"colormap": "Spectral"}, "p50": {"q": 50}}


def as_written(float_image):
    """what cv2.imwrite stores for the reference's float image * 255 (round half to even, saturating)"""
    return np.clip(np.rint(float_image * 255), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("frame", ["a", "b"])
@pytest.mark.parametrize("case", sorted(VIZ_KW))
def test_viz_inv_depth_statement_equals_the_reference(frame, case):
    got = viz_ref.viz_inv_depth(Z["viz_%s_inv" % frame], **VIZ_KW[case])
    assert np.array_equal(got, as_written(Z["viz_%s_%s" % (frame, case)]))


@pytest.mark.parametrize("frame", ["a", "b"])
def test_log_colouring_statement_equals_the_reference_outside_the_guard_band(frame):
    """The statement takes the log in double and rounds once, numpy's float32 log may differ from that in the last place: pixels whose exact
    x * 256 lies within the band of an integer may differ by one index (the band: three ulps of log(v) at the largest |log v| of the frame,
    scaled by 256 / hi -- the derivation is in test_gpu_depth_viz.py), all others are equal."""
    depth = Z["log_%s_depth" % frame]
    got, exact, idx = viz_ref.log_color(depth)
    band = log_band(depth)
    near = np.abs(exact - np.rint(exact)) < band
    assert near.sum() <= max(2, 0.01 * near.size)         # the frame's minimum and maximum sit on the boundaries 0 and 256 by construction
    assert np.array_equal(got[~near], Z["log_%s_color" % frame][~near])
    assert viz_ref.within_one_index(Z["log_%s_color" % frame], idx, viz_ref.table("Spectral", "trunc"))[near].all()


def log_band(depth):
    logs = np.log(depth.astype(np.float64))
    hi = logs.max() - logs.min()
    return 3 * float(np.spacing(np.float32(np.abs(logs).max()))) * 256 / hi


def test_d3r_statement_equals_the_reference():
    assert viz_ref.d3r_count(Z["d3r_gt"], Z["d3r_pred"], Z["d3r_pairs"]) == int(Z["d3r_agree"].sum())
    for i in range(0, len(Z["d3r_pairs"]), 37):                                           # and pair by pair
        assert viz_ref.d3r_count(Z["d3r_gt"], Z["d3r_pred"], Z["d3r_pairs"][i:i + 1]) == int(Z["d3r_agree"][i])


def random_percentile_cases(count, seed=0):
    rs = np.random.RandomState(seed)
    for _ in range(count):
        n = int(rs.choice([1, 2, 3, 5, 17, 100, 1920, rs.randint(1, 4000)]))
        a = (rs.rand(n) * rs.choice([1e-3, 1.0, 80.0])).astype(np.float32)
        if rs.rand() < 0.2:
            a = np.round(a, 1)                                                            # ties
        if rs.rand() < 0.2:
            a[rs.rand(n) < 0.5] = 0
        q = [95, 100, 0, 50, 95.0, float(rs.rand() * 100)][rs.randint(6)]
        yield a, q


def test_host_interpolation_equals_np_percentile_bit_for_bit():
    from mindtheedge_amd.utils.depth import percentile_lerp, percentile_position
    for a, q in random_percentile_cases(12000):
        ref = np.percentile(a, q)
        assert ref.dtype == np.float32
        s = np.sort(a)
        k, gamma = percentile_position(len(a), q)
        got = percentile_lerp(s[k], s[min(k + 1, len(a) - 1)], gamma)
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), (len(a), q, ref, got)
        assert viz_ref.percentile(a, q).tobytes() == ref.tobytes()
    big = np.float32(0.5) + np.arange(96 * 320, dtype=np.float32)                         # a virtual index past float32's integer range of halves
    k, gamma = percentile_position(len(big), 95)
    assert percentile_lerp(big[k], big[k + 1], gamma).tobytes() == np.percentile(big, 95).tobytes()


def test_positive_only_pick_is_the_percentile_of_the_positive_values():
    for a, q in random_percentile_cases(300, seed=1):
        if (a > 0).any():
            assert viz_ref.percentile(a, q, positive_only=True).tobytes() == np.percentile(a[a > 0], q).tobytes()


def test_index_rule_equals_matplotlib_and_tables_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.rand(20000).astype(np.float32), np.float32([0, 1, 0.999999, 0.5, 1 / 256, 255 / 256, -0.1, 1.7]),
                        (np.arange(257) / 256).astype(np.float32)])
    for name in ("plasma", "Spectral"):
        cm, t = matplotlib.colormaps[name], viz_ref.float_table(name)
        assert t.shape == (256, 3) and np.array_equal(t, np.asarray(cm(np.arange(256)))[:, :3])
        assert np.array_equal(t[viz_ref.color_index(x)], cm(np.clip(x, 0, 1))[:, :3])


def test_color_tables_of_the_package_follow_their_callers_rule():
    from mindtheedge_amd.utils.depth import color_table
    for name in ("plasma", "Spectral"):
        for rule in ("rint", "trunc"):
            t = color_table(name, rule)
            assert t.dtype == np.uint8 and t.shape == (256, 3) and np.array_equal(t, viz_ref.table(name, rule))
    assert (color_table("plasma", "rint") != color_table("plasma", "trunc")).any()
    with pytest.raises(ValueError):
        color_table("viridis", "rint")


def test_divisor_and_log_range_dtypes():
    from mindtheedge_amd.utils.depth import log_color_range, viz_divisor
    p = np.float32(0.31234567)
    assert viz_divisor(p).tobytes() == np.float32(p + np.float32(1e-6)).tobytes()           # np.percentile's float32 result: a float32 sum
    assert viz_divisor(0.3).tobytes() == np.float32(0.3 + 1e-6).tobytes()                   # a Python float: the double sum, rounded
    depth = Z["log_a_depth"]
    lo, hi = log_color_range(depth.min(), depth.max())
    logs = np.log(depth.astype(np.float64)).astype(np.float32)
    assert lo.tobytes() == logs.min().tobytes() and hi.tobytes() == np.float32(logs.max() - logs.min()).tobytes()


def test_viz_entry_points_are_declared_built_and_exported():
    from mindtheedge_amd import _build, _lib
    assert "depth_viz.hip" in _build.SOURCES
    protos = _lib.parse_header()
    assert VIZ_ENTRY_POINTS <= set(protos)
    assert _lib.RETURNS["mte_order_stats_work_bytes"].__name__ == "c_long" and "mte_order_stats_work_bytes" in _lib.QUERIES
    assert [a for _, a in protos["mte_order_stats_f32"]] == ["x", "stride", "B", "n", "k", "positive_only", "out", "count_out", "work", "stream"]
    assert [a for _, a in protos["mte_colormap_u8"]] == ["x", "B", "H", "W", "divisor", "lo_hi", "table", "out", "stream"]
    assert [a for _, a in protos["mte_d3r_count"]] == ["gt", "pred", "H", "W", "index_work", "n", "pairs", "P", "count", "stream"]
    for lib in (_build.build(), _build.DEV_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T mte_" in l}
        assert VIZ_ENTRY_POINTS <= exported, (lib, VIZ_ENTRY_POINTS - exported)


def test_save_defaults():
    from mindtheedge_amd.utils.config import default_config, load_config
    for cfg in (default_config(), load_config()):
        assert cfg.save.folder == "" and cfg.save.pretrained == ""
        assert dict(cfg.save.depth) == {"rgb": True, "viz": True, "npz": True, "png": True, "multiscale": False}
    assert not (default_config().save or {}).get("folder")                                 # infer_edges.py's test stays falsy
    assert load_config(overrides={"save": {"folder": "/x"}}).save.depth.viz is True


def test_save_depth_without_a_folder_touches_nothing(tmp_path):
    from mindtheedge_amd.utils.config import default_config
    from mindtheedge_amd.utils.save import prepare_dataset_prefix, save_depth, save_paths_list
    cfg = default_config()
    assert save_depth({}, {}, (), cfg.datasets.test, cfg.save) is None                      # no key of batch / output is read
    cfg.datasets.test.update(path=["/data/KITTI_tiny"], split=["splits/test_files.txt"], depth_type=["velodyne"], cameras=[["camera_0"]])
    assert prepare_dataset_prefix(cfg.datasets.test, 0) == "KITTI_tiny-test_files-velodyne-camera_0"
    save_paths_list(["a", "b"], str(tmp_path), "l.txt")
    assert open(os.path.join(tmp_path, "l.txt")).read() == "a\nb\n"


def test_split_line_parsing_and_kitti_bin_refusal(tmp_path):
    sys.path.insert(0, ROOT)
    import infer_edges as ie
    assert ie.parse_split_columns("img/0.png d/0.png e/0_000.png lidar/0.npz n/0_000.png re/0.png x y\n") == ("img/0.png", "lidar/0.npz")
    with pytest.raises(ValueError):
        ie.parse_split_columns("img/0.png d/0.png\n")
    split = os.path.join(tmp_path, "s.txt")
    with open(split, "w") as f:
        f.write("a.png b c l0.png\n\nb.png b c l1.bin\n")
    assert ie.read_split_columns(split) == [("a.png", "l0.png"), ("b.png", "l1.bin")]
    with pytest.raises(ValueError, match="291-299"):
        ie.check_split_lidar("l1.bin", "KITTI")
    ie.check_split_lidar("l1.bin", "GTA")
    ie.check_split_lidar("l0.png", "KITTI")


def test_split_frame_is_the_pil_pipeline_with_the_reference_crop(tmp_path):
    sys.path.insert(0, ROOT)
    import infer_edges as ie
    from PIL import Image
    rs = np.random.RandomState(3)
    path = os.path.join(tmp_path, "f.png")
    Image.fromarray(rs.randint(0, 256, size=(70, 110, 3)).astype(np.uint8)).save(path)
    plain = ie.load_frame(path, (64, 96))
    assert np.array_equal(ie.load_split_frame(path, (64, 96)).numpy(), plain.numpy())
    crop = ie.load_split_frame(path, (64, 96), (32, 64))
    assert crop.shape == (3, 32, 64) and np.array_equal(crop.numpy(), plain.numpy()[:, 32:, 16:80])


def test_ordinal_ladder_and_ground_truth_read(tmp_path):
    from PIL import Image
    from mindtheedge_amd.utils.depth_analysis import ord_pair_count, read_ord_gt
    assert [ord_pair_count(n) for n in (10000, 9999, 5000, 4999, 2000, 1999, 1000, 999, 200)] == [5000, 2500, 2500, 1000, 1000, 500, 500, 100, 100]
    with pytest.raises(ValueError):
        ord_pair_count(199)
    g16 = Z["ord_gt_0"]
    path = os.path.join(tmp_path, "g.png")
    Image.fromarray(g16).save(path)
    assert np.array_equal(read_ord_gt(path), (g16 >> 8).astype(np.uint8))
