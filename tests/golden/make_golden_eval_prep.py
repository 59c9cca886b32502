"""Generates tests/golden/eval_prep.npz from the upstream reference (development container only): the parts of ``validation_transforms``
(packnet_code/packnet_sfm/datasets/transforms.py:53-97) that run without OpenCV -- ``parse_crop_borders``, ``crop_sample_input``,
``resize_image`` and ``resize_depth_preserve`` -- on one 70 x 150 frame, once with ``crop_eval_borders`` and once without, and
``prepare_dataset_prefix`` (utils/logging.py:35-63) on a few dataset sections.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval_prep.py

torchvision is not installed there: ``transforms.Resize`` is the PIL stub of make_golden_image_prep.py.  The two cv2.resize calls of the
transform are not in the fixture (cv2 is not available): the uint8 bilinear and the nearest resize are parity-unpinned."""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import                                   # noqa: E402
import make_golden_image_prep as mgi                # noqa: E402

FRAME = (70, 150)
CASES = {"nocrop": (), "crop": (2, 66, 5, 140)}      # (top, height, left, width)
PREFIX_CASES = [
    {"path": ["/data/kitti/KITTI_raw"], "split": ["splits/eigen_val_files.txt"], "depth_type": ["groundtruth"], "cameras": [[]]},
    {"path": ["/data/gta/GTA.v2", "/data/kitti/KITTI_raw"], "split": ["val_edges.txt", "{}_files.txt"], "depth_type": ["", "velodyne"],
     "cameras": [["camera_01"], ["a", "b"]]},
    {"path": ["relative/root"], "split": [""], "depth_type": [""], "cameras": [[]]},
]


class _Section(dict):
    __getattr__ = dict.__getitem__


def main():
    assert ref_import.reference_available()
    mgi._install_torchvision_stub()
    ref_import.install_stubs()
    from packnet_code.packnet_sfm.datasets import augmentations as A
    from packnet_code.packnet_sfm.utils.misc import parse_crop_borders
    from packnet_code.packnet_sfm.utils.logging import prepare_dataset_prefix
    g = np.random.default_rng(11)
    h, w = FRAME
    rgb = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    input_depth = ((g.random((h, w)) < 0.1) * (1 + 79 * g.random((h, w)))).astype(np.float32)
    depth = ((g.random((h, w)) < 0.2) * (1 + 79 * g.random((h, w)))).astype(np.float32)
    edge = ((g.random((h, w)) < 0.1) * 255).astype(np.uint8)
    rgb_edge = ((g.random((h, w)) < 0.1) * 255).astype(np.uint8)
    out = {"rgb": rgb, "input_depth": input_depth, "rgb_edge": rgb_edge, "case_names": np.array(list(CASES))}
    for name, crop in CASES.items():
        sample = {"rgb": Image.fromarray(rgb), "input_depth": input_depth.astype(np.float64), "depth": depth.copy(), "edge": edge.copy(),
                  "rgb_edge": rgb_edge.copy()}
        borders = parse_crop_borders(crop, sample["rgb"].size[::-1])
        if len(crop) > 0:
            sample = A.crop_sample_input(sample, borders)
        assert np.array_equal(sample["depth"], depth) and np.array_equal(sample["edge"], edge)       # supervision keeps its frame
        size = list(sample["rgb"].size)
        shape = (size[1] - size[1] % 32, size[0] - size[0] % 32)
        assert shape == (64, 128), shape
        pre = name + "_"
        out[pre + "crop"] = np.array(crop, dtype=np.int64)
        out[pre + "borders"] = np.array(borders, dtype=np.int64)
        out[pre + "rgb_edge_cropped_shape"] = np.array(sample["rgb_edge"].shape)
        out[pre + "rgb_edge_cropped_sum"] = np.array(int(sample["rgb_edge"].astype(np.int64).sum()))
        out[pre + "rgb_out"] = np.asarray(A.resize_image(sample["rgb"], shape))
        out[pre + "input_depth_out"] = A.resize_depth_preserve(sample["input_depth"], shape)[:, :, 0].astype(np.float32)
    prefixes = []
    for section in PREFIX_CASES:
        prefixes.append({"section": section, "prefix": [prepare_dataset_prefix(_Section(section), i) for i in range(len(section["path"]))]})
    out["prefix_cases"] = np.array(json.dumps(prefixes))
    path = os.path.join(HERE, "eval_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
