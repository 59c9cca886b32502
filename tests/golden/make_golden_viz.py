"""Generates tests/golden/viz.npz from the upstream reference (development container only), run as it is:

  * ``viz_inv_depth`` (packnet_code/packnet_sfm/utils/depth.py:67-101) on small random frames: default, a given normalizer, filter_zeros, both maps;
  * the colour block of ``infer_and_save_depth`` (infer_edges.py, from the line that takes the log of the prediction to the line that forms the
    uint8 image).  It sits in the middle of a function that needs a network, so the generator compiles exactly those lines of the file, read at
    run time, and executes them on a random depth frame;
  * ``d3r`` (packnet_code/packnet_sfm/utils/d3r.py) on a fixed pair list, with the dtypes ``run_ord_metrics`` hands it (a float64 map of
    8-bit values, a float32 prediction);
  * ``run_ord_metrics`` (infer_edges.py), compiled from the file the same way (its module imports cv2 and pandas), under ``np.random.seed``.
    ``cv2.imread`` is stood in for by an 8-bit read through PIL (16-bit PNG: the high byte) -- the parity-unpinned part.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_viz.py
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import                                   # noqa: E402

ORD_SEED = 7


def log_uniform(rs, shape, lo=1.0, hi=80.0):
    return np.exp(np.log(lo) + rs.rand(*shape) * (np.log(hi) - np.log(lo))).astype(np.float32)


def reference_function(path, name, namespace):
    """compile one top-level function of a reference file without importing the file"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    return namespace[name]


def reference_color_block(path):
    """the statements of infer_and_save_depth from the first one that calls np.log to the one that assigns the uint8 image"""
    with open(path) as f:
        src = f.read()
    tree = ast.parse(src, path)
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "infer_and_save_depth")
    body = fn.body
    first = next(i for i, s in enumerate(body) if "np.log(" in ast.get_source_segment(src, s))
    last = next(i for i, s in enumerate(body) if i > first and "astype(np.uint8)" in ast.get_source_segment(src, s))
    return compile(ast.Module(body=body[first:last + 1], type_ignores=[]), path, "exec")


def imread_8bit(path):
    from PIL import Image
    im = Image.open(path)
    a = np.asarray(im)
    if a.dtype != np.uint8:
        a = (a.astype(np.int64) >> 8).astype(np.uint8)
    return np.stack([a, a, a], axis=2) if a.ndim == 2 else a[:, :, ::-1]


def main():
    import torch
    ref_import.install_stubs()
    import matplotlib as mpl
    import matplotlib.cm as cm
    import matplotlib.pyplot as plt
    from packnet_code.packnet_sfm.utils.depth import viz_inv_depth
    from packnet_code.packnet_sfm.utils.d3r import d3r
    from packnet_code.packnet_sfm.datasets.augmentations import resize_depth_preserve
    out = {"numpy_version": np.array(np.__version__), "matplotlib_version": np.array(mpl.__version__)}
    rs = np.random.RandomState(0)

    # ---- viz_inv_depth
    for name, shape in (("a", (24, 80)), ("b", (5, 7))):
        inv = (rs.rand(*shape) * 0.4).astype(np.float32)
        inv[rs.rand(*shape) < 0.15] = 0.0
        inv[0, 0], inv[-1, -1] = -0.05, 1.5
        out["viz_%s_inv" % name] = inv
        for tag, kw in (("default", {}), ("norm", {"normalizer": 0.3}), ("fz", {"filter_zeros": True}), ("spectral", {"colormap": "Spectral"}),
                        ("p50", {"percentile": 50})):
            res = viz_inv_depth(torch.from_numpy(inv.copy()).unsqueeze(0), **kw)      # upstream divides its input in place: a copy
            assert res.shape == shape + (3,) and res.dtype == np.float64
            out["viz_%s_%s" % (name, tag)] = res

    # ---- the log colouring
    block = reference_color_block(os.path.join(ref_import.REFERENCE_ROOT, "infer_edges.py"))
    for name, shape in (("a", (24, 80)), ("b", (5, 7))):
        depth = log_uniform(rs, shape)
        ns = {"np": np, "mpl": mpl, "cm": cm, "plt": plt, "pred_numpy": depth.copy()}
        exec(block, ns)
        assert ns["colormapped_im"].dtype == np.uint8 and ns["colormapped_im"].shape == shape + (3,)
        out["log_%s_depth" % name] = depth
        out["log_%s_color" % name] = ns["colormapped_im"]

    # ---- d3r on the dtypes run_ord_metrics hands it
    gt = (rs.rand(24, 80) < 0.6) * rs.randint(1, 256, size=(24, 80))
    gt = gt.astype(np.float64)
    pred = (gt * (1 + 0.08 * rs.randn(24, 80)) + 0.5 + 3 * rs.rand(24, 80)).astype(np.float32)
    centers = np.where(gt > 0)
    n = len(centers[0])
    pairs = rs.randint(0, n, size=(400, 2))
    ratio = d3r(gt, pred, centers, pairs)
    out["d3r_gt"], out["d3r_pred"], out["d3r_pairs"] = gt.astype(np.uint8), pred, pairs.astype(np.int32)
    out["d3r_agree"] = np.asarray(ratio).astype(np.uint8)
    assert 0 < out["d3r_agree"].sum() < len(pairs)

    # ---- run_ord_metrics over two frames: 16-bit ground truths of twice the prediction's size
    from PIL import Image
    cv2 = types.SimpleNamespace(imread=imread_8bit)
    run_ord_metrics = reference_function(os.path.join(ref_import.REFERENCE_ROOT, "infer_edges.py"), "run_ord_metrics",
                                         {"np": np, "cv2": cv2, "resize_depth_preserve": resize_depth_preserve, "d3r": d3r})
    with tempfile.TemporaryDirectory() as tmp:
        gts, preds = [], []
        for i, density in enumerate((0.9, 0.08)):                       # after the resize: >= 1000 valid pixels (500 pairs), >= 200 (100 pairs)
            g16 = ((rs.rand(48, 160) < density) * rs.randint(256, 65536, size=(48, 160))).astype(np.uint16)
            small = resize_depth_preserve((g16 >> 8).astype(np.uint8), (24, 80))[:, :, 0]
            p = (small * (1 + 0.1 * rs.randn(24, 80)) + 1 + 5 * rs.rand(24, 80)).astype(np.float32)
            Image.fromarray(g16).save(os.path.join(tmp, "gt_%d.png" % i))
            np.save(os.path.join(tmp, "pred_%d.npy" % i), p)
            gts.append(os.path.join(tmp, "gt_%d.png" % i))
            preds.append(os.path.join(tmp, "pred_%d.npy" % i))
            out["ord_gt_%d" % i], out["ord_pred_%d" % i] = g16, p
            out["ord_valid_%d" % i] = np.array(int((small > 0).sum()))
        for name, paths in (("gt.txt", gts), ("pred.txt", preds)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write("".join(p + "\n" for p in paths))
        np.random.seed(ORD_SEED)
        out["ord_error"] = run_ord_metrics(os.path.join(tmp, "gt.txt"), os.path.join(tmp, "pred.txt"))
    out["ord_seed"] = np.array(ORD_SEED)
    assert 1000 <= out["ord_valid_0"] and 200 <= out["ord_valid_1"] < 1000

    path = os.path.join(HERE, "viz.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "ord_error", out["ord_error"], "valid", out["ord_valid_0"], out["ord_valid_1"])


if __name__ == "__main__":
    main()
