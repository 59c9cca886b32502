"""Fixture generator of the edge benchmark and the per-frame depth metrics -- development container only (needs the upstream
reference next to this repository, see ref_import.py).  Nothing from the reference is copied: its functions RUN here and
only the arrays they read and return are stored.

Two more stubs than ref_import installs, both local to this generator:
  * ``bsds_metric.bsds``: py-bsds500 is not available.  ``correspond_pixels.correspond_pixels`` is the exact matcher of
    tests/edge_benchmark_ref.py (maximum-cardinality matching within max_dist x diagonal); ``thin`` is never called
    (the reference passes apply_thinning=False).
  * ``cv2.imread``: reads a PNG with PIL into H x W x 3 uint8.

Pinned (tests/golden/edge_benchmark.npz):
  1. the reference's ``_pred_eval`` on lossless PNG edge images (two annotations, a list crop);
  2. ``compute_rec_prec_f1`` on pooled counts and ``mean_recall_at_precision_range`` over both ranges;
  3. ``DensePredictionAnalyzer.eval_frame`` plus the ``DataLoader`` resize branch: 24x40 with a crop, 24x40 with a mask image,
     ground truth 48x80 against a 24x40 prediction, a frame with no valid pixel.

    python tests/golden/make_golden_edge_benchmark.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import edge_benchmark_ref as ebr  # noqa: E402

ANNOTATIONS = ("kitti_de_000114_10.png", "kitti_de_000076_10.png")
CROP = [44, 1197, 153, 371]


def install_local_stubs():
    from PIL import Image
    ref_import.install_stubs()
    cv2 = sys.modules["cv2"]

    def imread(path, *a):
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)[:, :, ::-1])
    cv2.imread = imread

    def correspond_pixels(bmap1, bmap2, max_dist=0.0075, outlier_cost=100):
        b1, b2 = np.asarray(bmap1) != 0, np.asarray(bmap2) != 0
        r2 = ebr.radius2(b1.shape, max_dist)
        m = ebr.max_matching_size(b1 * 255.0, b2 * 255.0, r2)
        # the reference reads only (match > 0).sum(): any maps with m marked pixels serve
        m1, m2 = np.zeros(b1.size, np.int64), np.zeros(b2.size, np.int64)
        m1[np.nonzero(b1.reshape(-1))[0][:m]] = 1
        m2[np.nonzero(b2.reshape(-1))[0][:m]] = 1
        return m1.reshape(b1.shape), m2.reshape(b2.shape), 0.0, 0.0
    bsds = types.ModuleType("bsds_metric.bsds")
    bsds.correspond_pixels = types.SimpleNamespace(correspond_pixels=correspond_pixels)
    bsds.thin = types.SimpleNamespace(binary_thin=None)
    pkg = types.ModuleType("bsds_metric")
    pkg.bsds = bsds
    sys.modules["bsds_metric"], sys.modules["bsds_metric.bsds"] = pkg, bsds


def noisy_prediction(gt, seed, shift=(1, 2), salt=0.01, dropout=0.10):
    """the annotation shifted by (dy, dx), with `salt` of all pixels switched on and `dropout` of the edge pixels removed"""
    g = np.random.default_rng(seed)
    p = np.zeros_like(gt, dtype=bool)
    p[shift[0]:, shift[1]:] = gt[:gt.shape[0] - shift[0], :gt.shape[1] - shift[1]] > 0
    p &= g.random(gt.shape) >= dropout
    p |= g.random(gt.shape) < salt
    return p


def main():
    from PIL import Image
    install_local_stubs()
    import eval_depth_edges as ede
    import eval_depth as ed
    out = {}
    tmp = tempfile.mkdtemp()

    # 1. _pred_eval on lossless PNGs
    for k, name in enumerate(ANNOTATIONS):
        gt_path = os.path.join(HERE, name)
        gt = np.asarray(Image.open(gt_path), dtype=np.uint8) * 255
        pred = noisy_prediction(gt, seed=k)
        pred_path = os.path.join(tmp, "pred_%d.png" % k)
        Image.fromarray((pred * 255).astype(np.uint8)).save(pred_path)
        r = ede._pred_eval(pred_path, gt_path, str(CROP))
        out["pred_eval_%d_pred_bits" % k] = np.packbits(pred)
        out["pred_eval_%d_counts" % k] = np.array([r.count_r_overall[0], r.sum_r_overall[0], r.count_p_overall[0], r.sum_p_overall[0]], np.float64)
        out["pred_eval_%d_rec_prec" % k] = np.array([r.recall[0], r.precision[0]], np.float64)
    out["pred_eval_crop"] = np.array(CROP, np.int64)
    out["pred_eval_shape"] = np.array(gt.shape, np.int64)

    # 2. pooled counts -> precision / recall -> AUC
    g = np.random.default_rng(7)
    sum_p = np.floor(90000.0 * 0.7 ** np.arange(12))                          # fewer predicted pixels at higher thresholds ...
    sum_r = np.full(12, 41234.0)
    cnt = np.floor(sum_p * (np.linspace(0.08, 0.8, 12) + 0.01 * g.random(12)))  # ... of which a growing share is matched
    for name, args in (("guard_none", (0.0, 0.0, 0.0, 0.0)), ("guard_nopred", (0.0, 512.0, 0.0, 0.0)), ("guard_nogt", (0.0, 0.0, 0.0, 77.0))):
        a = [np.array([v]) for v in args]
        out["pool_" + name] = np.array([args, [float(v[0]) for v in ede.compute_rec_prec_f1(*a)] + [0.0]])
    prec, rec = [], []
    for t in range(12):
        r_, p_, _ = ede.compute_rec_prec_f1(cnt[t:t + 1], sum_r[t:t + 1], cnt[t:t + 1], sum_p[t:t + 1])
        prec.append(p_[0]); rec.append(r_[0])
    pr = np.vstack((prec, rec)).transpose()
    out["pool_counts"] = np.stack([cnt, sum_r, cnt, sum_p])
    out["pool_precision_recall"] = pr
    out["pool_auc"] = np.array([ede.mean_recall_at_precision_range(pr), ede.mean_recall_at_precision_range(pr, small_lim=0.12, large_lim=0.65)])

    # 3. eval_frame (+ the DataLoader resize branch)
    def frame(h, w, seed, scale=1):
        g = np.random.default_rng(seed)
        H, W = h * scale, w * scale
        gt = np.floor(g.random((H, W)) * 90 * 256) / 256.0                     # 16-bit png / 256: exact in float32 too
        gt[g.random((H, W)) < 0.5] = 0.0
        gt[g.random((H, W)) < 0.05] = -1.0
        d = (np.abs(g.standard_normal((h, w))) * 4 + g.random((h, w)) * 60 + 0.5).astype(np.float32)
        return gt, d

    def run_case(name, gt, d, crop, mask, lo=1.0, hi=80.0):
        cfg = types.SimpleNamespace(eval_mask_image_list='', min_depth=lo, max_depth=hi, gt_crop=crop)
        an = ed.DensePredictionAnalyzer(cfg)
        np.save(os.path.join(tmp, "gt.npy"), gt)
        np.save(os.path.join(tmp, "d.npy"), d)
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(os.path.join(tmp, "im.png"))
        for n, v in (("im", "im.png"), ("gt", "gt.npy"), ("d", "d.npy")):
            with open(os.path.join(tmp, n + ".txt"), "w") as f:
                f.write(os.path.join(tmp, v) + "\n")
        dl = ed.DataLoader(os.path.join(tmp, "im.txt"), os.path.join(tmp, "gt.txt"), os.path.join(tmp, "d.txt"))
        _, gt_l, d_l = dl[0]
        v = an.eval_frame(0, gt_l, d_l, mask)["vals"]
        out[name + "_gt"], out[name + "_pred"] = gt, d
        out[name + "_gt_resized"] = np.asarray(gt_l, np.float64)
        out[name + "_crop"] = np.array(crop, np.int64)
        if mask is not None:
            out[name + "_mask"] = mask
        out[name + "_limits"] = np.array([lo, hi])
        out[name + "_vals"] = np.array([v["mean_rel_err"], v["std_rel_err"], v["abs_rel_err"], v["accuracy_1p1"], v["accuracy_1p25"]], np.float64)
        gl = an._process_depth_gt_for_evaluation(gt_l, lo, hi, crop, mask)
        valid = gl != -1
        dev = np.maximum(np.abs(d_l / (gl + np.finfo(float).eps)), np.abs(gl / (d_l + np.finfo(float).eps)))
        out[name + "_counts"] = np.array([valid.sum(), (valid & (dev < 1.1)).sum(), (valid & (dev < 1.25)).sum()], np.int64)

    gt, d = frame(24, 40, 1)
    run_case("frame_crop", gt, d, [3, 35, 5, 22], None)
    gt, d = frame(24, 40, 2)
    m = (np.random.default_rng(3).random((24, 40)) < 0.6).astype(np.uint8) * 255
    run_case("frame_mask", gt, d, [0, 0, 0, 0], m)
    gt, d = frame(24, 40, 4, scale=2)
    run_case("frame_resize", gt, d, [2, 38, 1, 23], None)
    gt, d = frame(24, 40, 5)
    run_case("frame_empty", gt, d, [3, 35, 5, 22], None, lo=200.0, hi=300.0)

    path = os.path.join(HERE, "edge_benchmark.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.endswith(("_vals", "_counts", "_auc", "_rec_prec")):
            print(k, out[k])


if __name__ == "__main__":
    import warnings
    warnings.filterwarnings("ignore")
    main()
