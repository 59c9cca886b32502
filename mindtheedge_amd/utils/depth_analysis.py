"""Per-frame depth metrics of the reference's analysis stage on the device (eval_depth.py: DataLoader.__getitem__ :170-187,
DensePredictionAnalyzer.eval_frame :348-410, the metric maps :432-456; the `analysis` stage of infer_edges.py:174-183).

  frame_depth_metrics    mean / std / abs relative error and the two accuracies of one frame (or a batch) over the valid mask
  run_depth_metrics      the loop over two path lists that writes frames_depth_metrics.csv and mean_frames_depth_metrics.csv

Arithmetic is float64 throughout, as numpy >= 2 computes it from a float32 prediction and a float64 ground truth; the two accuracies
are what np.nanmean returns for a float32 0/1 map (the float32 sum over the count, rounded to float32) and are formed on the
host from the kernel's exact integer counts.  Left out on purpose: the D3R ordinal error, the plots, the pickle.
No CPU path: host tensors raise MteError.
"""
import csv
import os

import numpy as np
import torch

COLUMNS = ["frm_idx", "mean_rel_err", "std_rel_err", "abs_rel_err", "accuracy_1p1", "accuracy_1p25", "median_scale_factor"]   # eval_depth.py:229-237


def _accuracy(k, n):
    return float(np.float32(np.float32(k) / np.int64(n))) if n else float('nan')


def frame_depth_metrics(gt, pred, min_depth, max_depth, gt_crop=None, mask=None):
    """gt: CUDA [H,W] or [B,H,W] metres (float64 kept as it is; -1 or 0 = invalid), pred: CUDA float map(s).  A ground truth of
    another size is first brought to the prediction's size with resize_depth_preserve (eval_depth.py:183-185).  The mask is
    min_depth < gt < max_depth inside gt_crop = [x0, x1, y0, y1], or where the `mask` image is > 0.
    -> dict of python floats / ints (lists for a batch): mean_rel_err, std_rel_err, abs_rel_err, accuracy_1p1, accuracy_1p25,
    valid, count_1p1, count_1p25.  An empty mask gives NaN like np.nanmean.  One host read."""
    from .. import kernels as K
    K._require_gpu(gt)
    K._require_gpu(pred)
    squeeze = pred.dim() == 2
    p = (pred.unsqueeze(0) if squeeze else pred).detach().float().contiguous()
    g = gt.unsqueeze(0) if gt.dim() == 2 else gt
    if g.shape[1:] != p.shape[1:]:
        from ..datasets.kitti_edges import resize_depth_preserve
        g = resize_depth_preserve(g.float(), tuple(p.shape[1:]))
    g = g.detach().double().contiguous()
    B, H, W = p.shape
    if g.shape[0] != B:
        raise ValueError("one ground truth per prediction")
    m = None
    if mask is not None:
        K._require_gpu(mask)
        m = ((mask.unsqueeze(0) if mask.dim() == 2 else mask) > 0).to(torch.uint8).expand(B, H, W).contiguous()
        crop = (0, W, 0, H)
    else:
        if gt_crop is None:
            raise ValueError("gt_crop = [x0, x1, y0, y1] or a mask image")
        crop = [int(np.int32(v)) for v in gt_crop]
    out = torch.empty((B, 5), dtype=torch.float64, device=p.device)
    counts = torch.empty((B, 3), dtype=torch.int64, device=p.device)
    K.lib.mte_frame_depth_metrics(g.data_ptr(), p.data_ptr(), m.data_ptr() if m is not None else None, B, H, W, float(min_depth), float(max_depth),
                                  crop[0], crop[1], crop[2], crop[3], out.data_ptr(), counts.data_ptr(), K._stream())
    both = torch.cat([out, counts.double()], dim=1).cpu().numpy()              # counts < 2^30: exact in a double
    res = {"mean_rel_err": [], "std_rel_err": [], "abs_rel_err": [], "accuracy_1p1": [], "accuracy_1p25": [], "valid": [], "count_1p1": [], "count_1p25": []}
    for r in both:
        n, n11, n125 = int(r[5]), int(r[6]), int(r[7])
        res["mean_rel_err"].append(float(r[0])); res["std_rel_err"].append(float(r[1])); res["abs_rel_err"].append(float(r[2]))
        res["accuracy_1p1"].append(_accuracy(n11, n)); res["accuracy_1p25"].append(_accuracy(n125, n))
        res["valid"].append(n); res["count_1p1"].append(n11); res["count_1p25"].append(n125)
    return {k: v[0] for k, v in res.items()} if squeeze else res


def load_depth_gt(path):
    """eval_depth.py:192-201: .npy as it is, 16-bit .png / 256 (0 where the png is 0)"""
    if path.endswith('.npy'):
        return np.load(path)
    if path.endswith('.png'):
        from PIL import Image
        return np.array(Image.open(path), dtype=int).astype(np.float64) / 256.
    raise ValueError("Depth GT must be in .png or .npy format.")


def run_depth_metrics(gt_list, pred_list, out_dir, min_depth, max_depth, gt_crop=None, mask_list=None):
    """The analysis loop (infer_edges.py:174-183): one row per frame into <out_dir>/frames_depth_metrics.csv and the column means into
    <out_dir>/mean_frames_depth_metrics.csv, with the reference's column names (pandas' to_csv layout: an unnamed index column).
    gt_list / pred_list (/ mask_list): paths, one per frame.  -> the rows."""
    from PIL import Image
    rows = []
    for i, (gp, pp) in enumerate(zip(gt_list, pred_list)):
        gt = torch.from_numpy(np.ascontiguousarray(load_depth_gt(gp.strip()))).cuda()
        pred = torch.from_numpy(np.load(pp.strip()).astype(np.float32)).cuda()
        mask = None
        if mask_list is not None:
            mask = torch.from_numpy(np.asarray(Image.open(mask_list[i].strip()).convert('L'), dtype=np.uint8).copy()).cuda()
        r = frame_depth_metrics(gt, pred, min_depth, max_depth, gt_crop=gt_crop, mask=mask)
        rows.append([i, r["mean_rel_err"], r["std_rel_err"], r["abs_rel_err"], r["accuracy_1p1"], r["accuracy_1p25"], 1])
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "frames_depth_metrics.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + COLUMNS)
        for i, r in enumerate(rows):
            w.writerow([i] + r)
    with open(os.path.join(out_dir, "mean_frames_depth_metrics.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "0"])
        a = np.array(rows, np.float64).reshape(-1, len(COLUMNS))
        with np.errstate(all='ignore'):
            means = a.mean(0) if len(rows) else np.full(len(COLUMNS), np.nan)
        for name, v in zip(COLUMNS, means):
            w.writerow([name, v])
    return rows
