"""Per-frame depth metrics of the reference's analysis stage on the device (eval_depth.py: DataLoader.__getitem__ :170-187,
DensePredictionAnalyzer.eval_frame :348-410, the metric maps :432-456; the `analysis` stage of infer_edges.py:174-183).

  frame_depth_metrics    mean / std / abs relative error and the two accuracies of one frame (or a batch) over the valid mask
  run_depth_metrics      the loop over two path lists that writes frames_depth_metrics.csv and mean_frames_depth_metrics.csv
  run_ord_metrics        the D3R ordinal error per frame (infer_edges.py:369-402, utils/d3r.py): the pairs are drawn on the host from
                         numpy's stream in the reference's order, the agreeing pairs are counted on the device (an integer)

Arithmetic is float64 throughout, as numpy >= 2 computes it from a float32 prediction and a float64 ground truth; the two accuracies
are what np.nanmean returns for a float32 0/1 map (the float32 sum over the count, rounded to float32) and are formed on the
host from the kernel's exact integer counts.  Left out on purpose: the plots, the pickle.
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


# ---- the ordinal error (infer_edges.py:369-402 run_ord_metrics, utils/d3r.py), csrc/depth_viz.hip::mte_d3r_count ------------------------

ORD_PAIRS = (5000, 2500, 1000, 500, 100)
ORD_IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


def read_ord_gt(path):
    """The ground truth as run_ord_metrics reads it: channel 0 of an 8-bit BGR read.  A 16-bit PNG becomes its high byte (>> 8), a colour
    image its blue channel; parity-unpinned against OpenCV's imread."""
    from PIL import Image
    im = Image.open(path)
    if im.mode in ('I;16', 'I;16B', 'I;16L', 'I'):
        return (np.asarray(im).astype(np.int64) >> 8).clip(0, 255).astype(np.uint8)
    if im.mode in ('L', '1'):
        return np.asarray(im.convert('L'), dtype=np.uint8)
    return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8)[:, :, 2])


def ord_pair_count(n_valid):
    """The first rung of the ladder that 2 * pairs valid pixels can fill; upstream runs off the list below 200."""
    for pairs in ORD_PAIRS:
        if n_valid >= 2 * pairs:
            return pairs
    raise ValueError("{} valid ground-truth pixels: the ordinal error needs at least {}".format(n_valid, 2 * ORD_PAIRS[-1]))


def index_valid(gt):
    """gt: CUDA float32 [H,W] -> (workspace holding the raster-order list of pixels > 0, their number).  One 4-byte host read."""
    from .. import kernels as K
    K._require_gpu(gt)
    H, W = int(gt.shape[0]), int(gt.shape[1])
    work = torch.empty((K.lib.mte_lidar_perturb_work_bytes(H, W) + 7) // 8, dtype=torch.int64, device=gt.device)
    K.lib.mte_lidar_index(gt.data_ptr(), H, W, work.data_ptr(), K._stream())
    return work, int(work[:1].view(torch.int32)[0].item())


def d3r_count(gt, pred, pairs, index=None):
    """gt, pred: CUDA [H,W]; pairs: int [P,2] ordinals into the raster-order list of pixels with gt > 0 (``np.where(gt > 0)``) -> the number of
    pairs whose ordinal relation at tolerance 0.03 agrees (the sum of utils/d3r.py's ord_ratio), a Python int.  index: index_valid(gt)'s result."""
    from .. import kernels as K
    K._require_gpu(gt)
    K._require_gpu(pred)
    g, p = gt.detach().float().contiguous(), pred.detach().float().contiguous()
    if g.dim() != 2 or g.shape != p.shape:
        raise ValueError("expected two [H,W] maps of one size, got {} and {}".format(tuple(gt.shape), tuple(pred.shape)))
    work, n = index if index is not None else index_valid(g)
    pr = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2).astype(np.int32))
    if len(pr) == 0 or n == 0:
        raise ValueError("no pairs or no valid ground-truth pixel")
    if pr.min() < 0 or pr.max() >= n:
        raise ValueError("pair ordinals must lie in [0, {})".format(n))
    pd = torch.from_numpy(pr).to(g.device)
    count = torch.empty(1, dtype=torch.int32, device=g.device)
    K.lib.mte_d3r_count(g.data_ptr(), p.data_ptr(), int(g.shape[0]), int(g.shape[1]), work.data_ptr(), n, pd.data_ptr(), len(pr), count.data_ptr(),
                        K._stream())
    return int(count.item())


def frame_ord_error(gt_u8, pred):
    """One frame of run_ord_metrics: gt_u8 a host uint8 [h,w] map, pred a host float32 [H,W] prediction -> 1 - agreeing pairs / pairs.  The pairs
    are the first 2 P entries of one ``np.random.permutation(n)``, as upstream draws them."""
    pred_dev = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).cuda()
    gt_dev = torch.from_numpy(np.ascontiguousarray(gt_u8)).cuda().float()
    from ..datasets.kitti_edges import resize_depth_preserve
    gt_dev = resize_depth_preserve(gt_dev, tuple(pred_dev.shape[:2])).contiguous()
    work, n = index_valid(gt_dev)
    P = ord_pair_count(n)
    perm = np.random.permutation(n)[:2 * P]
    return 1 - d3r_count(gt_dev, pred_dev, perm.reshape(P, 2), index=(work, n)) / P


def _lines(list_or_path):
    if isinstance(list_or_path, str):
        with open(list_or_path) as f:
            return [l.split('\n')[0] for l in f.readlines()]
    return [l.strip() for l in list_or_path]


def run_ord_metrics(gt_list, pred_list):
    """gt_list / pred_list: the paths of two list files (as upstream) or the lists themselves -> float64 [frames] ordinal errors."""
    gts, preds = _lines(gt_list), _lines(pred_list)
    ord_error = np.zeros(len(preds))
    for i in range(len(preds)):
        ord_error[i] = frame_ord_error(read_ord_gt(gts[i]), np.load(preds[i]))
    return ord_error
