"""CPU references of the edge benchmark (numpy / scipy only; nothing here touches the GPU).

* ``max_matching_size``: the exact matcher -- adjacency ``dx^2 + dy^2 <= r2`` between the predicted and the annotated edge pixels,
  then ``scipy.sparse.csgraph.maximum_bipartite_matching`` (Hopcroft-Karp).  The size of a maximum matching is unique.
* ``brute_force_matching_size``: exhaustive search, for maps with a handful of pixels.
* ``greedy_matching_size``: first-fit greedy in one of the four raster scan orders, nearest partner first -- what a matcher that
  is only MAXIMAL would return.
* ``frame_depth_metrics``: float64 numpy restatement of the per-frame depth metrics of the analysis stage.
* ``pr_evaluation_ref`` / ``compute_rec_prec_f1`` / ``mean_recall_at_precision_range``: the benchmark's pipeline on the host
  (oracle.canny_oracle for the resize and the Canny step, the exact matcher, pooled counts).
"""
import functools
import math

import numpy as np

EPS = float(np.finfo(float).eps)


def radius2(shape, max_dist):
    """r2 = floor((max_dist * sqrt(H^2 + W^2))^2), in double: two pixels may be paired iff dx^2 + dy^2 <= r2."""
    H, W = int(shape[0]), int(shape[1])
    r = float(max_dist) * math.sqrt(float(H * H + W * W))
    return int(math.floor(r * r))


def edge_pixels(im):
    """(ys, xs) of the edge pixels of a 0..255 image: v / 255 > 0.5"""
    return np.nonzero(np.asarray(im, np.float64) / 255.0 > 0.5)


def offsets(r2):
    """admissible (dy, dx), nearest first (ties: raster order)"""
    r = int(math.isqrt(r2))
    out = [(dy * dy + dx * dx, dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r2]
    return [(dy, dx) for _, dy, dx in sorted(out)]


def adjacency(pred, gt, r2):
    """scipy CSR matrix [n_pred, n_gt] of the admissible pairs"""
    from scipy.sparse import csr_matrix
    H, W = pred.shape
    py, px = edge_pixels(pred)
    gy, gx = edge_pixels(gt)
    gid = -np.ones((H, W), np.int64)
    gid[gy, gx] = np.arange(len(gy))
    rows, cols = [], []
    for dy, dx in offsets(r2):
        y, x = py + dy, px + dx
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        j = np.where(ok, gid[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], -1)
        keep = j >= 0
        rows.append(np.nonzero(keep)[0])
        cols.append(j[keep])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(len(py), len(gy)))


def max_matching_size(pred, gt, r2):
    from scipy.sparse.csgraph import maximum_bipartite_matching
    a = adjacency(np.asarray(pred), np.asarray(gt), r2)
    if a.shape[0] == 0 or a.shape[1] == 0 or a.nnz == 0:
        return 0
    return int((maximum_bipartite_matching(a, perm_type='column') >= 0).sum())


def brute_force_matching_size(pred, gt, r2):
    a = adjacency(np.asarray(pred), np.asarray(gt), r2).toarray().astype(bool)
    nbr = [np.nonzero(row)[0].tolist() for row in a]

    @functools.lru_cache(maxsize=None)
    def best(i, used):
        if i == len(nbr):
            return 0
        top = best(i + 1, used)                              # leave pixel i unmatched
        for j in nbr[i]:
            if not used & (1 << j):
                top = max(top, 1 + best(i + 1, used | (1 << j)))
        return top
    return best(0, 0)


def greedy_matching_size(pred, gt, r2, flip_y=False, flip_x=False):
    """first fit: predicted pixels in raster order (rows top-down or bottom-up, columns left-right or right-left), each
    takes its nearest free partner"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if flip_y:
        pred, gt = pred[::-1], gt[::-1]
    if flip_x:
        pred, gt = pred[:, ::-1], gt[:, ::-1]
    H, W = pred.shape
    free = np.asarray(gt, np.float64) / 255.0 > 0.5
    free = free.copy()
    offs = offsets(r2)
    n = 0
    for y, x in zip(*edge_pixels(pred)):
        for dy, dx in offs:
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and free[v, u]:
                free[v, u] = False
                n += 1
                break
    return n


def check_mates(pred, gt, r2, mate, matched):
    """a returned partner map is a valid matching of `matched` pairs"""
    pred, gt, mate = np.asarray(pred), np.asarray(gt), np.asarray(mate)
    H, W = pred.shape
    p = np.asarray(pred, np.float64) / 255.0 > 0.5
    g = (np.asarray(gt, np.float64) / 255.0 > 0.5).reshape(-1)
    assert np.all(mate[~p] == -1)
    idx = np.nonzero(mate.reshape(-1) >= 0)[0]
    partner = mate.reshape(-1)[idx]
    assert len(idx) == matched
    assert np.all(partner < H * W) and np.all(g[partner])
    dy, dx = partner // W - idx // W, partner % W - idx % W
    assert np.all(dy * dy + dx * dx <= r2)
    assert len(np.unique(partner)) == len(partner)


def random_maps(n, H, W, density, seed):
    g = np.random.default_rng(seed)
    pred = (g.random((n, H, W)) < density).astype(np.float32) * 255.0
    gt = (g.random((n, H, W)) < density).astype(np.float32) * 255.0
    return pred, gt


# ---- counts -> precision / recall -> AUC (restated; pinned by the golden fixtures generated from the reference's own code)

def compute_rec_prec_f1(count_r, sum_r, count_p, sum_p):
    rec = count_r / (sum_r + (sum_r == 0))
    prec = count_p / (sum_p + (sum_p == 0))
    f1 = 2.0 * prec * rec / (prec + rec + ((prec + rec) == 0))
    return rec, prec, f1


def mean_recall_at_precision_range(arr, small_lim=0.0, large_lim=1.0):
    x = np.array(range(int(small_lim * 100), int(large_lim * 100))) / 100
    y = np.interp(x, arr[:, 0], arr[:, 1])
    return np.mean(np.clip(y, 0, 1))


def edge_from_depth_ref(depth, new_shape, min_depth, max_depth, thresh_1, thresh_2):
    """edge_from_depth on the host: oracle.canny_oracle's resize and Canny around the fixed-scale quantisation"""
    from oracle import canny_oracle as co
    d = np.asarray(depth, np.float32)
    if new_shape is not None and tuple(d.shape) != (new_shape[1], new_shape[0]):
        d = co.resize_linear(d, new_shape[0], new_shape[1])
    return co.canny(quantise_fixed(d, min_depth, max_depth), thresh_1, thresh_2)


def quantise_fixed(d, min_depth, max_depth):
    d = np.array(d, np.float32)
    d[d < min_depth] = min_depth
    d[d > max_depth] = max_depth
    return (d * np.float32(255.0 / max_depth)).astype(np.uint8)


def pr_evaluation_ref(depths, gt_edges, edge_thresh_range=range(20, 241, 20), gt_crop=(44, 1197, 153, 371), min_depth=0.0,
                      max_depth=80.0, max_dist=0.002):
    precision, recall = [], []
    for t in edge_thresh_range:
        cr = sr = cp = sp = 0.0
        for d, g in zip(depths, gt_edges):
            g = np.asarray(g)
            e = edge_from_depth_ref(d, (g.shape[1], g.shape[0]), min_depth, max_depth, int(t / 2), int(t))
            if len(gt_crop) > 0:
                e, g = e[gt_crop[2]:gt_crop[3], gt_crop[0]:gt_crop[1]], g[gt_crop[2]:gt_crop[3], gt_crop[0]:gt_crop[1]]
            m = max_matching_size(e, g, radius2(e.shape, max_dist))
            cr += m; cp += m
            sr += len(edge_pixels(g)[0]); sp += len(edge_pixels(e)[0])
        rec, prec, _ = compute_rec_prec_f1(np.array([cr]), np.array([sr]), np.array([cp]), np.array([sp]))
        precision.append(prec[0]); recall.append(rec[0])
    return precision, recall


# ---- per-frame depth metrics (restated from the analysis stage; pinned by the golden fixtures)

def frame_depth_metrics(gt, pred, min_depth, max_depth, gt_crop=None, mask=None):
    gt = np.asarray(gt, np.float64)
    d = np.asarray(pred)
    valid = np.logical_and(gt > min_depth, gt < max_depth)
    if mask is None:
        cm = np.zeros(gt.shape, bool)
        cm[int(gt_crop[2]):int(gt_crop[3]), int(gt_crop[0]):int(gt_crop[1])] = True
    else:
        cm = np.asarray(mask) > 0
    valid &= cm
    g, d = gt[valid], d[valid].astype(np.float64)
    n = int(valid.sum())
    rel = (d - g) / (g + EPS)
    dev = np.maximum(np.abs(d / (g + EPS)), np.abs(g / (d + EPS)))
    n11, n125 = int((dev < 1.1).sum()), int((dev < 1.25).sum())
    with np.errstate(all='ignore'):
        nan = float('nan')
        return {"mean_rel_err": rel.mean() if n else nan, "std_rel_err": rel.std() if n else nan,
                "abs_rel_err": np.abs(rel).mean() if n else nan,
                "accuracy_1p1": accuracy_from_counts(n11, n), "accuracy_1p25": accuracy_from_counts(n125, n),
                "valid": n, "count_1p1": n11, "count_1p25": n125}


def accuracy_from_counts(k, n):
    """np.nanmean of a float32 0/1 map: the float32 sum (exact below 2^24) over the count, rounded to float32"""
    return float(np.float32(np.float32(k) / np.int64(n))) if n else float('nan')
