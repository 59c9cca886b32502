"""The reference's edge benchmark on the device: eval_depth_edges.py (Canny edges of the predicted depth at twelve thresholds, a
one-to-one correspondence of predicted and annotated edge pixels, pooled precision / recall per threshold, "AUC (edges)").

  correspond_pixels_count   the matcher (csrc/edge_match.hip): size of a maximum matching under dx^2 + dy^2 <= r2.  PARITY
                            UNPINNED against py-bsds500 (not available); exact against an independent solver (tests/)
  edge_from_depth           edge.py:73-93: resize_linear -> clamp -> fixed-scale Canny (parity-unpinned restatements of OpenCV)
  pr_evaluation             eval_depth_edges.py:232-348: pooled counts per threshold -> (precision_vec, recall_vec)
  mean_recall_at_precision_range   eval_depth_edges.py:365-375, host numpy on the twelve points like upstream

Left out on purpose: the JPEG round trip of the predicted edge images, thin.binary_thin (the reference passes
apply_thinning=False), the plots and the pickle.  No CPU path: host tensors raise MteError.
"""
import math

import numpy as np
import torch

from .edge import _edge_maps, resize_linear

STATUS = {1: "init_mate is not a valid matching", 2: "phase bound hit", 3: "level bound hit", 4: "path-walk bound hit",
          5: "queue overflow", 6: "gt_of out of range"}
MAX_R2 = 64
WORKSPACE_BUDGET = 1 << 30          # bytes of matcher workspace per launch: the instances of a run go in batches of this size


def radius2(shape, max_dist):
    """r2 = floor((max_dist * sqrt(H^2 + W^2))^2) in double: the integer the kernel compares dx^2 + dy^2 with."""
    H, W = int(shape[-2]), int(shape[-1])
    r = float(max_dist) * math.sqrt(float(H * H + W * W))
    return int(math.floor(r * r))


def edge_match(pred, gt, r2, gt_of=None, init_mate=None, return_mates=False):
    """pred [B,H,W], gt [Bg,H,W] CUDA edge images (0..255) -> int32 device tensor [B,4] = (matched, n_pred, n_gt, status)
    (and, return_mates, the int32 [B,H,W] partner map).  No host read."""
    from .. import kernels as K
    K._require_gpu(pred)
    K._require_gpu(gt)
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[1:] != gt.shape[1:]:
        raise ValueError("pred [B,H,W] and gt [Bg,H,W] of one size, got {} and {}".format(tuple(pred.shape), tuple(gt.shape)))
    p, g = pred.detach().float().contiguous(), gt.detach().float().contiguous()
    B, H, W = p.shape
    Bg = g.shape[0]
    if gt_of is None:
        if Bg != B:
            raise ValueError("gt_of is needed when pred and gt differ in number")
        gt_of = torch.arange(B, dtype=torch.int32, device=p.device)
    else:
        gt_of = torch.as_tensor(gt_of, dtype=torch.int32).to(p.device).contiguous()
        if gt_of.numel() != B:
            raise ValueError("gt_of needs one entry per predicted map")
    if init_mate is not None:
        K._require_gpu(init_mate)
        init_mate = init_mate.to(torch.int32).contiguous()
        if tuple(init_mate.shape) != (B, H, W):
            raise ValueError("init_mate is int32 [B,H,W]")
    nbytes = K.lib.mte_edge_match_workspace_bytes(B, H, W, int(r2))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=p.device)
    result = torch.empty((B, 4), dtype=torch.int32, device=p.device)
    mates = torch.empty((B, H, W), dtype=torch.int32, device=p.device) if return_mates else None
    K.lib.mte_edge_match(p.data_ptr(), g.data_ptr(), gt_of.data_ptr(), B, Bg, H, W, int(r2),
                         init_mate.data_ptr() if init_mate is not None else None, ws.data_ptr(), nbytes, result.data_ptr(),
                         mates.data_ptr() if return_mates else None, K._stream())
    return (result, mates) if return_mates else result


def correspond_pixels_count(pred, gt, max_dist=0.0075, gt_of=None):
    """Counts of correspond_pixels(pred, gt, max_dist) as the benchmark uses them: CUDA [H,W] or [B,H,W] edge images ->
    numpy int64 [B,3] (or [3]) = (matched, n_pred, n_gt).  gt may hold fewer maps than pred: gt_of[b] names pred[b]'s.
    One host read per call.  Raises MteError when an instance did not finish (status != 0)."""
    from .. import kernels as K
    squeeze = pred.dim() == 2
    p = pred.unsqueeze(0) if squeeze else pred
    g = gt.unsqueeze(0) if gt.dim() == 2 else gt
    r2 = radius2(p.shape, max_dist)
    H, W = p.shape[-2:]
    per = K.lib.mte_edge_match_workspace_bytes(1, H, W, r2)
    step = max(1, WORKSPACE_BUDGET // max(per, 1))
    if gt_of is not None:
        gt_of = torch.as_tensor(gt_of, dtype=torch.int32)
    parts = []
    for s in range(0, p.shape[0], step):
        sub = None if gt_of is None else gt_of[s:s + step]
        gg = g[s:s + step] if gt_of is None else g
        parts.append(edge_match(p[s:s + step], gg, r2, gt_of=sub))
    res = torch.cat(parts).cpu().numpy().astype(np.int64)
    bad = np.nonzero(res[:, 3])[0]
    if len(bad):
        raise K.MteError("edge matcher: instance %d ended with status %d (%s)" % (bad[0], res[bad[0], 3], STATUS.get(int(res[bad[0], 3]), "?")))
    return res[0, :3] if squeeze else res[:, :3]


def canny_fixed_scale(depth, min_depth, max_depth, thresholds, return_vis=False):
    """vis = uint8(clamp(depth, min_depth, max_depth) * float32(255 / max_depth)), then Canny for up to twelve threshold pairs:
    CUDA [H,W] or [B,H,W] -> float32 [P,B,H,W] (or [P,H,W]) with 255 on edges.  PARITY UNPINNED like canny_from_depth."""
    import ctypes
    from .. import kernels as K
    (d,), squeeze = _edge_maps(depth)
    B, H, W = d.shape
    P = len(thresholds)
    if not 1 <= P <= 12:
        raise ValueError("1..12 threshold pairs")
    th = (ctypes.c_int * (2 * P))(*[int(v) for pair in thresholds for v in pair])
    vis = torch.empty((B, H, W), dtype=torch.uint8, device=d.device) if return_vis else None
    state = torch.empty((P, B, H, W), dtype=torch.uint8, device=d.device)
    sweeps = 8
    flags = torch.empty(sweeps + 1, dtype=torch.int32, device=d.device)
    factor = float(np.float32(255.0 / float(max_depth)))
    K.lib.mte_canny_begin_fixed(d.data_ptr(), B, H, W, float(min_depth), float(max_depth), factor, P, ctypes.addressof(th),
                                vis.data_ptr() if return_vis else None, state.data_ptr(), K._stream())
    for _ in range(H * W // sweeps + 2):                # as canny_from_depth: a hard bound, one host read per 8 sweeps
        K.lib.mte_canny_propagate(state.data_ptr(), flags.data_ptr(), sweeps, P * B, H, W, K._stream())
        if int(flags[sweeps].item()) == 0:
            break
    else:
        raise K.MteError("Canny hysteresis did not reach a fixed point")
    edges = torch.empty((P, B, H, W), dtype=torch.float32, device=d.device)
    K.lib.mte_canny_finish(state.data_ptr(), edges.data_ptr(), P * B, H, W, K._stream())
    if squeeze:
        edges, vis = edges[:, 0], (vis[0] if return_vis else None)
    return (edges, vis) if return_vis else edges


def edge_from_depth(depth, new_shape, min_depth=0.0, max_depth=80.0, thresh_1=20, thresh_2=40):
    """edge.py:73-93 on a CUDA depth map [H,W] (or [B,H,W]): cv2.resize to new_shape = (W, H) (None: as it is), clamp to
    [min_depth, max_depth], uint8(depth * 255 / max_depth), cv2.Canny(thresh_1, thresh_2) -> float32 edge image, 255 on edges."""
    d = depth.float()
    if new_shape is not None and (int(new_shape[1]), int(new_shape[0])) != tuple(d.shape[-2:]):
        d = resize_linear(d, (int(new_shape[1]), int(new_shape[0])))
    return canny_fixed_scale(d, min_depth, max_depth, ((thresh_1, thresh_2),))[0]


def compute_rec_prec_f1(count_r, sum_r, count_p, sum_p):
    """eval_depth_edges.py:147-161, with its `+ (x == 0)` guards"""
    rec = count_r / (sum_r + (sum_r == 0))
    prec = count_p / (sum_p + (sum_p == 0))
    f1 = 2.0 * prec * rec / (prec + rec + ((prec + rec) == 0))
    return rec, prec, f1


def pr_evaluation(depths, gt_edges, edge_thresh_range=range(20, 241, 20), gt_crop=(44, 1197, 153, 371), min_depth=0.0, max_depth=80.0,
                  max_dist=0.002, timings=None):
    """eval_depth_edges.py:232-348.  depths: CUDA depth maps (metres), gt_edges: CUDA annotation images (0/255), one per frame
    (a multi-scale list is thinned to its first entries like upstream).  Per frame: every threshold's Canny image in one
    pass, cropped, and matched against the frame's one annotation; the instances go to the matcher in batches that share
    each frame's annotation, one host read per batch.  -> (precision_vec, recall_vec), one float per threshold.
    timings (a dict) receives the seconds spent in 'canny', 'match' and 'host_read' (each closed by a stream synchronise)."""
    import time
    from .. import kernels as K
    depths, gt_edges = list(depths), list(gt_edges)
    if len(gt_edges) > len(depths):
        gt_edges = gt_edges[0:len(gt_edges):int(len(gt_edges) / len(depths))]
    thresholds = [(int(t / 2), int(t)) for t in edge_thresh_range]
    T = len(thresholds)
    counts = np.zeros((T, 3), np.int64)                     # matched, n_pred, n_gt pooled over the frames
    tm = {"canny": 0.0, "match": 0.0, "host_read": 0.0}

    def lap(key, t0):
        if timings is not None:
            torch.cuda.current_stream().synchronize()
            tm[key] += time.perf_counter() - t0
        return time.perf_counter()

    pend_p, pend_g, pend_bytes = [], [], 0                  # frames of one cropped size wait here until the budget is used

    def flush():
        nonlocal pend_p, pend_g, pend_bytes
        if not pend_p:
            return
        t0 = time.perf_counter()
        p, g = torch.cat(pend_p), torch.stack(pend_g)
        gt_of = torch.arange(len(pend_g), dtype=torch.int32).repeat_interleave(T)
        res = edge_match(p, g, radius2(p.shape, max_dist), gt_of=gt_of)
        t0 = lap("match", t0)
        r = res.cpu().numpy().astype(np.int64)
        lap("host_read", t0)
        if r[:, 3].any():
            b = int(np.nonzero(r[:, 3])[0][0])
            raise K.MteError("edge matcher: instance %d ended with status %d (%s)" % (b, r[b, 3], STATUS.get(int(r[b, 3]), "?")))
        counts[:] += r[:, :3].reshape(-1, T, 3).sum(0)
        pend_p, pend_g, pend_bytes = [], [], 0

    for d, g in zip(depths, gt_edges):
        K._require_gpu(d)
        K._require_gpu(g)
        t0 = time.perf_counter()
        d = d.float()
        if tuple(d.shape) != tuple(g.shape):
            d = resize_linear(d, tuple(g.shape))
        e = canny_fixed_scale(d, min_depth, max_depth, thresholds)                     # [T,H,W]
        g = g.float()
        if len(gt_crop) > 0:
            e, g = e[:, gt_crop[2]:gt_crop[3], gt_crop[0]:gt_crop[1]], g[gt_crop[2]:gt_crop[3], gt_crop[0]:gt_crop[1]]
        e, g = e.contiguous(), g.contiguous()
        lap("canny", t0)
        if pend_p and pend_p[0].shape[1:] != e.shape[1:]:
            flush()
        nbytes = K.lib.mte_edge_match_workspace_bytes(T, e.shape[1], e.shape[2], 0)
        if pend_p and pend_bytes + nbytes > WORKSPACE_BUDGET:
            flush()
        pend_p.append(e); pend_g.append(g); pend_bytes += nbytes
    flush()
    if timings is not None:
        timings.update(tm)
    m, n_pred, n_gt = counts[:, 0].astype(np.float64), counts[:, 1].astype(np.float64), counts[:, 2].astype(np.float64)
    precision_vec, recall_vec = [], []
    for t in range(T):                                       # one pooled point per threshold, as upstream's loop
        rec, prec, _ = compute_rec_prec_f1(m[t:t + 1], n_gt[t:t + 1], m[t:t + 1], n_pred[t:t + 1])
        precision_vec.append(prec[0]); recall_vec.append(rec[0])
    return precision_vec, recall_vec


def mean_recall_at_precision_range(arr, small_lim=0.0, large_lim=1.0):
    """eval_depth_edges.py:365-375 on the [T,2] (precision, recall) points: mean of the recall interpolated at precision
    small_lim, small_lim + 0.01, ... < large_lim, clipped to [0, 1]."""
    arr = np.asarray(arr, np.float64)
    interp_x = np.array(range(int(small_lim * 100), int(large_lim * 100))) / 100
    interp_y = np.interp(interp_x, arr[:, 0], arr[:, 1])
    interp_y[interp_y < 0] = 0
    interp_y[interp_y > 1] = 1
    return np.mean(interp_y)


def read_edge_png(path):
    """annotation PNG (1-bit or 8-bit) -> float32 numpy [H,W] on the 0 / 255 scale (first channel, as cv2.imread(...)[:, :, 0])"""
    from PIL import Image
    im = Image.open(path)
    if im.mode == '1':
        return np.asarray(im, dtype=np.uint8).astype(np.float32) * 255.0
    a = np.asarray(im.convert('RGB') if im.mode not in ('L',) else im)
    return np.ascontiguousarray(a[..., 2] if a.ndim == 3 else a).astype(np.float32)


def evaluate_lists(pred_paths, gt_paths, range_min=0.12, range_max=0.65, **kw):
    """.npy predictions and .png annotations -> (precision_vec, recall_vec, AUC over all range, AUC over partial range)"""
    depths = [torch.from_numpy(np.load(p.strip()).astype(np.float32)).cuda() for p in pred_paths]
    gts = [torch.from_numpy(read_edge_png(p.strip())).cuda() for p in gt_paths]
    precision_vec, recall_vec = pr_evaluation(depths, gts, **kw)
    pr = np.vstack((precision_vec, recall_vec)).transpose()
    return precision_vec, recall_vec, mean_recall_at_precision_range(pr), mean_recall_at_precision_range(pr, range_min, range_max)
