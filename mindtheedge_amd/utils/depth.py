"""inv2depth / depth2inv (reference packnet_sfm/utils/depth.py:104-144).  The training path fuses both into the loss
kernels; these helpers serve inference post-processing (H3) on the small fp32 output maps.  Further down: the validation metrics and
the visualisation of the inference side on the device (viz_inv_depth, depth_log_color, write_depth; csrc/depth_viz.hip)."""
import torch


def inv2depth(inv_depth):
    if isinstance(inv_depth, (list, tuple)):
        return [inv2depth(i) for i in inv_depth]
    return 1. / inv_depth.clamp(min=1e-6)


def depth2inv(depth):
    if isinstance(depth, (list, tuple)):
        return [depth2inv(d) for d in depth]
    inv = 1. / depth.clamp(min=1e-6)
    inv[depth <= 0.] = 0.
    return inv


# ---- validation metrics on device (reference utils/depth.py:202-361) ---------------------------

_FUSE_METHODS = {'mean': 0, 'max': 1, 'min': 2}
_SCALE_FNS = {'resize': 0, 'top-center': 1}


def _f32_maps(*tensors):
    from .. import kernels as K
    out = []
    for t in tensors:
        K._require_gpu(t)
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError("expected a [B,1,H,W] map, got {}".format(tuple(t.shape)))
        out.append(t.detach().float().contiguous())
    return out


def fuse_inv_depth(inv_depth, inv_depth_hat, method='mean'):
    """Reference utils/depth.py:202-227 (tiny elementwise op; the fused kernel below does not call it)."""
    if method == 'mean':
        return 0.5 * (inv_depth + inv_depth_hat)
    if method == 'max':
        return torch.max(inv_depth, inv_depth_hat)
    if method == 'min':
        return torch.min(inv_depth, inv_depth_hat)
    raise ValueError('Unknown post-process method {}'.format(method))


def post_process_inv_depth(inv_depth, inv_depth_flipped, method='mean'):
    """Flip-TTA fusion of an inverse depth map with the prediction on the mirrored image (reference
    utils/depth.py:230-256) as one kernel: un-flip, fuse, and blend the 5 % border ramps."""
    from .. import kernels as K
    if method not in _FUSE_METHODS:
        raise ValueError('Unknown post-process method {}'.format(method))
    a, f = _f32_maps(inv_depth, inv_depth_flipped)
    if a.shape != f.shape:
        raise ValueError("shape mismatch {} vs {}".format(tuple(a.shape), tuple(f.shape)))
    out = torch.empty_like(a)
    B, _, H, W = a.shape
    K.lib.mte_post_process_inv_depth(a.data_ptr(), f.data_ptr(), out.data_ptr(), B, H, W, _FUSE_METHODS[method], K._stream())
    return out


def compute_depth_metrics(config, gt, pred, use_gt_scale=True):
    """(abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) of ``pred`` against ``gt``, averaged over the batch, as a
    float32[7] DEVICE tensor (reference utils/depth.py:259-325; ``config`` carries crop / min_depth / max_depth /
    scale_output as there).  No host synchronisation: valid-pixel selection, scale_depth, the two medians and the
    reductions all run inside ``mte_depth_metrics``."""
    from .. import kernels as K
    scale_fn = getattr(config, 'scale_output', 'resize')
    if scale_fn not in _SCALE_FNS:
        raise NotImplementedError('Depth scale function {} not implemented.'.format(scale_fn))
    g, p = _f32_maps(gt, pred)
    B, _, H, W = g.shape
    if p.shape[0] != B:
        raise ValueError("batch mismatch {} vs {}".format(B, p.shape[0]))
    h, w = p.shape[-2:]
    nbytes = K.lib.mte_depth_metrics_workspace_bytes(B)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    out = torch.empty(7, dtype=torch.float32, device=g.device)
    K.lib.mte_depth_metrics(g.data_ptr(), p.data_ptr(), B, H, W, h, w, _SCALE_FNS[scale_fn], int(getattr(config, 'crop', '') == 'garg'),
                            float(config.min_depth), float(config.max_depth), int(bool(use_gt_scale)), ws.data_ptr(), nbytes,
                            out.data_ptr(), K._stream())
    return out


# ---- visualisation on device (csrc/depth_viz.hip; reference utils/depth.py:36-101, infer_edges.py:355-366) ----------

_TABLES = {}


def color_table(name, rule, device=None):
    """The 256 x 3 table of ``plasma`` or ``Spectral`` (utils/colormaps.json, float64 as text, written by tools/make_colormaps.py) as uint8 under
    the caller's rule: 'rint' = ``cm(x) * 255`` handed to cv2.imwrite (round half to even, saturating; parity-unpinned against OpenCV's
    saturate_cast), 'trunc' = ``(cm(x) * 255).astype(np.uint8)``.  device None -> the numpy array, else a cached CUDA tensor."""
    import json
    import os
    import numpy as np
    key = (name, rule)
    if key not in _TABLES:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'colormaps.json')) as f:
            z = json.load(f)
        if name not in z or name == 'matplotlib_version':
            raise ValueError("colormap {!r}: only {} ship with the package".format(name, [k for k in z if k != 'matplotlib_version']))
        t = np.array(z[name], dtype=np.float64) * 255
        if rule == 'rint':
            t = np.clip(np.rint(t), 0, 255).astype(np.uint8)
        elif rule == 'trunc':
            t = t.astype(np.uint8)
        else:
            raise ValueError("rule is 'rint' or 'trunc'")
        _TABLES[key] = np.ascontiguousarray(t)
    if device is None:
        return _TABLES[key]
    dkey = (name, rule, str(device))
    if dkey not in _TABLES:
        _TABLES[dkey] = torch.from_numpy(_TABLES[key]).to(device)
    return _TABLES[dkey]


def percentile_position(n, q):
    """Where ``np.percentile(a, q)`` (method 'linear') looks in a sorted float32 array of n values: (k, gamma) with k the lower neighbour's
    index and gamma the float32 weight.  numpy >= 2 divides q by float32(100) and forms the virtual index (n - 1) * q in float32 when the data
    are float32 (numpy/lib/_function_base_impl.py: percentile, _quantile, _get_indexes, _get_gamma)."""
    import numpy as np
    quantile = np.true_divide(q, np.float32(100))
    virtual = np.float32((int(n) - 1) * quantile)
    if virtual >= n - 1:
        return int(n) - 1, np.float32(virtual - np.float32(-1))
    if virtual < 0:
        return 0, np.float32(virtual)
    prev = np.floor(virtual)
    return int(prev), np.float32(virtual - prev)


def percentile_lerp(a, b, gamma):
    """numpy's _lerp for float32 neighbours a <= b: a + (b - a) * t below t = 0.5, b - (b - a) * (1 - t) from there on, every step float32."""
    import numpy as np
    a, b, t = np.float32(a), np.float32(b), np.float32(gamma)
    diff = np.float32(b - a)
    if t >= 0.5:
        return np.float32(b - np.float32(diff * np.float32(1 - t)))
    return np.float32(a + np.float32(diff * t))


def order_stats(x, k, positive_only=False):
    """x: CUDA float32 [B,n] (or [n] together with a list of k: the same values under several k); k: int or a list of B ints.
    -> (float32 [B,2] device tensor: the k-th and (k+1)-th smallest (0-based, clamped to the last), int32 [B] device tensor: how many values
    took part).  Exact; inputs must be finite.  No host read."""
    import numpy as np
    from .. import kernels as K
    K._require_gpu(x)
    src = x.detach().float().contiguous()
    ks = [int(k)] if np.isscalar(k) else [int(v) for v in k]
    if src.dim() == 1:
        B, n, stride = len(ks), int(src.shape[0]), 0
    else:
        B, n = int(src.shape[0]), int(src[0].numel())
        stride = n
        if len(ks) == 1:
            ks = ks * B
    if len(ks) != B:
        raise ValueError("{} images, {} ranks".format(B, len(ks)))
    dev = src.device
    kd = torch.tensor(ks, dtype=torch.int32).to(dev)
    out = torch.empty((B, 2), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    work = torch.empty(K.lib.mte_order_stats_work_bytes(B) // 4, dtype=torch.int32, device=dev)
    K.lib.mte_order_stats_f32(src.data_ptr(), stride, B, n, kd.data_ptr(), int(bool(positive_only)), out.data_ptr(), cnt.data_ptr(),
                              work.data_ptr(), K._stream())
    return out, cnt


def percentile_f32(x, q, positive_only=False):
    """``np.percentile(x, q)`` (or of ``x[x > 0]``) of a CUDA float32 tensor of finite values, bit for bit, as np.float32.  One 8-byte host
    read (two with positive_only: the count first, as k depends on it).  An empty selection raises like numpy's IndexError."""
    import numpy as np
    flat = x.detach().float().reshape(-1)
    n = int(flat.numel())
    if positive_only:
        _, cnt = order_stats(flat, [0], True)
        n = int(cnt.item())
    if n == 0:
        raise IndexError("percentile of an empty selection")
    k, gamma = percentile_position(n, q)
    pair, _ = order_stats(flat, [k], positive_only)
    a, b = pair[0].cpu().numpy()
    return percentile_lerp(a, b, gamma)


def colormap_u8(x, table, divisor=None, lo_hi=None):
    """x: CUDA float32 [B,H,W]; table: uint8 [256,3] CUDA; divisor float32 [B] or lo_hi float32 [B,2] (the log mode) -> uint8 [B,H,W,3]."""
    from .. import kernels as K
    K._require_gpu(x)
    src = x.detach().float().contiguous()
    B, H, W = (int(s) for s in src.shape)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=src.device)
    K.lib.mte_colormap_u8(src.data_ptr(), B, H, W, divisor.data_ptr() if divisor is not None else None,
                          lo_hi.data_ptr() if lo_hi is not None else None, table.data_ptr(), out.data_ptr(), K._stream())
    return out


def viz_divisor(normalizer):
    """What ``inv_depth /= (normalizer + 1e-6)`` divides a float32 array by: the float32 sum for a float32 normalizer (np.percentile's
    result), the rounded double sum for a Python float."""
    import numpy as np
    return np.float32(normalizer + 1e-6)


def viz_inv_depth(inv_depth, normalizer=None, percentile=95, colormap='plasma', filter_zeros=False):
    """Reference utils/depth.py:67-101 on a CUDA tensor [1,H,W] or [H,W] -> uint8 [H,W,3] on the device: what the reference's callers
    write after ``* 255`` through cv2.imwrite (RGB order; the reference's float image in [0,1] is this / 255 up to that rounding).  The
    input is not modified (upstream divides a numpy input in place)."""
    import numpy as np
    from .. import kernels as K
    K._require_gpu(inv_depth)
    x = inv_depth.detach().float()
    if x.dim() == 3:
        x = x.squeeze(0)
    if x.dim() != 2:
        raise ValueError("expected [1,H,W] or [H,W], got {}".format(tuple(inv_depth.shape)))
    if normalizer is None:
        normalizer = percentile_f32(x, percentile, positive_only=filter_zeros)
    d = torch.from_numpy(np.array([viz_divisor(normalizer)], dtype=np.float32)).to(x.device)
    return colormap_u8(x.unsqueeze(0), color_table(colormap, 'rint', x.device), divisor=d)[0]


def log_color_range(vmin, vmax):
    """(lo, hi) of the log colouring: lo = float32(log(min)), hi = float32(float32(log(max)) - lo); the logs in double, rounded once."""
    import numpy as np
    lo = np.float32(np.log(np.float64(vmin)))
    return lo, np.float32(np.float32(np.log(np.float64(vmax))) - lo)


def depth_log_color(depth):
    """The ``Spectral`` image of infer_edges.py:355-366: log(depth) shifted to start at 0, divided by its maximum, looked up with matplotlib's
    index rule, ``* 255`` truncated.  depth: CUDA [H,W] (or [1,H,W]) of finite values > 0 -> uint8 [H,W,3] on the device.  log is monotone,
    so the range comes from the frame's minimum and maximum (one 16-byte host read)."""
    import numpy as np
    from .. import kernels as K
    K._require_gpu(depth)
    x = depth.detach().float()
    if x.dim() == 3:
        x = x.squeeze(0)
    if x.dim() != 2:
        raise ValueError("expected [1,H,W] or [H,W], got {}".format(tuple(depth.shape)))
    n = int(x.numel())
    pair, _ = order_stats(x.reshape(-1), [0, n - 2])
    pair = pair.cpu().numpy()
    lo, hi = log_color_range(pair[0, 0], pair[1, 1])
    lo_hi = torch.from_numpy(np.array([[lo, hi]], dtype=np.float32)).to(x.device)
    return colormap_u8(x.unsqueeze(0), color_table('Spectral', 'trunc', x.device), lo_hi=lo_hi)[0]


def write_depth(filename, depth, intrinsics=None):
    """Reference utils/depth.py:36-64: ``.npz`` with ``depth`` and ``intrinsics``; ``.png`` = ``(depth * 256).int()`` as ToPILImage writes an
    int32 tensor: a 32-bit 'I' image, which PIL stores as a 16-bit PNG (values clipped to 0..65535 = depths below 256 m)."""
    import numpy as np
    if torch.is_tensor(depth):
        depth = depth.detach().squeeze().cpu()
    if torch.is_tensor(intrinsics):
        intrinsics = intrinsics.detach().cpu()
    if filename.endswith('.npz'):
        np.savez_compressed(filename, depth=depth, intrinsics=intrinsics)
    elif filename.endswith('.png'):
        from PIL import Image
        d = depth if torch.is_tensor(depth) else torch.as_tensor(np.asarray(depth))
        Image.fromarray(np.clip((d * 256).int().numpy(), 0, 65535).astype(np.uint16)).save(filename)
    else:
        raise NotImplementedError('Depth filename not valid.')
