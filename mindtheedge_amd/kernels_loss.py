"""Loss-side and optimizer-side bindings of the C ABI (split out of kernels.py in round 6: the fused depth-edge + silog losses, the bilinear resize of the
edge loss and the host form of the Adam step).  Reference: packnet_sfm/losses/grad_loss.py:15-177 (GradLayer / GradLoss / comp_cross_entropy),
losses/supervised_loss.py (silog), models/SemiSupEdgeModel.py (all-scales edge loss), models/model_wrapper.py:142-180 (Adam).  `kernels` re-exports every
name defined here, so callers keep writing kernels.DepthLossesFn etc."""
import ctypes

import torch

from . import _lib as _L
from . import kernels as _K          # (imported at the END of kernels.py: its helpers are looked up at call time)
from ._lib import MteError          # noqa: F401  (the library handle is kernels.lib at call time: bench.py swaps it for a timing proxy)


class EdgeLossFn(torch.autograd.Function):
    """weight * class-balanced BCE of sigmoid(directional Sobel(depth) - thresh) against soft edge labels.
    GradLoss.forward ('cross_entropy'), grad_loss.py:122-219, fused with inv2depth when from_inv."""

    @staticmethod
    def forward(ctx, pred, edge, normal, mask, weight, pos_to_neg, from_inv, is_grad, is_sigmoid, thresh, want_gmap):
        B, _, H, W = edge.shape
        pred, edge = pred.contiguous().float(), edge.contiguous().float()
        normal = None if normal is None else normal.contiguous().float()
        mask = None if mask is None else mask.contiguous().float()
        dev = pred.device
        sums = _K._zeros((_K.lib.mte_edge_loss_sums_elems(B, H, W),), torch.float64, dev)
        coef = torch.empty((2 * B + 1,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        gmap = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_gmap else None
        st = _K._stream()
        _K.lib.mte_edge_loss_fwd(pred.data_ptr(), edge.data_ptr(), _K._ptr(normal), _K._ptr(mask), sums.data_ptr(), _K._ptr(gmap),
                              B, H, W, int(from_inv), int(is_grad), int(is_sigmoid), float(thresh), st)
        _K.lib.mte_edge_loss_finalize(sums.data_ptr(), B, edge.numel(), float(weight), float(pos_to_neg), int(mask is not None),
                                   1.0, 0, loss.data_ptr(), coef.data_ptr(), st)
        ctx.save_for_backward(pred, edge, normal, mask, coef)
        ctx.cfg = (B, H, W, int(from_inv), int(is_grad), int(is_sigmoid), float(thresh))
        if want_gmap:
            ctx.mark_non_differentiable(gmap)
        return loss, gmap

    @staticmethod
    def backward(ctx, gloss, _g):
        pred, edge, normal, mask, coef = ctx.saved_tensors
        B, H, W, from_inv, is_grad, is_sigmoid, thresh = ctx.cfg
        dpred = torch.empty_like(pred)
        gl = gloss.contiguous().float()
        _K.lib.mte_edge_loss_bwd(pred.data_ptr(), edge.data_ptr(), _K._ptr(normal), _K._ptr(mask), coef.data_ptr(), gl.data_ptr(),
                              dpred.data_ptr(), B, H, W, from_inv, is_grad, is_sigmoid, thresh, _K._stream())
        return (dpred,) + (None,) * 10


class EdgeLossKindFn(torch.autograd.Function):
    """weight * (base + dice) for the other edge-loss choices of GradLoss.forward (grad_loss.py:139-156): kind 0 class-balanced BCE
    ('cross_entropy', only reached here with the dice term), 1 attention_loss2 with one alpha for the batch ('attention_loss'),
    2 attention_loss2 with the per-pixel 15x15 box alpha ('spatially_adaptive') -- losses/attention_loss.py:21-49; dice adds
    1000 (sum p^2 + sum t^2 + 1e-4) / (2 sum p t + 1e-4) / N.  One forward and one backward launch, fused with inv2depth when from_inv."""

    @staticmethod
    def forward(ctx, pred, edge, normal, mask, kind, dice, weight, pos_to_neg, from_inv, is_grad, is_sigmoid, thresh, want_gmap):
        B, _, H, W = edge.shape
        pred, edge = pred.contiguous().float(), edge.contiguous().float()
        normal = None if normal is None else normal.contiguous().float()
        mask = None if mask is None else mask.contiguous().float()
        if tuple(pred.shape) != tuple(edge.shape) or (normal is not None and tuple(normal.shape) != tuple(edge.shape)):
            raise MteError("prediction / label shapes differ: %s vs %s" % (tuple(pred.shape), tuple(edge.shape)))
        if mask is not None and tuple(mask.shape) != tuple(edge.shape):
            raise MteError("mask shape %s differs from the label's %s" % (tuple(mask.shape), tuple(edge.shape)))
        dev = pred.device
        work = torch.empty((_K.lib.mte_edge_loss_kind_work_elems(B, H, W),), dtype=torch.float64, device=dev)
        coef = torch.empty((2 * B + 5,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        gmap = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_gmap else None
        cfg = (B, H, W, int(kind), int(dice), int(from_inv), int(is_grad), int(is_sigmoid), float(thresh))
        _K.lib.mte_edge_loss_kind_fwd(pred.data_ptr(), edge.data_ptr(), _K._ptr(normal), _K._ptr(mask), _K._ptr(gmap), *cfg,
                                      float(weight), float(pos_to_neg), work.data_ptr(), loss.data_ptr(), coef.data_ptr(), _K._stream())
        ctx.save_for_backward(pred, edge, normal, mask, coef)
        ctx.cfg = cfg
        if want_gmap:
            ctx.mark_non_differentiable(gmap)
        return loss, gmap

    @staticmethod
    def backward(ctx, gloss, _g):
        pred, edge, normal, mask, coef = ctx.saved_tensors
        dpred = torch.empty_like(pred)
        gl = gloss.contiguous().float()
        _K.lib.mte_edge_loss_kind_bwd(pred.data_ptr(), edge.data_ptr(), _K._ptr(normal), _K._ptr(mask), coef.data_ptr(), gl.data_ptr(),
                                      dpred.data_ptr(), *ctx.cfg, _K._stream())
        return (dpred,) + (None,) * 12


class BilinearResizeFn(torch.autograd.Function):
    """F.interpolate(x, size=(H, W), mode='bilinear') for fp32 [B,1,h,w] maps -- the resize GradLoss.forward applies when the
    prediction and the label differ in size (grad_loss.py:127)."""

    @staticmethod
    def forward(ctx, x, H, W):
        x = x.contiguous().float()
        B, C, h, w = x.shape
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        _K.lib.mte_resize_bilinear_fwd(x.data_ptr(), y.data_ptr(), B * C, h, w, H, W, _K._stream())
        ctx.geom = (B, C, h, w, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, h, w, H, W = ctx.geom
        dy = dy.contiguous().float()
        dx = torch.empty((B, C, h, w), dtype=torch.float32, device=dy.device)
        _K.lib.mte_resize_bilinear_bwd(dy.data_ptr(), dx.data_ptr(), B * C, h, w, H, W, _K._stream())
        return dx, None, None


class _EdgeScale(ctypes.Structure):       # mte_edge_scale of include/mte_kernels.h
    _fields_ = [("pred", ctypes.c_void_p), ("edge", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("gmap", ctypes.c_void_p), ("dpred", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int)]


class DepthLossesFn(torch.autograd.Function):
    """Every loss term of SemiSupEdgeModel.forward (models/SemiSupEdgeModel.py:137-151) in ONE forward and ONE backward launch:
    the depth-edge loss of all scales (compute_edge_loss_with_all_scales, :164-198; GradLoss 'cross_entropy' fused with
    inv2depth) and, when `gt_depth` is given, the sparse silog loss of scale 0 -- both read the same inverse-depth maps.
    -> fp32 [S] (+1): weight * balanced BCE per scale, then the silog loss when gt_depth is given."""

    @staticmethod
    def forward(ctx, weight, pos_to_neg, thresh, from_inv, mask, gt_depth, edges, normals, *preds):
        S = len(preds)
        B = preds[0].shape[0]
        dev = preds[0].device
        preds = [p.contiguous().float() for p in preds]
        edges = [e.contiguous().float() for e in edges]
        normals = [None if n is None else n.contiguous().float() for n in normals]
        mask = None if mask is None else mask.contiguous().float()
        if mask is not None and any(tuple(mask.shape[-2:]) != tuple(p.shape[-2:]) for p in preds):
            raise MteError("one full-resolution mask for every scale is an upstream bug that only works with mask=None")
        gt = None if gt_depth is None else gt_depth.contiguous().float()
        arr = (_EdgeScale * S)()
        for o, p, e, n in zip(arr, preds, edges, normals):
            if tuple(p.shape) != tuple(e.shape) or (n is not None and tuple(n.shape) != tuple(e.shape)):
                raise MteError("prediction / label shapes differ: %s vs %s" % (tuple(p.shape), tuple(e.shape)))
            o.pred, o.edge, o.normal, o.mask = p.data_ptr(), e.data_ptr(), _K._ptr(n), _K._ptr(mask)
            o.gmap = o.dpred = None
            o.H, o.W = p.shape[-2], p.shape[-1]
        work = _K._zeros((_K.lib.mte_edge_loss_work_elems(ctypes.addressof(arr), S, B),), torch.float64, dev)
        losses = torch.empty((S + (1 if gt is not None else 0),), dtype=torch.float32, device=dev)
        coef = torch.empty((S * (2 * B + 1),), dtype=torch.float32, device=dev)
        aux = torch.empty((2,), dtype=torch.float32, device=dev) if gt is not None else None
        _K.lib.mte_edge_loss_multi_fwd(ctypes.addressof(arr), S, B, int(from_inv), 1, 1, float(thresh), float(weight), float(pos_to_neg),
                                    _K._ptr(gt), work.data_ptr(), losses.data_ptr(), coef.data_ptr(),
                                    losses.data_ptr() + 4 * S if gt is not None else 0, _K._ptr(aux), _K._stream())
        ctx.save_for_backward(coef, mask, gt, aux, *preds, *edges, *[n for n in normals if n is not None])
        ctx.cfg = (S, B, int(from_inv), float(thresh), [n is not None for n in normals])
        return losses

    @staticmethod
    def backward(ctx, glosses):
        S, B, from_inv, thresh, has_n = ctx.cfg
        coef, mask, gt, aux = ctx.saved_tensors[:4]
        rest = ctx.saved_tensors[4:]
        preds, edges, nrm = rest[:S], rest[S:2 * S], list(rest[2 * S:])
        normals = [nrm.pop(0) if h else None for h in has_n]
        dpreds = [torch.empty_like(p) for p in preds]
        arr = (_EdgeScale * S)()
        for o, p, e, n, d in zip(arr, preds, edges, normals, dpreds):
            o.pred, o.edge, o.normal, o.mask, o.gmap, o.dpred = p.data_ptr(), e.data_ptr(), _K._ptr(n), _K._ptr(mask), None, d.data_ptr()
            o.H, o.W = p.shape[-2], p.shape[-1]
        gl = glosses.contiguous().float()
        _K.lib.mte_edge_loss_multi_bwd(ctypes.addressof(arr), S, B, from_inv, 1, 1, thresh, coef.data_ptr(), gl.data_ptr(), _K._ptr(gt),
                                    _K._ptr(aux), gl.data_ptr() + 4 * S if gt is not None else 0, _K._stream())
        return (None,) * 8 + tuple(dpreds)


class _EdgePairScale(ctypes.Structure):   # mte_edge_pair_scale of include/mte_kernels.h
    _fields_ = [("pred", ctypes.c_void_p * 2), ("dpred", ctypes.c_void_p * 2), ("edge", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("H", ctypes.c_int), ("W", ctypes.c_int)]


def _pair_raw(name, *args):
    """A pair entry point called raw, to see MTE_ERR_UNSUPPORTED (-3, include/mte_kernels.h) instead of an exception: -> True when it ran"""
    rc = getattr(_L.lib.load(), name)(*args)
    if rc not in (0, -3):
        raise MteError("%s failed: %s" % (name, _L._ERRORS.get(rc, rc)))
    return rc == 0


class DepthLossesPairFn(torch.autograd.Function):
    """Every loss term of SemiSupEdgeCompletionModel.forward (models/SemiSupEdgeCompletionModel.py:128-165) in ONE forward and ONE backward
    launch: the depth-edge loss of all scales and, when `gt_depth` is given, the sparse silog loss of scale 0, for the RGB predictions
    (branch 0) and the RGB+LiDAR predictions (branch 1) against the same labels, which are read once (the <2> instantiation of csrc/edge_fast.hpp, behind the pair entry points of csrc/edge_loss.hip).
    apply(weight, pos_to_neg, thresh, gt_depth, edges, normals, *preds_rgb, *preds_rgbd) -> fp32 [2, S (+1)]: per branch weight * balanced BCE
    per scale, then that branch's silog loss when gt_depth is given.  Where the library answers MTE_ERR_UNSUPPORTED (a scale outside the
    training configuration: no normals, W % 4 != 0, an unaligned base) the same numbers come from two DepthLossesFn applications."""

    @staticmethod
    def _scales(preds, edges, normals, dpreds):
        S = len(edges)
        arr = (_EdgePairScale * S)()
        for s, o in enumerate(arr):
            for br in range(2):
                o.pred[br] = preds[br * S + s].data_ptr()
                o.dpred[br] = None if dpreds is None else dpreds[br * S + s].data_ptr()
            o.edge, o.normal = edges[s].data_ptr(), _K._ptr(normals[s])
            o.H, o.W = edges[s].shape[-2], edges[s].shape[-1]
        return arr

    @staticmethod
    def forward(ctx, weight, pos_to_neg, thresh, gt_depth, edges, normals, *preds):
        S = len(edges)
        if len(preds) != 2 * S or not 1 <= S <= 4:
            raise MteError("%d label scales (1 to 4) need %d predictions, got %d" % (S, 2 * S, len(preds)))
        B = preds[0].shape[0]
        dev = preds[0].device
        preds = [p.contiguous().float() for p in preds]
        edges = [e.contiguous().float() for e in edges]
        normals = [None if n is None else n.contiguous().float() for n in normals]
        gt = None if gt_depth is None else gt_depth.contiguous().float()
        for i, p in enumerate(preds):
            e, n = edges[i % S], normals[i % S]
            if tuple(p.shape) != tuple(e.shape) or (n is not None and tuple(n.shape) != tuple(e.shape)):
                raise MteError("prediction / label shapes differ: %s vs %s" % (tuple(p.shape), tuple(e.shape)))
        arr = DepthLossesPairFn._scales(preds, edges, normals, None)
        n_out = S + (1 if gt is not None else 0)
        work = _K._zeros((_K.lib.mte_edge_loss_pair_work_elems(ctypes.addressof(arr), S, B),), torch.float64, dev)
        losses = torch.empty((2, S), dtype=torch.float32, device=dev)
        coef = torch.empty((2 * S * (2 * B + 1),), dtype=torch.float32, device=dev)
        sil = torch.empty((2,), dtype=torch.float32, device=dev) if gt is not None else None
        aux = torch.empty((4,), dtype=torch.float32, device=dev) if gt is not None else None
        ctx.pair = _pair_raw("mte_edge_loss_pair_fwd", ctypes.addressof(arr), S, B, float(thresh), float(weight), float(pos_to_neg), _K._ptr(gt),
                             work.data_ptr(), losses.data_ptr(), coef.data_ptr(), _K._ptr(sil), _K._ptr(aux), _K._stream())
        ctx.cfg = (S, B, float(thresh), [n is not None for n in normals])
        if ctx.pair:
            ctx.save_for_backward(coef, gt, aux, *preds, *edges, *[n for n in normals if n is not None])
            return losses if gt is None else torch.cat([losses, sil[:, None]], dim=1)
        # outside the training configuration: two single launches on the existing kernels, the same outputs
        ctx.single = []
        out = torch.empty((2, n_out), dtype=torch.float32, device=dev)
        for br in range(2):
            with torch.enable_grad():
                leaves = [p.detach().requires_grad_(True) for p in preds[br * S:(br + 1) * S]]
                one = DepthLossesFn.apply(weight, pos_to_neg, thresh, True, None, gt, edges, normals, *leaves)
            ctx.single.append((leaves, one))
            out[br] = one.detach()
        return out

    @staticmethod
    def backward(ctx, glosses):
        S, B, thresh, has_n = ctx.cfg
        gl = glosses.contiguous().float()
        if not ctx.pair:
            grads = []
            for br, (leaves, one) in enumerate(ctx.single):
                grads += list(torch.autograd.grad(one, leaves, gl[br]))
            return (None,) * 6 + tuple(grads)
        coef, gt, aux = ctx.saved_tensors[:3]
        rest = ctx.saved_tensors[3:]
        preds, edges, nrm = rest[:2 * S], rest[2 * S:3 * S], list(rest[3 * S:])
        normals = [nrm.pop(0) if h else None for h in has_n]
        dpreds = [torch.empty_like(p) for p in preds]
        arr = DepthLossesPairFn._scales(preds, edges, normals, dpreds)
        gedge = gl[:, :S].contiguous()
        gsil = gl[:, S].contiguous() if gt is not None else None
        if not _pair_raw("mte_edge_loss_pair_bwd", ctypes.addressof(arr), S, B, thresh, coef.data_ptr(), gedge.data_ptr(), _K._ptr(gt),
                         _K._ptr(aux), _K._ptr(gsil), _K._stream()):
            raise MteError("mte_edge_loss_pair_bwd refused what mte_edge_loss_pair_fwd took")
        return (None,) * 6 + tuple(dpreds)


class SilogFn(torch.autograd.Function):
    """10*sqrt(mean(d^2) - 0.85*mean(d)^2), d = log(10(inv+1e-5)) - log(10/depth) over depth > 0
    (SupervisedLoss 'sparse-silog' at scale 0: supervised_loss.py:57-69,155-216 + depth2inv)."""

    @staticmethod
    def forward(ctx, inv, depth):
        inv, depth = inv.contiguous().float(), depth.contiguous().float()
        dev = inv.device
        sums = torch.empty((3,), dtype=torch.float64, device=dev)
        aux = torch.empty((2,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _K.lib.mte_silog_fwd(inv.data_ptr(), depth.data_ptr(), inv.numel(), sums.data_ptr(), 1.0, 0, loss.data_ptr(), aux.data_ptr(), _K._stream())
        ctx.save_for_backward(inv, depth, aux)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        inv, depth, aux = ctx.saved_tensors
        dinv = torch.empty_like(inv)
        gl = gloss.contiguous().float()
        _K.lib.mte_silog_bwd(inv.data_ptr(), depth.data_ptr(), aux.data_ptr(), gl.data_ptr(), dinv.data_ptr(), inv.numel(), 0, _K._stream())
        return dinv, None


class _SupScale(ctypes.Structure):        # mte_sup_scale of include/mte_kernels.h
    _fields_ = [("pred", ctypes.c_void_p), ("dpred", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int)]


class _UpsampleMap(ctypes.Structure):     # mte_upsample_map of include/mte_kernels.h
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int)]


# supervised methods in the order get_loss_func tests the suffixes (supervised_loss.py:73-87): the id the kernels take
SUPERVISED_METHODS = ('l1', 'mse', 'berhu', 'silog', 'abs_rel')


class SupervisedLossFn(torch.autograd.Function):
    """sum_s f(inv_s + 1e-5, depth2inv(depth) nearest-resized to scale s) / n over the n = len(inv_depths) <= 4 scales
    (SupervisedLoss.calculate_loss / forward, supervised_loss.py:155-216).  method: index into SUPERVISED_METHODS; sparse keeps the
    pixels with depth > 0.  depth: metric depth [B,1,Hd,Wd] of any size.  One forward launch (two for BerHu) and one backward launch."""

    @staticmethod
    def forward(ctx, method, sparse, depth, *inv_depths):
        preds = [p.contiguous().float() for p in inv_depths]
        depth = depth.contiguous().float()
        _K._require_gpu(preds[0])
        B = preds[0].shape[0]
        if not 1 <= len(preds) <= 4:
            raise MteError("1 to 4 scales, got %d" % len(preds))
        for p in preds + [depth]:
            if p.dim() != 4 or p.shape[0] != B or p.shape[1] != 1:
                raise MteError("maps must be [B,1,H,W] with one B, got %s" % (tuple(p.shape),))
        arr = SupervisedLossFn._scales(preds, None)
        dev = preds[0].device
        work = torch.empty((_K.lib.mte_supervised_loss_work_elems(ctypes.addressof(arr), len(preds), B),), dtype=torch.float64, device=dev)
        coef = torch.empty((16,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _K.lib.mte_supervised_loss_fwd(ctypes.addressof(arr), len(preds), B, depth.data_ptr(), depth.shape[2], depth.shape[3], int(method),
                                       int(sparse), work.data_ptr(), loss.data_ptr(), None, coef.data_ptr(), _K._stream())
        ctx.save_for_backward(depth, coef, *preds)
        ctx.cfg = (int(method), int(sparse))
        return loss

    @staticmethod
    def _scales(preds, dpreds):
        arr = (_SupScale * len(preds))()
        for i, (o, p) in enumerate(zip(arr, preds)):
            o.pred, o.dpred, o.H, o.W = p.data_ptr(), (None if dpreds is None else dpreds[i].data_ptr()), p.shape[2], p.shape[3]
        return arr

    @staticmethod
    def backward(ctx, gloss):
        depth, coef, *preds = ctx.saved_tensors
        dpreds = [torch.empty_like(p) for p in preds]
        arr = SupervisedLossFn._scales(preds, dpreds)
        gl = gloss.contiguous().float()
        _K.lib.mte_supervised_loss_bwd(ctypes.addressof(arr), len(preds), preds[0].shape[0], depth.data_ptr(), depth.shape[2], depth.shape[3],
                                       *ctx.cfg, coef.data_ptr(), gl.data_ptr(), _K._stream())
        return (None, None, None) + tuple(dpreds)


class NearestUpsampleFn(torch.autograd.Function):
    """[F.interpolate(x, size=(H, W), mode='nearest') for x in maps] for fp32 [B,1,h,w] maps with H % h == 0 and W % w == 0 -- the
    upsample_depth_maps step of SfmModel (model_utils.py:154-176).  One forward and one backward launch for all maps."""

    @staticmethod
    def forward(ctx, H, W, *maps):
        xs = [m.contiguous().float() for m in maps]
        _K._require_gpu(xs[0])
        B = xs[0].shape[0]
        if not 1 <= len(xs) <= 4:
            raise MteError("1 to 4 maps, got %d" % len(xs))
        for x in xs:
            if x.dim() != 4 or x.shape[0] != B or x.shape[1] != 1:
                raise MteError("maps must be [B,1,h,w] with one B, got %s" % (tuple(x.shape),))
        ys = [torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) for x in xs]
        arr = (_UpsampleMap * len(xs))()
        for o, x, y in zip(arr, xs, ys):
            o.src, o.dst, o.h, o.w = x.data_ptr(), y.data_ptr(), x.shape[2], x.shape[3]
        _K.lib.mte_upsample_nearest_fwd(ctypes.addressof(arr), len(xs), B, int(H), int(W), _K._stream())
        ctx.sizes = [(x.shape[2], x.shape[3]) for x in xs]
        ctx.HW = (B, int(H), int(W))
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        B, H, W = ctx.HW
        gs = [g.contiguous().float() for g in gys]
        dxs = [torch.empty((B, 1, h, w), dtype=torch.float32, device=gs[0].device) for h, w in ctx.sizes]
        arr = (_UpsampleMap * len(gs))()
        for o, g, d, (h, w) in zip(arr, gs, dxs, ctx.sizes):
            o.src, o.dst, o.h, o.w = g.data_ptr(), d.data_ptr(), h, w
        _K.lib.mte_upsample_nearest_bwd(ctypes.addressof(arr), len(gs), B, H, W, _K._stream())
        return (None, None) + tuple(dxs)


def adam_step_flat(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, gscale=1.0):
    """In-place fused Adam over flat fp32 device buffers."""
    _K._require_gpu(p)
    _K.lib.mte_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                      float(eps), int(step), float(gscale), _K._stream())
    _K.bump_weights_epoch()


def adamw_step_flat(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, gscale=1.0):
    """In-place fused Adam with weight decay over flat fp32 device buffers: torch.optim.Adam(weight_decay) or, decoupled, torch.optim.AdamW."""
    _K._require_gpu(p)
    _K.lib.mte_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                          float(eps), float(weight_decay), int(bool(decoupled)), int(step), float(gscale), _K._stream())
    _K.bump_weights_epoch()


def sgd_step_flat(p, g, buf, step, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, gscale=1.0):
    """In-place fused torch.optim.SGD over flat fp32 device buffers; ``buf`` (zero before step 1) may be None when momentum is 0."""
    _K._require_gpu(p)
    _K.lib.mte_sgd_step(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), p.numel(), float(lr), float(momentum),
                        float(dampening), float(weight_decay), int(bool(nesterov)), int(step), float(gscale), _K._stream())
    _K.bump_weights_epoch()


def grad_accumulate_flat(dst, src, assign=False, stream=None):
    """dst <- dst + src in fp32 with one rounding per element, or with ``assign`` dst <- src (a bit copy), over two disjoint flat fp32
    device buffers of one size: ONE streaming launch (the micro-batch sum of gradient accumulation)."""
    _K._require_gpu(dst)
    _K._require_gpu(src)
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
        raise MteError("grad_accumulate_flat takes two contiguous float32 buffers of one size")
    _K.lib.mte_grad_accumulate(dst.data_ptr(), src.data_ptr(), dst.numel(), int(bool(assign)), _K._stream() if stream is None else stream)


def _flat_pair(name, a, b):
    _K._require_gpu(a)
    _K._require_gpu(b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel() or not (a.is_contiguous() and b.is_contiguous()):
        raise MteError(name + " takes two contiguous float32 buffers of one size")


def ema_update_flat(ema, p, scal, ctl=None, stream=None):
    """ema <- d * ema + omd * p in fp32 (two multiplications and one addition, each rounded once) over two disjoint flat fp32 device
    buffers of one size: ONE streaming launch.  ``scal`` = {d, omd}: two float32 values on the DEVICE, or a (d, omd) pair of Python
    numbers for the host-scalar entry point (``ctl`` must then be None).  ``ctl``: mte_grad_norm_clip's word; with ctl[1] set the
    launch leaves ``ema`` alone."""
    _flat_pair("ema_update_flat", ema, p)
    st = _K._stream() if stream is None else stream
    if torch.is_tensor(scal):
        _K._require_gpu(scal)
        if scal.dtype != torch.float32 or scal.numel() < 2 or (ctl is not None and (ctl.dtype != torch.float32 or ctl.numel() < 2)):
            raise MteError("ema_update_flat: scal holds two and ctl at least two float32 values")
        _K.lib.mte_ema_update_dev(ema.data_ptr(), p.data_ptr(), ema.numel(), scal.data_ptr(), None if ctl is None else ctl.data_ptr(), st)
    else:
        if ctl is not None:
            raise MteError("ema_update_flat: ctl goes with device scalars")
        _K.lib.mte_ema_update(ema.data_ptr(), p.data_ptr(), ema.numel(), float(scal[0]), float(scal[1]), st)


def flat_swap(a, b, stream=None):
    """a <-> b bit for bit over two disjoint flat fp32 device buffers of one size: ONE streaming launch, no temporary"""
    _flat_pair("flat_swap", a, b)
    _K.lib.mte_flat_swap(a.data_ptr(), b.data_ptr(), a.numel(), _K._stream() if stream is None else stream)


def grad_norm_work(n, device):
    """the zeroed work buffer of grad_norm_clip_flat for n gradient elements (records and ticket; allocate once, reuse every step)"""
    return torch.zeros((int(_K.lib.mte_grad_norm_work_bytes(int(n))) + 7) // 8, dtype=torch.float64, device=device)


def grad_norm_clip_flat(g, work, ctl, gscale=1.0, max_norm=float('inf'), skip_nonfinite=False, stream=None):
    """Global L2 norm of the flat fp32 gradient ``g`` in one read-only launch with a fixed summation order; leaves ``ctl`` (four floats on
    the device) = {min(max_norm / (|gscale| * norm + 1e-6), 1), skip flag, |gscale| * norm, skipped steps} for the ``_ctl_dev`` optimizer
    steps and the fp64 sum of squares in ``work[0]``.  No host synchronisation."""
    _K._require_gpu(g)
    _K.lib.mte_grad_norm_clip(g.data_ptr(), g.numel(), float(gscale), float(max_norm), int(bool(skip_nonfinite)), work.data_ptr(), ctl.data_ptr(),
                              _K._stream() if stream is None else stream)
