"""Golden vectors of the edge-loss choices beyond 'cross_entropy' (GradLoss with 'cross_entropy_dice', 'attention_loss',
'attention_loss_dice', 'spatially_adaptive', 'spatially_adaptive_dice'; packnet_sfm/losses/grad_loss.py:139-156,
losses/attention_loss.py:21-49): runs the REAL reference on seeded inputs and stores inputs + outputs.  Development container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edge_kinds.py

loss_edge_kinds_inputs.npz      the shared inputs (B = 2, 40 x 72 maps)
loss_edge_kinds_<type>.npz      per case: loss, g map, d loss / d input
loss_edge_kinds_model.npz       SemiSupEdgeModel.compute_edge_loss_with_all_scales with 'spatially_adaptive_dice' on four scales
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
from make_golden import rnd, save  # noqa: E402

TYPES = ("cross_entropy_dice", "attention_loss", "attention_loss_dice", "spatially_adaptive", "spatially_adaptive_dice")
WEIGHT = 10.0
B, H, W = 2, 40, 72


def smooth_depth(name, shape, lo=2.0, hi=9.0):
    """a depth map whose Sobel responses span the sigmoid's working range (g - 4 in about [-4, 8])"""
    b, _, h, w = shape
    yy = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    xx = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    ph = rnd(name + ".ph", (b, 1, 1, 1), 0.0, 6.0)
    base = 0.5 * (lo + hi) + 0.5 * (hi - lo) * torch.sin(xx * 0.21 + ph) * torch.cos(yy * 0.17 - ph)
    step = (xx > w * 0.6).float() * 1.5                                  # a depth edge
    return base + step + rnd(name + ".noise", shape, -0.3, 0.3)


def inputs():
    shape = (B, 1, H, W)
    depth = smooth_depth("kinds.depth", shape)
    on = (rnd("kinds.on", shape, 0, 1) < 0.15).float()
    hard = (rnd("kinds.hard", shape, 0, 1) < 0.5).float()
    edge = on * (hard + (1 - hard) * rnd("kinds.soft", shape, 0.05, 0.95))          # soft labels mixed with exact 0 and 1
    sparse = torch.zeros(shape)                                                        # empty 15x15 windows + windows at the border
    sparse[0, 0, 0, 0] = sparse[0, 0, H - 1, W - 1] = sparse[0, 0, 20, 36] = 1.0
    sparse[1, 0, 3, W - 2] = sparse[1, 0, H - 5, 4] = 1.0
    sparse[1, 0, 18, 30:34] = torch.tensor([1.0, 0.5, 1.0, 0.25])
    normal = rnd("kinds.n", shape, -math.pi, math.pi)
    mask_bin = (rnd("kinds.mb", shape, 0, 1) < 0.7).float()
    mask_soft = rnd("kinds.ms", shape, 0, 1)
    prob = rnd("kinds.p", shape, 0.0, 1.0)
    prob.view(-1)[::17] = 0.0
    prob.view(-1)[5::23] = 1.0
    depth_half = smooth_depth("kinds.dhalf", (B, 1, H // 2, W // 2))
    depth_sat = depth + 60.0 * (rnd("kinds.sat", shape, 0, 1) < 0.3).float()    # huge responses: p == 1.0f
    return dict(depth=depth, edge=edge, sparse=sparse, normal=normal, mask_bin=mask_bin, mask_soft=mask_soft, prob=prob,
                depth_half=depth_half, depth_sat=depth_sat)


# case -> (input, label, mask, normal, is_grad, is_sigmoid)
CASES = {
    "nomask": ("depth", "edge", None, "normal", True, True),
    "binmask": ("depth", "edge", "mask_bin", "normal", True, True),
    "softmask": ("depth", "edge", "mask_soft", "normal", True, True),
    "nonormal": ("depth", "edge", None, None, True, True),
    "dee": ("prob", "edge", None, None, False, False),
    "sparse": ("depth", "sparse", None, "normal", True, True),
    "half": ("depth_half", "edge", None, "normal", True, True),
    "sat": ("depth_sat", "edge", None, "normal", True, True),
}


def model_inputs():
    sizes = [(64, 128), (32, 64), (16, 32), (8, 16)]
    out = {}
    for s, (h, w) in enumerate(sizes):
        sfx = "" if s == 0 else "_%d" % s
        out["inv%d" % s] = 1.0 / smooth_depth("kinds.model.d%d" % s, (B, 1, h, w))
        on = (rnd("kinds.model.on%d" % s, (B, 1, h, w), 0, 1) < 0.1).float()
        out["edge" + sfx] = on * (rnd("kinds.model.e%d" % s, (B, 1, h, w), 0, 1) < 0.6).float()
        out["normal" + sfx] = rnd("kinds.model.n%d" % s, (B, 1, h, w), -math.pi, math.pi)
    return out


def main():
    ns = ref_import.import_reference()
    inp = inputs()
    save("loss_edge_kinds_inputs", **inp)
    for t in TYPES:
        head = ns.GradLoss(t, True, [], WEIGHT, 1.0)
        out = {}
        for cname, (x, e, m, n, is_grad, is_sigmoid) in CASES.items():
            xin = inp[x].clone().requires_grad_(True)
            loss, g = head(xin, inp[e], None if m is None else inp[m], is_grad, is_sigmoid, 4, None if n is None else inp[n])
            (dx,) = torch.autograd.grad(loss, xin)
            out["loss_" + cname], out["g_" + cname], out["dx_" + cname] = loss, g, dx
        save("loss_edge_kinds_" + t, **out)
    # model level: compute_edge_loss_with_all_scales (SemiSupEdgeModel.py:164-198) on four scales, mask None, through the
    # reference's own method with a minimal `self`
    mi = model_inputs()
    head = ns.GradLoss("spatially_adaptive_dice", True, [], WEIGHT, 1.0)

    def edge_loss(pred, gt_edges, gt_mask=None, is_grad=True, is_sigmoid=True, sigmoid_thresh=4, gt_normals=None):
        return head(pred, gt_edges, gt_mask, is_grad, is_sigmoid, sigmoid_thresh, gt_normals)

    me = types.SimpleNamespace(edge_loss=edge_loss, edges_depth_edge_loss_all_scales=True)
    invs = [mi["inv%d" % s].clone().requires_grad_(True) for s in range(4)]
    batch = {k: v for k, v in mi.items() if not k.startswith("inv")}
    loss = ns.SemiSupEdgeModel.compute_edge_loss_with_all_scales(me, invs, batch, None, True, True, 4)
    dinv = torch.autograd.grad(loss, invs)
    save("loss_edge_kinds_model", **mi, loss=loss, **{"dinv%d" % s: d for s, d in enumerate(dinv)})


if __name__ == "__main__":
    main()
