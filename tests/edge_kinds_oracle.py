"""CPU restatement of the edge-loss choices beyond 'cross_entropy' (packnet_sfm/losses/grad_loss.py:139-156 and
losses/attention_loss.py:21-49), in plain PyTorch: the yardstick of tests/test_edge_loss_kinds_cpu.py and
tests/test_gpu_edge_loss_kinds.py.  GradLayer and the class-balanced BCE come from oracle.loss_oracle."""
import torch
import torch.nn.functional as F

from oracle.loss_oracle import balanced_bce, grad_layer, inv2depth

ACCEPTED = ("cross_entropy_dice", "attention_loss", "attention_loss_dice", "spatially_adaptive", "spatially_adaptive_dice")
REJECTED = ("dice", "dice_grad_edge", "grad_L1")


def parse(edge_loss_type):
    """-> (kind, dice) as the reference's substring tests pick them; kind None = no base loss."""
    kind = None
    for name, k in (("cross_entropy", 0), ("attention_loss", 1), ("spatially_adaptive", 2)):
        if name in edge_loss_type:
            kind = k
    return kind, "dice" in edge_loss_type


def box_alpha(target):
    """1 - box15(t) / 225 (zero padding); 0.5 where that is >= float32(1 - 1e-14) = 1.0f."""
    s = F.conv2d(target, torch.ones(1, 1, 15, 15, dtype=target.dtype), padding=7) / 225
    a = 1 - s
    a[a >= (1.0 - 1e-14)] = 0.5
    return a


def attention_loss2(p, t, mask=None, spatially_adaptive=False):
    eps = 1e-14
    if not spatially_adaptive:
        num_pos = torch.sum(t == 1).float()
        num_neg = torch.sum(t == 0).float()
        alpha = num_neg / (num_pos + num_neg)
    else:
        alpha = box_alpha(t)
    pc = torch.clamp(p, min=eps, max=1.0 - eps)
    w = t * alpha * (4 ** ((1.0 - pc) ** 0.5)) + (1.0 - t) * (1.0 - alpha) * (4 ** (pc ** 0.5))
    w = w.detach()
    if mask is not None:
        w = w * mask
    return torch.mean(F.binary_cross_entropy(p, t, w, reduction="none"))


def dice_term(p, t):
    return 1000 * ((torch.sum(p ** 2) + torch.sum(t ** 2) + 0.0001) / (2 * torch.sum(p * t) + 0.0001)) / t.numel()


def grad_loss(edge_loss_type, output, gt_edge, gt_mask=None, is_grad=True, is_sigmoid=True, sigmoid_thresh=4.0, gt_normals=None,
              weight=1.0, pos_to_neg=1.0):
    """GradLoss.forward for any accepted type string -> (loss, g.detach())."""
    kind, dice = parse(edge_loss_type)
    if kind is None:
        raise NotImplementedError(edge_loss_type)
    if gt_mask is not None and tuple(gt_mask.shape) != tuple(gt_edge.shape):
        raise ValueError("mask / label shapes differ")
    if tuple(output.shape[-2:]) != tuple(gt_edge.shape[-2:]):
        output = F.interpolate(output, size=tuple(gt_edge.shape[-2:]), mode="bilinear")
    g = grad_layer(output, gt_normals) if is_grad else output
    p = torch.sigmoid(g - sigmoid_thresh) if is_sigmoid else g
    if kind == 0:
        loss = balanced_bce(gt_edge, gt_mask, p, pos_to_neg)
    else:
        loss = attention_loss2(p, gt_edge, gt_mask, kind == 2)
    if dice:
        loss = loss + dice_term(p, gt_edge)
    return weight * loss, g.detach()


def edge_loss_all_scales(edge_loss_type, inv_depths, batch, mask=None, weight=1.0, pos_to_neg=1.0):
    """SemiSupEdgeModel.compute_edge_loss_with_all_scales (SemiSupEdgeModel.py:164-198) with is_grad = is_sigmoid = True, thresh 4."""
    total = 0.0
    for s in range(4):
        sfx = "" if s == 0 else "_%d" % s
        loss, _ = grad_loss(edge_loss_type, inv2depth(inv_depths[s]), batch["edge" + sfx], mask, True, True, 4.0,
                            batch.get("normal" + sfx), weight, pos_to_neg)
        total = total + loss
    return total / 4.0
