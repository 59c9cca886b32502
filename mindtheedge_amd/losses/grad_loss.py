"""Depth-edge loss head on the fused gfx950 stencil -- drop-in for packnet_sfm/losses/grad_loss.py:
``GradLoss(edge_loss_type, use_external_edges_for_loss, edge_loss_class_list_to_mask_out,
depth_edges_loss_weight, depth_edges_loss_pos_to_neg_weight)`` and
``head(output, gt_edge, gt_mask=None, is_grad=True, is_sigmoid=True, sigmoid_thresh=4, gt_normals=None)
-> (loss, output_grad.detach())`` (reference :98-159).
"""
import torch
import torch.nn as nn

from .. import kernels as K


class GradLayer(nn.Module):
    """Edge-strength map of the reference GradLayer (grad_loss.py:14-95): sqrt(v^2+h^2+1e-6), or |directional
    Sobel| chosen per pixel by the normal angle.  Returns (x_mag, None, None): the reference's extra x_v/x_h
    outputs are unused on the training path and are not produced."""

    def forward(self, x, normal=None):
        zeros = torch.zeros_like(x)
        _, g = K.EdgeLossFn.apply(x, zeros, normal, None, 1.0, 1.0, False, True, True, 4.0, True)
        return g, None, None


# base losses of grad_loss.py:143-150 in the order the reference tests them (plain substring tests: the LAST one present wins)
EDGE_LOSS_KINDS = (('cross_entropy', 0), ('attention_loss', 1), ('spatially_adaptive', 2))


def parse_edge_loss_type(edge_loss_type):
    """-> (kind, dice): kind 0 class-balanced BCE, 1 attention_loss2, 2 spatially adaptive attention_loss2; dice adds the dice term
    ('dice' in the string, grad_loss.py:153).  A string without a base loss fails upstream (UnboundLocalError in forward); here it
    raises NotImplementedError at construction."""
    kind = None
    for name, k in EDGE_LOSS_KINDS:
        if name in edge_loss_type:
            kind = k
    if kind is None:
        raise NotImplementedError("edge_loss_type %r names no base loss (one of %s)"
                                  % (edge_loss_type, ", ".join(n for n, _ in EDGE_LOSS_KINDS)))
    return kind, 'dice' in edge_loss_type


class GradLoss(nn.Module):
    def __init__(self, edge_loss_type, use_external_edges_for_loss=True, edge_loss_class_list_to_mask_out=[],
                 depth_edges_loss_weight=1.0, depth_edges_loss_pos_to_neg_weight=1.0):
        super().__init__()
        self.loss_kind, self.dice = parse_edge_loss_type(edge_loss_type)
        if len(edge_loss_class_list_to_mask_out) > 0:
            raise NotImplementedError("segmentation-class masking is dead code upstream (list re-set to [] at grad_loss.py:181)")
        self.grad_layer = GradLayer()
        self.weight = depth_edges_loss_weight
        self.depth_edges_loss_pos_to_neg_weight = depth_edges_loss_pos_to_neg_weight
        self.edge_loss_type = edge_loss_type
        self.use_external_edges_for_loss = use_external_edges_for_loss
        self.edge_loss_class_list_to_mask_out = edge_loss_class_list_to_mask_out

    def forward(self, output, gt_edge, gt_mask=None, is_grad=True, is_sigmoid=True, sigmoid_thresh=4, gt_normals=None,
                from_inv_depth=False, return_grad_map=True):
        """`from_inv_depth=True` (extension) fuses inv2depth into the stencil: `output` is then the network's
        inverse depth.  `return_grad_map=False` skips writing the detached edge-strength map."""
        K._require_gpu(output)
        if tuple(output.shape[-2:]) != tuple(gt_edge.shape[-2:]):
            # reference :127: F.interpolate(output, size=label size, mode='bilinear').  The reference resizes the DEPTH (its
            # caller applied inv2depth already); with the fused inv2depth the reciprocal is therefore taken first here too.
            if from_inv_depth:
                output = 1.0 / output.clamp(min=1e-6)
                from_inv_depth = False
            output = K.BilinearResizeFn.apply(output, gt_edge.shape[-2], gt_edge.shape[-1])
        if self.loss_kind == 0 and not self.dice:
            loss, g = K.EdgeLossFn.apply(output, gt_edge, gt_normals if is_grad else None, gt_mask, self.weight,
                                         self.depth_edges_loss_pos_to_neg_weight, from_inv_depth, is_grad, is_sigmoid,
                                         float(sigmoid_thresh), return_grad_map)
            return loss, g
        loss, g = K.EdgeLossKindFn.apply(output, gt_edge, gt_normals if is_grad else None, gt_mask, self.loss_kind, self.dice,
                                         self.weight, self.depth_edges_loss_pos_to_neg_weight, from_inv_depth, is_grad, is_sigmoid,
                                         float(sigmoid_thresh), return_grad_map)
        return loss, g
