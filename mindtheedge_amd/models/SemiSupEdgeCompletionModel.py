"""SemiSupEdgeCompletionModel: depth prediction AND depth completion with the depth-edge loss on both predictions -- drop-in for
packnet_sfm/models/SemiSupEdgeCompletionModel.py (forward :96-180, compute_edge_loss_with_all_scales :182-216).

In training the depth network runs twice, RGB only and RGB + sparse LiDAR (`input_depth`, PackNetSAN01(with_san=True)), and returns
`inv_depths`, `inv_depths_rgbd` and the feature-matching `depth_loss`.  With sup(.) the supervised loss, E(.) = mean_s GradLoss(inv2depth(.)_s,
edge_s, normal_s) and w = supervised_loss_weight (1 here):

    supervised      = w sup(rgb) / 2 + weight_rgbd w sup(rgbd) / 2
    edge_loss       = depth_edges_loss_weight E(rgb)
    edge_lidar_loss = E(rgbd)
    loss            = depth_loss + supervised + (edge_loss + edge_lidar_loss) / 2

The reference's quirks are kept, because checkpoints and curves are compared against it:
  * `edge_lidar_loss` is scaled neither by `depth_edges_loss_weight` nor by `weight_rgbd` (reference :152-154,165): with the shipped
    weight 10 the RGB+LiDAR edge term counts a tenth of the RGB one;
  * `weight_rgbd` reaches the supervised term only, and both supervised terms are halved (:146,159);
  * the metric 'supervised_loss' is the combined, halved term; the loss object's own metric is the LAST call's (RGB+LiDAR).
Where the reference breaks, this model says why: a training batch without `input_depth` dies upstream on an unbound `edge_lidar_loss` (:165);
here it raises a ValueError that names the missing key and the setting that provides it.

In the shipped-like configuration (four scales, GradLoss('cross_entropy') head, 'sparse-silog' on one scale, labels at the predictions' sizes,
no `rgb_edge` mask) all ten loss terms of a step -- 2 x 4 edge losses and 2 silog losses -- run as ONE forward and ONE backward launch that
read the labels once (kernels.DepthLossesPairFn, csrc/edge_fast.hpp; ``fuse_losses``).  Every other configuration takes the per-scale
path of SemiSupEdgeModel, once per branch, on the existing kernels.  Eval mode is SfmModel.forward, unchanged.
"""
from .SemiSupEdgeModel import SemiSupEdgeModel
from .SfmModel import SfmModel
from .model_utils import merge_outputs


class SemiSupEdgeCompletionModel(SemiSupEdgeModel):
    _train_with_lidar = True     # the loss consumes the RGB+LiDAR pass: depth_net_flipping forwards 'input_depth' while training

    def __init__(self, supervised_loss_weight=0.9, weight_rgbd=1.0, depth_edges_loss_weight=10.0, **kwargs):
        super().__init__(supervised_loss_weight=supervised_loss_weight, depth_edges_loss_weight=depth_edges_loss_weight, **kwargs)
        self._input_keys = ['rgb', 'input_depth', 'edge', 'rgb_edge', 'normal']          # reference :42-49
        if self.edges_depth_edge_loss_all_scales:
            self._input_keys += ['edge_1', 'edge_2', 'edge_3', 'normal_1', 'normal_2', 'normal_3']
        self.weight_rgbd = weight_rgbd

    def _fused_pair_losses(self, inv_depths, inv_depths_rgbd, batch):
        """-> (edge_rgb, edge_rgbd, sup_rgb [1], sup_rgbd [1]) from one forward / one backward launch, or None when the configuration
        needs the per-scale path (the conditions of SemiSupEdgeModel._fused_losses, and no `rgb_edge` mask)."""
        from .. import kernels as K
        from ..losses.grad_loss import GradLoss
        head = getattr(self, 'edge_loss_head', None)
        sup = self._supervised_loss
        if (not self.edges_depth_edge_loss_all_scales or not isinstance(head, GradLoss) or head.edge_loss_type != 'cross_entropy'
                or getattr(sup, 'supervised_method', None) != 'sparse-silog' or getattr(sup, 'n', 0) != 1
                or batch.get('rgb_edge') is not None or len(inv_depths) < 4 or len(inv_depths_rgbd) < 4
                or not inv_depths[0].is_cuda or tuple(batch['depth'].shape[-2:]) != tuple(inv_depths[0].shape[-2:])):
            return None
        sfx = ['', '_1', '_2', '_3']
        edges = [batch['edge' + s] for s in sfx]
        normals = [batch.get('normal' + s) for s in sfx]
        if any(tuple(e.shape[-2:]) != tuple(i.shape[-2:]) or tuple(e.shape[-2:]) != tuple(j.shape[-2:])
               for e, i, j in zip(edges, inv_depths, inv_depths_rgbd)):
            return None
        losses = K.DepthLossesPairFn.apply(head.weight, head.depth_edges_loss_pos_to_neg_weight, float(self.SIGMOID_THRESH), batch['depth'],
                                           edges, normals, *inv_depths[:4], *inv_depths_rgbd[:4])
        sup.add_metric('supervised_loss', losses[1, 4])           # as after the reference's second supervised call
        return losses[0, :4].sum() / 4, losses[1, :4].sum() / 4, losses[0, 4:5], losses[1, 4:5]

    def forward(self, batch, return_logs=False, progress=0.0, **kwargs):
        if not self.training:
            return SfmModel.forward(self, batch, return_logs=return_logs, **kwargs)
        if batch.get('input_depth') is None:
            raise ValueError("SemiSupEdgeCompletionModel trains on RGB + LiDAR: the batch has no 'input_depth' "
                             "(set datasets.train.input_depth_type, or train SemiSupEdgeModel)")
        out = SfmModel.forward(self, batch, return_logs=return_logs, **kwargs)
        if 'inv_depths_rgbd' not in out:
            raise ValueError("the depth network returned no 'inv_depths_rgbd' for a batch with 'input_depth': "
                             "SemiSupEdgeCompletionModel needs a network with the sparse branch (model.depth_net.with_san)")
        inv, inv_rgbd = out['inv_depths'], out['inv_depths_rgbd']
        fused = self._fused_pair_losses(inv, inv_rgbd, batch) if self.fuse_losses else None
        if fused is not None:
            edge_rgb, edge_rgbd, sup_rgb, sup_rgbd = fused
        else:
            mask = batch.get('rgb_edge')
            edge_rgb = self.compute_edge_loss_with_all_scales(inv, batch, mask, is_grad=True, is_sigmoid=True, sigmoid_thresh=self.SIGMOID_THRESH)
            sup_rgb = self.supervised_loss(inv, batch['depth'], return_logs=return_logs, progress=progress)['loss']
            edge_rgbd = self.compute_edge_loss_with_all_scales(inv_rgbd, batch, mask, is_grad=True, is_sigmoid=True, sigmoid_thresh=self.SIGMOID_THRESH)
            sup_rgbd = self.supervised_loss(inv_rgbd, batch['depth'], return_logs=return_logs, progress=progress)['loss']
        w = self.supervised_loss_weight
        supervised_loss = (w * sup_rgb) / 2 + (self.weight_rgbd * w * sup_rgbd) / 2
        edge_loss = self.depth_edges_loss_weight * edge_rgb
        edge_lidar_loss = edge_rgbd                                # not scaled: see the module docstring
        loss = supervised_loss + (edge_loss + edge_lidar_loss) / 2
        if 'depth_loss' in out:
            loss = out['depth_loss'] + loss
        metrics = {'metrics': {'edge_loss': edge_loss.detach(), 'edge_lidar_loss': edge_lidar_loss.detach(),
                               'supervised_loss': supervised_loss.detach()}}
        return {'loss': loss, **merge_outputs(out, metrics)}
