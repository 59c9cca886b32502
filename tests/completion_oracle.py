"""CPU restatement of the training losses of the two completion models (packnet_sfm/models/SemiSupEdgeCompletionModel.py:128-165,
SemiSupCompletionModel.py:108-124), composed in the caller's dtype (float64 in the tests) from the pinned pieces: oracle.loss_oracle
(edge_loss_all_scales, supervised_silog_loss) and tests/supervised_oracle.py.  Pinned by tests/golden/completion_2x32x64.npz
(tests/golden/make_golden_completion.py runs the reference's two classes); the yardstick of tests/test_completion_cpu.py and
tests/test_gpu_completion.py."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import loss_oracle as lo            # noqa: E402
import supervised_oracle as so                  # noqa: E402


def _sup(method, n, inv_depths, depth):
    if method == "sparse-silog" and n == 1 and tuple(depth.shape[-2:]) == tuple(inv_depths[0].shape[-2:]):
        return lo.supervised_silog_loss(inv_depths[0], depth)
    return so.supervised_loss(method, n, inv_depths, depth)


def edge_completion_loss(inv, inv_rgbd, depth_loss, batch, weight_rgbd=1.0, depth_edges_loss_weight=10.0, head_weight=10.0, pos_to_neg=1.0,
                         supervised_loss_weight=1.0, method="sparse-silog", n=1):
    """SemiSupEdgeCompletionModel.forward, training branch, supervised_loss_weight == 1.  The RGB+LiDAR edge term takes neither
    depth_edges_loss_weight nor weight_rgbd (reference :152-154,165), and both supervised terms are halved (:146,159).
    -> dict(loss [1], edge_loss, edge_lidar_loss, supervised_loss)"""
    mask = batch.get("rgb_edge")
    w = supervised_loss_weight
    edge = depth_edges_loss_weight * lo.edge_loss_all_scales(inv, batch, mask, head_weight, pos_to_neg)
    edge_lidar = lo.edge_loss_all_scales(inv_rgbd, batch, mask, head_weight, pos_to_neg)
    sup = (w * _sup(method, n, inv, batch["depth"]).unsqueeze(0)) / 2 + (weight_rgbd * w * _sup(method, n, inv_rgbd, batch["depth"]).unsqueeze(0)) / 2
    loss = torch.zeros(1, dtype=inv[0].dtype) + depth_loss + sup + (edge + edge_lidar) / 2
    return {"loss": loss, "edge_loss": edge.detach(), "edge_lidar_loss": edge_lidar.detach(), "supervised_loss": sup.detach()}


def completion_loss(inv, inv_rgbd, depth_loss, batch, weight_rgbd=1.0, supervised_loss_weight=1.0, method="sparse-silog", n=1):
    """SemiSupCompletionModel.forward, training branch.  The returned metric is the reference's: the loss object hands the same
    metrics dict to both supervised calls, so its 'supervised_loss' holds the RGB+LiDAR value when the model returns it.
    -> dict(loss [1], supervised_loss)"""
    w = supervised_loss_weight
    s_rgb, s_rgbd = _sup(method, n, inv, batch["depth"]), _sup(method, n, inv_rgbd, batch["depth"])
    loss = torch.zeros(1, dtype=inv[0].dtype) + w * s_rgb.unsqueeze(0) + weight_rgbd * w * s_rgbd.unsqueeze(0) + depth_loss
    return {"loss": loss, "supervised_loss": s_rgbd.detach()}
