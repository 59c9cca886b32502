"""Generates tests/golden/completion_2x32x64.npz from the upstream reference (development container only): one training forward /
backward of SemiSupEdgeCompletionModel (packnet_code/packnet_sfm/models/SemiSupEdgeCompletionModel.py:96-180) and of
SemiSupCompletionModel (.../SemiSupCompletionModel.py:76-124) over a stub depth network that returns fixed `inv_depths`,
`inv_depths_rgbd` and `depth_loss` -- inputs, loss, metrics and the gradients with respect to all eight maps.  weight_rgbd = 0.5 and
depth_edges_loss_weight = 10 so that both quirks of the edge model show (the RGB+LiDAR edge term takes neither weight).

    python tests/golden/make_golden_completion.py
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import                                   # noqa: E402
from oracle import loss_oracle as lo                # noqa: E402

B, H, W = 2, 32, 64
WEIGHT_RGBD, MODEL_EDGE_WEIGHT, HEAD_WEIGHT, POS_TO_NEG = 0.5, 10.0, 10.0, 1.0


class StubNet(nn.Module):
    """the two passes of PackNetSAN01 in training mode, as fixed leaves (fresh lists per call: SupervisedLoss overwrites its argument's entries)"""

    def __init__(self, inv, inv_rgbd, depth_loss):
        super().__init__()
        self.inv, self.inv_rgbd, self.depth_loss = inv, inv_rgbd, depth_loss

    def forward(self, rgb, input_depth=None, **kwargs):
        assert input_depth is not None
        return {"inv_depths": list(self.inv), "inv_depths_rgbd": list(self.inv_rgbd), "depth_loss": self.depth_loss * 1.0}


def maps(seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.05 + 1.9 * torch.rand(B, 1, H >> s, W >> s, generator=g)).requires_grad_(True) for s in range(4)]


def main():
    assert ref_import.reference_available()
    ns = ref_import.import_reference()
    from packnet_code.packnet_sfm.models.SemiSupEdgeCompletionModel import SemiSupEdgeCompletionModel
    from packnet_code.packnet_sfm.models.SemiSupCompletionModel import SemiSupCompletionModel
    torch.set_num_threads(8)
    batch = lo.synthetic_batch(B, H, W, seed=21)
    g = torch.Generator().manual_seed(22)
    batch["edge"] = (torch.rand(B, 1, H, W, generator=g) < 0.08).float() * torch.rand(B, 1, H, W, generator=g)       # denser labels than the 3 % recipe
    batch["depth"] = (torch.rand(B, 1, H, W, generator=g) < 0.1).float() * (1.0 + 79.0 * torch.rand(B, 1, H, W, generator=g))
    batch["input_depth"] = batch["depth"] * (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
    inv, inv_rgbd = maps(23), maps(24)
    depth_loss = torch.tensor(0.3125, requires_grad=True)
    net = StubNet(inv, inv_rgbd, depth_loss)
    out = {"batch." + k: v for k, v in batch.items()}
    out.update({"inv%d" % s: t.detach() for s, t in enumerate(inv)})
    out.update({"inv_rgbd%d" % s: t.detach() for s, t in enumerate(inv_rgbd)})
    out.update(depth_loss=depth_loss.detach(), weight_rgbd=np.float64(WEIGHT_RGBD), depth_edges_loss_weight=np.float64(MODEL_EDGE_WEIGHT),
               head_weight=np.float64(HEAD_WEIGHT), pos_to_neg=np.float64(POS_TO_NEG))
    common = dict(supervised_loss_weight=1.0, weight_rgbd=WEIGHT_RGBD, supervised_method="sparse-silog", supervised_num_scales=1,
                  upsample_depth_maps=False, flip_lr_prob=0.0)

    def run(model, tag, metric_names):
        model.add_depth_net(net)
        model.train()
        for t in inv + inv_rgbd + [depth_loss]:
            t.grad = None
        o = model(dict(batch))
        o["loss"].sum().backward()
        out[tag + ".loss"] = o["loss"].detach()
        for m in metric_names:
            out[tag + "." + m] = o["metrics"][m]
        for s in range(4):
            out["%s.grad_inv%d" % (tag, s)] = torch.zeros_like(inv[s]) if inv[s].grad is None else inv[s].grad.clone()
            out["%s.grad_inv_rgbd%d" % (tag, s)] = torch.zeros_like(inv_rgbd[s]) if inv_rgbd[s].grad is None else inv_rgbd[s].grad.clone()
        out[tag + ".grad_depth_loss"] = depth_loss.grad.clone()
        print(tag, "loss", float(o["loss"].sum()), {m: float(o["metrics"][m]) for m in metric_names})

    edge_model = SemiSupEdgeCompletionModel(depth_edges_loss_weight=MODEL_EDGE_WEIGHT, edges_depth_edge_loss_all_scales=True, **common)
    edge_model.add_edge_loss(ns.GradLoss("cross_entropy", True, [], HEAD_WEIGHT, POS_TO_NEG))
    run(edge_model, "edge", ["edge_loss", "edge_lidar_loss", "supervised_loss"])
    run(SemiSupCompletionModel(**common), "plain", ["supervised_loss"])
    assert math.isfinite(float(out["edge.loss"].sum())) and math.isfinite(float(out["plain.loss"].sum()))
    np.savez_compressed(os.path.join(HERE, "completion_2x32x64.npz"),
                        **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
