"""Golden vectors of the supervised losses (SupervisedLoss with {sparse-,}{l1,mse,berhu,silog,abs_rel} minus dense berhu, over 1, 2 and 4
scales; packnet_sfm/losses/supervised_loss.py:13-216) and of SemiSupEdgeModel's training loss with 'sparse-l1' on four scales, with and
without upsample_depth_maps (models/SfmModel.py:92-94, model_utils.py:154-176): runs the REAL reference on seeded inputs and stores
inputs + outputs.  Development container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_supervised.py

loss_supervised_inputs.npz        the shared inputs: 'base' (B = 2, ground truth and scale 0 at 32 x 64, then halvings) and 'ragged'
                                  (ground truth 45 x 75, predictions 45 x 75, 23 x 38, 12 x 19, 6 x 10); about half of the depth is 0
loss_supervised_<method>.npz      per (set, n): loss, d loss / d inv_s for s < n
loss_supervised_model.npz         SemiSupEdgeModel training loss and d loss / d inv_s through a stub depth network, upsampling off / on
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
from make_golden import rnd, save  # noqa: E402
from oracle import loss_oracle as lo  # noqa: E402
import supervised_oracle as so  # noqa: E402

B = 2
SETS = {"base": ((32, 64), [(32, 64), (16, 32), (8, 16), (4, 8)]),
        "ragged": ((45, 75), [(45, 75), (23, 38), (12, 19), (6, 10)])}
NS = (1, 2, 4)


def inputs():
    out = {}
    for name, ((hd, wd), sizes) in SETS.items():
        valid = (rnd("sup.%s.valid" % name, (B, 1, hd, wd), 0, 1) < 0.5).float()
        out[name + ".depth"] = valid * rnd("sup.%s.depth" % name, (B, 1, hd, wd), 1.0, 50.0)
        for s, (h, w) in enumerate(sizes):
            out["%s.inv%d" % (name, s)] = rnd("sup.%s.inv%d" % (name, s), (B, 1, h, w), 0.02, 1.0)
    return out


class StubNet(nn.Module):
    """a depth network that returns fixed inverse-depth maps (the leaves the gradients are taken against)"""

    def __init__(self, invs):
        super().__init__()
        self.invs = invs

    def forward(self, rgb=None, **kwargs):
        return {"inv_depths": list(self.invs)}


def main():
    ns = ref_import.import_reference()
    inp = inputs()
    save("loss_supervised_inputs", **inp)
    for method in so.ACCEPTED:
        out = {}
        for name, (_, sizes) in SETS.items():
            for n in NS:
                invs = [inp["%s.inv%d" % (name, s)].clone().requires_grad_(True) for s in range(4)]
                sup = ns.SupervisedLoss(supervised_method=method, supervised_num_scales=n)
                loss = sup(list(invs), ns.depth2inv(inp[name + ".depth"]))["loss"]
                grads = torch.autograd.grad(loss.sum(), invs[:n], allow_unused=True)
                out["%s.n%d.loss" % (name, n)] = loss.detach()
                for s, g in enumerate(grads):
                    out["%s.n%d.dinv%d" % (name, n, s)] = torch.zeros_like(invs[s]) if g is None else g
        save("loss_supervised_" + method.replace("-", "_"), **out)
    # model level: SemiSupEdgeModel.forward (SemiSupEdgeModel.py:98-162) with 'sparse-l1' on four scales and the all-scales edge loss
    H, W = 64, 128
    batch = lo.synthetic_batch(B, H, W, seed=11)
    valid = (rnd("sup.model.valid", (B, 1, H, W), 0, 1) < 0.5).float()
    batch["depth"] = valid * rnd("sup.model.depth", (B, 1, H, W), 1.0, 50.0)
    invs0 = [rnd("sup.model.inv%d" % s, (B, 1, H >> s, W >> s), 0.02, 1.0) for s in range(4)]
    out = {"batch." + k: v for k, v in batch.items()}
    out.update({"inv%d" % s: t for s, t in enumerate(invs0)})
    for tag, up in (("plain", False), ("up", True)):
        invs = [t.clone().requires_grad_(True) for t in invs0]
        model = ns.SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-l1",
                                    supervised_num_scales=4, edges_depth_edge_loss_all_scales=True, upsample_depth_maps=up,
                                    flip_lr_prob=0.0)
        model.add_depth_net(StubNet(invs))
        model.add_edge_loss(ns.GradLoss("cross_entropy", True, [], 10.0, 1.0))
        model.train()
        o = model(dict(batch))
        grads = torch.autograd.grad(o["loss"].sum(), invs)
        out[tag + ".loss"] = o["loss"].detach()
        out[tag + ".edge_loss"] = o["metrics"]["edge_loss"]
        out[tag + ".supervised_loss"] = o["metrics"]["supervised_loss"]
        for s, g in enumerate(grads):
            out["%s.dinv%d" % (tag, s)] = g
    save("loss_supervised_model", **out)


if __name__ == "__main__":
    main()
