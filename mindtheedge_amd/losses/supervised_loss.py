"""Supervised losses on fused gfx950 reductions -- drop-in for packnet_sfm/losses/supervised_loss.py (SupervisedLoss.forward :183-216,
calculate_loss :155-180, get_loss_func :73-87, BerHuLoss :13-54, SilogLoss :57-69).
"""
import torch
import torch.nn as nn

from .. import kernels as K
from ..kernels_loss import SUPERVISED_METHODS


class LossBase(nn.Module):
    def __init__(self):
        super().__init__()
        self._logs = {}
        self._metrics = {}

    @property
    def logs(self):
        return self._logs

    @property
    def metrics(self):
        return self._metrics

    def add_metric(self, key, val):
        self._metrics[key] = val.detach()


def parse_supervised_method(supervised_method):
    """-> (method id, sparse) as get_loss_func picks the loss: the first of the suffixes l1, mse, berhu, silog, abs_rel the string
    ends with; sparse when it starts with 'sparse'.  An unknown suffix raises ValueError, as upstream."""
    for mid, suffix in enumerate(SUPERVISED_METHODS):
        if supervised_method.endswith(suffix):
            return mid, supervised_method.startswith('sparse')
    raise ValueError('Unknown supervised loss {}'.format(supervised_method))


class SupervisedLoss(LossBase):
    """Supervised loss over the first `supervised_num_scales` (1..4) inverse-depth maps: sum_s f(inv_s + 1e-5, gt_inv_s) / n with
    gt_inv_s = depth2inv(depth) nearest-resized to scale s, f = mean l1 / mse / berhu / silog / abs_rel over the pixels with a valid
    ground truth (sparse) or over every pixel (dense).

    `progressive_scaling` is accepted and, as in the reference, has no effect: upstream's ProgressiveScaling tests `is_list` on an
    np.float32 array, which is never true, so the loss always uses `supervised_num_scales` scales.

    Dense 'berhu' is rejected at construction: upstream it fails in forward (torch.cat of the 4-D difference and the 1-D masked square).
    """

    def __init__(self, supervised_method='sparse-l1', supervised_num_scales=4, progressive_scaling=0.0, **kwargs):
        super().__init__()
        self.method_id, self.sparse = parse_supervised_method(supervised_method)
        if SUPERVISED_METHODS[self.method_id] == 'berhu' and not self.sparse:
            raise NotImplementedError("dense %r fails in the reference: BerHuLoss concatenates the 4-D |pred - gt| with the 1-D "
                                      "masked squares (torch.cat raises); use 'sparse-berhu'" % supervised_method)
        if not 1 <= supervised_num_scales <= 4:
            raise NotImplementedError("supervised_num_scales=%d: 1 to 4 scales are built (PackNetSAN01 returns four)" % supervised_num_scales)
        self.supervised_method = supervised_method
        self.n = supervised_num_scales
        self.progressive_scaling = progressive_scaling

    @property
    def logs(self):
        return {'supervised_num_scales': self.n}

    def forward(self, inv_depths, gt_depth, return_logs=False, progress=0.0, gt_is_inverse=False):
        """inv_depths: list of predicted inverse-depth maps; gt_depth: metric depth [B,1,H,W] with 0 = invalid, of any size (matched to
        each scale by nearest).  (The reference receives depth2inv(depth); pass gt_is_inverse=True for that calling convention --
        the valid set {gt_inv > 0} == {depth > 0} is identical.)  Unlike the reference, the caller's list is NOT mutated (upstream
        replaces inv_depths[s] by its masked 1-D gather, supervised_loss.py:175)."""
        if len(inv_depths) < self.n:
            raise ValueError("supervised_num_scales=%d but %d inverse-depth maps were given" % (self.n, len(inv_depths)))
        gt = gt_depth
        if gt_is_inverse:
            gt = torch.where(gt_depth > 0, 1.0 / gt_depth.clamp(min=1e-30), torch.zeros_like(gt_depth))
        if (self.supervised_method == 'sparse-silog' and self.n == 1
                and tuple(gt.shape[-2:]) == tuple(inv_depths[0].shape[-2:])):
            loss = K.SilogFn.apply(inv_depths[0], gt)
        else:
            loss = K.SupervisedLossFn.apply(self.method_id, self.sparse, gt, *inv_depths[:self.n])
        self.add_metric('supervised_loss', loss)
        return {'loss': loss.unsqueeze(0), 'metrics': self.metrics}
