"""SemiSupCompletionModel: the original PackNet-SAN recipe, one network that predicts depth from RGB and completes it from RGB + sparse
LiDAR, with the supervised loss on both predictions -- drop-in for packnet_sfm/models/SemiSupCompletionModel.py (forward :76-124).

    loss = w sup(rgb) + weight_rgbd w sup(rgbd) + depth_loss        (w = supervised_loss_weight, 1 here; depth_loss: feature matching)

Kept from the reference: the returned metrics are the dict of the FIRST supervised call (:109-111,123).  The loss object hands out the same
dict on every call, so after the second call its 'supervised_loss' entry holds the RGB+LiDAR value, as upstream.  A training batch without
`input_depth` gives the RGB term alone upstream (:113 is simply skipped); a completion model that silently trains RGB-only is a
configuration error, so this one raises a ValueError that names `input_depth` and `datasets.train.input_depth_type`.

No new kernel: SupervisedLoss twice (one launch each way).  Eval mode is SfmModel.forward, unchanged.
"""
from .SfmModel import SfmModel
from .model_utils import merge_outputs
from ..losses.supervised_loss import SupervisedLoss


class SemiSupCompletionModel(SfmModel):
    _train_with_lidar = True     # the loss consumes the RGB+LiDAR pass: depth_net_flipping forwards 'input_depth' while training

    def __init__(self, supervised_loss_weight=0.9, weight_rgbd=1.0, **kwargs):
        super().__init__(**kwargs)
        assert 0. < supervised_loss_weight <= 1., "Model requires (0, 1] supervision"
        if supervised_loss_weight != 1.0:
            raise NotImplementedError("self-supervised photometric term (supervised_loss_weight < 1) is out of scope; "
                                      "the shipped YAML uses 1.0")
        self.supervised_loss_weight = supervised_loss_weight
        self._supervised_loss = SupervisedLoss(**kwargs)
        self._network_requirements.remove('pose_net')
        self._train_requirements.append('gt_depth')
        self._input_keys = ['rgb', 'input_depth', 'intrinsics']    # reference :39
        self.weight_rgbd = weight_rgbd

    @property
    def logs(self):
        return {**super().logs, **self._supervised_loss.logs}

    def supervised_loss(self, inv_depths, gt_depth, return_logs=False, progress=0.0):
        return self._supervised_loss(inv_depths, gt_depth, return_logs=return_logs, progress=progress)

    def forward(self, batch, return_logs=False, progress=0.0, **kwargs):
        if not self.training:
            return SfmModel.forward(self, batch, return_logs=return_logs, **kwargs)
        if batch.get('input_depth') is None:
            raise ValueError("SemiSupCompletionModel trains on RGB + LiDAR: the batch has no 'input_depth' "
                             "(set datasets.train.input_depth_type)")
        out = SfmModel.forward(self, batch, return_logs=return_logs, **kwargs)
        if 'inv_depths_rgbd' not in out:
            raise ValueError("the depth network returned no 'inv_depths_rgbd' for a batch with 'input_depth': "
                             "SemiSupCompletionModel needs a network with the sparse branch (model.depth_net.with_san)")
        sup_output = self.supervised_loss(out['inv_depths'], batch['depth'], return_logs=return_logs, progress=progress)
        loss = self.supervised_loss_weight * sup_output['loss']
        sup_output2 = self.supervised_loss(out['inv_depths_rgbd'], batch['depth'], return_logs=return_logs, progress=progress)
        loss = loss + self.weight_rgbd * self.supervised_loss_weight * sup_output2['loss']
        if 'depth_loss' in out:
            loss = loss + out['depth_loss']
        return {'loss': loss, **merge_outputs(out, sup_output)}
