"""Registry + step API the reference trainer talks to (packnet_sfm/models/model_wrapper.py): ``setup_model``,
``setup_depth_net``, ``setup_depth_edge_loss`` (:561-672), ``configure_optimizers`` (:142-180), ``training_step``
(:197-213), ``depth`` (:318-321), and the depth half of validation: ``evaluate_depth`` (:328-352), ``validation_step``
(:215-225), ``validation_epoch_end`` (:255-277) with the metrics computed on the device.
With config.datasets.validation.path / split set the metric keys carry the reference's dataset prefix (``dataset_prefix``) and rank 0
prints one line per dataset and epoch; ``test_step`` / ``test_epoch_end`` give the depth metrics of a test split.  The loaders themselves
are datasets/kitti_edges.py::make_loader / make_val_loaders / make_test_loaders; wandb logging is not rebuilt."""
import random
from collections import OrderedDict

import torch
import torch.nn as nn

from ..utils.load import load_class, load_class_args_create, load_network, filter_args
from ..losses.grad_loss import GradLoss
from ..utils.depth import inv2depth, post_process_inv_depth, compute_depth_metrics
from .model_utils import stack_batch, flip_lr


def set_random_seed(seed):
    if seed >= 0:
        random.seed(seed)
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)


def setup_depth_net(config, prepared, **kwargs):
    depth_net = load_class_args_create(config.name, paths=['networks.depth'], args={**config, **kwargs})
    if not prepared and config.checkpoint_path != '':
        depth_net = load_network(depth_net, config.checkpoint_path, ['depth_net', 'disp_network'], ema=bool(config.get('checkpoint_ema')))
    return depth_net


def setup_depth_edge_loss(config):
    return GradLoss(config.edges.edge_loss_type, config.edges.use_external_edges_for_loss,
                    config.edges.edge_loss_class_list_to_mask_out, config.edges.depth_edges_loss_weight,
                    config.edges.depth_edge_loss_pos_to_neg_weight)


def setup_model(config, prepared, **kwargs):
    model = load_class(config.model.name, paths=['models'])(**{**config.model.loss, **kwargs})
    if 'depth_net' in model.network_requirements:
        # the depth-edge estimator and the completion models run the RGB+LiDAR pass: their network owns the sparse branch (with_san is not a
        # reference key; an explicit model.depth_net.with_san wins)
        wants_san = config.model.name.startswith('EdgeEstimation') or config.model.name.endswith('CompletionModel')
        extra = {'with_san': True} if wants_san and 'with_san' not in config.model.depth_net else {}
        model.add_depth_net(setup_depth_net(config.model.depth_net, prepared, **extra))
    if 'pose_net' in model.network_requirements:
        raise NotImplementedError("pose networks are outside this build's scope")
    if config.edges.train_depth_edges:
        model.add_edge_loss(setup_depth_edge_loss(config))
    if not prepared and config.model.checkpoint_path != '':
        model = load_network(model, config.model.checkpoint_path, 'model', ema=bool(config.model.get('checkpoint_ema')))
    if config.is_multi_gpu:
        raise NotImplementedError("nn.DataParallel is replaced by one process per GPU: launch with torch.distributed.run")
    return model


class ModelWrapper(nn.Module):
    def __init__(self, config, resume=None, logger=None, load_datasets=False):
        super().__init__()
        self.config, self.logger, self.resume = config, logger, resume
        set_random_seed(config.arch.seed)
        self.model = self.optimizer = self.scheduler = None
        self.current_epoch = 0
        self.metrics_name = 'depth'
        self.metrics_keys = ('abs_rel', 'sqr_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3')
        self.metrics_modes = ('', '_pp', '_gt', '_pp_gt')
        self.model = setup_model(config, prepared=resume is not None)
        self._train_dataloader = self._val_dataloaders = None
        self.trainer = None
        if resume and 'state_dict' in resume:
            # reference :88-94: prefix-stripped, shape-checked, NON-strict (a checkpoint written by the reference always
            # carries the sparse-branch tensors model.depth_net.mconvs.*, which this network only owns when with_san=True);
            # 'epoch' is the 0-based index of the epoch that had finished when the file was written -> resume at epoch + 1
            self.model = load_network(self.model, resume['state_dict'], 'model')
            if 'epoch' in resume:
                self.current_epoch = resume['epoch'] + 1

    @property
    def depth_net(self):
        return self.model.depth_net

    @property
    def pose_net(self):
        return getattr(self.model, 'pose_net', None)

    @property
    def progress(self):
        return self.current_epoch / self.config.arch.max_epochs

    def configure_optimizers(self, process_group=None):
        """config.model.optimizer.name ('Adam', 'AdamW', 'LAMB' or 'SGD') over depth_net.parameters() (param group 'Depth') + StepLR, as the
        reference: the keyword arguments are the keys of config.model.optimizer.depth that torch.optim.<name> accepts (filter_args), so
        lr, weight_decay, betas, eps, momentum, dampening and nesterov work when a YAML names them.  The optimizer is the fused flat
        one of that name and carries the bucketed RCCL gradient averaging when torch.distributed is initialised.
        config.model.optimizer.clip_grad_norm / skip_nonfinite_steps (this package's keys, beside `name`) switch on the device-side
        gradient-norm clipping and non-finite step guard of FusedFlatOptimizer; config.arch.accumulate_grad_batches > 1 its gradient
        accumulation over micro-batches; config.model.optimizer.ema_decay > 0 (with ema_warmup) its exponential moving average of the
        weights, which Trainer.validate swaps in when ema_validate is set.  A resumed file's 'state_dict_ema' / 'ema' entries restore
        the average and its update count; without them the average starts from the loaded weights at count 0.
        config.model.optimizer.tensor_scales (a list of rules {pattern, max_ndim, lr_scale, weight_decay_scale}, see
        resolve_tensor_scales) gives tensors their own multiples of the group's lr and weight_decay -- the fused SEG steps, still one
        param group; config.model.optimizer.log_tensor_stats = k > 0 makes the trainer print per-tensor gradient statistics.
        name 'LAMB' builds FusedLAMB from the keys of `depth` that torch.optim.AdamW accepts; config.model.optimizer.lamb_exclude
        (rules {pattern, max_ndim}, resolve_lamb_exclude; default [{max_ndim: 1}]: biases and GroupNorm affine tensors) names the
        tensors that keep plain AdamW arithmetic and lamb_max_trust (0 = no cap) caps the trust ratio; both are read only for LAMB.
        config.model.optimizer.warmup_steps = W > 0 is the per-step linear lr warm-up of FusedFlatOptimizer (Adam, AdamW, LAMB)."""
        import torch.distributed as dist
        from ..trainers.data_parallel import (FlatParameters, BucketedAllReduce, FusedAdam, FusedLAMB, FusedSGD, broadcast_parameters,
                                              reference_parameter_names, resolve_lamb_exclude, resolve_tensor_scales)
        opt_cfg = self.config.model.optimizer
        built = {'Adam': FusedAdam, 'AdamW': FusedAdam, 'LAMB': FusedLAMB, 'SGD': FusedSGD}
        if opt_cfg.name not in built:
            raise NotImplementedError("optimizer '{}' is not built: model.optimizer.name is one of {} (fused flat steps, "
                                      "without amsgrad and maximize)".format(opt_cfg.name, sorted(built)))
        # LAMB is no torch class: its `depth` keys are AdamW's
        kwargs = filter_args(getattr(torch.optim, 'AdamW' if opt_cfg.name == 'LAMB' else opt_cfg.name), opt_cfg.depth)
        for key in ('amsgrad', 'maximize'):
            if kwargs.pop(key, False):
                raise NotImplementedError("{}: true is not built: the fused {} steps are {} without amsgrad and maximize"
                                          .format(key, opt_cfg.name, sorted(built)))
        for key in ('params', 'foreach', 'capturable', 'differentiable', 'fused'):     # how torch would run its own step: no meaning here
            kwargs.pop(key, None)
        if opt_cfg.name == 'AdamW':
            kwargs['decoupled_weight_decay'] = True
        if 'betas' in kwargs:
            kwargs['betas'] = tuple(kwargs['betas'])
        flat = FlatParameters(self.depth_net.parameters())
        reducer = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
            broadcast_parameters(flat, group=process_group)
            reducer = BucketedAllReduce(flat, process_group)
        # arch.accumulate_grad_batches micro-batches per optimizer step; a trainer that was given its own value hands it over (Trainer.fit
        # attaches itself before it asks for the optimizer)
        accumulate = getattr(self.trainer, 'accumulate_grad_batches', None)
        if accumulate is None:
            accumulate = self.config.arch.accumulate_grad_batches or 1
        # model.optimizer.tensor_scales: rules -> one (lr_scale, weight_decay_scale) per trained tensor by its reference name and shape
        # (resolve_tensor_scales); no rule, or rules that leave every tensor at (1, 1), build the optimizer that was always built
        local = dict(self.depth_net.named_parameters())
        rules = opt_cfg.get('tensor_scales') or []
        name_of = {id(p): n for n, p in local.items()}
        names, shapes = [name_of[id(p)] for p in flat.natural_params], [tuple(p.shape) for p in flat.natural_params]
        if rules:
            kwargs['tensor_scales'] = resolve_tensor_scales(names, shapes, rules)
        if opt_cfg.name == 'LAMB':
            # model.optimizer.lamb_exclude / lamb_max_trust: read for this name only
            exclude = opt_cfg.get('lamb_exclude')
            kwargs['adapt'] = resolve_lamb_exclude(names, shapes, [{'max_ndim': 1}] if exclude is None else exclude)
            kwargs['max_trust'] = float(opt_cfg.get('lamb_max_trust') or 0.0)
            kwargs.pop('decoupled_weight_decay', None)       # always decoupled
        if int(opt_cfg.get('warmup_steps') or 0):
            kwargs['warmup_steps'] = int(opt_cfg.get('warmup_steps'))
        optimizer = built[opt_cfg.name](flat, reducer=reducer, name='Depth', clip_grad_norm=float(opt_cfg.clip_grad_norm or 0.0),
                                        skip_nonfinite=bool(opt_cfg.skip_nonfinite_steps), accumulate_grad_batches=accumulate,
                                        ema_decay=float(opt_cfg.get('ema_decay') or 0.0),
                                        ema_warmup=True if opt_cfg.get('ema_warmup') is None else bool(opt_cfg.get('ema_warmup')), **kwargs)
        self.ema_validate = True if opt_cfg.get('ema_validate') is None else bool(opt_cfg.get('ema_validate'))
        self.log_tensor_stats = int(opt_cfg.get('log_tensor_stats') or 0)
        optimizer.set_index_space(reference_parameter_names(self.depth_net), local)
        sched = getattr(torch.optim.lr_scheduler, self.config.model.scheduler.name)
        scheduler = sched(optimizer, **filter_args(sched, self.config.model.scheduler))
        if self.resume:
            if 'optimizer' in self.resume:
                optimizer.load_state_dict(self.resume['optimizer'])
            if 'scheduler' in self.resume:
                scheduler.load_state_dict(self.resume['scheduler'])
            if optimizer.ema_decay > 0.0 and 'state_dict_ema' in self.resume and 'ema' in self.resume:
                # the averaged depth-network tensors under their reference names, as set_index_space numbers them
                cut = 'depth_net.'
                named = {k[k.find(cut) + len(cut):]: v for k, v in self.resume['state_dict_ema'].items() if cut in k}
                optimizer.load_ema(named, self.resume['ema']['num_updates'])
        self.optimizer, self.scheduler = optimizer, scheduler
        return optimizer, scheduler

    # dataset readers are outside this build's scope: the entry point hands the loaders over and the
    # trainer asks for them the way the reference's does (trainers/common_trainer.py:66-67)
    def set_dataloaders(self, train=None, val=None):
        self._train_dataloader, self._val_dataloaders = train, val

    def train_dataloader(self):
        if self._train_dataloader is None:
            raise RuntimeError("no training data: call set_dataloaders(train=...) (train_edges.py --synthetic / --data)")
        return self._train_dataloader

    def val_dataloader(self):
        return self._val_dataloaders or []

    def training_step(self, batch, *args):
        batch = stack_batch(batch)
        output = self.model(batch, progress=self.progress)
        return {'loss': output['loss'], 'metrics': output['metrics']}

    @torch.no_grad()
    def evaluate_depth(self, batch, args=None):
        """Depth metrics of one validation batch, entirely on the device: prediction, prediction on the mirrored
        input, flip-TTA fusion, and the 7 metrics x 4 modes ('', '_pp', '_gt', '_pp_gt') -- reference :328-352.
        The depth metrics stay DEVICE tensors (float32[7]) and never synchronise with the host; the optional edge metrics
        (batch carries 'edge') read one convergence flag per 8 hysteresis sweeps of the Canny step."""
        inv_depths = self.model(batch)['inv_depths'][0]
        inv_depth = inv_depths[0][:, 0:1, :, :]
        depth = inv2depth(inv_depth)
        flipped = dict(batch)
        for key in ('rgb', 'input_depth', 'rgb_edge'):
            if key in flipped:
                flipped[key] = flip_lr(flipped[key])
        inv_depth_flipped = self.model(flipped)['inv_depths'][0][0][:, 0:1, :, :]
        inv_depth_pp = post_process_inv_depth(inv_depth, inv_depth_flipped, method='mean')
        depth_pp = inv2depth(inv_depth_pp)
        metrics = OrderedDict()
        if 'depth' in batch:
            for mode in self.metrics_modes:
                metrics[self.metrics_name + mode] = compute_depth_metrics(
                    self.config.model.params, gt=batch['depth'], pred=depth_pp if 'pp' in mode else depth,
                    use_gt_scale='gt' in mode)
        if 'edge' in batch:
            # reference :354-371 + compute_edge_metrics :373-440: Canny on the FIRST image's predicted depth (three settings)
            # (resized to the edge image's size) against its ground-truth edge image -> (precision, recall, F1) x 3.  The
            # resize and Canny steps restate OpenCV's published algorithms and are parity-unpinned (oracle/canny_oracle.py);
            # the chamfer part is pinned.  The depth-edge estimators' output already is an edge probability: it is thresholded
            # instead (:403-415).  datasets.validation.gt_crop[dataset_idx] restricts the scored window (:422-433).
            from ..utils.edge import compute_edge_metrics_from_depth, compute_edge_metrics_from_probability
            dataset_idx = int(args[1]) if args is not None and len(args) > 1 and args[1] is not None else 0
            gt_crops = (self.config.datasets.get('validation') or {}).get('gt_crop') or []
            gt_crop = gt_crops[dataset_idx] if len(gt_crops) > 0 else None
            estimator = self.config.model.name.startswith(('EdgeEstimation', 'EdgeClassification'))
            gt_edge = batch['edge'][0, 0].float() * 255

            def edge_metrics(inv):
                if estimator:
                    return compute_edge_metrics_from_probability(inv[0, 0], gt_edge, gt_crop=gt_crop)
                return compute_edge_metrics_from_depth(inv2depth(inv)[0, 0], gt_edge, gt_crop=gt_crop)
            if estimator:
                # the estimator MODEL halves the network's output (EdgeEstimationLIDARModel.forward); the reference thresholds the
                # network's own RGB output, one more forward (:353-356)
                metrics['edges'] = edge_metrics(self.depth(batch['rgb'], rgb_edge=batch.get('rgb_edge'))['inv_depths'][0][0][:, 0:1, :, :])
            else:
                metrics['edges'] = edge_metrics(inv_depth)
            if 'input_depth' in batch and getattr(self.model.depth_net, 'with_san', False):
                # reference :357-368: the same metrics of the RGB+LiDAR prediction (the completion models validate both)
                inv_input = self.depth(batch['rgb'], batch['input_depth'], rgb_edge=batch.get('rgb_edge'))['inv_depths'][0][0][:, 0:1, :, :]
                metrics['edges_input'] = edge_metrics(inv_input)
        return {'metrics': metrics, 'inv_depth': inv_depth_pp}

    def validation_step(self, batch, *args):
        output = self.evaluate_depth(stack_batch(batch), args)
        return {'idx': batch.get('idx'), **output['metrics']}

    def dataset_prefix(self, mode, dataset_idx=0):
        """The reference's metric prefix of dataset ``dataset_idx`` of config.datasets.<mode> (prepare_dataset_prefix, utils/logging.py:35-63):
        the path's stem, then -<split stem>, -<depth_type> and -<camera> where given; None when the section names no path / split."""
        import os
        section = (self.config.datasets.get(mode) or {}) if self.config.get('datasets') else {}
        paths, splits = section.get('path') or [], section.get('split') or []
        if len(paths) <= dataset_idx or len(splits) <= dataset_idx:
            return None
        prefix = os.path.splitext(paths[dataset_idx].split('/')[-1])[0]
        if splits[dataset_idx] != '' and '{' not in splits[dataset_idx]:
            prefix += '-{}'.format(os.path.splitext(os.path.basename(splits[dataset_idx]))[0])
        depth_types, cameras = section.get('depth_type') or [''], section.get('cameras') or [[]]
        if len(depth_types) > dataset_idx and depth_types[dataset_idx] != '':
            prefix += '-{}'.format(depth_types[dataset_idx])
        if len(cameras) > dataset_idx and len(cameras[dataset_idx]) == 1:
            prefix += '-{}'.format(cameras[dataset_idx][0])
        return prefix

    def test_step(self, batch, *args):
        """reference :227-236: the depth metrics of one test batch; with config.save.folder set, save_depth (utils/save.py) writes the
        sample's depth, RGB and colour files first"""
        batch = stack_batch(batch)
        output = self.evaluate_depth({k: v for k, v in batch.items() if k != 'edge'}, args)
        save = self.config.get('save')
        if save and save.get('folder'):
            from ..utils.save import save_depth
            save_depth(batch, output, args, self.config.datasets.test, save)
        return {'idx': batch.get('idx'), **output['metrics']}

    def test_epoch_end(self, output_data_batch, dataset_idx=0):
        """reference :294-311: the depth metrics only, under the test section's prefix"""
        return self._epoch_end(output_data_batch, self.dataset_prefix('test', dataset_idx), edges=False)

    def validation_epoch_end(self, output_data_batch, dataset_idx=0):
        """Mean of the per-batch metrics over the epoch (and over ranks) -> {'depth-abs_rel_pp_gt': float, ...}; with
        config.datasets.validation.path / split set the keys carry the reference's prefix instead (create_dict, utils/reduce.py:119-154):
        '<prefix>-abs_rel_pp_gt', '<prefix>-precision_0' ('<prefix>-precision_0_input' for the RGB+LiDAR prediction, the reference's '_input' mode).
        One host read per epoch."""
        prefix = self.dataset_prefix('validation', dataset_idx)
        out = self._epoch_end(output_data_batch, prefix, edges=True)
        import torch.distributed as dist
        if prefix is not None and out and not (dist.is_available() and dist.is_initialized() and dist.get_rank() != 0):
            self.print_metrics(out, prefix)
        return out

    def print_metrics(self, metrics, prefix):
        """one line per dataset and epoch (reference :444-470 prints a table): the seven depth metrics in the four modes"""
        parts = []
        for mode in self.metrics_modes:
            vals = ' '.join('{:.4f}'.format(metrics.get('{}-{}{}'.format(prefix, key, mode), float('nan'))) for key in self.metrics_keys)
            parts.append('{}: {}'.format(mode.lstrip('_') or 'raw', vals))
        print('validation epoch {} | {} | {} | {}'.format(self.current_epoch, prefix, ' '.join(self.metrics_keys), ' | '.join(parts)), flush=True)

    def _epoch_end(self, output_data_batch, prefix, edges):
        import torch.distributed as dist
        names = [self.metrics_name + m for m in self.metrics_modes]
        rows = [torch.stack([o[n] for n in names]) for o in output_data_batch if all(n in o for n in names)]
        dev = rows[0].device if rows else (torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else 'cpu')
        total = torch.stack(rows).sum(0) if rows else torch.zeros((len(names), len(self.metrics_keys)), device=dev)
        count = torch.tensor(float(len(rows)), device=dev)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(total)                           # every rank takes part, also one whose shard was empty
            dist.all_reduce(count)
        if float(count) == 0.0:
            return {}
        mean = (total / count).cpu()
        from .. import kernels as K
        K.check_device_errors()                              # the validation forwards of the epoch have finished (host read above)
        out = {'{}-{}{}'.format(self.metrics_name if prefix is None else prefix, key, mode): float(mean[i, j])
               for i, mode in enumerate(self.metrics_modes) for j, key in enumerate(self.metrics_keys)}
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        for name in (('edges', 'edges_input') if edges else ()):     # 'edges_input': the RGB+LiDAR prediction's (evaluate_depth, reference :365-368)
            edge_rows = [o[name] for o in output_data_batch if name in o]
            if edge_rows or multi:                           # (precision, recall, F1) x the three Canny settings, reference :431-438
                etotal = torch.stack(edge_rows).double().sum(0) if edge_rows else torch.zeros(9, dtype=torch.float64, device=dev)
                ecount = torch.tensor(float(len(edge_rows)), device=etotal.device, dtype=etotal.dtype)
                if multi:                                    # unconditional: a rank without edge rows must not leave the others waiting
                    dist.all_reduce(etotal)
                    dist.all_reduce(ecount)
            if (edge_rows or multi) and float(ecount) > 0:
                emean = (etotal / ecount).cpu()
                for k in range(emean.numel() // 3):
                    for j, key in enumerate(('precision', 'recall', 'f1')):
                        if prefix is None:
                            out['{}-{}_{}'.format(name, key, k)] = float(emean[3 * k + j])
                        else:
                            out['{}-{}_{}{}'.format(prefix, key, k, '_input' if name == 'edges_input' else '')] = float(emean[3 * k + j])
        return out

    def depth(self, *args, **kwargs):
        out = self.model.depth_net(*args, **kwargs)
        if not self.model.depth_net.training:
            # inference has no optimizer step to poll the device error word (a GroupNorm cluster wait that gave up): one read of host memory, no
            # synchronisation -- a give-up of THIS forward surfaces at the latest at the next call (infer_edges.infer_depth waits and polls itself)
            from .. import kernels as K
            from .._lib import MteError
            try:
                K.check_device_errors()
            except MteError:
                # the poll may see the first cluster kernel's report with later ones of the same forward still queued: they set the word again, and the
                # NEXT forward would be blamed for it.  This one is lost anyway: wait for it and take its remaining reports with it
                torch.cuda.synchronize()
                try:
                    K.check_device_errors()
                except MteError:
                    pass
                raise
        return out

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs)
