"""Minimal attribute-dict configuration with the reference's defaults for the keys the hot path reads
(packnet_code/configs/default_config.py:8-292; yacs is not required).  ``load_config(yaml_path)`` overlays a reference
YAML (e.g. configs/train_packnet_san_kitti_with_edges.yaml) on the defaults."""
import copy


class Cfg(dict):
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v

    @staticmethod
    def wrap(d):
        if isinstance(d, dict):
            return Cfg({k: Cfg.wrap(v) for k, v in d.items()})
        return d


_DEFAULTS = {
    'is_multi_gpu': False,
    # accumulate_grad_batches (this package's key): micro-batches per optimizer step.  The reference reaches its global batch through Horovod
    # (8 per GPU x N GPUs); k > 1 runs that effective batch on fewer cards (FusedFlatOptimizer.accumulate).  1 = every batch steps.
    'arch': {'seed': 42, 'min_epochs': 1, 'max_epochs': 50, 'validate_first': False, 'accumulate_grad_batches': 1},
    'model': {
        # checkpoint_ema (here and under depth_net): load checkpoint_path's averaged weights ('state_dict_ema') instead of the raw ones
        'name': 'SemiSupEdgeModel', 'checkpoint_path': '', 'checkpoint_ema': False,
        # name: 'Adam', 'AdamW' or 'SGD' (default_config.py: model.optimizer.name).  depth: the keys torch.optim.<name> accepts reach the fused
        # optimizer -- lr, weight_decay, betas, eps (Adam, AdamW); lr, weight_decay, momentum, dampening, nesterov (SGD); amsgrad / maximize: true
        # are not built (ModelWrapper.configure_optimizers).  clip_grad_norm (0 = off): torch.nn.utils.clip_grad_norm_'s max_norm over all trained
        # tensors; skip_nonfinite_steps: a step whose gradient holds an inf or a NaN changes nothing.  Both are this package's own keys and sit
        # beside `name`, not under `depth`, so filter_args never hands them to torch.optim; both off = the step as it always was.
        # ema_decay (0 = off): FusedFlatOptimizer keeps an exponential moving average of the trained tensors with that decay (ema_warmup: the
        # decay of the t-th update is min(ema_decay, (1 + t) / (10 + t))); ema_validate: validation, and with it save_top_k, runs on the average.
        # tensor_scales ([] = off): rules {pattern: regex on the reference parameter name, max_ndim, lr_scale, weight_decay_scale} that give tensors
        # multiples of the group's lr / weight_decay (first matching rule per attribute; trainers/data_parallel.py::resolve_tensor_scales).
        # log_tensor_stats (0 = off): k > 0 prints, after each training log line, the k tensors with the largest gradient norm and every tensor
        # whose gradient holds an inf or a NaN.
        # name 'LAMB': AdamW with layer-wise trust ratios (FusedLAMB; `depth` takes torch.optim.AdamW's keys), for the large effective batches
        # that accumulate_grad_batches reaches.  lamb_exclude: rules {pattern, max_ndim} in tensor_scales' matching language; a matching tensor
        # keeps plain AdamW arithmetic (the default excludes the tensors of at most one dimension: biases and GroupNorm affine tensors;
        # [] adapts everything).  lamb_max_trust (0 = no cap): upper limit of the trust ratio.  Both are read only when name is 'LAMB'.
        # warmup_steps (0 = off): W > 0 multiplies the lr the step kernels see by min(1, k / W) at optimizer step k; the group's lr, and with
        # it StepLR and the checkpoint, is untouched (Adam, AdamW, LAMB; SGD keeps no step count in its checkpoint and raises).
        'optimizer': {'name': 'Adam', 'depth': {'lr': 0.0002, 'weight_decay': 0.0}, 'clip_grad_norm': 0.0, 'skip_nonfinite_steps': False,
                      'ema_decay': 0.0, 'ema_warmup': True, 'ema_validate': True, 'tensor_scales': [], 'log_tensor_stats': 0,
                      'warmup_steps': 0, 'lamb_exclude': [{'max_ndim': 1}], 'lamb_max_trust': 0.0},
        'scheduler': {'name': 'StepLR', 'step_size': 10, 'gamma': 0.5},
        'params': {'crop': '', 'min_depth': 0.0, 'max_depth': 80.0, 'scale_output': 'resize'},     # default_config.py:84-87
        'loss': {'supervised_method': 'sparse-l1', 'supervised_num_scales': 4, 'supervised_loss_weight': 0.9,
                 'depth_edges_loss_weight': 1.0, 'edges_depth_edge_loss_all_scales': False, 'upsample_depth_maps': False,
                 'flip_lr_prob': 0.5, 'progressive_scaling': 0.0},
        'depth_net': {'name': 'PackNetSAN01', 'checkpoint_path': '', 'checkpoint_ema': False, 'version': '1A', 'dropout': 0.0,
                      'freeze_encoder': False, 'freeze_decoder': False, 'freeze_san': False, 'input_channels': 3,
                      'is_depth_aux_net': False, 'output_channels': 1},
    },
    'edges': {'train_depth_edges': True, 'depth_edges_loss_weight': 10.0, 'use_external_edges_for_loss': True,
              'edge_loss_type': 'cross_entropy', 'edge_loss_class_list_to_mask_out': [],
              'depth_edge_loss_pos_to_neg_weight': 1.0},
    # jittering / crop_train_borders: () = off.  The reference's default_config.py:166 jitters with (0.2, 0.2, 0.2, 0.05) and crops
    # nothing; a run that wants the reference's recipe sets  datasets.augmentation.jittering: [0.2, 0.2, 0.2, 0.05]  in its YAML.
    # lidar_scale / lidar_add / lidar_drop_rate, input_depth_type, is_infer_rgb / is_infer_lidar: default_config.py:169-171,184,217,223-224
    # validation / test sections, crop_eval_borders, gt_crop: default_config.py:168,192-225 (no validation split = no validation)
    'datasets': {'augmentation': {'image_shape': (384, 1280), 'jittering': (), 'crop_train_borders': (), 'crop_eval_borders': (),
                                  'lidar_scale': (), 'lidar_add': (), 'lidar_drop_rate': 0.0},
                 # num_workers: 0 = SplitLoader (one sample at a time on the training stream).  The reference's default_config.py sets 16 DataLoader
                 # processes; here > 0 selects the prefetching loader (datasets/prefetch.py) with that many decode THREADS (at most 16), `prefetch`
                 # batches ahead; a run that wants it sets  datasets.train.num_workers: 8  in its YAML.
                 'train': {'batch_size': 8, 'input_depth_type': [''], 'num_workers': 0, 'prefetch': 2},
                 'validation': {'batch_size': 1, 'dataset': [], 'path': [], 'split': [], 'depth_type': [''], 'input_depth_type': [''],
                                'cameras': [[]], 'gt_crop': []},
                 'test': {'batch_size': 1, 'dataset': [], 'path': [], 'split': [], 'depth_type': [''], 'cameras': [[]],
                          'input_depth_type': [''], 'is_infer_rgb': True, 'is_infer_lidar': True}},
    # monitor / monitor_index / mode: default_config.py:26-28.  save_top_k stays -1 here (the reference's default is 5): one file per epoch
    # unless a config asks for the top-k policy (models/model_checkpoint.py::CheckpointPolicy)
    'checkpoint': {'filepath': '', 'save_top_k': -1, 'monitor': 'loss', 'monitor_index': 0, 'mode': 'auto'},
    # default_config.py:228-238: folder '' = ModelWrapper.test_step saves nothing (utils/save.py)
    'save': {'folder': '', 'depth': {'rgb': True, 'viz': True, 'npz': True, 'png': True, 'multiscale': False}, 'pretrained': ''},
}


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v


def default_config():
    return Cfg.wrap(copy.deepcopy(_DEFAULTS))


def load_config(yaml_path=None, overrides=None):
    cfg = copy.deepcopy(_DEFAULTS)
    if yaml_path:
        import yaml
        with open(yaml_path) as f:
            _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        _merge(cfg, overrides)
    return Cfg.wrap(cfg)
