"""Checkpoint FORMAT of the reference (checkpoint half): packnet_sfm/models/model_checkpoint.py:71-81
writes ``{'config', 'epoch', 'state_dict', 'optimizer', 'scheduler'}`` (+ ``'state_dict_ema'``, ``'ema'`` when the optimizer averages its weights) with ``state_dict`` keys ``model.depth_net.*`` and
the optimizer layout of the configured torch class (``torch.optim.Adam`` / ``AdamW`` / ``SGD``); packnet_sfm/utils/load.py:117-201 reads it back (and TRI's published
``PackNetSAN01_*.ckpt`` files, whose extra sparse-branch tensors are skipped by the shape-checked, non-strict load in
``utils/load.py::load_network``).  ``save_checkpoint`` writes one file, ``load_checkpoint`` reads one; ``CheckpointPolicy`` is the
keep-the-best-k part of the reference's ModelCheckpoint around them (its S3 sync, code tarball, F1 file-name suffix and save_freq
deletion loop are not rebuilt)."""
import os

import torch


def _plain(obj):
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_plain(v) for v in obj)
    return obj


def save_checkpoint(filepath, model_wrapper):
    """One ``.ckpt`` in the reference layout.  Tensors are written from the host (flat-buffer views are cloned)."""
    os.makedirs(os.path.dirname(os.path.abspath(filepath)), exist_ok=True)
    from .. import kernels as K
    if torch.cuda.is_available():
        K.join_side_stream()
        torch.cuda.synchronize()
    ckpt = {
        'config': _plain(dict(model_wrapper.config)),
        'epoch': model_wrapper.current_epoch,
        'state_dict': {k: v.detach().cpu().clone() for k, v in model_wrapper.state_dict().items()},
        'optimizer': model_wrapper.optimizer.state_dict() if model_wrapper.optimizer is not None else None,
        'scheduler': model_wrapper.scheduler.state_dict() if model_wrapper.scheduler is not None else None,
    }
    if ckpt['optimizer'] is not None:
        # every tensor of a state entry, whatever the optimizer keeps (Adam / AdamW: step, exp_avg, exp_avg_sq; SGD: momentum_buffer)
        ckpt['optimizer']['state'] = {i: {k: v.cpu() if torch.is_tensor(v) else v for k, v in st.items()}
                                      for i, st in ckpt['optimizer']['state'].items()}
    opt = model_wrapper.optimizer
    if opt is not None and getattr(opt, 'ema_decay', 0.0) > 0.0:
        # a run that averages its weights: 'state_dict_ema' has the keys of 'state_dict' with every trained tensor taken from the average
        # (buffers and untrained tensors are the raw file's), 'ema' the schedule's state.  'state_dict' stays the raw weights: the
        # reference and every loader read the file as before, and a resume is exact.
        averaged = opt.ema_named()
        ckpt['state_dict_ema'] = dict(ckpt['state_dict'])
        for k, p in model_wrapper.named_parameters():
            if id(p) in averaged and k in ckpt['state_dict_ema']:
                ckpt['state_dict_ema'][k] = averaged[id(p)].detach().cpu().clone()
        ckpt['ema'] = opt.ema_state()
    torch.save(ckpt, filepath)
    return filepath


def load_checkpoint(filepath):
    """-> the checkpoint dict, ready for ``ModelWrapper(config, resume=ckpt)`` (drops None optimizer / scheduler entries)."""
    from ..utils.load import read_checkpoint
    ckpt = read_checkpoint(filepath)
    return {k: v for k, v in ckpt.items() if v is not None}


def monitor_mode(monitor, mode='auto'):
    """'min' / 'max' as given; 'auto' = 'max' when the monitored name contains 'acc' or 'a1' or starts with 'fmeasure', else 'min'
    (reference model_checkpoint.py:46-55)."""
    if mode in ('min', 'max'):
        return mode
    if mode != 'auto':
        raise ValueError("checkpoint.mode must be 'auto', 'min' or 'max', got {!r}".format(mode))
    return 'max' if ('acc' in monitor or 'a1' in monitor or monitor.startswith('fmeasure')) else 'min'


class CheckpointPolicy:
    """The keep-the-best-k policy of the reference's ModelCheckpoint (models/model_checkpoint.py:99-216) around ``save_checkpoint``.

    ``save(model_wrapper, metrics)`` is called once per finished epoch with the list of validation dicts of that epoch (one per dataset,
    as Trainer.validate returns them; None or [] without validation):

      * save_top_k == -1, or no validation metrics: ``<dirpath>/epoch=N.ckpt`` every epoch, nothing deleted -- the behaviour without a policy
      * otherwise the monitored value is ``metrics[monitor_index]['<prefix>-<monitor>']`` (the dataset's prefix as
        ModelWrapper.dataset_prefix gives it; a key that ends in '-<monitor>' when the wrapper knows no prefix), the file is
        ``epoch=N_<monitor>=<value:.3f>.ckpt``, the best ``save_top_k`` files stay (0 keeps all) and the file that drops out is deleted;
        an epoch that does not make the top k writes nothing.

    Left out of the reference's class: the S3 sync, the code tarball, the ``_rgb_f1_.._lidar_f1_..`` file-name suffix, and the loop that
    deletes earlier epochs' files by ``save_freq``."""

    def __init__(self, dirpath, monitor='loss', monitor_index=0, mode='auto', save_top_k=-1):
        self.dirpath, self.monitor, self.monitor_index = str(dirpath), monitor, int(monitor_index)
        self.save_top_k = int(save_top_k)
        self.mode = monitor_mode(monitor, mode)
        self.best_k = {}                                  # path -> monitored value

    @classmethod
    def from_config(cls, dirpath, checkpoint_cfg):
        c = checkpoint_cfg or {}
        return cls(dirpath, c.get('monitor') or 'loss', c.get('monitor_index') or 0, c.get('mode') or 'auto',
                   -1 if c.get('save_top_k') is None else c.get('save_top_k'))

    def monitored(self, model_wrapper, metrics):
        if not metrics or len(metrics) <= self.monitor_index or not metrics[self.monitor_index]:
            return None
        row = metrics[self.monitor_index]
        prefix = model_wrapper.dataset_prefix('validation', self.monitor_index) if hasattr(model_wrapper, 'dataset_prefix') else None
        if prefix is not None and '{}-{}'.format(prefix, self.monitor) in row:
            return float(row['{}-{}'.format(prefix, self.monitor)])
        hits = [k for k in row if k.endswith('-' + self.monitor)]
        if len(hits) != 1:
            raise KeyError("checkpoint.monitor {!r} is not among the validation metrics {}".format(self.monitor, sorted(row)))
        return float(row[hits[0]])

    def save(self, model_wrapper, metrics=None):
        """-> the path written, or None when this epoch did not make the top k"""
        epoch = model_wrapper.current_epoch
        current = None if self.save_top_k == -1 else self.monitored(model_wrapper, metrics)
        if current is None:
            return save_checkpoint(os.path.join(self.dirpath, 'epoch={}.ckpt'.format(epoch)), model_wrapper)
        path = os.path.join(self.dirpath, 'epoch={}_{}={:.3f}.ckpt'.format(epoch, self.monitor, current))
        k = self.save_top_k
        better = (lambda a, b: a < b) if self.mode == 'min' else (lambda a, b: a > b)
        if k > 0 and len(self.best_k) >= k:
            worst = (max if self.mode == 'min' else min)(self.best_k, key=self.best_k.get)
            if not better(current, self.best_k[worst]):
                return None
            del self.best_k[worst]
            if worst != path and os.path.isfile(worst):
                os.remove(worst)
        self.best_k[path] = current
        return save_checkpoint(path, model_wrapper)
