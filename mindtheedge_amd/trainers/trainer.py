"""One-process-per-GPU trainer: the MI355X replacement of CommonTrainer/HorovodTrainer
(packnet_sfm/trainers/common_trainer.py:22-185, horovod_trainer.py).  Same surface: ``Trainer(**config.arch,
checkpoint=None).fit(module)``, ``proc_rank``, ``world_size``, ``is_rank_0``.  The inner loop is the reference's
zero_grad -> to-device -> training_step -> backward -> optimizer.step, minus its 4-6 ``.item()`` host syncs per step:
running means are accumulated on the device and read once per ``log_every`` steps."""
import contextlib
import os

import torch
import torch.distributed as dist


def sample_to_cuda(data, device):
    if isinstance(data, dict):
        return {k: sample_to_cuda(v, device) for k, v in data.items()}
    if isinstance(data, (list, tuple)):
        return [sample_to_cuda(v, device) for v in data]
    if torch.is_tensor(data):
        return data.to(device, non_blocking=True)
    return data


def accumulation_groups(n_batches, k):
    """Sizes of the accumulation groups that n_batches micro-batches form at k per optimizer step, in order: full groups of k and,
    where k does not divide n_batches, one trailing short group (which steps too).  (5, 2) -> [2, 2, 1]; k = 1 -> all ones."""
    if int(k) < 1 or int(n_batches) < 0:
        raise ValueError("accumulation_groups({}, {}): n_batches >= 0 and k >= 1".format(n_batches, k))
    full, rest = divmod(int(n_batches), int(k))
    return [int(k)] * full + ([rest] if rest else [])


def _with_group_end(dataloader, k):
    """(batch, True for the last micro-batch of its accumulation group) for every batch of the loader.  With a length the groups are
    accumulation_groups(len, k); a loader without one is read one batch ahead, which finds the same ends."""
    if k == 1:
        for batch in dataloader:
            yield batch, True
    elif hasattr(dataloader, '__len__'):
        ends, at = set(), 0
        for size in accumulation_groups(len(dataloader), k):
            at += size
            ends.add(at)
        for i, batch in enumerate(dataloader):
            yield batch, (i + 1) in ends
    else:
        it, end, in_group = iter(dataloader), object(), 0
        ahead = next(it, end)
        while ahead is not end:
            batch, ahead = ahead, next(it, end)
            in_group += 1
            last = in_group == k or ahead is end
            if last:
                in_group = 0
            yield batch, last


def tensor_stats_lines(stats, k, trust=None):
    """The log lines of model.optimizer.log_tensor_stats = k from FusedFlatOptimizer.tensor_stats(): the k tensors with the largest
    gradient norm (non-finite norms first), then every tensor whose gradient holds an inf or a NaN, by name.  ``trust``
    (FusedLAMB.trust_ratios(), else None): each tensor line ends with that tensor's trust ratio; without it the lines are what they were."""
    def key(s):
        return (0, 0.0) if s['grad_norm'] != s['grad_norm'] or s['grad_norm'] == float('inf') else (1, -s['grad_norm'])
    lines = ['  grad top {} | {} | norm {:.4g} | amax {:.4g} | weight norm {:.4g} | lr x{:g} | wd x{:g}'.format(
        i + 1, s['name'], s['grad_norm'], s['grad_amax'], s['weight_norm'], s['lr_scale'], s['weight_decay_scale'])
        for i, s in enumerate(sorted(stats, key=key)[:int(k)])]
    if trust is not None:
        q_of = {r['name']: r['trust_ratio'] for r in trust}
        lines = [line + ' | trust {:.4g}'.format(q_of[s['name']]) for line, s in zip(lines, sorted(stats, key=key)[:int(k)])]
    lines += ['  grad non-finite | {} | {} of {} elements'.format(s['name'], s['nonfinite'], s['numel']) for s in stats if s['nonfinite'] > 0]
    return lines


class Trainer:
    def __init__(self, min_epochs=0, max_epochs=50, validate_first=False, checkpoint=None, log_every=50, accumulate_grad_batches=None,
                 **kwargs):
        self.min_epochs, self.max_epochs, self.validate_first = min_epochs, max_epochs, validate_first
        self.checkpoint, self.log_every = checkpoint, log_every
        # micro-batches per optimizer step (arch.accumulate_grad_batches); None: what the module's configuration says
        if accumulate_grad_batches is not None and int(accumulate_grad_batches) < 1:
            raise ValueError("Invalid accumulate_grad_batches value: {} (an integer >= 1; 1 = off)".format(accumulate_grad_batches))
        self.accumulate_grad_batches = None if accumulate_grad_batches is None else int(accumulate_grad_batches)
        self.distributed = int(os.environ.get('WORLD_SIZE', '1')) > 1
        if self.distributed and not dist.is_initialized():
            local = int(os.environ.get('LOCAL_RANK', '0'))
            torch.cuda.set_device(local)
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        self.device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None

    @property
    def proc_rank(self):
        return dist.get_rank() if dist.is_initialized() else 0

    @property
    def world_size(self):
        return dist.get_world_size() if dist.is_initialized() else 1

    @property
    def is_rank_0(self):
        return self.proc_rank == 0

    def fit(self, module, train_dataloader=None, epochs=None, val_dataloaders=None):
        """``fit(module)`` as the reference (trainers/common_trainer.py:42-91): the module hands over its optimizer, scheduler
        and dataloaders (``module.train_dataloader()`` / ``module.val_dataloader()``); the loaders may also be passed in."""
        if self.device is None:
            raise RuntimeError("mindtheedge_amd trains on MI355X GPUs only")
        module.trainer = self
        module.to(self.device)
        optimizer, scheduler = module.configure_optimizers()
        if self.accumulate_grad_batches not in (None, getattr(optimizer, 'accumulate_grad_batches', 1)):
            raise ValueError("Trainer(accumulate_grad_batches={}) but the module's optimizer was built with {}".format(
                self.accumulate_grad_batches, getattr(optimizer, 'accumulate_grad_batches', 1)))
        if train_dataloader is None:
            train_dataloader = module.train_dataloader()
        if val_dataloaders is None:
            val_dataloaders = module.val_dataloader() if hasattr(module, 'val_dataloader') else None
        history = []
        if val_dataloaders and self.validate_first:
            history.append({'validation': self.validate(val_dataloaders, module)})
        for epoch in range(module.current_epoch, epochs if epochs is not None else self.max_epochs):
            if hasattr(getattr(train_dataloader, 'sampler', None), 'set_epoch'):
                train_dataloader.sampler.set_epoch(epoch)
            history.append(self.train(train_dataloader, module, optimizer))
            if val_dataloaders:
                history[-1]['validation'] = self.validate(val_dataloaders, module)
            # as the reference (:80-91): save BEFORE the epoch counter advances, so 'epoch' in the file is the 0-based index of
            # the epoch that just finished and a resume continues at epoch + 1 (one file per epoch, no top-k policy)
            # a CheckpointPolicy (models/model_checkpoint.py) given as ``checkpoint`` decides from the epoch's validation metrics instead
            if self.checkpoint and self.is_rank_0:
                if hasattr(self.checkpoint, 'save'):
                    self.checkpoint.save(module, history[-1].get('validation'))
                else:
                    from ..models.model_checkpoint import save_checkpoint
                    save_checkpoint(os.path.join(str(self.checkpoint), 'epoch={}.ckpt'.format(module.current_epoch)), module)
            module.current_epoch += 1
            scheduler.step()
        return history

    def validate(self, dataloaders, module):
        """Reference CommonTrainer.validate (trainers/common_trainer.py:187-210): every validation dataset in turn,
        ``module.validation_step`` per batch, ``module.validation_epoch_end`` per dataset -> [metrics dict per dataset].
        The per-batch metrics stay on the device; the epoch end reads them once."""
        was_training = module.training
        module.eval()
        results = []
        # an optimizer that keeps a weight EMA (model.optimizer.ema_decay > 0) validates on the average unless ema_validate is off: the
        # block swaps the average in and the raw weights back (FusedFlatOptimizer.ema_weights), so the checkpoint policy ranks epochs by it
        opt = getattr(module, 'optimizer', None)
        averaged = opt is not None and getattr(opt, 'ema_decay', 0.0) > 0.0 and getattr(module, 'ema_validate', True)
        with (opt.ema_weights() if averaged else contextlib.nullcontext()):
            for n, dataloader in enumerate(dataloaders):
                outputs = [module.validation_step(sample_to_cuda(batch, self.device), i, n) for i, batch in enumerate(dataloader)]
                results.append(module.validation_epoch_end(outputs, n))
        module.train(was_training)
        return results

    def train(self, dataloader, module, optimizer):
        module.train()
        run = torch.zeros(3, device=self.device)               # loss, supervised, edge running sums (device side)
        n, last = 0, None
        # gradient accumulation: k micro-batches per optimizer step (1: every batch steps, the loop below is the plain one).  The loss sums
        # stay per batch; the gradient norm is one per optimizer step and is averaged over those
        k = getattr(optimizer, 'accumulate_grad_batches', 1)
        nsteps = 0
        # a clipping / guarding optimizer leaves ctl = {clip coefficient, skip flag, gradient norm, skipped steps} on the device: the norm
        # joins the running sums (a skipped step's norm is inf or NaN and counts as 0), the count is read with them
        ctl = getattr(optimizer, 'ctl', None)
        gsum = torch.zeros((), device=self.device) if ctl is not None else None

        def read():
            """the running means as Python numbers (+ mean gradient norm and skipped steps with a ctl): one host read"""
            return (run / n).tolist() if ctl is None else torch.cat([run / n, (gsum / max(nsteps, 1)).reshape(1), ctl[3:4]]).tolist()

        for i, (batch, steps) in enumerate(_with_group_end(dataloader, k)):
            optimizer.zero_grad()
            batch = sample_to_cuda(batch, self.device)
            if steps:
                output = module.training_step(batch, i, None)
                output['loss'].backward()
                optimizer.step()
                nsteps += 1
            else:                                               # not the last of its group: no collective, the gradient joins the group's sum
                with optimizer.no_sync():
                    output = module.training_step(batch, i, None)
                    output['loss'].backward()
                optimizer.accumulate()
            m = output['metrics']
            zero = run.new_zeros(())
            run += torch.stack([output['loss'].detach().sum(), m.get('supervised_loss', zero).sum(), m.get('edge_loss', zero).sum()])
            if ctl is not None and steps:
                gsum += torch.where(torch.isfinite(ctl[2]), ctl[2], torch.zeros_like(ctl[2]))
            n += 1
            if self.is_rank_0 and self.log_every and n % self.log_every == 0:
                last = read()                                   # the only host sync
                line = 'step {} | Avg. {:.4f} | Sup. {:.4f} | Edge RGB {:.4f}'.format(n, *last[:3])
                if ctl is not None:
                    line += ' | Grad norm {:.4f} | Skipped {}'.format(last[3], int(last[4]))
                print(line, flush=True)
                if getattr(module, 'log_tensor_stats', 0) > 0 and hasattr(optimizer, 'tensor_stats'):
                    # model.optimizer.log_tensor_stats: one more read-only launch and host read per log line; the gradient buffer still
                    # holds this batch's gradient (zero_grad comes with the next batch)
                    trust = optimizer.trust_ratios() if hasattr(optimizer, 'trust_ratios') else None      # LAMB only: one more host read
                    for extra in tensor_stats_lines(optimizer.tensor_stats(), module.log_tensor_stats, trust):
                        print(extra, flush=True)
        if n:
            last = read()
        out = {'steps': n, 'avg_loss': last[0] if last else None, 'avg_supervised': last[1] if last else None,
               'avg_edge': last[2] if last else None}
        if ctl is not None:
            out.update(avg_grad_norm=last[3] if last else None, skipped_steps=int(last[4]) if last else 0)
        if k > 1:
            out['optimizer_steps'] = nsteps
        return out
