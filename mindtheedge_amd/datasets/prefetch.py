"""Prefetching training loader: ``SplitLoader``'s batches, bit for bit, without its per-sample host reads.

  worker threads   decode the files of up to ``prefetch`` batches ahead (batch_prep.decode_train_record: PIL / numpy only; Pillow's
                   decoders release the GIL).  They never touch the device or its runtime.
  consumer thread  (the one that iterates) draws the batch's random numbers, packs the raw arrays and a descriptor table into one pinned
                   arena, queues ONE upload and a fixed handful of launches (batch_prep.prepare_targets, image_prep) on the current stream.

The random draws stay where ``SplitLoader`` makes them: ``draw_color_jitter`` (Python's ``random``) and the LiDAR perturbation
(``np.random``) are drawn on the consumer thread, per sample in batch order, when the batch is handed over -- not when it is decoded --
so the global draw sequence, including its interleaving with whatever the training loop draws between batches, is unchanged.

The LiDAR column (``input_depth_type``) rides along.  The workers decode its file raw and count the returns n of the cropped and resized
map (``lidar_prep.resized_cells``); at hand-over the consumer draws the perturbation for n points, counts the survivors n' from the drawn
offsets (``lidar_prep.count_survivors``) and draws the keep permutation for them -- the two counts ``augment_depth_values`` reads back from
the device, computed on the host instead.  The raw maps, the draws and a descriptor row per sample go up in the batch's one arena; the
resize of all maps is one more row per sample in ``mte_batch_prep``, the perturbation one ``mte_batch_lidar_perturb`` (nine launches
whatever the batch size).  That pass leaves the device's own counts beside the host's in a status array, copied into the slot's pinned
memory behind it and compared when the slot comes round again (its event has completed by then): a difference raises ``MteError`` naming
the batch -- the draws were sized for another map.  A batch with a velodyne ``.bin`` record (its count depends on the device projection)
and a stage built with ``batched_lidar=False`` go through the per-sample functions (``read_lidar_map``, ``resize_depth_preserve``,
``augment_depth_values``) at hand-over, with their two host reads per perturbed map.
"""
import collections
import weakref
from concurrent.futures import ThreadPoolExecutor

import torch

from . import batch_prep as bp

MAX_WORKERS = 16


def choose_loader(num_workers):
    """datasets.train.num_workers -> 'split' (0 / None: SplitLoader, the default) or 'prefetch' (> 0: PrefetchSplitLoader)"""
    n = int(num_workers or 0)
    if n < 0:
        raise ValueError("datasets.train.num_workers must be >= 0, got {}".format(num_workers))
    return 'prefetch' if n > 0 else 'split'


def epoch_batches(n, batch_size, rank, world, shuffle, seed, epoch):
    """SplitLoader's index order: seeded randperm (or file order), rank-strided, cut into batches, ragged tail dropped"""
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch)).tolist() if shuffle else list(range(n))
    mine = order[rank::world]
    return [mine[i * batch_size:(i + 1) * batch_size] for i in range(n // world // batch_size)]


def draw_handover(samples, borders, shape, jittering, lidar=None):
    """The random draws of one batch at hand-over, per sample in batch order like ds[j] for j in the batch: the colour jitter from
    ``random`` and, with lidar = (lidar_scale, lidar_add, lidar_drop_rate) for a batch whose column is batched and perturbed, the LiDAR
    perturbation from ``np.random`` (lidar_prep.draw_batch: perturbation for n, survivor count, keep permutation for n').  n comes from the
    worker's 'lidar_cells'; a decoder that did not count leaves it to be counted here.  -> (jitter parameters, per-sample LiDAR draws or []).
    Host only."""
    from . import image_prep as ip
    from . import lidar_prep as lp
    params, drawn = [], []
    for b, smp in enumerate(samples):
        params.append(ip.draw_color_jitter(jittering))
        if lidar is not None:
            cells = smp.get('lidar_cells')
            if cells is None:
                cells = lp.resized_cells(smp['lidar'], bp.crop_window(borders[b], *smp['lidar'].shape), shape)
            drawn += lp.draw_batch([cells], shape, lidar[0], lidar[1], lidar[2])
    return params, drawn


class _Slot:
    def __init__(self):
        self.host, self.dev, self.event = bp.HostArena(pin=True), None, None
        self.status, self.check = None, None            # pinned int32 [B,4] of the LiDAR pass; (event behind its copy, B, the batch's indices)


class DeviceStage:
    """Decoded records of one batch -> the collated device batch of KittiEdgeSplitDataset (mode 'train').  Consumer thread only.
    Keeps ``slots`` pairs of (pinned arena, device arena); a slot is reused after ``slots`` batches, guarded by an event recorded behind
    its upload -- queried first: in steady state it completed long before and nothing waits.  batched_lidar=False sends the LiDAR column
    of every batch through the per-sample functions (A/B timing, tests)."""

    def __init__(self, dataset, slots, batched_lidar=True):
        if dataset.mode != 'train':
            raise ValueError("the prefetching loader builds training batches; evaluation uses EvalLoader")
        self.ds = dataset
        self.slots = [_Slot() for _ in range(int(slots))]
        self.turn = 0
        self.batched_lidar = bool(batched_lidar)

    def decode(self, idx):
        """what a worker thread runs for one record"""
        ds = self.ds
        return bp.decode_train_record(ds.records[idx], ds.root, with_lidar=ds.with_input_depth, lidar_raw=self.batched_lidar,
                                      crop_borders=ds.crop_train_borders, shape=ds.shape)

    def _verify(self, slot):
        """the count check of the LiDAR pass that last used this slot (module docstring); waits only if that pass has not completed"""
        if slot.check is None:
            return
        from . import lidar_prep as lp
        event, B, indices = slot.check
        slot.check = None
        if not event.query():
            event.synchronize()
        lp.check_status(slot.status.numpy()[:B], 'the batch of records {}'.format(list(indices)))

    def verify_pending(self):
        """the count checks that are still outstanding (the loader calls it when an epoch is exhausted)"""
        for slot in self.slots:
            self._verify(slot)

    def _upload(self, arrays, rows):
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % len(self.slots)
        self._verify(slot)
        if slot.event is not None and not slot.event.query():
            slot.event.synchronize()                                      # the slot's previous upload still reads the pinned buffer
        _, _, total = bp.arena_layout(arrays, sum(r is not None for r in rows))
        slot.host.reserve(total)
        if slot.dev is None or slot.dev.numel() < slot.host.capacity:
            slot.dev = torch.empty(slot.host.capacity, dtype=torch.uint8, device=self.ds.device)
        t_off, offs, total, live = bp.pack_arena(slot.host, arrays, rows)
        slot.dev[:total].copy_(slot.host.tensor[:total], non_blocking=True)
        slot.event = torch.cuda.Event()
        slot.event.record()
        return slot, t_off, offs, len(live)

    def _lidar(self, smp, borders, out):
        """the LiDAR column of one sample, as KittiEdgeSplitDataset.__getitem__ (per sample, with its host reads)"""
        import numpy as np
        from . import lidar_prep as lp
        from .kitti_edges import resize_depth_preserve
        ds = self.ds

        def as_read(raw):                                                 # read_png_depth's arithmetic on a map the workers kept raw
            return raw if raw.dtype != np.uint16 else np.where(raw == 0, np.float32(-1.), raw.astype(np.float32) / np.float32(256.)).astype(np.float32)

        if smp.get('lidar') is not None:                                  # decoded ahead, but a .bin record shares its batch
            lidar = torch.from_numpy(np.ascontiguousarray(as_read(smp['lidar']))).to(ds.device)
        else:
            d_full = None
            if smp['depth'] is not None and smp['lidar_path'].endswith('.bin'):  # only the projection looks at the depth map
                d_full = as_read(smp['depth'])
            lidar = lp.read_lidar_map(smp['lidar_path'], ds.device, depth_map=d_full)
        if borders is not None:
            lidar = lidar[borders[1]:borders[3], borders[0]:borders[2]].contiguous()
        lidar = resize_depth_preserve(lidar, ds.shape)
        out['lidar'].append(lidar.unsqueeze(0))
        if len(ds.lidar_scale) > 0 and len(ds.lidar_add) > 0:
            out['input_depth'].append(lp.augment_depth_values(lidar, ds.lidar_scale, ds.lidar_add, ds.lidar_drop_rate).unsqueeze(0))
        else:
            out['input_depth'].append(lidar.clone().unsqueeze(0))

    def __call__(self, samples, indices):
        from . import image_prep as ip
        from . import lidar_prep as lp
        from ..utils.edge import resize_linear
        from .kitti_edges import normal_target
        ds = self.ds
        H, W = ds.shape
        B = len(samples)
        borders = [ip.parse_crop_borders(ds.crop_train_borders, s['rgb'].shape[:2]) if ds.crop_train_borders else None for s in samples]
        with_lidar = ds.with_input_depth and all(s.get('lidar_path') for s in samples)
        if ds.with_input_depth and not with_lidar and any(s.get('lidar_path') for s in samples):
            raise KeyError("the records of one batch carry different maps (LiDAR column)")
        batched = with_lidar and self.batched_lidar and bp.lidar_batchable(samples)
        perturbed = len(ds.lidar_scale) > 0 and len(ds.lidar_add) > 0
        arrays, rows, keys, fallbacks, winner_elems, out_elems = bp.plan_targets(samples, borders, ds.shape, lidar=batched)
        n_maps = len(arrays)
        # the batched column draws here, before the arena is packed (its draws ride in it); the per-sample one behind the upload
        lidar = {'lidar': [], 'input_depth': []}
        params, extra = draw_handover(samples, borders, ds.shape, ds.jittering,
                                      (ds.lidar_scale, ds.lidar_add, ds.lidar_drop_rate) if batched and perturbed else None)
        packed = arrays + [s['rgb'] for s in samples] + lp.batch_arrays(extra)
        if extra:                                                         # the perturbation's table, behind the arrays its offsets point to
            _, ahead, _ = bp.arena_layout(packed, sum(r is not None for r in rows))
            packed.append(lp.pack_batch_rows(extra, ahead[n_maps + B:]).reshape(-1))
        slot, t_off, offs, n_rows = self._upload(packed, rows + [None] * (len(packed) - n_maps))
        if with_lidar and not batched:
            for b, smp in enumerate(samples):
                self._lidar(smp, borders[b], lidar)
        frames = []
        for b, smp in enumerate(samples):
            h, w = smp['rgb'].shape[:2]
            off = offs[n_maps + b]
            frame = slot.dev[off:off + h * w * 3].view(h, w, 3)
            if borders[b] is not None or (w, h) != (W, H):
                frame = ip.resize_image_u8(frame, (H, W), crop=borders[b])
            frames.append(frame)
        batch = {'idx': list(indices)}
        frames = torch.stack(frames)
        if ds.jittering:
            batch['rgb'], batch['rgb_original'] = ip.color_jitter_to_tensor(frames, params, want_original=True)
        else:
            batch['rgb'] = ip.color_jitter_to_tensor(frames)
        targets = bp.prepare_targets(slot.dev, slot.host.tensor, t_off, n_rows, keys, B, winner_elems, out_elems)
        for key, b, i, (x0, y0, ch, cw) in fallbacks:                    # a normal map that is not at its target size: the per-map path
            a = arrays[i]
            src = slot.dev[offs[i]:offs[i] + a.size].view(a.shape)[y0:y0 + ch, x0:x0 + cw]
            targets[key][b, 0].copy_(resize_linear(normal_target(src), tuple(targets[key].shape[-2:])))
        if 'depth' in targets:
            batch['depth'] = targets.pop('depth')
        if batched:
            batch['lidar'] = targets.pop('lidar')
            if perturbed:
                if slot.status is None or slot.status.numel() < 4 * B:
                    slot.status = torch.empty((B, 4), dtype=torch.int32, pin_memory=True)
                batch['input_depth'], status = lp.perturb_batch(batch['lidar'], slot.dev, slot.host.tensor, offs[-1])
                slot.status[:B].copy_(status, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                slot.check = (event, B, list(indices))
            else:
                batch['input_depth'] = batch['lidar'].clone()
        elif with_lidar:
            batch['lidar'], batch['input_depth'] = torch.stack(lidar['lidar']), torch.stack(lidar['input_depth'])
        batch.update(targets)
        return batch


class PrefetchSplitLoader:
    """``SplitLoader``'s surface (``__len__``, ``__iter__``, ``sampler.set_epoch``, ``shuffle``), index order and batches, with the file
    decoding on ``min(num_workers, 16)`` threads up to ``prefetch`` batches ahead and one batched preparation pass per batch on the device.

    An exception raised in a worker surfaces at the ``next()`` of the batch it belongs to.  Leaving the iterator early, exhausting it, or
    ``close()`` cancels what is pending and joins the threads.  The LiDAR column is decoded ahead and prepared in the batched pass; its
    count check (module docstring) raises at the ``next()`` that reuses the batch's slot, or when the epoch is exhausted.  ``device_stage`` / ``decode`` replace the device stage and the per-record decoder (tests run the loader without a GPU)."""

    def __init__(self, dataset, batch_size, rank=0, world=1, shuffle=True, seed=0, num_workers=4, prefetch=2, device_stage=None, decode=None,
                 batched_lidar=True):
        if int(num_workers) < 1 or int(prefetch) < 1:
            raise ValueError("num_workers and prefetch must be >= 1, got {} and {}".format(num_workers, prefetch))
        self.ds, self.bs, self.rank, self.world, self.shuffle, self.seed, self.epoch = dataset, batch_size, rank, world, shuffle, seed, 0
        self.num_workers, self.prefetch = min(int(num_workers), MAX_WORKERS), int(prefetch)
        self.sampler = self
        self._stage = device_stage if device_stage is not None else DeviceStage(dataset, self.prefetch + 2, batched_lidar=batched_lidar)
        self._decode = decode if decode is not None else self._stage.decode
        self._active = None

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.ds) // self.world // self.bs

    def close(self):
        """ends the running iterator, if any: pending decodes are cancelled, the worker threads joined"""
        gen = self._active() if self._active is not None else None
        self._active = None
        if gen is not None:
            gen.close()

    def __iter__(self):
        self.close()
        gen = self._run(epoch_batches(len(self.ds), self.bs, self.rank, self.world, self.shuffle, self.seed, self.epoch))
        self._active = weakref.ref(gen)
        return gen

    def _run(self, batches):
        pool = ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix='mte-decode')
        pending = collections.deque()
        upcoming = iter(batches)

        def submit():
            idxs = next(upcoming, None)
            if idxs is not None:
                pending.append((idxs, [pool.submit(self._decode, j) for j in idxs]))

        try:
            for _ in range(self.prefetch):
                submit()
            while pending:
                idxs, futures = pending.popleft()
                submit()                                                   # `prefetch` batches are in flight while this one is prepared
                samples = [f.result() for f in futures]                    # a worker's exception is raised here, at its batch
                yield self._stage(samples, idxs)
            verify = getattr(self._stage, 'verify_pending', None)
            if verify is not None:
                verify()                                                   # the last batches' LiDAR count checks: no slot reuse comes for them
        finally:
            for _, futures in pending:
                for f in futures:
                    f.cancel()
            pool.shutdown(wait=True)
