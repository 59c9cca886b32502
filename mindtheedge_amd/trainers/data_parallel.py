"""Flat parameter/gradient storage, bucketed gradient all-reduce (RCCL over xGMI) and the fused optimizers (Adam, AdamW, LAMB, SGD).

This is the MI355X-native replacement of the reference's dead Horovod path (``hvd.DistributedOptimizer`` in
packnet_sfm/trainers/horovod_trainer.py:53-55: average every parameter gradient across ranks, overlapped with
backward, waited in ``optimizer.step()``) and of ``torch.optim.Adam`` / ``AdamW`` / ``SGD`` (models/model_wrapper.py:142-180).

One process per GPU.  Parameters live in ONE flat fp32 buffer (77 M elements = 308 MB) and gradients in another, laid
out in *reverse execution order* so that gradient readiness during backward sweeps the buffer front to back.  The
gradient buffer is cut into ~32 MB buckets; a post-accumulate hook counts ready tensors per bucket and launches one
asynchronous ``all_reduce`` per bucket on RCCL's stream the moment the bucket is complete, so communication of the
decoder/late-encoder gradients overlaps the remaining backward.  xGMI is point-to-point (7 links/GPU): a few large
messages amortise the ring's per-link latency better than 218 small ones, and the two huge tensors
(pack5.conv 151 MB, pack4.conv 38 MB) finish early in backward, so their all-reduces hide under the high-resolution
layers' backward.  ``step()`` waits for the outstanding collectives and runs one fused optimizer kernel over the flat buffers.
"""
import contextlib
import os

import torch
import torch.distributed as dist


class FlatParameters:
    """Re-homes ``params`` into one flat fp32 buffer (+ one flat gradient buffer of the same layout)."""

    def __init__(self, params, reverse=True, align=64):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        order = list(reversed(params)) if reverse else list(params)
        # parameters that normally receive no gradient (PackNetSAN01's SAN fusion scalars without a LiDAR input) go to the tail:
        # in the first bucket they would keep it from ever completing during backward, and its all-reduce would run exposed
        order = [p for p in order if not getattr(p, '_mte_flat_tail', False)] + [p for p in order if getattr(p, '_mte_flat_tail', False)]
        dev = order[0].device
        offs, total = [], 0
        for p in order:
            offs.append(total)
            total += (p.numel() + align - 1) // align * align
        self.params, self.offsets, self.total, self.reverse = order, offs, total, reverse
        self.natural_params = params                       # the order the caller gave (torch.optim's state index space)
        self.offset_of = {id(p): o for p, o in zip(order, offs)}
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, o in zip(order, offs):
            view = self.flat[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.grad[o:o + p.numel()].view(p.shape)
        self.accum = None                                    # the micro-batch sum of gradient accumulation: see enable_accumulation
        self.sink = None
        if dev.type == "cuda":
            # backward kernels store conv / GroupNorm parameter gradients straight into self.grad (no per-tensor add)
            from .. import kernels as K
            self.sink = K.GradSink()
            for p in order:
                self.sink.register(p, p.grad)
            K.set_grad_sink(self.sink)

    def enable_accumulation(self):
        """``accum``: a second flat fp32 buffer of ``total`` elements (+4 B per parameter) that holds the sum of a group's earlier
        micro-batch gradients.  It exists only for an optimizer built with accumulate_grad_batches > 1."""
        if self.accum is None:
            self.accum = torch.zeros_like(self.grad)
        return self.accum

    def enable_ema(self):
        """``ema``: a flat fp32 buffer of ``total`` elements (+4 B per parameter) that holds the exponential moving average of ``flat``,
        laid out like it; it starts as a bit copy of the weights as they stand.  The attribute exists only for an optimizer built with
        ema_decay > 0."""
        if getattr(self, 'ema', None) is None:
            self.ema = self.flat.clone()
        return self.ema

    def segments(self, device=None):
        """The tensor layout of the flat buffers: one (begin, numel, slot) per tensor in FLAT order -- begin a multiple of ``align``,
        numel the tensor's true element count (the padding behind it is not part of it), slot the tensor's position in
        ``natural_params``.  With ``device``: (begins, numels) as two int64 tensors there instead, made on this call and not kept."""
        slot = {id(p): i for i, p in enumerate(self.natural_params)}
        segs = [(o, p.numel(), slot[id(p)]) for p, o in zip(self.params, self.offsets)]
        if device is None:
            return segs
        return (torch.tensor([s[0] for s in segs], dtype=torch.int64, device=device),
                torch.tensor([s[1] for s in segs], dtype=torch.int64, device=device))

    def block_classes(self, class_of_tensor, device=None):
        """The ``total / 64`` byte map of the SEG optimizer steps: entry b is the class of elements 64 b .. 64 b + 63.
        ``class_of_tensor``: one class id (0..255) per tensor in ``natural_params`` order.  Every tensor starts on a 64-element boundary,
        so a block belongs to one tensor; the padding blocks behind a tensor carry its class.  A uint8 tensor on the host, or on
        ``device`` when given (made on this call, not kept)."""
        if self.total % 64 or any(o % 64 for o in self.offsets):
            raise ValueError("block_classes needs a layout aligned to 64 elements")
        if len(class_of_tensor) != len(self.natural_params):
            raise ValueError("block_classes takes one class per tensor: {} for {} tensors".format(len(class_of_tensor), len(self.natural_params)))
        if any(int(c) != c or not 0 <= int(c) <= 255 for c in class_of_tensor):
            raise ValueError("class ids are integers in 0..255")
        out = torch.empty(self.total // 64, dtype=torch.uint8)
        ends = self.offsets[1:] + [self.total]
        for (o, _, slot), e in zip(self.segments(), ends):
            out[o // 64:e // 64] = int(class_of_tensor[slot])
        return out if device is None else out.to(device)

    def zero_grad(self):
        if self.grad.is_cuda:
            from .. import kernels as K
            K.join_side_stream()
        self.grad.zero_()
        if self.sink is not None:
            self.sink.reset()                                # every view may take one in-place store again
        for p, o in zip(self.params, self.offsets):          # re-attach if something replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view(p.shape)


class BucketedAllReduce:
    """Overlapped gradient averaging over a FlatParameters gradient buffer."""

    def __init__(self, flat, process_group=None, bucket_bytes=32 << 20, force=False, tail_bytes=2 << 20, message_bytes=32 << 20):
        self.flat, self.group = flat, process_group
        # A bucket never splits a tensor, so the 151 MB pack5.conv weight makes a 182 MB bucket: its all-reduce goes out as
        # <= message_bytes pieces (xGMI is point-to-point: a ring step moves message/world per link, and 32 MB pieces keep the
        # pipeline of RCCL's ring busy while letting later, smaller buckets interleave instead of queueing behind one giant
        # message).  SURVEY.md 7: "bucket must split tensors".
        self.message_elems = max(1, message_bytes // 4)
        self.launch_log = []        # per step: (bucket index, first element, elements, messages) in launch order
        self.exposed_events = None  # (start, end) device events around the wait in finish(): the exposed all-reduce time
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.buckets = []                                   # (start, end, n_tensors)
        cap = max(1, bucket_bytes // 4)
        start, count, self.bucket_of = 0, 0, {}
        for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
            end = flat.offsets[i + 1] if i + 1 < len(flat.params) else flat.total
            self.bucket_of[id(p)] = len(self.buckets)
            count += 1
            if end - start >= cap or i + 1 == len(flat.params):
                self.buckets.append((start, end, count))
                start, count = end, 0
        # The last bucket (the first layers of the encoder) completes only when backward ends, so its all-reduce is the one
        # that cannot hide: keep that exposed message small by cutting the final bucket where ~2 MB of gradients remain.
        if self.buckets and self.buckets[-1][2] > 1:
            s0, e0, n0 = self.buckets[-1]
            first = len(flat.params) - n0
            for j in range(first + 1, len(flat.params)):
                if (flat.total - flat.offsets[j]) * 4 <= tail_bytes and (flat.offsets[j] - s0) * 4 >= tail_bytes:
                    self.buckets[-1] = (s0, flat.offsets[j], j - first)
                    self.buckets.append((flat.offsets[j], e0, n0 - (j - first)))
                    for p in flat.params[j:]:
                        self.bucket_of[id(p)] = len(self.buckets) - 1
                    break
        self._ready = [0] * len(self.buckets)
        self._seen = set()          # a parameter may be announced by both the gradient sink and its autograd hook
        self._works = []
        self._hooks = []
        self._stream = None         # collectives are issued from here (see _launch)
        self.sync = True            # False inside no_sync(): gradients of a micro-batch that is not the last of its group stay local
        self._fold = None           # FlatParameters.accum while earlier micro-batches of the group wait in it (set by accumulate())
        self.active = self.world > 1 or (force and dist.is_available() and dist.is_initialized())   # force: single-rank RCCL tests
        if self.active:
            for p in flat.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad_ready))
            if getattr(flat, "sink", None) is not None:
                flat.sink.on_ready = self._on_grad_ready      # gradients written in place never reach AccumulateGrad

    def _on_grad_ready(self, p):
        if not self.sync:
            return
        if id(p) in self._seen:
            return
        self._seen.add(id(p))
        b = self.bucket_of[id(p)]
        self._ready[b] += 1
        if self._ready[b] == self.buckets[b][2]:
            s, e, _ = self.buckets[b]
            self._launch(s, e, b)

    def _messages(self, s, e):
        """[start, end) of a bucket cut into all-reduce messages of at most message_elems elements"""
        out = []
        while s < e:
            n = min(self.message_elems, e - s)
            out.append((s, s + n))
            s += n
        return out

    def fold_pending(self, accum):
        """From now until finish(): every bucket first takes ``accum``'s elements of its range, grad[s:e] += accum[s:e], and is reduced
        after that -- the earlier micro-batches of an accumulation group join the last one's gradient bucket by bucket, each once."""
        self._fold = accum

    def _launch(self, s, e, b=-1):
        msgs = self._messages(s, e)
        self.launch_log.append((b, s, e - s, len(msgs)))
        if not self.flat.grad.is_cuda:
            if self._fold is not None:
                self.flat.grad[s:e].add_(self._fold[s:e])
            for ms, me in msgs:
                self._works.append(dist.all_reduce(self.flat.grad[ms:me], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            return
        # The bucket's gradients were produced on the main stream AND on the weight-gradient side stream.  Order the
        # collective after both from a third stream, so that the main stream (the rest of backward) never stalls on
        # the side stream's lag at a bucket boundary.
        from .. import kernels as K
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        self._stream.wait_stream(torch.cuda.current_stream())
        K.side_streams_wait_into(self._stream)
        with torch.cuda.stream(self._stream):
            if self._fold is not None:
                # on the reduction stream, behind its waits for the main stream (accumulate()'s launches) and the side stream
                K.grad_accumulate_flat(self.flat.grad[s:e], self._fold[s:e], assign=False)
            for ms, me in msgs:
                self._works.append(dist.all_reduce(self.flat.grad[ms:me], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        """Wait for every launched collective; reduce buckets whose hooks never completed (unused parameters).
        Returns the factor that turns the summed gradient into the average (1/world)."""
        if self.flat.grad.is_cuda:
            from .. import kernels as K
            K.join_side_stream()
        if self.active:
            for b, (s, e, n) in enumerate(self.buckets):
                if self._ready[b] != n:
                    self._launch(s, e, b)
            timed = self.flat.grad.is_cuda
            if timed:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            for w in self._works:
                w.wait()
            if timed:
                ev1.record()                                # ev0 -> ev1 on the main stream = time the step waits for RCCL
                self.exposed_events = (ev0, ev1)
        self.last_launches = self.launch_log
        self._works, self._ready, self.launch_log = [], [0] * len(self.buckets), []
        self._seen.clear()
        self._fold = None
        return 1.0 / self.world

    def exposed_ms(self):
        """Device time the last finish() spent waiting for outstanding collectives (synchronises)."""
        if self.exposed_events is None:
            return 0.0
        self.exposed_events[1].synchronize()
        return float(self.exposed_events[0].elapsed_time(self.exposed_events[1]))

    def describe(self):
        """Static layout + the last step's launch order, for bench.py's JSON line."""
        return {"buckets_mb": [round((e - s) * 4 / 2**20, 2) for s, e, _ in self.buckets],
                "message_mb": round(self.message_elems * 4 / 2**20, 2),
                "messages_per_bucket": [len(self._messages(s, e)) for s, e, _ in self.buckets],
                "launch_order": [b for b, _, _, _ in getattr(self, "last_launches", [])],
                "launch_offsets_mb": [round(s * 4 / 2**20, 2) for _, s, _, _ in getattr(self, "last_launches", [])]}


def ema_decay_pair(t, decay, warmup=True):
    """(d32, omd32) of the t-th update (t = 1, 2, ...) of a weight EMA as Python floats that hold float32 values: d_t = min(decay,
    (1 + t) / (10 + t)) with the warm-up, else decay, in double precision; d32 = float32(d_t), omd32 = float32(1 - double(d32))"""
    import struct
    f32 = lambda x: struct.unpack('f', struct.pack('f', x))[0]
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + t) / (10.0 + t))
    d32 = f32(d)
    return d32, f32(1.0 - d32)


MAX_SCALE_CLASSES = 16                                       # the SEG kernels' class table (csrc/optim.hip: SEG_MAX_CLASSES)


def tensor_scale_classes(pairs):
    """[(lr_mult, wd_mult)] per tensor -> (classes, class_of_tensor): the distinct pairs in order of first appearance and every tensor's
    index into them.  Multipliers must be finite and >= 0; more than MAX_SCALE_CLASSES distinct pairs is a ValueError."""
    import math
    classes, index, class_of = [], {}, []
    for i, pair in enumerate(pairs):
        lm, wm = float(pair[0]), float(pair[1])
        for what, x in (('lr_scale', lm), ('weight_decay_scale', wm)):
            if not (math.isfinite(x) and x >= 0.0):
                raise ValueError("Invalid {} {} for tensor {}: multipliers are finite and >= 0".format(what, x, i))
        if (lm, wm) not in index:
            index[(lm, wm)] = len(classes)
            classes.append((lm, wm))
        class_of.append(index[(lm, wm)])
    if len(classes) > MAX_SCALE_CLASSES:
        raise ValueError("tensor_scales hold {} distinct (lr_scale, weight_decay_scale) pairs; the fused steps take at most {}".format(
            len(classes), MAX_SCALE_CLASSES))
    return classes, class_of


def match_tensor_rule(names, shapes, pattern=None, max_ndim=None):
    """The matching language of the per-tensor rules (tensor_scales, lamb_exclude): the positions of the tensors that a rule reaches --
    re.search(pattern, name) finds something (no pattern: every name) and, with max_ndim, the tensor has at most that many dimensions"""
    import re
    rx = re.compile(pattern) if pattern is not None else None
    return [i for i, (name, shape) in enumerate(zip(names, shapes))
            if not ((rx is not None and not rx.search(name)) or (max_ndim is not None and len(shape) > int(max_ndim)))]


def resolve_lamb_exclude(names, shapes, rules):
    """model.optimizer.lamb_exclude -> one ``adapt`` flag per tensor (FusedLAMB): a tensor that any rule {pattern, max_ndim} matches
    (match_tensor_rule, resolve_tensor_scales' language) is excluded from the layer-wise adaptation -- False: plain AdamW arithmetic, trust
    ratio 1 -- and every other tensor is adapted.  [] adapts everything.  An unknown key, a rule with neither key and a rule that matches
    no trained tensor are ValueErrors."""
    adapt = [True] * len(names)
    for rule in (rules or ()):
        rule = dict(rule)
        if set(rule) - {'pattern', 'max_ndim'} or not any(rule.get(k) is not None for k in ('pattern', 'max_ndim')):
            raise ValueError("lamb_exclude rule {}: keys are pattern and max_ndim, and a rule names at least one".format(rule))
        hits = match_tensor_rule(names, shapes, rule.get('pattern'), rule.get('max_ndim'))
        if not hits:
            raise ValueError("lamb_exclude rule with pattern {!r} (max_ndim {}) matches no trained tensor".format(
                rule.get('pattern'), rule.get('max_ndim')))
        for i in hits:
            adapt[i] = False
    return adapt


def warmup_factor(k, warmup_steps):
    """The linear learning-rate warm-up's factor at optimizer step k (1-based): min(1, k / W) in double precision, and exactly 1.0
    with W <= 0 (off).  A pure function of its arguments."""
    w = int(warmup_steps)
    if w <= 0:
        return 1.0
    return min(1.0, float(k) / float(w))


def resolve_tensor_scales(names, shapes, rules):
    """model.optimizer.tensor_scales -> one (lr_scale, weight_decay_scale) per tensor.

    names / shapes: the trained tensors' reference names and shapes, in one order.  rules: a list of {pattern, max_ndim, lr_scale,
    weight_decay_scale}: a rule MATCHES a tensor when re.search(pattern, name) finds something (no pattern: every name) and, with
    max_ndim, the tensor has at most that many dimensions.  For each tensor and each of the two attributes on its own, the first
    matching rule that names the attribute gives its value; a tensor that no such rule reaches gets 1.  A rule that matches no tensor
    at all is a ValueError that shows its pattern (a typo must not pass silently), as are an unknown key, a rule that names neither
    attribute, a negative or non-finite multiplier and more than MAX_SCALE_CLASSES distinct pairs."""
    keys = ('lr_scale', 'weight_decay_scale')
    out = [[None, None] for _ in names]
    for rule in (rules or ()):
        rule = dict(rule)
        unknown = set(rule) - {'pattern', 'max_ndim'} - set(keys)
        if unknown or not any(rule.get(k) is not None for k in keys):
            raise ValueError("tensor_scales rule {}: keys are pattern, max_ndim, lr_scale, weight_decay_scale, and a rule names at least "
                             "one of the two scales".format(rule))
        pattern, max_ndim = rule.get('pattern'), rule.get('max_ndim')
        hits = match_tensor_rule(names, shapes, pattern, max_ndim)
        for i in hits:
            for j, k in enumerate(keys):
                if rule.get(k) is not None and out[i][j] is None:
                    out[i][j] = float(rule[k])
        if not hits:
            raise ValueError("tensor_scales rule with pattern {!r} (max_ndim {}) matches no trained tensor".format(pattern, max_ndim))
    pairs = [(1.0 if a is None else a, 1.0 if b is None else b) for a, b in out]
    tensor_scale_classes(pairs)                              # the multipliers' and the class limit's ValueErrors
    return pairs


class _PinnedRing:
    """Asynchronous upload of a few per-step floats.  A copy from pageable memory makes the host wait for the stream (every step: the GPU
    then idles while the host catches up with the next forward pass); a ring of pinned slots keeps the upload asynchronous.  Each slot
    carries the event of its last upload and is rewritten only after that copy has executed (with HIP-graph replay or an unthrottled
    loop the host can run more than 16 steps ahead of the device; the wait is almost always already satisfied)."""
    SLOTS = 16

    def __init__(self, width):
        self.pinned = torch.empty((self.SLOTS, width), dtype=torch.float32).pin_memory()
        self.events = [None] * self.SLOTS

    def upload(self, dst, values, index):
        i = index % self.SLOTS
        if self.events[i] is not None:
            self.events[i].synchronize()
        slot = self.pinned[i]
        for k, v in enumerate(values):
            slot[k] = v
        dst.copy_(slot, non_blocking=True)
        ev = self.events[i] or torch.cuda.Event()
        ev.record()
        self.events[i] = ev


class FusedFlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: ONE HBM-bound kernel over the flat buffers per step, with everything around it -- the reducer's
    wait and its gradient scale, the gradient sink, the side stream, the weight-pack epoch and prefetch, the device error poll, the three
    per-step scalars in device memory (``hyper``, refreshed by ``advance()`` through a pinned ring, so that the launch is the same every
    step and replays from a HIP graph) and torch's own state-dict layout numbered in the reference's index space.  ``param_groups`` keeps
    torch's scheduler API (StepLR) working.  A subclass names its group defaults (torch's key set for its class) and the group keys a
    loaded file may set (LOAD_KEYS), and gives ``state_buffers`` ([(state-dict key, flat buffer)]), ``_hyper_values``, ``_launch``
    (device scalars), ``_launch_ctl`` (the same with ``ctl``) and ``_host_step`` (host scalars).

    Gradient-norm clipping and the non-finite step guard (``clip_grad_norm`` > 0: torch.nn.utils.clip_grad_norm_'s L2 rule with that
    max_norm; ``skip_nonfinite``: a step whose gradient holds an inf or a NaN changes nothing).  With both off -- the default -- the step
    is the one described above: no buffer, no launch, no entry point is added.  With either on, ``step()`` launches mte_grad_norm_clip
    over the flat gradient (one read-only pass, fp64 sums in a fixed order) and then the ``_ctl_dev`` form of the step, which reads
    ``ctl`` = {clip coefficient, skip flag, gradient norm, skipped steps} from device memory: the gradient buffer is never rescaled, both
    launches are identical every step (HIP-graph replay), and the host learns nothing -- ``grad_stats()`` is the one host read, for
    tests and logging.  Across ranks the norm is taken after the all-reduce has finished, over the summed buffer with gscale = 1/world;
    all-reduce leaves the same bits on every rank, so every rank forms the same ``ctl`` and skips the same steps.
    Deviation from a host-side guard: the host cannot know that a step was skipped, so ``steps`` advances anyway -- Adam's bias
    correction counts skipped steps, and SGD's first-step rule belongs to step 1 whether or not it was skipped; with a weight EMA
    (below) ``ema_updates`` advances on a skipped step too, so the EMA's warm-up ramp counts skipped steps as well.  Neither setting is
    part of ``state_dict()``: they come from the configuration, not from the file.

    Gradient accumulation (``accumulate_grad_batches`` = k > 1): up to k micro-batches share one optimizer step, so that one card runs
    the global batch a recipe was tuned for.  Every micro-batch is the zero_grad -> forward -> backward it always was; for all but the
    last of a group the caller runs forward and backward inside ``no_sync()`` (the reducer drops the ready announcements: no collective)
    and calls ``accumulate()`` in place of ``step()``: ONE mte_grad_accumulate launch adds the flat gradient into a second flat buffer,
    ``FlatParameters.accum`` (+4 B per parameter; the first of a group assigns, so the buffer is never cleared).  ``step()`` with j >= 1
    micro-batches pending folds ``accum`` back into the gradient before anything reads it -- bucket by bucket on the reduction stream
    in front of each bucket's all-reduce when a reducer is active (the all-reduce still overlaps the last micro-batch's backward), else
    in one launch over the whole buffer -- and scales by 1 / (world * (j + 1)).  Summation order: the gradient the step consumes is
    the fp32 sum (((g0 + g1) + ...) + g_j) per element, g_i the i-th micro-batch's gradient, each addition rounded once; it is what
    ``flat.grad`` holds after the step.  The norm launch and the ``_ctl_dev`` step see that sum with that scale: the clip applies to the
    averaged gradient, and an inf or NaN in any micro-batch skips the step.  A group may be shorter than k (an epoch's end).  ``steps``
    advances once per step().  With k = 1 -- the default -- there is no buffer and no launch, and ``step()`` with nothing pending is the
    step described above bit for bit.  Neither the setting nor ``accum`` is part of ``state_dict()``: checkpoints are written where
    no group is open.

    Weight EMA (``ema_decay`` = d in (0, 1)): ``FlatParameters.ema`` (+4 B per parameter, a bit copy of the weights at construction)
    follows the weights by e <- d_t * e + (1 - d_t) * p, ONE mte_ema_update_dev launch (12 B per parameter) on the current stream right
    after the step launch, once per step() and never per accumulate().  For the t-th update d_t = min(d, (1 + t) / (10 + t)) with
    ``ema_warmup`` (early updates forget the random initialisation quickly) and d_t = d without.  The host forms d32 = float32(d_t) and
    omd32 = float32(1 - double(d32)); ``advance()`` uploads both to ``ema_scal`` through a pinned ring of their own (``hyper`` stays three
    floats), so the launch is the same every step and replays from a HIP graph.  The kernel computes two fp32 multiplications and one
    fp32 addition per element, each rounded once (tests/ema_ref.py).  With a ``ctl`` the launch reads its skip flag: a skipped step leaves
    the average's bits alone; the clip coefficient is not the average's business.  As with ``steps``, the host cannot know that a step
    was skipped: ``ema_updates`` advances anyway, so the warm-up schedule counts skipped steps just as Adam's bias correction does.
    ``ema_weights()`` swaps weights and average for validation; ``ema_state()`` / ``load_ema()`` / ``ema_named()`` carry the average to
    and from checkpoints.  None of it is part of ``state_dict()``, which stays torch's layout.  With ema_decay = 0 -- the default --
    there is no buffer, no scalar pair and no launch.

    Per-tensor multipliers (``tensor_scales``: one (lr_mult, wd_mult) per parameter, in the order the parameters were handed to
    FlatParameters).  ``param_groups`` stays ONE group -- the checkpoint layout is torch's, numbered in the reference's index space --
    and the base ``lr`` stays in it, so a scheduler's change reaches every tensor.  Distinct pairs become classes (at most 16);
    ``seg_block_class`` (one byte per aligned 64-element block of the flat buffers) and ``seg_class_scales`` ({lr_mult, wd_mult} per
    class) are uploaded once, and ``step()`` launches the SEG entry point (mte_adamw_step_seg_dev / mte_sgd_step_seg_dev; with ``ctl``
    when clipping or the guard is on, behind the same global norm launch), also for plain Adam without weight decay.  Per class
    lr_c = float32(lr * lr_mult) and wd_c = float32(weight_decay * wd_mult); wd_c = 0 takes the no-decay arithmetic.  The launch is
    static: it replays from a captured graph.  Multipliers and tables are configuration, not ``state_dict()``.  ``None``, or every
    pair (1, 1), is OFF: no table, no attribute, and ``_launch`` / ``_launch_ctl`` are the launches described above.

    ``tensor_stats()``: per-tensor gradient norm, largest finite |g|, count of non-finite gradient elements and weight norm in ONE
    read-only launch (mte_tensor_stats) and one host read, whether or not ``tensor_scales`` is set; never launched by ``step()``.

    Per-step linear learning-rate warm-up (``warmup_steps`` = W > 0, for the classes with HAS_STEP, whose step count comes back from
    a checkpoint): step k (1-based, ``steps`` after counting) uploads lr * warmup_factor(k, W) = lr * min(1, k / W), formed in double,
    as ``hyper[0]``.  ``param_groups[0]['lr']`` is never changed, so StepLR, checkpoints and ``tensor_scales`` (which multiply
    ``hyper[0]`` on the device) compose with it.  W is configuration, not ``state_dict()``.  With W = 0 -- the default -- nothing is
    multiplied: ``hyper`` is formed exactly as it always was."""

    HAS_STEP = False                                        # torch keeps a 'step' entry per tensor (Adam) or none (SGD)
    LEGACY_FLAT = False                                      # reads the flat {'steps', <buffers>} layout of earlier builds (Adam only)
    LOAD_KEYS = ('lr', 'initial_lr')

    def __init__(self, flat, defaults, reducer=None, name='Depth', clip_grad_norm=0.0, skip_nonfinite=False, accumulate_grad_batches=1,
                 ema_decay=0.0, ema_warmup=True, tensor_scales=None, warmup_steps=0):
        if int(warmup_steps) != warmup_steps or int(warmup_steps) < 0:
            raise ValueError("Invalid warmup_steps value: {} (an integer >= 0; 0 = off)".format(warmup_steps))
        if int(warmup_steps) > 0 and not self.HAS_STEP:
            raise ValueError("warmup_steps > 0 needs an optimizer whose step count is part of its checkpoint (Adam, AdamW, LAMB): {} keeps "
                             "no step entry, so a resumed run could not know where in the warm-up it stands".format(type(self).__name__))
        self.warmup_steps = int(warmup_steps)
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("Invalid ema_decay value: {} (in [0, 1); 0 = off)".format(ema_decay))
        if tensor_scales is not None:
            tensor_scales = [(float(a), float(b)) for a, b in tensor_scales]
            if len(tensor_scales) != len(flat.natural_params):
                raise ValueError("tensor_scales holds {} pairs for {} trained tensors".format(len(tensor_scales), len(flat.natural_params)))
            classes, class_of = tensor_scale_classes(tensor_scales)
            if classes != [(1.0, 1.0)]:
                # only then: the default optimizer has no tables, none of these attributes and no SEG launch
                dev = flat.flat.device
                self.tensor_scales = tensor_scales
                self.seg_classes = classes
                self.seg_block_class = flat.block_classes(class_of, device=dev)
                self.seg_class_scales = torch.tensor([x for pair in classes for x in pair], dtype=torch.float32, device=dev)
        self._last_gscale = 1.0                               # the last step's gradient scale, for tensor_stats()
        if not float(clip_grad_norm) >= 0.0:
            raise ValueError("Invalid clip_grad_norm value: {} (0 = off)".format(clip_grad_norm))
        if int(accumulate_grad_batches) != accumulate_grad_batches or int(accumulate_grad_batches) < 1:
            raise ValueError("Invalid accumulate_grad_batches value: {} (an integer >= 1; 1 = off)".format(accumulate_grad_batches))
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self._pending = 0                                     # micro-batches of the open group that wait in flat.accum
        if self.accumulate_grad_batches > 1:
            flat.enable_accumulation()                        # only then: the default optimizer has no second gradient buffer
        self.clip_grad_norm, self.skip_nonfinite = float(clip_grad_norm), bool(skip_nonfinite)
        self.flatp = flat
        self.reducer = reducer
        super().__init__([{'params': flat.params, 'name': name}], defaults)
        self._group_keys = tuple(defaults)
        self.steps = 0
        self.hyper = torch.zeros(3, dtype=torch.float32, device=flat.flat.device)    # read by the kernel (see _hyper_values)
        self._hyper_ring = None
        if self.clip_grad_norm > 0.0 or self.skip_nonfinite:
            # only then: the default optimizer has no `ctl` attribute, no work buffer and no norm launch
            self.ctl = torch.zeros(4, dtype=torch.float32, device=flat.flat.device)
            self._norm_work = None                            # the norm launch's records and ticket: zeroed ONCE, here
            if flat.flat.is_cuda:
                from .. import kernels as K
                self._norm_work = K.grad_norm_work(flat.grad.numel(), flat.flat.device)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.ema_updates = 0                                  # updates of the average so far (t of the decay schedule)
        if self.ema_decay > 0.0:
            # only then: the default optimizer has no average, no `ema_scal` and no EMA launch
            flat.enable_ema()
            self.ema_scal = torch.zeros(2, dtype=torch.float32, device=flat.flat.device)     # {d32, omd32}, read by the kernel
            self._ema_ring = None

    def grad_stats(self):
        """{'grad_norm', 'clip_coef', 'skipped', 'skipped_steps'} of the last step as Python numbers: ONE host read (it waits for the
        device), for tests and logging"""
        c = self.ctl.tolist()
        return {'grad_norm': c[2], 'clip_coef': c[0], 'skipped': bool(c[1]), 'skipped_steps': int(c[3])}

    @torch.no_grad()
    def tensor_stats(self, with_weights=True):
        """One dict per trained tensor, in the order of the reference's numbering (set_index_space; positional names without it):
        {'name', 'numel', 'grad_norm' (|gscale| * sqrt(sum g^2) with the last step's gscale), 'grad_amax' (largest finite |g|, unscaled),
        'nonfinite' (inf / NaN elements of the gradient), 'weight_norm' (0.0 without ``with_weights``), 'lr_scale',
        'weight_decay_scale', 'grad_sq_sum' (the unscaled fp64 sum g^2)}.  ONE read-only launch over ``flat.grad`` as it stands (mte_tensor_stats; fp64 sums in an order the layout
        fixes) and ONE host read.  Call it after step() and before zero_grad(): the steps never rescale the gradient buffer, so it
        still holds the step's gradient (with accumulation, the group's sum)."""
        import math
        from .. import kernels as K
        flat = self.flatp
        K._require_gpu(flat.grad)
        segs = flat.segments()
        if getattr(self, '_stats_tables', None) is None:
            dev = flat.grad.device
            work = torch.zeros((int(K.lib.mte_tensor_stats_work_bytes(flat.total, len(segs))) + 7) // 8, dtype=torch.float64, device=dev)
            self._stats_tables = flat.segments(device=dev) + (work, torch.zeros(4 * len(segs), dtype=torch.float64, device=dev))
        begins, numels, work, out = self._stats_tables
        K.lib.mte_tensor_stats(flat.grad.data_ptr(), flat.flat.data_ptr() if with_weights else None, flat.total, begins.data_ptr(),
                               numels.data_ptr(), len(segs), work.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rows = out.view(-1, 4).tolist()                       # the one host read
        row_of = {id(p): r for p, r in zip(flat.params, rows)}
        slot_of = {id(p): i for i, p in enumerate(flat.natural_params)}
        scales = getattr(self, 'tensor_scales', None)
        res = []
        for pos, (name, p, _) in enumerate(self._space()):
            if p is None:
                continue
            sg, amax, nf, sp = row_of[id(p)]
            lm, wm = scales[slot_of[id(p)]] if scales is not None else (1.0, 1.0)
            res.append({'name': name if name is not None else str(pos), 'numel': p.numel(), 'grad_norm': abs(self._last_gscale) * math.sqrt(sg),
                        'grad_amax': amax, 'nonfinite': int(nf), 'weight_norm': math.sqrt(sp), 'lr_scale': lm, 'weight_decay_scale': wm,
                        'grad_sq_sum': sg})                   # the unscaled fp64 sum of squares as the launch left it
        return res

    def _norm_clip(self, K, gscale, stream):
        """ctl <- the clip coefficient / skip flag of the gradient as it stands (reduced and complete)"""
        K.grad_norm_clip_flat(self.flatp.grad, self._norm_work, self.ctl, gscale, self.clip_grad_norm if self.clip_grad_norm > 0.0 else float('inf'),
                              self.skip_nonfinite, stream)

    def zero_grad(self, set_to_none=False):
        self.flatp.zero_grad()

    @contextlib.contextmanager
    def no_sync(self):
        """``with optimizer.no_sync():`` around the forward and backward of a micro-batch that is not the last of its accumulation
        group: the reducer drops the ready announcements, so it counts nothing and launches no collective (without a reducer the
        block changes nothing)"""
        red = self.reducer
        prev = red is not None and red.sync
        if red is not None:
            red.sync = False
        try:
            yield
        finally:
            if red is not None:
                red.sync = prev

    @torch.no_grad()
    def accumulate(self):
        """In place of step() for a micro-batch that is not the last of its group: accum <- grad (the group's first) or accum + grad,
        one launch on the current stream.  No step is counted, no weight moves, the weights epoch and the device error word are left
        alone."""
        from .. import kernels as K
        k, flat, red = self.accumulate_grad_batches, self.flatp, self.reducer
        if k == 1:
            raise RuntimeError("accumulate() needs an optimizer built with accumulate_grad_batches > 1")
        if self._pending >= k - 1:
            raise RuntimeError("{} micro-batches are already accumulated: the {}-th of a group of accumulate_grad_batches = {} "
                               "ends in step()".format(self._pending, k, k))
        if red is not None and (red.launch_log or red._works):
            raise RuntimeError("the gradient all-reduce launched a collective during this micro-batch's backward: run the forward and "
                               "backward of a micro-batch that ends in accumulate() inside optimizer.no_sync()")
        if flat.grad.is_cuda:
            K.join_side_stream()                              # weight gradients arrive on the side queue
        if flat.sink is not None:
            flat.sink.end_step()
        if flat.grad.is_cuda:
            K.grad_accumulate_flat(flat.accum, flat.grad, assign=self._pending == 0)
        elif self._pending == 0:                              # host buffers (the gloo CPU tests), as BucketedAllReduce._launch
            flat.accum.copy_(flat.grad)
        else:
            flat.accum.add_(flat.grad)
        self._pending += 1
        if red is not None and red.active:
            red.fold_pending(flat.accum)                      # the next backward's buckets take accum before they are reduced

    @torch.no_grad()
    def step(self, closure=None):
        from .. import kernels as K
        if self.flatp.grad.is_cuda:
            K.join_side_stream()
        gscale = self.reducer.finish() if self.reducer is not None else 1.0
        if self._pending:
            if self.reducer is None or not self.reducer.active:
                K.grad_accumulate_flat(self.flatp.grad, self.flatp.accum, assign=False)      # (an active reducer folded bucket by bucket)
            gscale = 1.0 / ((self.reducer.world if self.reducer is not None else 1) * (self._pending + 1))
            self._pending = 0
        if self.flatp.sink is not None:
            self.flatp.sink.end_step()                       # (a forward pass's gradient-sink suspension lasts until its gradients are consumed)
        g = self.param_groups[0]
        if self.flatp.grad.is_cuda:
            # step count and learning rate reach the kernel through device memory, so the launch is identical every step (HIP-graph
            # replay); under capture the host side of the step (advance) is the replaying caller's job
            if not torch.cuda.is_current_stream_capturing():
                self.advance()
            stream = torch.cuda.current_stream().cuda_stream
            self._last_gscale = float(gscale)
            ctl = getattr(self, 'ctl', None)
            if ctl is not None:
                self._norm_clip(K, float(gscale), stream)
            if getattr(self, 'seg_block_class', None) is not None:
                self._launch_seg(K, g, float(gscale), (self.seg_block_class.data_ptr(), self.seg_class_scales.data_ptr(), len(self.seg_classes),
                                                       None if ctl is None else ctl.data_ptr()), stream)
            elif ctl is None:
                self._launch(K, g, float(gscale), stream)
            else:
                self._launch_ctl(K, g, float(gscale), stream)
            if self.ema_decay > 0.0:                         # the average follows the weights the step just wrote (or, skipped, left alone)
                K.ema_update_flat(self.flatp.ema, self.flatp.flat, self.ema_scal, getattr(self, 'ctl', None), stream)
            K.bump_weights_epoch()
        else:
            self.steps += 1
            self._last_gscale = float(gscale)
            if self.warmup_steps > 0:                        # the warm-up reaches the host-scalar entry points through a copy of the group
                g = dict(g, lr=float(g['lr']) * warmup_factor(self.steps, self.warmup_steps))
            self._host_step(K, g, gscale)                  # no CPU form: raises MteError on host buffers
        if self.flatp.grad.is_cuda:
            K.prefetch_weight_packs()                       # next step's kernel-ready weight packs, off the critical path
            if not torch.cuda.is_current_stream_capturing():
                K.check_device_errors()                     # a bounded inter-workgroup wait gave up somewhere: fail the step (one host-memory read)

    def advance(self):
        """Host side of one step: count it and hand the kernel its per-step scalars (same double-precision arithmetic as the
        host-scalar entry point) -- called by step(), or by a graph-replaying caller right before each replay."""
        self.steps += 1
        vals = self._hyper_values(self.param_groups[0])
        if self.warmup_steps > 0:                            # only then: without a warm-up nothing is multiplied
            vals[0] = vals[0] * warmup_factor(self.steps, self.warmup_steps)
        if self.hyper.is_cuda and not os.environ.get("MTE_ADAM_PAGEABLE_HYPER"):
            if self._hyper_ring is None:
                self._hyper_ring = _PinnedRing(3)
            self._hyper_ring.upload(self.hyper, vals, self.steps)
        else:
            self.hyper.copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=True)
        if self.ema_decay > 0.0:
            self.ema_updates += 1
            pair = ema_decay_pair(self.ema_updates, self.ema_decay, self.ema_warmup)
            if self.ema_scal.is_cuda:
                if self._ema_ring is None:
                    self._ema_ring = _PinnedRing(2)
                self._ema_ring.upload(self.ema_scal, pair, self.ema_updates)
            else:
                self.ema_scal.copy_(torch.tensor(pair, dtype=torch.float32))

    def _swap_ema(self):
        """flat <-> ema behind every queued reader of the parameters, then packs for the new weights"""
        from .. import kernels as K
        flat = self.flatp
        if flat.flat.is_cuda:
            K.join_side_stream()
            cur = torch.cuda.current_stream()
            for st in K._side["streams"]:                     # the weight-pack launches of prefetch_weight_packs() (see ema_weights)
                cur.wait_stream(st)
            K.flat_swap(flat.flat, flat.ema)
            K.bump_weights_epoch()
            K.prefetch_weight_packs()
        else:                                                 # host buffers: no kernel, the same exchange
            held = flat.flat.clone()
            flat.flat.copy_(flat.ema)
            flat.ema.copy_(held)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights():`` -- inside the block every trained tensor holds the AVERAGE (validation, top-k ranking,
        inference) and ``flat.ema`` holds the raw weights; on exit both are back bit for bit.  One mte_flat_swap launch each way: no
        second network, no temporary buffer, no host read.

        Ordering.  prefetch_weight_packs() queues pack launches on the side stream that READ the parameters.  ``join_side_stream()``
        waits only while the weight-gradient launches have marked the side streams dirty (``_side["dirty"]``); the prefetch does
        not set that mark, so the join alone does not cover it.  The current stream is therefore made to wait for every stream in
        ``_side["streams"]`` itself (``wait_stream``) before the swap launch -- on entry and again on exit, where the packs that the
        block's own prefetch queued read the average.  Then the weights epoch is bumped and the packs are prefetched from the
        swapped-in weights, as after a step.

        Raises RuntimeError with an accumulation group open (the gradients in ``accum`` belong to the raw weights) and under stream
        capture (the swap is not part of a training step's graph)."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("ema_weights() needs an optimizer built with ema_decay > 0")
        if self._pending > 0:
            raise RuntimeError("ema_weights() with an accumulation group open ({} micro-batches pending): step() first".format(self._pending))
        if self.flatp.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ema_weights() under stream capture: the swap is not part of a captured step")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def ema_state(self):
        """what a checkpoint keeps of the average beside its tensors"""
        return {'decay': self.ema_decay, 'warmup': self.ema_warmup, 'num_updates': self.ema_updates}

    def ema_named(self):
        """{id(parameter): the average of that tensor, a view into ``flat.ema``} for every trained tensor"""
        flat = self.flatp
        return {id(p): flat.ema[o:o + p.numel()].view(p.shape) for p, o in zip(flat.params, flat.offsets)}

    @torch.no_grad()
    def load_ema(self, named_tensors, num_updates):
        """Fill ``flat.ema`` from {reference parameter name: tensor} through the index space of set_index_space and set the update
        count.  A trained tensor the dictionary does not name keeps what the average holds (the weights it was built from)."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("load_ema() needs an optimizer built with ema_decay > 0")
        for name, p, o in self._space():
            if p is None or name is None or name not in named_tensors:
                continue
            t = named_tensors[name]
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError("averaged tensor {} has shape {}, parameter has {}".format(name, tuple(t.shape), tuple(p.shape)))
            self.flatp.ema[o:o + p.numel()].copy_(t.reshape(-1))
        self.ema_updates = int(num_updates)

    def set_index_space(self, names, local_names):
        """Number the optimizer state like the reference's ``torch.optim.<name>(depth_net.parameters())`` does.

        names: every parameter name of the reference network in ``depth_net.parameters()`` order -- frozen tensors and the
        sparse-branch (``mconvs.*``) tensors included, whether or not this build materialises them (reference
        models/model_wrapper.py:149-154 passes ALL of depth_net.parameters()).  local_names: {name: parameter} of the
        tensors that live in the flat buffers.  Without it the state is numbered by position in the flat parameter list."""
        self._index_names = list(names)
        self._local = {n: p for n, p in local_names.items() if id(p) in self.flatp.offset_of}

    def _space(self):
        """[(index-space name or None, parameter or None, flat offset)] in the reference's numbering."""
        if getattr(self, '_index_names', None) is None:
            return [(None, p, self.flatp.offset_of[id(p)]) for p in self.flatp.natural_params]
        out = []
        for n in self._index_names:
            p = self._local.get(n)
            out.append((n, p, self.flatp.offset_of[id(p)] if p is not None else -1))
        return out

    def state_dict(self):
        """The layout of the matching torch class ({'state': {i: {...}}, 'param_groups': [...]}: Adam / AdamW 'step', 'exp_avg',
        'exp_avg_sq'; SGD 'momentum_buffer').  Indices are
        positions in the reference's ``depth_net.parameters()`` (see set_index_space): 'params' has one entry per reference
        parameter, state entries exist for the tensors this build trains -- exactly what the reference's own optimizer holds, since
        its sparse-branch tensors never receive a gradient on the RGB-only path and so never get state either
        (models/model_checkpoint.py:71-81 stores optimizer.state_dict())."""
        space = self._space()
        state = {}
        bufs = self.state_buffers()
        if self.steps > 0 and bufs:
            for i, (_, p, o) in enumerate(space):
                if p is None:
                    continue
                n = p.numel()
                state[i] = {'step': torch.tensor(float(self.steps))} if self.HAS_STEP else {}
                for key, b in bufs:
                    state[i][key] = b[o:o + n].view(p.shape).clone()
        g = self.param_groups[0]
        group = {k: (tuple(g[k]) if k == 'betas' else g[k]) for k in self._group_keys}
        group.update({'name': g.get('name', 'Depth'), 'params': list(range(len(space)))})
        for k in ('initial_lr',):
            if k in g:
                group[k] = g[k]
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        # the file's hyper-parameters win, as in torch (amsgrad / maximize are not built and stay off); first, since SGD's momentum
        # decides whether a momentum buffer exists
        for g, s_ in zip(self.param_groups, sd.get('param_groups', ())):
            g.update({k: v for k, v in s_.items() if k in self.LOAD_KEYS})
        bufs = self.state_buffers()
        if 'state' not in sd:
            # flat layout written by earlier builds of this package: they had Adam only (a file without 'param_groups' loads too)
            if not self.LEGACY_FLAT:
                raise ValueError("{} reads torch's optimizer layout only ({{'state', 'param_groups'}}); got keys {}".format(
                    type(self).__name__, sorted(sd)))
            self.steps = sd['steps']
            for key, b in bufs:
                b.copy_(sd[key])
        else:
            space = self._space()
            groups = sd['param_groups']
            idx = [i for g in groups if g.get('name', 'Depth') == 'Depth' for i in g['params']] or list(groups[0]['params'])
            if len(idx) != len(space):
                # a dictionary numbered over the trainable tensors only (earlier builds of this package)
                trainable = [(n, p, o) for n, p, o in space if p is not None]
                if len(idx) != len(trainable):
                    raise ValueError("optimizer state holds {} 'Depth' parameters; this network numbers {} ({} of them trained here)"
                                     .format(len(idx), len(space), len(trainable)))
                space = trainable
            for _, b in bufs:
                b.zero_()
            steps = 0
            for i, (name, p, o) in zip(idx, space):
                st = sd['state'].get(i)
                if st is None or p is None or not bufs:         # no state yet / a tensor this build does not hold (mconvs.*)
                    continue
                if any(st.get(key) is None for key, _ in bufs):
                    continue                                    # torch's SGD writes momentum_buffer: None before a tensor's first gradient
                n = p.numel()
                for key, b in bufs:
                    if tuple(st[key].shape) != tuple(p.shape):
                        raise ValueError("optimizer state {} ({}) has shape {}, parameter has {}".format(
                            i, name, tuple(st[key].shape), tuple(p.shape)))
                    b[o:o + n].copy_(st[key].reshape(-1))
                # torch keeps a step per tensor (Adam; they advance together here) or none (SGD: a buffer means "past the first step")
                steps = max(steps, int(float(st['step'])) if self.HAS_STEP else 1)
            self.steps = steps


class FusedAdam(FusedFlatOptimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) -- or torch.optim.AdamW with ``decoupled_weight_decay=True`` -- as ONE HBM-bound
    kernel over the flat buffers (28 B/parameter: read p,g,m,v; write p,m,v).  Without weight decay the launch is mte_adam_step_dev;
    with it, mte_adamw_step_dev, which forms lr * weight_decay on the device from the step's own learning rate.

    The step runs over EVERY element of the flat buffers.  torch skips a parameter whose ``.grad`` is None in a step: neither decay nor
    moment update.  Here such a tensor has a zero gradient instead, so with a weight decay it still decays (and its moments decay
    towards zero, as they always did) -- the SAN fusion scalars on the RGB-only path are the one case in this network."""

    HAS_STEP = True
    LEGACY_FLAT = True
    LOAD_KEYS = ('lr', 'betas', 'eps', 'initial_lr', 'weight_decay', 'decoupled_weight_decay')

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, reducer=None, name='Depth', weight_decay=0.0,
                 decoupled_weight_decay=False, clip_grad_norm=0.0, skip_nonfinite=False, accumulate_grad_batches=1, ema_decay=0.0,
                 ema_warmup=True, tensor_scales=None, warmup_steps=0):
        if not 0.0 <= float(weight_decay):
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        super().__init__(flat, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                    capturable=False, differentiable=False, fused=None,
                                    decoupled_weight_decay=bool(decoupled_weight_decay)), reducer=reducer, name=name,
                         clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite, accumulate_grad_batches=accumulate_grad_batches,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, tensor_scales=tensor_scales, warmup_steps=warmup_steps)
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)

    def state_buffers(self):
        return [('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)]

    def _hyper_values(self, g):
        """lr, 1 - b1^t, sqrt(1 - b2^t)"""
        import math
        b1, b2 = g['betas']
        return [float(g['lr']), 1.0 - math.pow(float(b1), self.steps), math.sqrt(1.0 - math.pow(float(b2), self.steps))]

    def _bufs(self, g):
        return (self.flatp.flat.data_ptr(), self.flatp.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.flatp.flat.numel(), self.hyper.data_ptr(), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']))

    def _launch_ctl(self, K, g, gscale, stream):
        """clipped / guarded: weight_decay = 0 is adamw_kernel's WD_NONE instance, the Adam step operation for operation"""
        K.lib.mte_adamw_step_ctl_dev(*self._bufs(g), float(g['weight_decay']), int(bool(g['decoupled_weight_decay'])), gscale,
                                     self.ctl.data_ptr(), stream)

    def _launch_seg(self, K, g, gscale, tables, stream):
        """per-tensor multipliers: tables = (block classes, class scales, classes, ctl or None); also without a weight decay, where the
        learning-rate multipliers still act"""
        K.lib.mte_adamw_step_seg_dev(*self._bufs(g), float(g['weight_decay']), int(bool(g['decoupled_weight_decay'])), gscale, *tables, stream)

    def _launch(self, K, g, gscale, stream):
        wd = float(g['weight_decay'])
        bufs = self._bufs(g)
        if wd == 0.0:
            K.lib.mte_adam_step_dev(*bufs, gscale, stream)
        else:
            K.lib.mte_adamw_step_dev(*bufs, wd, int(bool(g['decoupled_weight_decay'])), gscale, stream)

    def _host_step(self, K, g, gscale):
        if float(g['weight_decay']) == 0.0:
            K.adam_step_flat(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq, self.steps, lr=g['lr'],
                             betas=g['betas'], eps=g['eps'], gscale=gscale)
        else:
            K.adamw_step_flat(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq, self.steps, lr=g['lr'], betas=g['betas'],
                              eps=g['eps'], weight_decay=g['weight_decay'], decoupled=g['decoupled_weight_decay'], gscale=gscale)


class FusedLAMB(FusedFlatOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning"): AdamW whose per-tensor update is rescaled by the trust ratio
    ||w|| / ||update||, as TWO HBM-bound launches over the flat buffers with no scratch buffer -- mte_lamb_moments (24 B/parameter: read
    p, g, m, v; write m, v; the per-tensor fp64 sums of p^2 and of the squared delta in a fixed order; ``trust``) and mte_lamb_apply
    (16 B/parameter: read p, m, v; write p).  Per element the arithmetic is the decoupled AdamW step's, and a tensor with trust ratio 1 --
    every excluded tensor -- gets mte_adamw_step_dev's result bit for bit (tests/lamb_ref.py states the step in float64).

    The group is torch.optim.AdamW's key set with ``decoupled_weight_decay=True``: the checkpoint layout, the reference's index space,
    StepLR and ``load_state_dict`` are AdamW's, and an AdamW checkpoint warm-starts LAMB (``exp_avg``, ``exp_avg_sq``, ``step``).
    ``adapt``: one bool per trained tensor in ``natural_params`` order (default: all True); False = plain AdamW arithmetic for that tensor
    (biases and normalisation affine tensors, by the usual practice: model.optimizer.lamb_exclude).  ``max_trust`` > 0 caps the ratio.
    ``tensor_scales`` pairs go into the per-tensor table {lr_mult, wd_mult, adapt} in device memory: the SEG block-class tables are never
    built for this class and there is no 16-class limit.  All three are configuration, not ``state_dict()``.

    ``step()`` launches the pair on the current stream, behind the norm launch when clipping or the guard is on (both launches read
    ``ctl``: the clip coefficient scales the gradient, a skipped step changes nothing).  Accumulation, the weight EMA, ``no_sync``,
    ``advance()``, the pinned ``hyper`` ring, the weights epoch and the error poll are FusedFlatOptimizer's, unchanged; both launches are
    the same every step and replay from a HIP graph.  Run it with ``warmup_steps`` (see FusedFlatOptimizer).

    Across ranks the sums are taken after the all-reduce has finished, over the summed gradient buffer (with gscale = 1/world) and the
    weights; the all-reduce leaves the same bits on every rank and the sums have one order, so every rank forms the same ``trust`` and
    the weights stay bit-equal across ranks.

    ``trust_ratios()`` reports the last step's ratios (one host read; never called by ``step()``)."""

    HAS_STEP = True
    LOAD_KEYS = ('lr', 'betas', 'eps', 'initial_lr', 'weight_decay')

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, reducer=None, name='Depth', adapt=None, max_trust=0.0,
                 clip_grad_norm=0.0, skip_nonfinite=False, accumulate_grad_batches=1, ema_decay=0.0, ema_warmup=True, tensor_scales=None,
                 warmup_steps=0):
        import math
        if not 0.0 <= float(weight_decay):
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if not float(max_trust) >= 0.0:
            raise ValueError("Invalid max_trust value: {} (0 = no cap)".format(max_trust))
        n_t = len(flat.natural_params)
        adapt = [True] * n_t if adapt is None else [bool(a) for a in adapt]
        scales = [(1.0, 1.0)] * n_t if tensor_scales is None else [(float(a), float(b)) for a, b in tensor_scales]
        if len(adapt) != n_t or len(scales) != n_t:
            raise ValueError("adapt / tensor_scales hold {} / {} entries for {} trained tensors".format(len(adapt), len(scales), n_t))
        for i, pair in enumerate(scales):
            if not all(math.isfinite(x) and x >= 0.0 for x in pair):
                raise ValueError("Invalid tensor_scales pair {} for tensor {}: multipliers are finite and >= 0".format(pair, i))
        # tensor_scales never reaches the base class: no SEG tables, no class limit
        super().__init__(flat, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                    capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True), reducer=reducer,
                         name=name, clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite,
                         accumulate_grad_batches=accumulate_grad_batches, ema_decay=ema_decay, ema_warmup=ema_warmup, tensor_scales=None,
                         warmup_steps=warmup_steps)
        self.adapt, self.max_trust, self.lamb_scales = adapt, float(max_trust), scales
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self._lamb_tables = None                             # device tables and work buffer: made at the first launch, then kept

    def state_buffers(self):
        return [('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)]

    def _hyper_values(self, g):
        """Adam's: lr, 1 - b1^t, sqrt(1 - b2^t); the step's own learning rate (warm-up included) is kept for trust_ratios()"""
        vals = FusedAdam._hyper_values(self, g)
        self._step_lr = vals[0] * warmup_factor(self.steps, self.warmup_steps)
        return vals

    def _tables(self, K):
        """(begins, numels, {lr_mult, wd_mult, adapt} per tensor, work, trust, sums) in FLAT order on the device; ``trust`` (T floats) and
        ``sums`` (2 T doubles) are views of ONE buffer, so that trust_ratios() is one host read"""
        if self._lamb_tables is None:
            flat = self.flatp
            dev = flat.flat.device
            segs = flat.segments()
            T = len(segs)
            begins, numels = flat.segments(device=dev)
            table = torch.tensor([x for _, _, slot in segs for x in (self.lamb_scales[slot][0], self.lamb_scales[slot][1],
                                                                      1.0 if self.adapt[slot] else 0.0)], dtype=torch.float32, device=dev)
            work = torch.zeros((int(K.lib.mte_lamb_work_bytes(flat.total, T)) + 7) // 8, dtype=torch.float64, device=dev)   # zeroed ONCE
            out = torch.zeros(2 * T + (T + 1) // 2, dtype=torch.float64, device=dev)
            self._lamb_out = out
            self._lamb_tables = (begins, numels, table, work, out[2 * T:].view(torch.float32)[:T], out[:2 * T])
        return self._lamb_tables

    def _pair(self, K, g, gscale, ctl, stream):
        K._require_gpu(self.flatp.flat)
        begins, numels, table, work, trust, sums = self._tables(K)
        flat, T = self.flatp, len(self.flatp.params)
        b1, b2 = float(g['betas'][0]), float(g['betas'][1])
        eps, wd = float(g['eps']), float(g['weight_decay'])
        K.lib.mte_lamb_moments(flat.flat.data_ptr(), flat.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), flat.total,
                               self.hyper.data_ptr(), b1, b2, eps, wd, gscale, self.max_trust, begins.data_ptr(), numels.data_ptr(),
                               table.data_ptr(), T, work.data_ptr(), trust.data_ptr(), sums.data_ptr(), ctl, stream)
        K.lib.mte_lamb_apply(flat.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), flat.total, self.hyper.data_ptr(), eps,
                             wd, begins.data_ptr(), numels.data_ptr(), table.data_ptr(), T, trust.data_ptr(), ctl, stream)

    def _launch(self, K, g, gscale, stream):
        self._pair(K, g, gscale, None, stream)

    def _launch_ctl(self, K, g, gscale, stream):
        self._pair(K, g, gscale, self.ctl.data_ptr(), stream)

    def _host_step(self, K, g, gscale):
        """no CPU form of the step: MteError on host buffers, as the siblings"""
        self._pair(K, g, gscale, None, None)

    @torch.no_grad()
    def trust_ratios(self):
        """One dict per trained tensor, in the order of the reference's numbering (set_index_space; positional names without it):
        {'name', 'trust_ratio' (q_t as the last step applied it), 'weight_norm' (sqrt(S_p), the weights BEFORE that step), 'update_norm'
        (sqrt(S_d) / lr_t: the norm of the paper's update direction; 0.0 where lr_t is 0), 'adapted'}.  ONE host read of what the
        last step's mte_lamb_moments launch left; no launch.  Before the first step every ratio reads 0."""
        import math
        import numpy as np
        from .. import kernels as K
        K._require_gpu(self.flatp.flat)
        self._tables(K)
        T = len(self.flatp.params)
        host = self._lamb_out.cpu()                           # the one host read
        sums, trust = host[:2 * T].view(-1, 2).tolist(), host[2 * T:].view(torch.float32)[:T].tolist()
        row_of = {id(p): (q, sp, sd) for p, q, (sp, sd) in zip(self.flatp.params, trust, sums)}
        slot_of = {id(p): i for i, p in enumerate(self.flatp.natural_params)}
        lr = float(np.float32(getattr(self, '_step_lr', 0.0)))       # hyper[0] of the last step
        res = []
        for pos, (name, p, _) in enumerate(self._space()):
            if p is None:
                continue
            q, sp, sd = row_of[id(p)]
            slot = slot_of[id(p)]
            lr_t = float(np.float32(lr) * np.float32(self.lamb_scales[slot][0]))
            res.append({'name': name if name is not None else str(pos), 'trust_ratio': q, 'weight_norm': math.sqrt(sp) if sp >= 0 else sp,
                        'update_norm': (math.sqrt(sd) if sd >= 0 else sd) / lr_t if lr_t > 0.0 else 0.0, 'adapted': bool(self.adapt[slot])})
        return res


class FusedSGD(FusedFlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) as ONE HBM-bound kernel over the flat buffers: 20 B/parameter
    with momentum (read p,g,buf; write p,buf), 12 B without (no buffer exists then).  torch's first-step rule (buf = g') reaches the
    kernel as the effective coefficients {lr, 0, 1} in ``hyper`` at step 1 and {lr, momentum, 1 - dampening} afterwards.

    As with FusedAdam the step covers every element: a tensor without a gradient in a step (torch skips it) sees a zero gradient here, so
    a weight decay still applies to it and its momentum buffer still decays."""

    LOAD_KEYS = ('lr', 'initial_lr', 'momentum', 'dampening', 'weight_decay', 'nesterov')

    def __init__(self, flat, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, reducer=None, name='Depth',
                 clip_grad_norm=0.0, skip_nonfinite=False, accumulate_grad_batches=1, ema_decay=0.0, ema_warmup=True, tensor_scales=None,
                 warmup_steps=0):
        if float(lr) < 0.0 or float(momentum) < 0.0 or float(weight_decay) < 0.0:
            raise ValueError("Invalid lr / momentum / weight_decay: {} / {} / {}".format(lr, momentum, weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(flat, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                                    maximize=False, foreach=None, differentiable=False, fused=None), reducer=reducer, name=name,
                         clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite, accumulate_grad_batches=accumulate_grad_batches,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, tensor_scales=tensor_scales, warmup_steps=warmup_steps)
        self.momentum_buffer = None
        self.state_buffers()

    def state_buffers(self):
        """the momentum buffer, allocated (zero) when the group first asks for momentum -- at construction or when a loaded file does"""
        if float(self.param_groups[0]['momentum']) == 0.0:
            return []
        if self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.flatp.flat)
        return [('momentum_buffer', self.momentum_buffer)]

    def _hyper_values(self, g):
        """lr, mu_eff, (1 - dampening)_eff"""
        import struct
        first = self.steps <= 1
        damp = struct.unpack('f', struct.pack('f', float(g['dampening'])))[0]     # from the float32 dampening, as mte_sgd_step forms it
        return [float(g['lr']), 0.0 if first else float(g['momentum']), 1.0 if first else 1.0 - damp]

    def _buf_ptr(self):
        bufs = self.state_buffers()
        return bufs[0][1].data_ptr() if bufs else None

    def _launch(self, K, g, gscale, stream):
        K.lib.mte_sgd_step_dev(self.flatp.flat.data_ptr(), self.flatp.grad.data_ptr(), self._buf_ptr(), self.flatp.flat.numel(),
                               self.hyper.data_ptr(), float(g['momentum']), float(g['weight_decay']), int(bool(g['nesterov'])), gscale, stream)

    def _launch_seg(self, K, g, gscale, tables, stream):
        """per-tensor multipliers: tables = (block classes, class scales, classes, ctl or None)"""
        K.lib.mte_sgd_step_seg_dev(self.flatp.flat.data_ptr(), self.flatp.grad.data_ptr(), self._buf_ptr(), self.flatp.flat.numel(),
                                   self.hyper.data_ptr(), float(g['momentum']), float(g['weight_decay']), int(bool(g['nesterov'])), gscale,
                                   *tables, stream)

    def _launch_ctl(self, K, g, gscale, stream):
        K.lib.mte_sgd_step_ctl_dev(self.flatp.flat.data_ptr(), self.flatp.grad.data_ptr(), self._buf_ptr(), self.flatp.flat.numel(),
                                   self.hyper.data_ptr(), float(g['momentum']), float(g['weight_decay']), int(bool(g['nesterov'])), gscale,
                                   self.ctl.data_ptr(), stream)

    def _host_step(self, K, g, gscale):
        bufs = self.state_buffers()
        K.sgd_step_flat(self.flatp.flat, self.flatp.grad, bufs[0][1] if bufs else None, self.steps, lr=g['lr'], momentum=g['momentum'],
                        dampening=g['dampening'], weight_decay=g['weight_decay'], nesterov=g['nesterov'], gscale=gscale)


def reference_parameter_names(depth_net):
    """Parameter names of the REFERENCE PackNetSAN01 in ``parameters()`` order.  torch yields a module's OWN parameters before
    those of its sub-modules, so the fusion vectors registered last in the constructor (networks/depth/PackNetSAN01.py:209-210)
    come first: ``weight, bias, encoder.*, decoder.*, mconvs.*``.  A network built without the sparse branch gets the branch's
    names from a meta-device instance (no memory) appended where the reference has them -- at the end -- so optimizer indices
    agree with checkpoints written by the reference and between ``with_san=True`` / ``False`` builds of this package."""
    names = [n for n, _ in depth_net.named_parameters()]
    if getattr(depth_net, 'with_san', True) or not hasattr(depth_net, 'mconvs'):
        return names
    with torch.device('meta'):
        from ..networks.layers.minkowski_encoder import MinkowskiEncoder
        branch = ['mconvs.' + n for n, _ in MinkowskiEncoder([32, 64, 128, 256, 512], with_uncertainty=False).named_parameters()]
    return names + branch


def broadcast_parameters(flat, src=0, group=None):
    """Rank-0 weights to every rank (Horovod's broadcast_parameters equivalent) -- one message."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.broadcast(flat.flat, src=src, group=group)
