"""GPU (-m gpu): gradient accumulation over micro-batches -- mte_grad_accumulate (csrc/optim.hip) bit for bit against ``a + b`` in NumPy
float32, FusedAdam / FusedSGD with ``accumulate_grad_batches`` against a plain optimizer fed the sequential fp32 sum (tests/accum_ref.py),
with clipping and the non-finite guard, on the real network, across two ranks and through the trainer.

Bounds.  The kernel is one fp32 addition per element: the result is ``np.float32(a) + np.float32(b)`` bit for bit (NaN positions equal;
which NaN comes out of an addition is not pinned).  A group of k = 2 or 4 is averaged by 1/k, a power of two: multiplying the summed
gradient by it in the kernel equals feeding a plain optimizer the scaled sum, so p, m and v are bit-equal.  k = 3 (1/3 rounds) is held to
tests/optim_ref.py within the bounds tests/test_gpu_optimizer_family.py derives.  Two separately computed backward passes of the network
agree to 1e-4 of the gradient's largest element (tests/test_gpu_data_parallel.py holds them to that), so the accumulated gradient is held
to the sum of two separately computed ones by the same bound."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import accum_ref as A
import optim_ref as R
from test_gpu_optimizer_family import SENT, _check, _check_p, _f, _gen, adam_counts, beq, sgd_counts

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD, TAIL = 64, 67                                                    # the range starts 64 elements into a larger buffer
TWO_TRIPS = 2 * 8192 * 256 * 4 + 5                                     # a second grid-stride trip under the 8192-workgroup cap, then the tail
SIZES = [1, 3, 4, 5, 1023, 262144 + 7, TWO_TRIPS]
INF, NAN = float("inf"), float("nan")
DEN = float(np.float32(1e-40))                                         # a denormal
BIG = float(np.finfo(np.float32).max)
# (dst, src) pairs: infinities, inf + (-inf), NaN on either side, signed zeros, denormals (their sum, their cancellation, one that becomes
# normal), overflow to inf
SPECIALS = [(INF, 1.0), (-INF, -INF), (INF, -INF), (NAN, 1.0), (1.0, NAN), (-0.0, -0.0), (-0.0, 0.0), (DEN, DEN), (DEN, -DEN),
            (float(np.float32(1.1e-38)), float(np.float32(1.0e-38))), (BIG, BIG), (1.0, -1.0), (-INF, 3.0)]
B1, B2, EPS, MU, LR = _f(0.9), _f(0.999), _f(1e-8), _f(0.9), 2.0 ** -6


@pytest.fixture(scope="module")
def L():
    """the raw ctypes handle: entry points return their codes instead of raising"""
    from mindtheedge_amd._lib import lib
    return lib.load()


def _st():
    from mindtheedge_amd import kernels as K
    return K._stream()


class Ranged:
    """n fp32 elements at a 64-element offset of a larger buffer whose other elements hold the NaN guard pattern"""

    def __init__(self, vals):
        self.n = vals.numel()
        self.raw = torch.full((LEAD + self.n + TAIL,), SENT, dtype=torch.int32, device="cuda")
        self.raw[LEAD:LEAD + self.n] = vals.contiguous().view(torch.int32).cuda()
        self.ptr = self.raw.data_ptr() + 4 * LEAD
        assert self.ptr % 16 == 0

    def bits(self):
        return self.raw[LEAD:LEAD + self.n].cpu()

    def sides_ok(self):
        return bool((self.raw[:LEAD] == SENT).all()) and bool((self.raw[LEAD + self.n:] == SENT).all())


def _pairs(n, seed, shift):
    """two random fp32 vectors with the special pairs planted at the front and, where there is room, at the end (the n & 3 tail);
    `shift` rotates the list so that the short sizes meet every pair over a few calls"""
    g = _gen(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sp = SPECIALS[shift:] + SPECIALS[:shift]
    for i, (x, y) in enumerate(sp[:n]):
        a[i], b[i] = x, y
    if n >= 2 * len(sp):
        for i, (x, y) in enumerate(sp):
            a[n - 1 - i], b[n - 1 - i] = x, y
    return a, b


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_is_one_fp32_addition_bit_for_bit(L, n):
    assert (TWO_TRIPS >> 2) > 8192 * 256 and TWO_TRIPS % 4 == 1
    for shift in range(0, len(SPECIALS), n) if n < len(SPECIALS) else [0]:
        a, b = _pairs(n, 8000 + n % 9973, shift)
        dst, src = Ranged(a), Ranged(b)
        src_before = src.raw.clone()
        assert L.mte_grad_accumulate(dst.ptr, src.ptr, n, 0, _st()) == OK
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            want = a.numpy() + b.numpy()
        assert want.dtype == np.float32
        got = dst.bits().view(torch.float32).numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), "NaN positions differ"
        assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), "not the fp32 sum bit for bit"
        assert dst.sides_ok() and torch.equal(src.raw, src_before), "an element outside the range, or the source, changed"
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", SIZES)
def test_assign_is_a_bit_copy(L, n):
    a, b = _pairs(n, 8100 + n % 9973, 0)
    bbits = b.view(torch.int32).clone()
    bbits[n // 2] = 0x7FC12345                                         # a NaN with a payload: a copy keeps it
    if n > 2:
        bbits[n - 1] = -3                                              # 0xFFFFFFFD: a negative NaN, payload bits set down to the lowest
    b = bbits.view(torch.float32)
    dst, src = Ranged(a), Ranged(b)
    assert L.mte_grad_accumulate(dst.ptr, src.ptr, n, 1, _st()) == OK
    torch.cuda.synchronize()
    assert torch.equal(dst.bits(), bbits) and torch.equal(src.bits(), bbits) and dst.sides_ok() and src.sides_ok()
    torch.cuda.empty_cache()


def test_accumulate_argument_errors_launch_nothing(L):
    a, b = torch.arange(16.0), torch.ones(16)
    dst, src = Ranged(a), Ranged(b)
    for assign in (0, 1):
        assert L.mte_grad_accumulate(dst.ptr, src.ptr, -1, assign, _st()) == ERR_ARG                 # n < 0
        assert L.mte_grad_accumulate(None, src.ptr, 16, assign, _st()) == ERR_ARG                    # null pointers
        assert L.mte_grad_accumulate(dst.ptr, None, 16, assign, _st()) == ERR_ARG
        assert L.mte_grad_accumulate(dst.ptr + 4, src.ptr, 8, assign, _st()) == ERR_ARG              # not 16-byte aligned
        assert L.mte_grad_accumulate(dst.ptr, src.ptr + 8, 8, assign, _st()) == ERR_ARG
        assert L.mte_grad_accumulate(dst.ptr, dst.ptr, 16, assign, _st()) == ERR_ARG                 # the same range
        assert L.mte_grad_accumulate(dst.ptr, dst.ptr + 16, 8, assign, _st()) == ERR_ARG             # overlapping ranges, either way round
        assert L.mte_grad_accumulate(dst.ptr + 16, dst.ptr, 8, assign, _st()) == ERR_ARG
        assert L.mte_grad_accumulate(dst.ptr, src.ptr, 0, assign, _st()) == OK                       # n = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(dst.bits().view(torch.float32), a) and torch.equal(src.bits().view(torch.float32), b) and dst.sides_ok() and src.sides_ok()
    assert L.mte_grad_accumulate(dst.ptr, dst.ptr + 32, 8, 0, _st()) == OK                           # adjacent halves of one buffer are disjoint
    torch.cuda.synchronize()
    assert torch.equal(dst.bits().view(torch.float32)[:8], a[:8] + a[8:]) and torch.equal(dst.bits().view(torch.float32)[8:], a[8:])


# ---- 2. the optimizers without a network -------------------------------------------------------------------------------------------------------------
SHAPES = [(5,), (64,), (10, 100), (70000,)]
KINDS = {"adam": dict(lr=LR, betas=(B1, B2), eps=EPS), "sgd_momentum": dict(lr=LR, momentum=MU)}


def _toy(seed=21, n_grads=8):
    """tensors of 5, 64, 1000 and 70 000 elements, |p| >= 0.5, and a sign per element that the gradients share (optim_ref's bounds
    assume sums that do not cancel)"""
    g = _gen(seed)
    signs = [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0) for s in SHAPES]
    values = [s * (torch.rand(s.shape, generator=g) + 0.5) for s in signs]
    grads = [[s * (torch.rand(s.shape, generator=g) + 0.01) for s in signs] for _ in range(n_grads)]
    return values, grads


def _fused(kind, values, **extra):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
    return params, (FusedAdam if kind == "adam" else FusedSGD)(FlatParameters(params), **KINDS[kind], **extra)


def _state_of(opt):
    return [opt.flatp.flat.clone()] + [b.clone() for _, b in opt.state_buffers()]


def _write(params, grads):
    for q, gr in zip(params, grads):
        q.grad.copy_(gr)


def _run_group(opt, params, micro):
    """one accumulation group: zero_grad / write / accumulate() for all but the last micro-batch, step() for the last.
    -> the flat gradient of every micro-batch as the optimizer saw it"""
    seen = []
    for i, grads in enumerate(micro):
        opt.zero_grad()
        _write(params, grads)
        seen.append(opt.flatp.grad.clone())
        if i + 1 < len(micro):
            with opt.no_sync():
                pass
            steps, weights = opt.steps, opt.flatp.flat.clone()
            opt.accumulate()
            assert opt.steps == steps and torch.equal(opt.flatp.flat, weights) and opt._pending == i + 1
        else:
            opt.step()
    assert opt._pending == 0
    return seen


def _flat_like(opt, tensors):
    """per-tensor values laid out as the optimizer's flat buffers are (zero in the alignment gaps)"""
    out = torch.zeros(opt.flatp.total)
    by_id = {id(p): t for p, t in zip(opt.flatp.natural_params, tensors)}
    for p, o in zip(opt.flatp.params, opt.flatp.offsets):
        out[o:o + p.numel()] = by_id[id(p)].flatten()
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("k,sizes", [(2, (2, 2)), (4, (4, 4)), (4, (2, 4))], ids=["k2", "k4", "k4_short_first"])
def test_accumulated_steps_equal_plain_steps_on_the_scaled_sum_bit_for_bit(kind, k, sizes):
    """two groups (the second one finds `accum` full of the first: its first accumulate() assigns).  A plain optimizer on a copy is fed
    fl(sum of the group) * (1 / size) -- exact, 1 / size being a power of two -- and ends with bit-equal p, m, v / momentum buffer.
    `k4_short_first`: an optimizer built with k = 4 that steps after 2 scales by 1/2."""
    from mindtheedge_amd import kernels as K
    try:
        values, grads = _toy()
        params, opt = _fused(kind, values, accumulate_grad_batches=k)
        assert opt.flatp.accum is not None and opt.flatp.accum.shape == opt.flatp.grad.shape
        K.set_grad_sink(None)
        plain_params, plain = _fused(kind, values)
        at = 0
        for step, size in enumerate(sizes):
            seen = _run_group(opt, params, grads[at:at + size])
            at += size
            total = A.sequential_sum(seen)
            assert beq(opt.flatp.grad.cpu(), total), "flat.grad after step() is not the sequential fp32 sum"
            plain.zero_grad()
            plain.flatp.grad.copy_(total * (1.0 / size))
            plain.step()
            torch.cuda.synchronize()
            assert opt.steps == plain.steps == step + 1
            for a, b in zip(_state_of(opt), _state_of(plain)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, k, step)
        assert not any("accum" in key for key in opt.state_dict()["param_groups"][0]) and set(opt.state_dict()) == {"state", "param_groups"}
    finally:
        K.set_grad_sink(None)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_group_of_three_follows_optim_ref(kind):
    """1/3 is not a power of two: the kernel multiplies the fp32 sum by float32(1/3), as optim_ref does on accum_ref's sum"""
    from mindtheedge_amd import kernels as K
    try:
        values, grads = _toy()
        params, opt = _fused(kind, values, accumulate_grad_batches=3)
        seen = _run_group(opt, params, grads[:3])
        torch.cuda.synchronize()
        p0, zero = _flat_like(opt, values), torch.zeros(opt.flatp.total)
        assert beq(opt.flatp.grad.cpu(), A.sequential_sum(seen))
        tag = "%s k=3" % kind
        if kind == "adam":
            pr, mr, vr, dp = A.adam_step(p0, seen, zero, zero, LR, B1, B2, EPS, 1)
            c = adam_counts(False, False)
            _check(tag, "m", opt.exp_avg.cpu(), mr, c["m"])
            _check(tag, "v", opt.exp_avg_sq.cpu(), vr, c["v"])
        else:
            pr, br, dp = A.sgd_step(p0, seen, zero, LR, MU, 0.0, 0.0, False, 1)
            c = sgd_counts(MU, False, False)
            _check(tag, "buf", opt.momentum_buffer.cpu(), br, c["buf"])
        _check_p(tag, opt.flatp.flat.cpu(), pr, dp, c["p"])
        assert opt.steps == 1
    finally:
        K.set_grad_sink(None)


def test_accumulate_misuse_raises_on_the_device():
    from mindtheedge_amd import kernels as K
    try:
        values, grads = _toy()
        params, opt = _fused("adam", values)
        with pytest.raises(RuntimeError, match="accumulate_grad_batches"):
            opt.accumulate()
        K.set_grad_sink(None)
        params, opt = _fused("adam", values, accumulate_grad_batches=2)
        _write(params, grads[0])
        opt.accumulate()
        _write(params, grads[1])
        with pytest.raises(RuntimeError, match="already accumulated"):
            opt.accumulate()
        opt.step()
        torch.cuda.synchronize()
        assert opt.steps == 1 and opt._pending == 0
    finally:
        K.set_grad_sink(None)


# ---- 3. clip and guard -----------------------------------------------------------------------------------------------------------------------------
def test_the_clip_sees_the_averaged_accumulated_gradient():
    """grad_stats()['grad_norm'] against the fp64 norm of (sequential sum) / 2, to the float32 rounding tests/test_gpu_grad_clip.py allows
    (2^-23 relative); the coefficient clips exactly when that norm exceeds max_norm, and the step equals a plain clipped step on the sum"""
    from mindtheedge_amd import kernels as K
    try:
        values, grads = _toy()
        probe = torch.cat([(a + b).flatten() for a, b in zip(grads[0], grads[1])]).double() * 0.5
        norm = float(probe.square().sum().sqrt())
        for max_norm, clips in ((0.5 * norm, True), (2.0 * norm, False)):
            params, opt = _fused("adam", values, accumulate_grad_batches=2, clip_grad_norm=max_norm)
            seen = _run_group(opt, params, grads[:2])
            stats = opt.grad_stats()
            total = float((A.sequential_sum(seen).double() * 0.5).square().sum().sqrt())
            print("accumulated clip: norm %.9g (fp64 %.9g) coef %.9g" % (stats["grad_norm"], total, stats["clip_coef"]))
            assert abs(stats["grad_norm"] - total) <= 2.0 ** -23 * total
            assert (stats["clip_coef"] < 1.0) == clips and stats["skipped"] is False
            K.set_grad_sink(None)
            plain_params, plain = _fused("adam", values, clip_grad_norm=max_norm)
            plain.flatp.grad.copy_(A.sequential_sum(seen) * 0.5)
            plain.step()
            torch.cuda.synchronize()
            for a, b in zip(_state_of(opt) + [opt.ctl], _state_of(plain) + [plain.ctl]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_an_inf_in_the_first_micro_batch_skips_the_step(kind):
    from mindtheedge_amd import kernels as K
    try:
        values, grads = _toy()
        params, opt = _fused(kind, values, accumulate_grad_batches=2, skip_nonfinite=True)
        _run_group(opt, params, grads[:2])                              # a finite group first: non-zero moments
        torch.cuda.synchronize()
        before = _state_of(opt)
        poisoned = [g.clone() for g in grads[2]]
        poisoned[3][12345] = INF
        _run_group(opt, params, [poisoned, grads[3]])
        stats = opt.grad_stats()
        assert stats["skipped"] is True and stats["skipped_steps"] == 1 and opt.steps == 2
        for a, b in zip(before, _state_of(opt)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        _run_group(opt, params, grads[4:6])                             # the next group starts clean: accum was assigned, not added to
        assert opt.grad_stats()["skipped"] is False and opt.grad_stats()["skipped_steps"] == 1
        assert all(bool(torch.isfinite(t).all()) for t in _state_of(opt)) and not torch.equal(before[0], opt.flatp.flat)
    finally:
        K.set_grad_sink(None)


# ---- 4. the default ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_default_has_no_second_buffer_and_steps_as_before(kind, monkeypatch):
    from mindtheedge_amd import kernels as K
    try:
        K.lib.load()
        values, grads = _toy()
        results = []
        for extra in ({}, dict(accumulate_grad_batches=1)):
            with monkeypatch.context() as mp_:
                def never(*a):
                    raise AssertionError("a k = 1 optimizer must not launch mte_grad_accumulate")
                mp_.setitem(K.lib.__dict__, "mte_grad_accumulate", never)
                params, opt = _fused(kind, values, **extra)
                assert opt.flatp.accum is None and opt.accumulate_grad_batches == 1
                for step in range(3):
                    opt.zero_grad()
                    _write(params, grads[step])
                    opt.step()
                torch.cuda.synchronize()
                results.append(_state_of(opt))
            K.set_grad_sink(None)
        for a, b in zip(*results):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        K.set_grad_sink(None)


# ---- 5. the network ---------------------------------------------------------------------------------------------------------------------------------
def _edge_model(completion):
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.models.SemiSupEdgeCompletionModel import SemiSupEdgeCompletionModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from oracle import packnet_oracle as po
    kw = dict(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog", supervised_num_scales=1,
              edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.0)
    if completion:
        from test_gpu_san import _randomise
        net = PackNetSAN01(dropout=None, version="1A", with_san=True)
        missing = net.load_state_dict(po.fixture_params(), strict=False)
        assert not missing.unexpected_keys and all(k.startswith("mconvs.") for k in missing.missing_keys)
        _randomise(net.mconvs, seed=9)
        model = SemiSupEdgeCompletionModel(**kw)
    else:
        net = PackNetSAN01(dropout=None, version="1A")
        net.load_state_dict(po.fixture_params(), strict=True)
        model = SemiSupEdgeModel(**kw)
    model.add_depth_net(net.cuda())
    model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
    model.train()
    return net, model


@pytest.mark.parametrize("completion", [False, True], ids=["rgb", "completion_suspended_sink"])
def test_the_accumulated_network_gradient_is_the_sum_of_the_two(completion):
    """fp32 mode, 64x128, B = 1, no dropout, no flip, fixture weights: two different batches through accumulate() + step() against the
    sum of their separately computed gradients.  The completion model's forward suspends the gradient sink (its graph uses parameters
    twice): there autograd adds into the zeroed buffer."""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedSGD
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        K.set_compute_dtype("fp32")
        K.set_grad_sink(None)
        net, model = _edge_model(completion)
        flat = FlatParameters(net.parameters())
        opt = FusedSGD(flat, lr=1e-12, accumulate_grad_batches=2)
        batches = [synthetic_batch(1, 64, 128, seed=s, device=dev, lidar=completion) for s in (50, 61)]

        def backward(batch):
            opt.zero_grad()
            model(batch)["loss"].sum().backward()

        single = []
        for b in batches:
            backward(b)
            K.join_side_stream()
            torch.cuda.synchronize()
            single.append(flat.grad.clone())
            flat.sink.end_step()
        assert float((single[0] - single[1]).abs().max()) > 0.0
        with opt.no_sync():
            backward(batches[0])
        assert flat.sink.suspended is completion                       # the route under test
        opt.accumulate()
        assert flat.sink.suspended is False
        backward(batches[1])
        assert flat.sink.suspended is completion
        opt.step()
        torch.cuda.synchronize()
        want = single[0] + single[1]
        err = float((flat.grad - want).abs().max() / want.abs().max())
        print("accumulated network gradient (%s): relative max error %.3g (bound 1e-4)" % ("completion" if completion else "rgb", err))
        assert err < 1e-4 and opt.steps == 1
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


# ---- 6. two ranks ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    """as tests/test_gpu_data_parallel.py: both ranks on cuda:0, gloo transport, the real model, ranks and micro-batches all different"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from mindtheedge_amd import kernels as K
        from mindtheedge_amd.trainers.data_parallel import FlatParameters, BucketedAllReduce, FusedAdam, broadcast_parameters
        from mindtheedge_amd.utils.synthetic import synthetic_batch
        K.set_compute_dtype("fp32")
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        net, model = _edge_model(False)
        flat = FlatParameters(net.parameters())
        broadcast_parameters(flat)
        batches = [synthetic_batch(1, 64, 128, seed=50 + 10 * m + rank, device=dev) for m in range(2)]
        msgs = []
        # (1) this rank's two local gradients, no reducer attached
        local = torch.zeros_like(flat.grad)
        for b in batches:
            flat.zero_grad()
            model(b)["loss"].sum().backward()
            K.join_side_stream()
            local += flat.grad
            flat.sink.end_step()
        # (2) the same two micro-batches as one accumulated, reduced step
        red = BucketedAllReduce(flat, bucket_bytes=8 << 20)
        assert red.active and len(red.buckets) >= 4
        opt = FusedAdam(flat, lr=1e-4, reducer=red, accumulate_grad_batches=2)
        opt.zero_grad()
        with opt.no_sync():
            model(batches[0])["loss"].sum().backward()
        if red._works or red.launch_log:
            msgs.append("a collective was launched under no_sync()")
        opt.accumulate()
        opt.zero_grad()
        model(batches[1])["loss"].sum().backward()
        launched = len(red._works)
        if launched < 3:
            msgs.append("only %d collectives were launched before finish()" % launched)
        opt.step()
        torch.cuda.synchronize()
        if sorted(b for b, _, _, _ in red.last_launches) != list(range(len(red.buckets))):
            msgs.append("buckets launched: %s" % [b for b, _, _, _ in red.last_launches])
        scale = 1.0 / (world * 2)
        want = local.cpu()
        dist.all_reduce(want)
        want = want * scale
        err = float((flat.grad.cpu() * scale - want).abs().max() / want.abs().max())
        if not err < 1e-4:
            msgs.append("averaged gradient: relative max error %g" % err)
        bits = flat.flat.view(torch.int32).to(torch.int64)
        mine = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=dev) % 8191)).sum()]).cpu()
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        if not torch.equal(every[0], every[1]):
            msgs.append("the ranks' weights differ after the step")
        if opt.steps != 1 or opt._pending != 0:
            msgs.append("steps %d pending %d" % (opt.steps, opt._pending))
        # (3) forgetting no_sync(): the buckets went out with one micro-batch's gradient, accumulate() refuses
        opt.zero_grad()
        model(batches[0])["loss"].sum().backward()
        try:
            opt.accumulate()
            msgs.append("accumulate() after a reduced backward did not raise")
        except RuntimeError as e:
            if "no_sync" not in str(e):
                msgs.append("wrong error: %s" % e)
        red.finish()
        torch.cuda.synchronize()
        q.put((rank, "ok err=%.3g launched=%d" % (err, launched) if not msgs else "; ".join(msgs)))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_accumulate_locally_and_reduce_once():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=280) for _ in procs]
    for p in procs:
        p.join(30)
    print(res)
    assert all(r[1].startswith("ok") for r in res), res


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------------------------------
def _wrapper():
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    over = {"model": {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                               "depth_edges_loss_weight": 1.0, "edges_depth_edge_loss_all_scales": True},
                      "depth_net": {"dropout": 0.5},
                      "optimizer": {"name": "AdamW", "depth": {"lr": 1e-4, "weight_decay": 0.01}, "clip_grad_norm": 10.0, "skip_nonfinite_steps": True}},
            "datasets": {"augmentation": {"image_shape": (64, 128)}, "train": {"batch_size": 1}}}
    torch.manual_seed(11)
    return ModelWrapper(load_config(None, over))


@pytest.mark.parametrize("k", [2, 1])
def test_the_trainer_groups_five_batches(k):
    import math
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.trainer import Trainer
    from mindtheedge_amd.utils.synthetic import SyntheticLoader
    try:
        trainer = Trainer(max_epochs=1, log_every=0, accumulate_grad_batches=k)
        wrap = _wrapper()
        loader = SyntheticLoader(1, 64, 128, 5, trainer.device)
        hist = trainer.fit(wrap, train_dataloader=loader, epochs=1)
        torch.cuda.synchronize()
        out = hist[0]
        assert out["steps"] == 5 and all(math.isfinite(out[key]) for key in ("avg_loss", "avg_supervised", "avg_edge", "avg_grad_norm"))
        assert out["skipped_steps"] == 0 and out["avg_grad_norm"] > 0.0
        if k == 2:
            assert out["optimizer_steps"] == 3 and wrap.optimizer.steps == 3 and wrap.optimizer.accumulate_grad_batches == 2
            assert wrap.optimizer._pending == 0
        else:
            assert "optimizer_steps" not in out and wrap.optimizer.steps == 5 and wrap.optimizer.flatp.accum is None
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


def test_train_edges_runs_the_shipped_accum_yaml(tmp_path, capsys):
    """train_edges.py configs/train_packnet_san_kitti_with_edges_accum.yaml --synthetic (frame size, batch and checkpoint folder set for the
    test): ten micro-batches at k = 8 are a full group and a short one -- two optimizer steps, which the checkpoint's Adam state counts"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    with open(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_accum.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["arch"]["accumulate_grad_batches"] == 8
    cfg["datasets"]["augmentation"]["image_shape"] = [64, 128]
    cfg["datasets"]["train"]["batch_size"] = 1
    cfg["checkpoint"].update(filepath="", save_top_k=-1)
    path, save = os.path.join(tmp_path, "cfg.yaml"), os.path.join(tmp_path, "run")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    old = sys.argv
    sys.argv = ["train_edges.py", path, "--synthetic", "--steps", "10", "--epochs", "1", "--save", save]
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        importlib.import_module("train_edges").main()
    finally:
        sys.argv = old
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")
    out = capsys.readouterr().out
    assert "'steps': 10" in out and "'optimizer_steps': 2" in out and "'skipped_steps': 0" in out and "'avg_grad_norm': " in out
    ck = load_checkpoint(os.path.join(save, "epoch=0.ckpt"))
    assert {int(float(st["step"])) for st in ck["optimizer"]["state"].values()} == {2}
    assert not any("accum" in k for k in ck["optimizer"]["param_groups"][0])


def test_graphed_train_step_refuses_an_accumulating_optimizer():
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.utils.graph import GraphedTrainStep
    try:
        values, _ = _toy()
        _, opt = _fused("adam", values, accumulate_grad_batches=2)
        with pytest.raises(NotImplementedError, match="accumulate_grad_batches"):
            GraphedTrainStep(torch.nn.Identity().train(), opt, {"rgb": torch.zeros(1, 3, 64, 128, device="cuda")})
    finally:
        K.set_grad_sink(None)
