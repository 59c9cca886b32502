"""GPU (-m gpu): the optimizer family of csrc/optim.hip -- Adam with L2 weight decay, AdamW, SGD (momentum, dampening, Nesterov, weight
decay) -- through the raw C ABI against the float64 statements of tests/optim_ref.py (pinned to torch.optim by
tests/test_optimizer_family_cpu.py), and FusedAdam / FusedSGD against torch.optim.{Adam, AdamW, SGD} in float64 under a StepLR schedule,
through their checkpoints, a HIP-graph replay and the training entry point.

Bounds.  The kernels run fp32 with contraction off; every operation rounds within u = 2^-24 relative (sqrt and divide correctly rounded).
The inputs give each element ONE sign for p, g and the moment / momentum buffer, so that no sum below cancels and relative errors
add.  Per element, counting the operations that feed an output (wd = 1 with a weight decay, else 0):

  Adam   g' = g * gscale [+ wd * p: a multiply and an add]                                       1 + 2 L2
         m  = b1 * m + (1 - b1) * g'             multiply, multiply, add on top of g'            4 + 2 L2   (worst case 4u / 5u)
         v  = b2 * v + (1 - b2) * g' * g'        three multiplies and an add on top of g'        5 + 2 L2   (worst case 6u / 8u: g' enters twice)
         dp = (lr / bc1) * (m / (sqrt(v) / bc2s + eps))   m's 3 + L2's 2, sqrt, divide, add, divide, multiply = 9 + 2 L2; AdamW adds
              (lr * wd) * p + ...: a multiply and an add = 9 + 2.  Worst case m + v / 2 + 8u = 15u / 17u (16u AdamW): the 8u hold the five
              operations and the three rounded scalars bc1, bc2s, lr / bc1 (lr * wd for AdamW).
  SGD    buf = mu * buf + omd * g'               multiply, multiply, add on top of g'            4 + 2 wd   (worst case 4u / 5u)
         dp  = lr * g''                          plain 2 + 2 wd; momentum buf + 1; Nesterov (g' + mu * buf) buf + 3   (worst case = count)

  m, v, buf are held to MARGIN * count * u relative; p to MARGIN * count * u of the update dp plus 2^-23 |p_ref| for the final
  subtraction's rounding (2^-24 |p|).  MARGIN = 2, for the per-launch scalars that reach the kernel rounded to C floats (the bias
  corrections, 1 - beta, lr / bc1, lr * wd, 1 - dampening), which the reference takes at their float32 values but combines in float64:
  they are the part of the worst cases above that the per-element count does not hold.  Every worst case is within 2 * count * u.
Each check prints measured error / bound."""
import ctypes  # noqa: F401
import os
import random
import sys

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
U, MARGIN = 2.0 ** -24, 2.0
SENT = 0x7FA5A5A5                                                     # a NaN bit pattern: the guard elements past n
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 4 * 8192 * 256 + 3                                              # every thread of the capped grid holds one vector, then a 3-element tail
WRAP = 4 * (8192 * 256 + 300) + 3                                     # 300 vectors more: a second trip through the vector loop
# lr, beta1, beta2, eps, gscale (0.25 is dyadic, 1/3 is not), weight decay
HYPERS = [(1e-4, 0.9, 0.999, 1e-8, 0.25, 0.01), (3e-2, 0.5, 0.9, 1e-3, 1.0 / 3.0, 0.1)]
# name, momentum, dampening, nesterov, with weight decay
SGD_VARIANTS = [("plain", 0.0, 0.0, 0, False), ("plain_wd", 0.0, 0.0, 0, True), ("momentum", 0.9, 0.0, 0, False),
                ("momentum_dampening_wd", 0.9, 0.1, 0, True), ("nesterov", 0.9, 0.0, 1, False), ("nesterov_wd", 0.9, 0.0, 1, True)]


@pytest.fixture(scope="module")
def L():
    """the raw ctypes handle: entry points return their codes instead of raising"""
    from mindtheedge_amd._lib import lib
    return lib.load()


def _st():
    from mindtheedge_amd import kernels as K
    return K._stream()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f(s):
    return float(np.float32(s))


def beq(a, b):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Flat:
    """n fp32 elements followed by `extra` guard elements, pre-filled with the NaN pattern"""

    def __init__(self, n, extra=67):
        self.n = n
        self.raw = torch.full((n + extra,), SENT, dtype=torch.int32, device="cuda")
        self.t = self.raw.view(torch.float32)
        self.ptr = self.t.data_ptr()

    def set(self, vals):
        self.t[:self.n] = vals.flatten().float().cuda()
        return self

    def get(self):
        return self.t[:self.n].cpu()

    def guard_ok(self):
        return bool((self.raw[self.n:] == SENT).all())


def _inputs(n, g, nonzero_state):
    """One sign per element for p, its gradients and its moment / buffer.  Gradients are exactly zero at 2::3; p (and v) are zero at 2::6:
    there g' = 0 meets v = 0 whatever the decay, and at 5::6 a zero gradient meets wd * p != 0 (v = 0 for AdamW and without decay).
    |p| >= 0.5: the few steps taken here move it by < 0.1, so it keeps its sign."""
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p0 = sign * (torch.rand(n, generator=g) + 0.5)
    p0[2::6] = 0.0

    def grad():
        x = sign * (torch.rand(n, generator=g) + 0.01)
        x[2::3] = 0.0
        return x
    if not nonzero_state:
        return p0, grad, torch.zeros(n), torch.zeros(n)
    m0 = sign * (torch.rand(n, generator=g) + 0.01) * 0.1
    m0[2::6] = 0.0
    v0 = (torch.rand(n, generator=g) + 0.01) * 0.01
    v0[2::6] = 0.0
    return p0, grad, m0, v0


def _check(tag, name, got, ref, count):
    err = (got.double() - ref).abs()
    bound = MARGIN * count * U * ref.abs()
    print("%s %s: max err / bound = %.3g" % (tag, name, float((err / bound.clamp(min=1e-300)).max())))
    assert bool((err <= bound).all()), (tag, name)


def _check_p(tag, got, ref, dp, count):
    err = (got.double() - ref).abs()
    bound = MARGIN * count * U * dp.abs() + 2.0 ** -23 * ref.abs()
    print("%s p: max err / bound = %.3g" % (tag, float((err / bound.clamp(min=1e-300)).max())))
    assert bool((err <= bound).all()), (tag, "p")


def adam_counts(wd, decoupled):
    l2 = 2 if wd and not decoupled else 0
    return {"m": 4 + l2, "v": 5 + l2, "p": 9 + (2 if wd else 0)}


def sgd_counts(mu, nesterov, wd):
    buf = 4 + (2 if wd else 0)
    return {"buf": buf, "p": (2 + (2 if wd else 0)) if not mu else buf + (3 if nesterov else 1)}


def _adamw_call(L, n, hyper, decoupled, step, p0, g, m0, v0):
    """one mte_adamw_step and one mte_adamw_step_dev from the same fp32 state: bit-equal to each other (guards included), g and the guards
    untouched, and within the module docstring's bounds of optim_ref.adam_step on the same fp32 inputs"""
    lr, b1, b2, eps, gscale, wd = hyper
    (p, m, v), (pd, md, vd) = [[Flat(n).set(t) for t in (p0, m0, v0)] for _ in range(2)]
    g_d = g.cuda()
    assert L.mte_adamw_step(p.ptr, g_d.data_ptr(), m.ptr, v.ptr, n, lr, b1, b2, eps, wd, decoupled, step, gscale, _st()) == OK
    hyp = R.adam_hyper(lr, b1, b2, step).cuda()
    assert L.mte_adamw_step_dev(pd.ptr, g_d.data_ptr(), md.ptr, vd.ptr, n, hyp.data_ptr(), b1, b2, eps, wd, decoupled, gscale, _st()) == OK
    torch.cuda.synchronize()
    for a, b in ((p, pd), (m, md), (v, vd)):
        assert torch.equal(a.raw, b.raw) and a.guard_ok()
    assert beq(g_d.cpu(), g)
    pr, mr, vr, dp = R.adam_step(p0, g, m0, v0, lr, b1, b2, eps, step, gscale, wd, bool(decoupled))
    pg, mg, vg = p.get(), m.get(), v.get()
    c = adam_counts(wd, decoupled)
    tag = "%s n=%d step=%d" % ("adamw" if decoupled else "adam+l2", n, step)
    _check(tag, "m", mg, mr, c["m"])
    _check(tag, "v", vg, vr, c["v"])
    _check_p(tag, pg, pr, dp, c["p"])
    return pg, mg, vg


def _sgd_call(L, n, lr, gscale, wd, mu, damp, nesterov, step, p0, g, b0):
    """as _adamw_call for mte_sgd_step / mte_sgd_step_dev; momentum = 0 passes a null buffer"""
    p, pd = Flat(n).set(p0), Flat(n).set(p0)
    b, bd = (Flat(n).set(b0), Flat(n).set(b0)) if mu else (None, None)
    g_d = g.cuda()
    assert L.mte_sgd_step(p.ptr, g_d.data_ptr(), b.ptr if mu else None, n, lr, mu, damp, wd, nesterov, step, gscale, _st()) == OK
    hyp = R.sgd_hyper(lr, mu, damp, step).cuda()
    assert L.mte_sgd_step_dev(pd.ptr, g_d.data_ptr(), bd.ptr if mu else None, n, hyp.data_ptr(), mu, wd, nesterov, gscale, _st()) == OK
    torch.cuda.synchronize()
    for x, y in ((p, pd), (b, bd)) if mu else ((p, pd),):
        assert torch.equal(x.raw, y.raw) and x.guard_ok()
    assert beq(g_d.cpu(), g)
    pr, br, dp = R.sgd_step(p0, g, b0 if mu else None, lr, mu, damp, wd, bool(nesterov), step, gscale)
    c = sgd_counts(mu, nesterov, wd)
    tag = "sgd mu=%g damp=%g nesterov=%d wd=%g n=%d step=%d" % (mu, damp, nesterov, wd, n, step)
    if mu:
        _check(tag, "buf", b.get(), br, c["buf"])
    _check_p(tag, p.get(), pr, dp, c["p"])
    return p.get(), (b.get() if mu else b0)


# ---- 1. per entry point against optim_ref, host and device scalars bit-equal ------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1027])
def test_adamw_step(L, n, decoupled):
    for hi, hyper in enumerate(HYPERS):
        g = _gen(2000 + 10 * n + hi)
        p, grad, m, v = _inputs(n, g, False)
        for step in (1, 2, 3):
            p, m, v = _adamw_call(L, n, hyper, decoupled, step, p, grad(), m, v)
        p, grad, m, v = _inputs(n, g, True)
        _adamw_call(L, n, hyper, decoupled, 1000, p, grad(), m, v)


@pytest.mark.parametrize("variant", SGD_VARIANTS, ids=[s[0] for s in SGD_VARIANTS])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1027])
def test_sgd_step(L, n, variant):
    _, mu, damp, nesterov, with_wd = variant
    for hi, (lr, gscale, wd) in enumerate([(1e-2, 0.25, 0.01), (3e-2, 1.0 / 3.0, 0.1)]):
        wd = wd if with_wd else 0.0
        g = _gen(3000 + 10 * n + hi)
        p, grad, b, _ = _inputs(n, g, False)
        for step in (1, 2, 3):                                        # step 1 from a zero buffer: buf = g' also with dampening
            p, b = _sgd_call(L, n, lr, gscale, wd, mu, damp, nesterov, step, p, grad(), b)
        p, grad, b, _ = _inputs(n, g, True)
        _sgd_call(L, n, lr, gscale, wd, mu, damp, nesterov, 1000, p, grad(), b)


# ---- 2. past the grid cap --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [BIG, WRAP])
def test_past_the_grid_cap(L, n):
    assert (BIG >> 2) == 8192 * 256 and (WRAP >> 2) > 8192 * 256 and n % 4 == 3
    g = _gen(2100)
    p, grad, m, v = _inputs(n, g, True)
    _adamw_call(L, n, HYPERS[1], 1, 1000, p, grad(), m, v)
    _sgd_call(L, n, 3e-2, 1.0 / 3.0, 0.1, 0.9, 0.1, 0, 1000, p, grad(), m)
    torch.cuda.empty_cache()


# ---- 3. compatibility: no weight decay = the Adam step that was there ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 1027])
def test_no_weight_decay_is_mte_adam_step_bit_for_bit(L, n):
    lr, b1, b2, eps, gscale, _ = HYPERS[1]
    g = _gen(2200 + n)
    p0, grad, m0, v0 = _inputs(n, g, True)
    g_d = grad().cuda()
    ref = [Flat(n).set(t) for t in (p0, m0, v0)]
    assert L.mte_adam_step(ref[0].ptr, g_d.data_ptr(), ref[1].ptr, ref[2].ptr, n, lr, b1, b2, eps, 5, gscale, _st()) == OK
    hyp = R.adam_hyper(lr, b1, b2, 5).cuda()
    for decoupled in (0, 1):
        a, d = ([Flat(n).set(t) for t in (p0, m0, v0)] for _ in range(2))
        assert L.mte_adamw_step(a[0].ptr, g_d.data_ptr(), a[1].ptr, a[2].ptr, n, lr, b1, b2, eps, 0.0, decoupled, 5, gscale, _st()) == OK
        assert L.mte_adamw_step_dev(d[0].ptr, g_d.data_ptr(), d[1].ptr, d[2].ptr, n, hyp.data_ptr(), b1, b2, eps, 0.0, decoupled, gscale, _st()) == OK
        torch.cuda.synchronize()
        for x, y, z in zip(ref, a, d):
            assert torch.equal(x.raw, y.raw) and torch.equal(x.raw, z.raw)


def _toy_params(seed=5, device="cuda"):
    """four small tensors of odd sizes, |p| >= 0.5, and a sign per element that the gradients share"""
    g = _gen(seed)
    signs = [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0) for s in [(3,), (5, 7), (1,), (64,)]]
    values = [s * (torch.rand(s.shape, generator=g) + 0.5) for s in signs]
    grads = [[s * (torch.rand(s.shape, generator=g) + 0.01) for s in signs] for _ in range(7)]
    return signs, values, grads


def test_default_fused_adam_still_launches_mte_adam_step_dev(L, monkeypatch):
    """FusedAdam(flat) with defaults: the step goes through mte_adam_step_dev with hyper = {lr, 1 - b1^t, sqrt(1 - b2^t)} -- the new entry
    point is not touched -- and gives what a direct call gives, bit for bit"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    try:
        K.lib.load()

        def never(*a):
            raise AssertionError("the default FusedAdam must not launch mte_adamw_step_dev")
        monkeypatch.setitem(K.lib.__dict__, "mte_adamw_step_dev", never)
        _, values, grads = _toy_params()
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        flat = FlatParameters(params)
        opt = FusedAdam(flat)
        assert opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[0]["lr"] == 1e-4
        n = flat.flat.numel()
        p, m, v = (Flat(n).set(t) for t in (flat.flat, opt.exp_avg, opt.exp_avg_sq))
        for step in (1, 2):
            for q, gr in zip(params, grads[step]):
                q.grad.copy_(gr)
            g_d = flat.grad.clone()
            opt.step()
            # the class forms the bias corrections in double from its own (double) betas
            hyp = torch.tensor([1e-4, 1.0 - 0.9 ** step, (1.0 - 0.999 ** step) ** 0.5], dtype=torch.float64).float().cuda()
            assert beq(opt.hyper.cpu(), hyp.cpu()) and opt.steps == step
            assert L.mte_adam_step_dev(p.ptr, g_d.data_ptr(), m.ptr, v.ptr, n, hyp.data_ptr(), 0.9, 0.999, 1e-8, 1.0, _st()) == OK
            torch.cuda.synchronize()
            assert beq(p.get(), flat.flat.cpu()) and beq(m.get(), opt.exp_avg.cpu()) and beq(v.get(), opt.exp_avg_sq.cpu())
    finally:
        K.set_grad_sink(None)


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    p, m, v = (Flat(8).set(torch.ones(8)) for _ in range(3))
    g = torch.ones(8).cuda()
    hyp = R.adam_hyper(1e-4, 0.9, 0.999, 1).cuda()
    gp, hp = g.data_ptr(), hyp.data_ptr()
    adam = (1e-4, 0.9, 0.999, 1e-8)
    assert L.mte_adamw_step(p.ptr, gp, m.ptr, v.ptr, 8, *adam, 0.01, 1, 0, 1.0, _st()) == ERR_ARG                       # step = 0
    assert L.mte_adamw_step(p.ptr, gp, m.ptr, v.ptr, 0, *adam, 0.01, 1, 1, 1.0, _st()) == ERR_ARG                       # n = 0
    assert L.mte_adamw_step(p.ptr, gp, None, v.ptr, 8, *adam, 0.01, 1, 1, 1.0, _st()) == ERR_ARG                        # a null moment
    assert L.mte_adamw_step(p.ptr, gp, m.ptr, v.ptr, 8, *adam, -0.01, 1, 1, 1.0, _st()) == ERR_ARG                      # a negative decay
    assert L.mte_adamw_step_dev(p.ptr, gp, m.ptr, v.ptr, 0, hp, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, _st()) == ERR_ARG       # n = 0
    assert L.mte_adamw_step_dev(p.ptr, gp, m.ptr, v.ptr, 8, None, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, _st()) == ERR_ARG     # a null hyper
    assert L.mte_sgd_step(p.ptr, gp, m.ptr, 8, 1e-2, 0.9, 0.0, 0.0, 0, 0, 1.0, _st()) == ERR_ARG                        # step = 0
    assert L.mte_sgd_step(p.ptr, gp, m.ptr, 0, 1e-2, 0.9, 0.0, 0.0, 0, 1, 1.0, _st()) == ERR_ARG                        # n = 0
    assert L.mte_sgd_step(p.ptr, gp, None, 8, 1e-2, 0.9, 0.0, 0.0, 0, 1, 1.0, _st()) == ERR_ARG                         # momentum without a buffer
    assert L.mte_sgd_step(p.ptr, gp, m.ptr, 8, 1e-2, 0.0, 0.0, 0.0, 1, 1, 1.0, _st()) == ERR_ARG                        # Nesterov without momentum
    assert L.mte_sgd_step(p.ptr, gp, m.ptr, 8, 1e-2, 0.9, 0.1, 0.0, 1, 1, 1.0, _st()) == ERR_ARG                        # Nesterov with dampening
    assert L.mte_sgd_step_dev(p.ptr, gp, m.ptr, 0, hp, 0.9, 0.0, 0, 1.0, _st()) == ERR_ARG                              # n = 0
    assert L.mte_sgd_step_dev(p.ptr, gp, m.ptr, 8, None, 0.9, 0.0, 0, 1.0, _st()) == ERR_ARG                            # a null hyper
    assert L.mte_sgd_step_dev(p.ptr, gp, None, 8, hp, 0.9, 0.0, 0, 1.0, _st()) == ERR_ARG                               # momentum without a buffer
    assert L.mte_sgd_step_dev(p.ptr, gp, m.ptr, 8, hp, 0.0, 0.0, 1, 1.0, _st()) == ERR_ARG                              # Nesterov without momentum
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert beq(t.get(), torch.ones(8)) and t.guard_ok()


# ---- 5. the classes against torch.optim under a schedule, and their checkpoints ------------------------------------------------------------------------
B1, B2, EPS, WD, MU, LR = _f(0.9), _f(0.999), _f(1e-8), _f(0.01), _f(0.9), 2.0 ** -6      # float32 values: both sides compute with the same scalars
DAMP = _f(0.6)
CLASS_CASES = {
    "adamw": ("adam", dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, decoupled_weight_decay=True), torch.optim.AdamW,
              dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD), adam_counts(True, True)["p"]),
    "adam_l2": ("adam", dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD), torch.optim.Adam,
                dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD), adam_counts(True, False)["p"]),
    "sgd_momentum": ("sgd", dict(lr=LR, momentum=MU), torch.optim.SGD, dict(lr=LR, momentum=MU), sgd_counts(MU, False, False)["p"]),
    "sgd_nesterov": ("sgd", dict(lr=LR, momentum=MU, nesterov=True), torch.optim.SGD, dict(lr=LR, momentum=MU, nesterov=True),
                     sgd_counts(MU, True, False)["p"]),
    # beyond the issue's four cases: weight decay under the schedule and a dampening whose 1 - dampening rounds differently from the
    # double than from the float32 value (see test_fused_sgd_device_scalars_equal_the_host_entry_point)
    "sgd_dampening_wd": ("sgd", dict(lr=LR, momentum=MU, dampening=DAMP, weight_decay=WD), torch.optim.SGD,
                         dict(lr=LR, momentum=MU, dampening=DAMP, weight_decay=WD), sgd_counts(MU, False, True)["p"]),
    "sgd_plain_wd": ("sgd", dict(lr=LR, weight_decay=WD), torch.optim.SGD, dict(lr=LR, weight_decay=WD), sgd_counts(0.0, False, True)["p"]),
}


def _fused(kind, values, kwargs):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
    return params, (FusedAdam if kind == "adam" else FusedSGD)(FlatParameters(params), **kwargs)


def _state_of(opt):
    return [opt.flatp.flat.clone()] + [b.clone() for _, b in opt.state_buffers()]


@pytest.mark.parametrize("case", sorted(CLASS_CASES))
def test_classes_follow_torch_under_a_schedule_and_through_a_checkpoint(case):
    """Five steps with StepLR(step_size=2, gamma=0.5) stepped in between, against the torch class in float64 on CPU copies: per parameter
    within the sum of the five single-step bounds (errors add at most linearly).  A decay that ignored the scheduler's learning rate, or a
    wrong first-step momentum rule, is orders of magnitude outside.  Then the checkpoint: state_dict() loads into the torch class, one more
    step agrees within the single-step bound, and a fresh fused optimizer that loads it continues bit-equal to the one that never stopped."""
    from mindtheedge_amd import kernels as K
    kind, kwargs, tcls, tkwargs, count = CLASS_CASES[case]
    try:
        _, values, grads = _toy_params()
        params, opt = _fused(kind, values, kwargs)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        tparams = [torch.nn.Parameter(v.double().clone()) for v in values]
        topt = tcls([{'params': tparams, 'name': 'Depth'}], **tkwargs)
        tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=2, gamma=0.5)
        bounds = [torch.zeros_like(t.data) for t in tparams]

        def one_step(step_grads, schedule):
            for q, t, gr, b in zip(params, tparams, step_grads, bounds):
                q.grad.copy_(gr)
                t.grad = gr.double()
            before = [t.detach().clone() for t in tparams]
            opt.step()
            topt.step()
            if schedule:
                sched.step()
                tsched.step()
            return [MARGIN * count * U * (b0 - t.detach()).abs() + 2.0 ** -23 * t.detach().abs() for b0, t in zip(before, tparams)]

        for step in range(5):
            for b, single in zip(bounds, one_step(grads[step], True)):
                b += single
        torch.cuda.synchronize()
        assert opt.param_groups[0]['lr'] == topt.param_groups[0]['lr'] == LR / 4 and opt.steps == 5
        for i, (q, t, b) in enumerate(zip(params, tparams, bounds)):
            err = (q.detach().cpu().double() - t.detach()).abs()
            print("%s tensor %d after 5 steps: max err / bound = %.3g" % (case, i, float((err / b).max())))
            assert bool((err <= b).all()), (case, i)

        # the checkpoint in torch's layout: into the real torch class over same-shaped CPU parameters ...
        sd = opt.state_dict()
        cparams = [torch.nn.Parameter(q.detach().cpu().double()) for q in params]
        copt = tcls([{'params': cparams, 'name': 'Depth'}], **{**tkwargs, 'lr': 0.5})
        copt.load_state_dict(sd)
        assert copt.param_groups[0]['lr'] == LR / 4 and copt.param_groups[0]['weight_decay'] == opt.param_groups[0]['weight_decay']
        # ... and into a fresh fused optimizer
        params2, opt2 = _fused(kind, [q.detach().cpu() for q in params], {**kwargs, 'lr': 0.5})
        opt2.load_state_dict(sd)
        assert all(torch.equal(a, b) for a, b in zip(_state_of(opt), _state_of(opt2)))
        for q, q2, c, gr in zip(params, params2, cparams, grads[5]):
            q.grad.copy_(gr)
            q2.grad.copy_(gr)
            c.grad = gr.double()
        before = [c.detach().clone() for c in cparams]
        opt.step()
        opt2.step()
        copt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_state_of(opt), _state_of(opt2)))       # the round trip continues bit-equal
        for i, (q, c, b0) in enumerate(zip(params, cparams, before)):
            err = (q.detach().cpu().double() - c.detach()).abs()
            b = MARGIN * count * U * (b0 - c.detach()).abs() + 2.0 ** -23 * c.detach().abs()
            print("%s tensor %d one step after the checkpoint: max err / bound = %.3g" % (case, i, float((err / b).max())))
            assert bool((err <= b).all()), (case, i)
    finally:
        K.set_grad_sink(None)


def test_fused_sgd_device_scalars_equal_the_host_entry_point(L):
    """FusedSGD's steps (scalars through device memory) against mte_sgd_step (host scalars) from the same state, bit for bit, with a
    dampening whose 1 - dampening rounds to another float32 from the double than from the float32 value: the class forms the
    coefficient as the entry point does"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedSGD
    damp = 0.6
    assert _f(1.0 - damp) != _f(1.0 - _f(damp))
    try:
        _, values, grads = _toy_params()
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        flat = FlatParameters(params)
        opt = FusedSGD(flat, lr=3e-2, momentum=0.9, dampening=damp, weight_decay=0.01)
        n = flat.flat.numel()
        p, b = Flat(n).set(flat.flat), Flat(n).set(opt.momentum_buffer)
        for step in (1, 2, 3):
            for q, gr in zip(params, grads[step]):
                q.grad.copy_(gr)
            g_d = flat.grad.clone()
            opt.step()
            assert beq(opt.hyper.cpu(), R.sgd_hyper(3e-2, 0.9, damp, step))
            assert L.mte_sgd_step(p.ptr, g_d.data_ptr(), b.ptr, n, 3e-2, 0.9, damp, 0.01, 0, step, 1.0, _st()) == OK
            torch.cuda.synchronize()
            assert beq(p.get(), flat.flat.cpu()) and beq(b.get(), opt.momentum_buffer.cpu())
    finally:
        K.set_grad_sink(None)


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------------------------------------
def test_graphed_adamw_steps_equal_eager_steps():
    """tests/test_gpu_graph_train.py's set-up (same net, same capture path, advance() before each replay inside GraphedTrainStep) with
    FusedAdam(weight_decay=0.01, decoupled_weight_decay=True): five replayed steps follow five eager steps at that file's tolerance"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    from mindtheedge_amd.utils.graph import GraphedTrainStep
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    dev = torch.device("cuda")
    batches = [synthetic_batch(2, 64, 128, s, dev) for s in (1, 2, 3, 4, 5)]
    try:
        K.set_compute_dtype("fp32")
        K.set_grad_sink(None)
        torch.manual_seed(3)
        net = PackNetSAN01(dropout=None, version="1A").cuda()
        model = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog",
                                 supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.5)
        model.add_depth_net(net)
        model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
        model.train()
        opt = FusedAdam(FlatParameters(net.parameters()), lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)
        step = GraphedTrainStep(model, opt, batches[0])
        assert step.graphed, step.error
        torch.cuda.synchronize()
        assert opt.steps == 0
        snap = (opt.flatp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.steps)

        def restore():
            opt.flatp.flat.copy_(snap[0]); opt.exp_avg.copy_(snap[1]); opt.exp_avg_sq.copy_(snap[2]); opt.steps = snap[3]
            K.bump_weights_epoch()
            K.prefetch_weight_packs()
            K.join_side_stream()
            torch.cuda.synchronize()

        restore()
        random.seed(11)
        eager, static = [], step.batch
        for b in batches:
            flip = model.draw_flip()
            step.batch = b
            eager.append(float(step._eager(flip)["loss"].sum()))
        step.batch = static
        model._pinned_flip = None
        p_eager = opt.flatp.flat.clone()
        assert opt.steps == 5
        restore()
        random.seed(11)
        got = [float(step(b)["loss"].sum()) for b in batches]
        torch.cuda.synchronize()
        assert opt.steps == 5
        for a, b in zip(got, eager):
            assert a == pytest.approx(b, rel=5e-4), (got, eager)
        assert float((opt.flatp.flat - p_eager).abs().max()) <= 5e-3
        assert float((opt.flatp.flat - snap[0]).abs().max()) > 0 and len(set(round(x, 4) for x in got)) > 1
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


# ---- 7. the entry point ------------------------------------------------------------------------------------------------------------------------------
def _train_edges_two_steps_and_resume(tmp_path, capsys, optimizer=None):
    """train_edges.py <the AdamW YAML> --synthetic (frame size, batch and checkpoint folder set for the test, as
    tests/test_gpu_entry_points.py does for the default config; `optimizer` replaces the YAML's optimizer block): two steps, a checkpoint,
    a resume for two more.  -> the two checkpoints"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    with open(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_adamw.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["model"]["optimizer"] == {"name": "AdamW", "depth": {"lr": 0.0001, "weight_decay": 0.01}}
    if optimizer is not None:
        cfg["model"]["optimizer"] = optimizer
    cfg["datasets"]["augmentation"]["image_shape"] = [64, 128]
    cfg["datasets"]["train"]["batch_size"] = 2
    cfg["checkpoint"].update(filepath="", save_top_k=-1)
    path = os.path.join(tmp_path, "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    save = os.path.join(tmp_path, "run")

    def run(argv):
        old = sys.argv
        sys.argv = argv
        try:
            if ROOT not in sys.path:
                sys.path.insert(0, ROOT)
            importlib.import_module("train_edges").main()
        finally:
            sys.argv = old
            K.set_grad_sink(None)
            K.set_compute_dtype("bf16")

    run(["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1", "--save", save])
    assert "'steps': 2" in capsys.readouterr().out
    ckpt_path = os.path.join(save, "epoch=0.ckpt")
    ckpt = load_checkpoint(ckpt_path)
    run(["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1", "--save", save, "--resume", ckpt_path])
    ck2 = load_checkpoint(os.path.join(save, "epoch=1.ckpt"))
    assert ckpt["epoch"] == 0 and ck2["epoch"] == 1
    moved = max(float((ck2["state_dict"][k].float() - ckpt["state_dict"][k].float()).abs().max()) for k in ckpt["state_dict"])
    assert 0 < moved < float("inf")
    return ckpt, ck2, moved


def test_train_edges_adamw_yaml_two_synthetic_steps_and_resume(tmp_path, capsys):
    """the shipped AdamW YAML: a checkpoint in torch.optim.AdamW's layout, a resume whose group carries the config's weight decay"""
    ckpt, ck2, moved = _train_edges_two_steps_and_resume(tmp_path, capsys)
    assert moved < 1e-2                                        # Adam at lr 1e-4: two steps move a weight by <= ~2 lr (+ the decay)
    for ck, steps in ((ckpt, 2), (ck2, 4)):
        group = ck["optimizer"]["param_groups"][0]
        assert group["weight_decay"] == 0.01 and group["decoupled_weight_decay"] is True and group["lr"] == 0.0001
        assert {int(float(st["step"])) for st in ck["optimizer"]["state"].values()} == {steps}


def test_train_edges_sgd_with_momentum_two_synthetic_steps_and_resume(tmp_path, capsys):
    """the same run with model.optimizer = SGD with momentum: the checkpoint holds torch.optim.SGD's layout (a host momentum_buffer per
    trained tensor, no step entry), the resume reads it and the buffers go on changing"""
    block = {"name": "SGD", "depth": {"lr": 0.000001, "momentum": 0.9, "weight_decay": 0.0001}}
    ckpt, ck2, _ = _train_edges_two_steps_and_resume(tmp_path, capsys, block)
    for ck in (ckpt, ck2):
        group = ck["optimizer"]["param_groups"][0]
        assert group["momentum"] == 0.9 and group["weight_decay"] == 0.0001 and group["lr"] == 0.000001 and group["nesterov"] is False
        assert len(ck["optimizer"]["state"]) == 218
        assert all(set(st) == {"momentum_buffer"} and st["momentum_buffer"].device.type == "cpu" for st in ck["optimizer"]["state"].values())
    changed = [i for i, st in ckpt["optimizer"]["state"].items()
               if not torch.equal(st["momentum_buffer"], ck2["optimizer"]["state"][i]["momentum_buffer"])]
    assert len(changed) >= 216                                 # all but the two fusion vectors, which see no gradient without a LiDAR input
