"""GPU (-m gpu): gradient-norm clipping and the non-finite step guard of csrc/optim.hip -- mte_grad_norm_clip against the float64
statement of tests/clip_ref.py (pinned to torch.nn.utils.clip_grad_norm_ by tests/test_grad_clip_cpu.py), the `_ctl_dev` step entry points
against their plain forms and tests/optim_ref.py, and FusedAdam / FusedSGD with ``clip_grad_norm`` / ``skip_nonfinite`` against
clip_grad_norm_ + torch.optim in float64, through a HIP-graph replay, two ranks and the training entry point.

Bounds.  The norm kernel adds exact fp64 squares: with integer gradients |g| <= 3 every partial sum is an integer below 2^53 and the sum S
is exact whatever the order; with random gradients S is a sum of n non-negative terms, within n * 2^-53 relative of the reference's (which
adds in another order).  ctl[2] = float32(norm) and ctl[0] = float32(coef) are roundings of fp64 values that differ from the reference's by
that much, so they sit within one fp32 ulp of the reference's rounded values.  The step kernels keep the bounds
tests/test_gpu_optimizer_family.py derives for them: the clip coefficient enters as ONE fp32 multiply of the gradient scale, which the
reference takes at its float32 value.  Each check prints measured error / bound."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import clip_ref as C
import optim_ref as R
from test_gpu_optimizer_family import (HYPERS, MARGIN, SGD_VARIANTS, U, WRAP, Flat, _check, _check_p, _f, _gen, _inputs, _toy_params,
                                       adam_counts, beq, sgd_counts)

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, NU = 256, 8                                                        # the norm kernel's grid cap (NORM_CAP), 256 threads each, and NORM_UNROLL
FULL = 4 * G * 256 + 3                                                # every thread holds one vector, then a 3-element tail
TRIP2 = 4 * (G * 256 + 300) + 3                                       # 300 vectors more: a second trip
UNROLL = 4 * (NU * G * 256 + 300) + 3                                 # NORM_UNROLL trips in one unrolled pass, then one more
INF = float("inf")


@pytest.fixture(scope="module")
def L():
    """the raw ctypes handle: entry points return their codes instead of raising"""
    from mindtheedge_amd._lib import lib
    return lib.load()


def _st():
    from mindtheedge_amd import kernels as K
    return K._stream()


class Work:
    """the norm launch's work buffer, zeroed once, followed by guard doubles"""
    SENT = -12345.5

    def __init__(self, L, n):
        self.bytes = int(L.mte_grad_norm_work_bytes(n))
        assert self.bytes == 16 + 8 * min(G, max(1, ((n >> 2) + 255) // 256))
        self.words = (self.bytes + 7) // 8
        self.t = torch.zeros(self.words + 8, dtype=torch.float64, device="cuda")
        self.t[self.words:] = self.SENT
        self.ptr = self.t.data_ptr()

    def S(self):
        return float(self.t[0])

    def guard_ok(self):
        ticket = int(self.t[1:2].view(torch.int32)[0])
        return bool((self.t[self.words:] == self.SENT).all()) and ticket == 0


def _ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


def _close32(got, ref64):
    """got (a float32 the kernel stored) within one fp32 ulp of float32(ref64); NaN and inf must match exactly"""
    ref = np.float32(ref64)
    if not np.isfinite(ref):
        return (np.isnan(ref) and np.isnan(got)) or float(got) == float(ref)
    return abs(float(got) - float(ref)) <= _ulp32(ref)


def _norm_call(L, g_cpu, gscale, max_norm, skip=0, ctl0=None, work=None, exact=False):
    """one mte_grad_norm_clip over g_cpu held in a guarded buffer; checks g, the guards and the ticket, and S / ctl against clip_ref.
    -> (ctl as numpy float32[4], S)"""
    n = g_cpu.numel()
    g = Flat(n).set(g_cpu)
    before = g.raw.clone()
    ctl = Flat(4).set(torch.zeros(4) if ctl0 is None else torch.as_tensor(ctl0, dtype=torch.float32))
    prev = ctl.get().numpy().copy()
    work = work or Work(L, n)
    assert L.mte_grad_norm_clip(g.ptr, n, gscale, max_norm, skip, work.ptr, ctl.ptr, _st()) == OK
    torch.cuda.synchronize()
    assert torch.equal(g.raw, before), "the gradient or its guard changed"
    assert ctl.guard_ok() and work.guard_ok()
    got, S = ctl.get().numpy(), work.S()
    ref = C.grad_norm_clip(g_cpu, gscale, max_norm)
    want = C.ctl(g_cpu, gscale, max_norm, skip, float(prev[3]))
    if np.isfinite(ref["S"]):
        err = abs(S - ref["S"])
        bound = 0.0 if exact else n * 2.0 ** -53 * ref["S"]
        print("norm n=%d gscale=%g max_norm=%g: S err %.3g (bound %.3g); norm %.9g coef %.9g" % (n, gscale, max_norm, err, bound, got[2], got[0]))
        assert err <= bound
    else:
        assert (np.isnan(ref["S"]) and np.isnan(S)) or S == ref["S"]
    assert _close32(got[2], ref["norm"]) and _close32(got[0], ref["coef"]), (got, ref)
    assert got[1] == want[1] and got[3] == want[3], (got, want)
    return got, S


# ---- 1. the norm entry point against clip_ref ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1027, FULL, TRIP2, UNROLL])
def test_grad_norm_clip_against_the_reference(L, n, gscale):
    assert (FULL >> 2) == G * 256 and (TRIP2 >> 2) > G * 256 and (UNROLL >> 2) > NU * G * 256
    gen = _gen(7000 + n % 9973)
    ints = torch.randint(-3, 4, (n,), generator=gen).float()
    ints[0] = 3.0                                                     # never all zero
    rnd = torch.randn(n, generator=gen) * 0.3
    for grad, exact in ((ints, True), (rnd, False)):
        norm = C.grad_norm_clip(grad, gscale, INF)["norm"]
        for max_norm in (0.5 * norm, 2.0 * norm, INF):               # below, above, infinite
            got, _ = _norm_call(L, grad, gscale, max_norm, exact=exact)
            assert (got[0] < 1.0) == (max_norm < norm)
            if max_norm == INF:
                assert got[0] == 1.0
    torch.cuda.empty_cache()


# ---- 2. coverage by position -----------------------------------------------------------------------------------------------------------------------
def _positions(n):
    n4 = n >> 2
    pos = {0, 4 * n4 - 1, n - 3, n - 2, n - 1, 4 * 256, 4 * G * 256 - 1}         # first; last vector element; the tail; workgroup 1's first; trip 1's last
    if n == UNROLL:
        pos |= {4 * (2 * G * 256 + 5) + 1, 4 * (NU - 1) * G * 256, 4 * NU * G * 256}   # inside the unrolled pass: its third and its last trip; the first element after it
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("n", [TRIP2, UNROLL])
def test_every_position_is_counted_once(L, n):
    """a zero gradient with one element set to 3.0: S == 9.0 exactly wherever it sits -- the last element of the second trip (= the last
    vector element), the tail, the first element of workgroup 1 among them"""
    work = Work(L, n)
    g = torch.zeros(n)
    for p in _positions(n):
        g[p] = 3.0
        got, S = _norm_call(L, g, 1.0, INF, work=work, exact=True)
        assert S == 9.0 and got[2] == 3.0 and got[0] == 1.0, (p, S, got)
        g[p] = 0.0


@pytest.mark.parametrize("bad", [INF, float("nan")], ids=["inf", "nan"])
def test_a_non_finite_element_is_seen_at_every_position(L, bad):
    """skip_nonfinite = 1: ctl[1] == 1 and ctl[3] counts up by one per call; skip_nonfinite = 0: ctl[1] == 0 and ctl[0] is 0 (inf) or
    NaN, as the reference; a finite call in between leaves the count alone"""
    n = TRIP2
    work = Work(L, n)
    g = torch.ones(n)
    count = 0.0
    for p in _positions(n):
        g[p] = bad
        got, _ = _norm_call(L, g, 0.25, 5.0, skip=1, ctl0=[0.5, 0.0, 0.0, count], work=work)
        count += 1.0
        assert got[1] == 1.0 and got[3] == count
        got, _ = _norm_call(L, g, 0.25, 5.0, skip=0, ctl0=[0.5, 1.0, 0.0, count], work=work)
        assert got[1] == 0.0 and got[3] == count and (got[0] == 0.0 if bad == INF else np.isnan(got[0]))
        g[p] = 1.0
    got, _ = _norm_call(L, g, 0.25, 5.0, skip=1, ctl0=[0.5, 1.0, 0.0, count], work=work)
    assert got[1] == 0.0 and got[3] == count


# ---- 3. repeat and replay ------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_repeats_and_replays_bit_equal(L):
    """the same call twice on one work buffer, then three replays of a captured graph of it: ctl and S come out bit-equal every time, so
    the ticket went back to zero and the sum has one order"""
    n = TRIP2
    gen = _gen(7100)
    g = Flat(n).set(torch.randn(n, generator=gen))
    work, ctl = Work(L, n), Flat(4).set(torch.zeros(4))

    def call():
        assert L.mte_grad_norm_clip(g.ptr, n, 0.25, 3.0, 1, work.ptr, ctl.ptr, _st()) == OK

    def result():
        torch.cuda.synchronize()
        assert work.guard_ok() and ctl.guard_ok()
        out = (ctl.raw.clone(), work.t[:1].clone().view(torch.int64))
        ctl.t[:3] = -1.0                                              # the next run has to write them again
        work.t[0] = -1.0
        return out

    call()
    first = result()
    call()
    assert all(torch.equal(a, b) for a, b in zip(first, result()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    result()                                                          # (a capture runs nothing)
    for _ in range(3):
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(first, result()))
    ref = C.grad_norm_clip(g.get(), 0.25, 3.0)
    assert _close32(first[0].view(torch.float32)[2].item(), ref["norm"]) and first[0].view(torch.float32)[0].item() < 1.0


def test_norm_argument_errors(L):
    g, ctl, work = Flat(8).set(torch.ones(8)), Flat(4).set(torch.zeros(4)), Work(L, 8)
    assert L.mte_grad_norm_work_bytes(0) == 0 and L.mte_grad_norm_work_bytes(-5) == 0
    assert L.mte_grad_norm_clip(None, 8, 1.0, 1.0, 0, work.ptr, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 8, 1.0, 1.0, 0, None, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 8, 1.0, 1.0, 0, work.ptr, None, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 0, 1.0, 1.0, 0, work.ptr, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 8, 1.0, 0.0, 0, work.ptr, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 8, 1.0, -1.0, 0, work.ptr, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_grad_norm_clip(g.ptr, 8, 1.0, float("nan"), 0, work.ptr, ctl.ptr, _st()) == ERR_ARG
    torch.cuda.synchronize()
    assert beq(ctl.get(), torch.zeros(4)) and ctl.guard_ok() and work.guard_ok() and work.S() == 0.0


# ---- 4. the step entry points with a ctl the test writes itself ----------------------------------------------------------------------------------------
ADAM_WD = [("none", 0.0, 0), ("l2", None, 0), ("decoupled", None, 1)]           # None: the HYPERS entry's weight decay
SIZES = [1, 2, 3, 4, 5, 6, 7, 1027, WRAP]                                        # WRAP: past the step kernels' own grid cap


def _ctl(coef, flag):
    return Flat(4).set(torch.tensor([coef, flag, 123.0, 7.0]))


def _adam_three_ways(L, n, hyper, wd, decoupled, step, p0, g, m0, v0, tag):
    """from one fp32 state: the plain device step; the ctl step with {1, 0} (bit-equal to it); with {0.37, 0} (within the family's bounds
    of optim_ref at gscale_eff = float32(gscale * 0.37)); with {0.37, 1} and {NaN, 1} (nothing changes)"""
    lr, b1, b2, eps, gscale, _ = hyper
    g_d, hyp = g.cuda(), R.adam_hyper(lr, b1, b2, step).cuda()
    plain = [Flat(n).set(t) for t in (p0, m0, v0)]
    assert L.mte_adamw_step_dev(plain[0].ptr, g_d.data_ptr(), plain[1].ptr, plain[2].ptr, n, hyp.data_ptr(), b1, b2, eps, wd, decoupled, gscale, _st()) == OK

    def ctl_step(coef, flag):
        st, ctl = [Flat(n).set(t) for t in (p0, m0, v0)], _ctl(coef, flag)
        assert L.mte_adamw_step_ctl_dev(st[0].ptr, g_d.data_ptr(), st[1].ptr, st[2].ptr, n, hyp.data_ptr(), b1, b2, eps, wd, decoupled, gscale,
                                        ctl.ptr, _st()) == OK
        torch.cuda.synchronize()
        assert all(t.guard_ok() for t in st) and ctl.guard_ok() and beq(ctl.get(), torch.tensor([coef, flag, 123.0, 7.0]))
        return st

    one = ctl_step(1.0, 0.0)
    assert all(torch.equal(a.raw, b.raw) for a, b in zip(plain, one)), tag
    clipped = ctl_step(0.37, 0.0)
    eff = float(np.float32(gscale) * np.float32(0.37))
    pr, mr, vr, dp = R.adam_step(p0, g, m0, v0, lr, b1, b2, eps, step, eff, wd, bool(decoupled))
    c = adam_counts(wd, decoupled)
    _check(tag, "m", clipped[1].get(), mr, c["m"])
    _check(tag, "v", clipped[2].get(), vr, c["v"])
    _check_p(tag, clipped[0].get(), pr, dp, c["p"])
    for coef in (0.37, float("nan")):
        kept = ctl_step(coef, 1.0)
        assert all(beq(k.get(), t) for k, t in zip(kept, (p0, m0, v0))), tag
    assert beq(g_d.cpu(), g)


@pytest.mark.parametrize("wdcase", ADAM_WD, ids=[w[0] for w in ADAM_WD])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_step_ctl(L, n, wdcase):
    name, wd, decoupled = wdcase
    for hi, hyper in enumerate(HYPERS if n <= 1027 else HYPERS[1:]):
        p, grad, m, v = _inputs(n, _gen(7200 + 10 * (n % 997) + hi), True)
        _adam_three_ways(L, n, hyper, hyper[5] if wd is None else wd, decoupled, 1000, p, grad(), m, v, "adam_ctl %s n=%d" % (name, n))
    if n > 1027:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("variant", SGD_VARIANTS, ids=[s[0] for s in SGD_VARIANTS])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_step_ctl(L, n, variant):
    name, mu, damp, nesterov, with_wd = variant
    lr, gscale, wd = 3e-2, 1.0 / 3.0, (0.1 if with_wd else 0.0)
    p0, grad, b0, _ = _inputs(n, _gen(7300 + 10 * (n % 997)), True)
    g = grad()
    g_d, step = g.cuda(), 1000
    hyp = R.sgd_hyper(lr, mu, damp, step).cuda()
    tag = "sgd_ctl %s n=%d" % (name, n)

    def state():
        return Flat(n).set(p0), (Flat(n).set(b0) if mu else None)

    p, b = state()
    assert L.mte_sgd_step_dev(p.ptr, g_d.data_ptr(), b.ptr if mu else None, n, hyp.data_ptr(), mu, wd, nesterov, gscale, _st()) == OK

    def ctl_step(coef, flag):
        q, c, ctl = *state(), _ctl(coef, flag)
        assert L.mte_sgd_step_ctl_dev(q.ptr, g_d.data_ptr(), c.ptr if mu else None, n, hyp.data_ptr(), mu, wd, nesterov, gscale, ctl.ptr, _st()) == OK
        torch.cuda.synchronize()
        assert q.guard_ok() and (c is None or c.guard_ok()) and ctl.guard_ok()
        return q, c

    q, c = ctl_step(1.0, 0.0)
    assert torch.equal(p.raw, q.raw) and (not mu or torch.equal(b.raw, c.raw)), tag
    q, c = ctl_step(0.37, 0.0)
    eff = float(np.float32(gscale) * np.float32(0.37))
    pr, br, dp = R.sgd_step(p0, g, b0 if mu else None, lr, mu, damp, wd, bool(nesterov), step, eff)
    cnt = sgd_counts(mu, nesterov, wd)
    if mu:
        _check(tag, "buf", c.get(), br, cnt["buf"])
    _check_p(tag, q.get(), pr, dp, cnt["p"])
    for coef in (0.37, float("nan")):
        q, c = ctl_step(coef, 1.0)
        assert beq(q.get(), p0) and (not mu or beq(c.get(), b0)), tag
    assert beq(g_d.cpu(), g)
    if n > 1027:
        torch.cuda.empty_cache()


def test_a_null_ctl_is_an_argument_error(L):
    p, m, v = (Flat(8).set(torch.ones(8)) for _ in range(3))
    g = torch.ones(8).cuda()
    hyp = R.adam_hyper(1e-4, 0.9, 0.999, 1).cuda()
    ctl = _ctl(1.0, 0.0)
    assert L.mte_adamw_step_ctl_dev(p.ptr, g.data_ptr(), m.ptr, v.ptr, 8, hyp.data_ptr(), 0.9, 0.999, 1e-8, 0.01, 1, 1.0, None, _st()) == ERR_ARG
    assert L.mte_adamw_step_ctl_dev(p.ptr, g.data_ptr(), m.ptr, v.ptr, 0, hyp.data_ptr(), 0.9, 0.999, 1e-8, 0.01, 1, 1.0, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_adamw_step_ctl_dev(p.ptr, g.data_ptr(), m.ptr, v.ptr, 8, None, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_sgd_step_ctl_dev(p.ptr, g.data_ptr(), m.ptr, 8, hyp.data_ptr(), 0.9, 0.0, 0, 1.0, None, _st()) == ERR_ARG
    assert L.mte_sgd_step_ctl_dev(p.ptr, g.data_ptr(), None, 8, hyp.data_ptr(), 0.9, 0.0, 0, 1.0, ctl.ptr, _st()) == ERR_ARG
    assert L.mte_sgd_step_ctl_dev(p.ptr, g.data_ptr(), m.ptr, 8, hyp.data_ptr(), 0.0, 0.0, 1, 1.0, ctl.ptr, _st()) == ERR_ARG
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert beq(t.get(), torch.ones(8)) and t.guard_ok()


# ---- 5. the classes against clip_grad_norm_ + torch.optim ----------------------------------------------------------------------------------------------
B1, B2, EPS, WD, MU, LR = _f(0.9), _f(0.999), _f(1e-8), _f(0.01), _f(0.9), 2.0 ** -6
MAX_NORM = 5.0
FACTORS = [0.5, 2.0, 0.5, 3.0, 0.25]                                  # the toy gradients' norm is about 5.9: steps 2 and 4 clip
CLIP_CASES = {
    "adam": ("adam", dict(lr=LR, betas=(B1, B2), eps=EPS), torch.optim.Adam, dict(lr=LR, betas=(B1, B2), eps=EPS),
             adam_counts(False, False)["p"]),
    "adamw": ("adam", dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, decoupled_weight_decay=True), torch.optim.AdamW,
              dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD), adam_counts(True, True)["p"]),
    "sgd_momentum": ("sgd", dict(lr=LR, momentum=MU), torch.optim.SGD, dict(lr=LR, momentum=MU), sgd_counts(MU, False, False)["p"]),
}


def _fused(kind, values, kwargs):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
    return params, (FusedAdam if kind == "adam" else FusedSGD)(FlatParameters(params), **kwargs)


def _state_of(opt):
    return [opt.flatp.flat.clone()] + [b.clone() for _, b in opt.state_buffers()]


@pytest.mark.parametrize("case", sorted(CLIP_CASES))
def test_clipped_classes_follow_torch_under_a_schedule(case):
    """Five steps with StepLR(step_size=2, gamma=0.5) in between and clip_grad_norm = 5, against clip_grad_norm_ + the torch class in
    float64 on CPU copies: per parameter within the sum of the five single-step bounds of
    test_classes_follow_torch_under_a_schedule_and_through_a_checkpoint; grad_stats()['grad_norm'] against the norm torch returns, per
    step (a float32 rounding of an fp64 norm: 2^-23 relative)"""
    from mindtheedge_amd import kernels as K
    kind, kwargs, tcls, tkwargs, count = CLIP_CASES[case]
    try:
        _, values, grads = _toy_params()
        params, opt = _fused(kind, values, dict(kwargs, clip_grad_norm=MAX_NORM))
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        tparams = [torch.nn.Parameter(v.double().clone()) for v in values]
        topt = tcls([{'params': tparams, 'name': 'Depth'}], **tkwargs)
        tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=2, gamma=0.5)
        bounds = [torch.zeros_like(t.data) for t in tparams]
        clipped = []
        for step in range(5):
            for q, t, gr in zip(params, tparams, grads[step]):
                q.grad.copy_(gr * FACTORS[step])
                t.grad = (gr * FACTORS[step]).double()
            before = [t.detach().clone() for t in tparams]
            total = float(torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM))
            opt.step()
            topt.step()
            sched.step()
            tsched.step()
            stats = opt.grad_stats()
            print("%s step %d: norm %.9g (torch %.9g) coef %.9g" % (case, step + 1, stats['grad_norm'], total, stats['clip_coef']))
            assert abs(stats['grad_norm'] - total) <= 2.0 ** -23 * total
            assert (stats['clip_coef'] < 1.0) == (total > MAX_NORM) and stats['skipped'] is False and stats['skipped_steps'] == 0
            clipped.append(total > MAX_NORM)
            for b, b0, t in zip(bounds, before, tparams):
                b += MARGIN * count * U * (b0 - t.detach()).abs() + 2.0 ** -23 * t.detach().abs()
        assert clipped == [False, True, False, True, False]
        assert opt.param_groups[0]['lr'] == topt.param_groups[0]['lr'] == LR / 4 and opt.steps == 5
        for i, (q, t, b) in enumerate(zip(params, tparams, bounds)):
            err = (q.detach().cpu().double() - t.detach()).abs()
            print("%s tensor %d after 5 clipped steps: max err / bound = %.3g" % (case, i, float((err / b).max())))
            assert bool((err <= b).all()), (case, i)
        assert not any("clip" in k or "nonfinite" in k for k in opt.state_dict()['param_groups'][0])
    finally:
        K.set_grad_sink(None)


# ---- 6. a poisoned step ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kwargs", [("adam", dict(lr=LR, weight_decay=WD)), ("sgd", dict(lr=LR, momentum=MU))], ids=["adam_l2", "sgd_momentum"])
def test_a_poisoned_step_is_dropped_on_the_device(kind, kwargs):
    """five steps, the third with one NaN in its gradient.  skip_nonfinite=True: parameters and state after step 3 are bit-equal to those
    after step 2, steps 4 and 5 move finite parameters, one step is counted as skipped (the host's step count is 5 all the same).  Without
    the guard -- the default optimizer, and clipping alone -- the same sequence ends with NaN parameters."""
    from mindtheedge_amd import kernels as K

    def run(extra):
        _, values, grads = _toy_params()
        params, opt = _fused(kind, values, dict(kwargs, **extra))
        states, stats = [], []
        for step in range(5):
            for i, (q, gr) in enumerate(zip(params, grads[step])):
                q.grad.copy_(gr)
                if step == 2 and i == 1:
                    q.grad.view(-1)[17] = float("nan")
            opt.step()
            states.append(_state_of(opt))
            stats.append(opt.grad_stats() if extra else None)
        torch.cuda.synchronize()
        return opt, states, stats

    try:
        opt, states, stats = run(dict(skip_nonfinite=True))
        assert all(torch.equal(a, b) for a, b in zip(states[1], states[2]))
        assert not any(torch.equal(a, b) for a, b in zip(states[0], states[1]))
        for a, b in ((2, 3), (3, 4)):
            assert not torch.equal(states[a][0], states[b][0])
        assert all(bool(torch.isfinite(t).all()) for t in states[4])
        assert [s['skipped'] for s in stats] == [False, False, True, False, False]
        assert [s['skipped_steps'] for s in stats] == [0, 0, 1, 1, 1] and opt.steps == 5
        assert all(s['clip_coef'] == 1.0 for i, s in enumerate(stats) if i != 2) and np.isnan(stats[2]['grad_norm'])
        K.set_grad_sink(None)
        for extra in ({}, dict(clip_grad_norm=1e6)):
            _, states, _ = run(extra)
            assert bool(torch.isnan(states[4][0]).any()), extra
            K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


# ---- 7. defaults ------------------------------------------------------------------------------------------------------------------------------------
def test_the_default_step_launches_nothing_new_and_the_ctl_path_changes_no_arithmetic(L, monkeypatch):
    """a default FusedAdam / FusedSGD has no `ctl`, and its step calls none of the new entry points; the same steps with the guard on
    (finite gradients, coefficient exactly 1) give bit-equal parameters and state"""
    from mindtheedge_amd import kernels as K
    try:
        K.lib.load()
        for kind, kwargs in (("adam", dict(lr=LR)), ("adam", dict(lr=LR, weight_decay=WD, decoupled_weight_decay=True)),
                             ("sgd", dict(lr=LR, momentum=MU, weight_decay=WD))):
            _, values, grads = _toy_params()
            with monkeypatch.context() as mp_:
                for name in ("mte_grad_norm_clip", "mte_adamw_step_ctl_dev", "mte_sgd_step_ctl_dev", "mte_grad_norm_work_bytes") + \
                        (("mte_adamw_step_dev",) if kwargs.get("weight_decay", 0.0) == 0.0 else ()):
                    def never(*a, _name=name):
                        raise AssertionError("the default step must not call " + _name)
                    mp_.setitem(K.lib.__dict__, name, never)
                params, opt = _fused(kind, values, kwargs)
                assert not hasattr(opt, "ctl") and not hasattr(opt, "_norm_work") and opt.clip_grad_norm == 0.0 and opt.skip_nonfinite is False
                for step in range(3):
                    for q, gr in zip(params, grads[step]):
                        q.grad.copy_(gr)
                    opt.step()
                torch.cuda.synchronize()
                want = _state_of(opt)
            K.set_grad_sink(None)
            params, opt = _fused(kind, values, dict(kwargs, skip_nonfinite=True))
            for step in range(3):
                for q, gr in zip(params, grads[step]):
                    q.grad.copy_(gr)
                opt.step()
                assert opt.grad_stats()['clip_coef'] == 1.0 and opt.grad_stats()['grad_norm'] > 0.0
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(want, _state_of(opt))), (kind, kwargs)
            K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


# ---- 8. graph replay ---------------------------------------------------------------------------------------------------------------------------------
def test_graphed_clipped_adamw_steps_equal_eager_steps_bit_for_bit():
    """the two launches of a clipped step (norm, then mte_adamw_step_ctl_dev) captured once and replayed five times, advance() before each
    replay as GraphedTrainStep does, against five eager step() calls from the same state on the same gradients: parameters, moments and
    ctl bit-equal after every step, with steps that clip and steps that do not, and one that is skipped"""
    from mindtheedge_amd import kernels as K
    try:
        _, values, grads = _toy_params()
        kwargs = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, decoupled_weight_decay=True, clip_grad_norm=MAX_NORM, skip_nonfinite=True)
        params, opt = _fused("adam", values, kwargs)
        flat = opt.flatp

        def set_grads(step):
            for i, (q, gr) in enumerate(zip(params, grads[step])):
                q.grad.copy_(gr * FACTORS[step])
                if step == 2 and i == 3:
                    q.grad.view(-1)[5] = float("inf")

        snap = (_state_of(opt), opt.steps)
        eager = []
        for step in range(5):
            set_grads(step)
            opt.step()
            eager.append(_state_of(opt) + [opt.ctl.clone()])
        torch.cuda.synchronize()
        assert [bool(e[-1][1]) for e in eager] == [False, False, True, False, False] and float(eager[1][-1][0]) < 1.0 == float(eager[0][-1][0])
        for b, v in zip([flat.flat] + [b for _, b in opt.state_buffers()], snap[0]):
            b.copy_(v)
        opt.steps = snap[1]
        opt.ctl.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stream = torch.cuda.current_stream().cuda_stream
            opt._norm_clip(K, 1.0, stream)
            opt._launch_ctl(K, opt.param_groups[0], 1.0, stream)
        for step in range(5):
            set_grads(step)
            opt.advance()
            graph.replay()
            torch.cuda.synchronize()
            got = _state_of(opt) + [opt.ctl.clone()]
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, eager[step])), step
        assert opt.steps == 5 and opt.grad_stats()['skipped_steps'] == 1
    finally:
        K.set_grad_sink(None)


def test_graphed_clipped_training_steps_follow_eager_steps():
    """test_graphed_adamw_steps_equal_eager_steps's set-up with clip_grad_norm and the guard on: the whole training step (backward's
    atomics included, hence that test's tolerances) captured by GraphedTrainStep with the norm launch and the ctl step inside; the last
    replay's ctl holds a finite norm and the coefficient that belongs to it"""
    import random
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
        opt = FusedAdam(FlatParameters(net.parameters()), lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, clip_grad_norm=1.0,
                        skip_nonfinite=True)
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
        p_eager, stats_eager = opt.flatp.flat.clone(), opt.grad_stats()
        restore()
        random.seed(11)
        got = [float(step(b)["loss"].sum()) for b in batches]
        torch.cuda.synchronize()
        stats = opt.grad_stats()
        print("graphed clipped steps: eager %s, replayed %s" % (stats_eager, stats))
        assert opt.steps == 5 and stats['skipped_steps'] == 0
        for st in (stats, stats_eager):
            assert np.isfinite(st['grad_norm']) and st['grad_norm'] > 0.0 and st['skipped'] is False
            assert st['clip_coef'] == pytest.approx(min(1.0, 1.0 / (st['grad_norm'] + 1e-6)), rel=1e-6)
        for a, b in zip(got, eager):
            assert a == pytest.approx(b, rel=5e-4), (got, eager)
        assert float((opt.flatp.flat - p_eager).abs().max()) <= 5e-3
        assert float((opt.flatp.flat - snap[0]).abs().max()) > 0 and len(set(round(x, 4) for x in got)) > 1
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


# ---- 9. two ranks ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    """as tests/test_gpu_data_parallel.py: both ranks on cuda:0, gloo transport.  Different gradients per rank, clipping on, two steps."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        from mindtheedge_amd.trainers.data_parallel import FlatParameters, BucketedAllReduce, FusedAdam
        torch.cuda.set_device(0)
        _, values, grads = _toy_params()
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        flat = FlatParameters(params)
        red = BucketedAllReduce(flat)
        assert red.active and red.world == 2
        opt = FusedAdam(flat, lr=LR, reducer=red, clip_grad_norm=2.0, skip_nonfinite=True)
        msgs = []
        for step in range(2):
            opt.zero_grad()
            for q_, gr in zip(params, grads[2 * step + rank]):
                q_.grad.copy_(gr * (3.0 if step else 0.25))              # step 1 below max_norm, step 2 above
            local = flat.grad.cpu()
            opt.step()
            torch.cuda.synchronize()
            both = [torch.zeros_like(local) for _ in range(world)]
            dist.all_gather(both, local)
            summed = both[0] + both[1]
            if not torch.equal(flat.grad.cpu().view(torch.int32), summed.view(torch.int32)):
                msgs.append("step %d: the gradient buffer is not the sum of the ranks' gradients" % step)
            ref = C.grad_norm_clip(summed, 0.5, 2.0)                    # the averaged gradient: gscale = 1/world over the summed buffer
            ctl = opt.ctl.cpu()
            if not (_close32(float(ctl[2]), ref["norm"]) and _close32(float(ctl[0]), ref["coef"]) and float(ctl[1]) == 0.0):
                msgs.append("step %d: ctl %s, reference %s" % (step, ctl.tolist(), ref))
            if (ref["coef"] < 1.0) != bool(step):
                msgs.append("step %d: coefficient %g" % (step, ref["coef"]))
            mine = torch.cat([ctl, flat.flat.cpu()]).view(torch.int32)
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            if not torch.equal(every[0], every[1]):
                msgs.append("step %d: ctl or parameters differ between the ranks" % step)
        q.put((rank, "ok" if not msgs else "; ".join(msgs)))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_form_the_same_ctl_and_parameters():
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
    assert all(r[1] == "ok" for r in res), res


# ---- 10. the entry point -----------------------------------------------------------------------------------------------------------------------------
def _train_edges(tmp_path, capsys, yaml_name, resume):
    """train_edges.py <yaml> --synthetic (frame size, batch, checkpoint folder and a log line per step set for the test): two steps, and
    with `resume` a checkpoint and two more.  -> captured output"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    with open(os.path.join(ROOT, "configs", yaml_name)) as f:
        cfg = yaml.safe_load(f)
    cfg["datasets"]["augmentation"]["image_shape"] = [64, 128]
    cfg["datasets"]["train"]["batch_size"] = 2
    cfg["checkpoint"].update(filepath="", save_top_k=-1)
    cfg["arch"]["log_every"] = 1
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
    if resume:
        run(["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1", "--save", save, "--resume", os.path.join(save, "epoch=0.ckpt")])
    return capsys.readouterr().out, save


def test_train_edges_clip_yaml_logs_the_gradient_norm_and_resumes(tmp_path, capsys):
    import re
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    out, save = _train_edges(tmp_path, capsys, "train_packnet_san_kitti_with_edges_clip.yaml", True)
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 4
    for l in lines:
        assert re.fullmatch(r"step \d+ \| Avg\. \S+ \| Sup\. \S+ \| Edge RGB \S+ \| Grad norm \d+\.\d{4} \| Skipped 0", l), l
    assert out.count("'avg_grad_norm': ") == 2 and out.count("'skipped_steps': 0") == 2 and out.count("'steps': 2") == 2
    ck, ck2 = load_checkpoint(os.path.join(save, "epoch=0.ckpt")), load_checkpoint(os.path.join(save, "epoch=1.ckpt"))
    for c, steps in ((ck, 2), (ck2, 4)):
        group = c["optimizer"]["param_groups"][0]
        assert group["weight_decay"] == 0.01 and group["decoupled_weight_decay"] is True
        assert not any("clip" in k or "nonfinite" in k for k in group)
        assert {int(float(st["step"])) for st in c["optimizer"]["state"].values()} == {steps}
    moved = max(float((ck2["state_dict"][k].float() - ck["state_dict"][k].float()).abs().max()) for k in ck["state_dict"])
    assert 0 < moved < 1e-2


def test_train_edges_default_yaml_logs_what_it_always_did(tmp_path, capsys):
    import re
    out, _ = _train_edges(tmp_path, capsys, "train_packnet_san_kitti_with_edges_adamw.yaml", False)
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 2
    for l in lines:
        assert re.fullmatch(r"step \d+ \| Avg\. \S+ \| Sup\. \S+ \| Edge RGB \S+", l), l
    assert "Grad norm" not in out and "avg_grad_norm" not in out and "skipped_steps" not in out
