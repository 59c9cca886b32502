"""GPU (-m gpu): the LAMB step of csrc/optim.hip -- mte_lamb_moments + mte_lamb_apply -- through the raw C ABI against the float64
statement of tests/lamb_ref.py (pinned to the paper's Algorithm 2 and to optim_ref.adam_step by tests/test_lamb_cpu.py), bit for bit
against mte_adamw_step_dev where the trust ratio is 1, and FusedLAMB / the lr warm-up / the entry point on top.

Buffers are tests/test_gpu_optimizer_family.py's `Flat` (guard elements past n, pre-filled with a NaN pattern), and the padding behind every
tensor holds that NaN too: after every call guards and padding are untouched, and no sum has read them (a NaN would show).

Bounds.  u = 2^-24, MARGIN = 2 and the one-sign-per-element inputs are that file's, and so is its operation count of the decoupled AdamW
update d: c_d = 9 without a decay, 11 with one (m's 3 and g', sqrt, divide, add, divide, multiply; the decay's multiply and add).  p and m
share a sign, so lrwd * p and the Adam term never cancel and relative errors add.  lr_t, wd_t are float32 by definition on both sides.
  m, v     bit-equal to what mte_adamw_step_dev (decoupled) leaves from the same inputs: the same device function on the same inputs.
  S_d      every d is within c_d u relative, its square within 2 c_d u, and all squares are positive: S_d within 2 c_d u (the fp64
           additions add numel * 2^-53, nothing at this scale).  S_p: exact squares of the inputs, fp64 additions: numel * 2^-53, the
           project's bound for the norm launch.
  trust    r = lr_t sqrt(S_p) / sqrt(S_d): sqrt(S_d) within c_d u, then q = float32(r), one rounding: c_d + 1.
  p        dp = q * d: d's c_d, q's c_d + 1, one rounding for the product: 2 c_d + 2 for an adapted tensor (c_d where q = 1 exactly:
           1 * d is exact), plus 2^-23 |p_ref| for the final subtraction, as that file holds every step.
Each check prints measured error / bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import lamb_ref as LR
import optim_ref as R
import test_gpu_optimizer_family as F
from test_gpu_optimizer_family import ERR_ARG, HYPERS, MARGIN, OK, ROOT, SENT, U, Flat, L, _f, _st, beq  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 32768                                                             # csrc/optim.hip: STAT_CHUNK
NAN = float("nan")
SCALES = [(1.0, 1.0), (0.5, 2.0), (1.5, 0.0), (2.0, 0.5)]                 # lr_mult, wd_mult: cycled over the ordinary tensors
# Layout A.  1..3-element tails, one chunk exactly, one element more, the ticket path with 2, 3 and 3 chunks (the last ragged by 5 /
# whole); then the special tensors: all-zero weights, zero gradient and state at wd = 0, two excluded tensors (one of them two chunks)
A_NUMELS = [1, 2, 3, 5, 7, 64, 1027, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 3 * CHUNK, 200, 130, 100, CHUNK + 7]
A_ZERO_P, A_ZERO_D, A_EXCLUDED = 11, 12, (13, 14)
A_TABLE = [SCALES[i % 4] + (1.0,) for i in range(11)] + [(1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (0.5, 2.0, 0.0), (1.0, 1.0, 0.0)]
B_NUMELS = [64] * 1100                                                     # 1100 chunks > the 1024-workgroup cap: the chunk loop wraps
B_TABLE = [SCALES[i % 4] + (0.0 if i % 7 == 3 else 1.0,) for i in range(1100)]


class Layout:
    def __init__(self, numels, table):
        self.numels, self.table, self.begins, self.n = list(numels), [tuple(r) for r in table], [], 0
        for m in numels:
            self.begins.append(self.n)
            self.n += (m + 63) // 64 * 64
        self.T = len(numels)
        self.inside = torch.zeros(self.n, dtype=torch.bool)
        for b, m in zip(self.begins, numels):
            self.inside[b:b + m] = True

    def sub(self, t):
        """tensor t alone, in a one-entry table over the same buffers"""
        one = Layout.__new__(Layout)
        one.numels, one.table, one.begins, one.n, one.T = [self.numels[t]], [self.table[t]], [self.begins[t]], self.n, 1
        one.inside = torch.zeros(self.n, dtype=torch.bool)
        one.inside[self.begins[t]:self.begins[t] + self.numels[t]] = True
        return one

    def with_table(self, table):
        return Layout(self.numels, table)

    def scatter(self, parts):
        """per-tensor values -> a flat host tensor whose padding is NaN"""
        host = torch.full((self.n,), NAN)
        for b, m, x in zip(self.begins, self.numels, parts):
            host[b:b + m] = x
        return host


LA, LB = Layout(A_NUMELS, A_TABLE), Layout(B_NUMELS, B_TABLE)


def _inputs(lay, seed, nonzero_state, special=True):
    """F._inputs per tensor (one sign per element for p, g, m) -> flat p, a gradient maker, m, v; layout A's special tensors on top"""
    g = F._gen(seed)
    per = [F._inputs(m, g, nonzero_state) for m in lay.numels]
    zero_p, zero_d = (A_ZERO_P, A_ZERO_D) if special and lay.numels == A_NUMELS else (None, None)

    def fix(parts, which):
        parts = [x.clone() for x in parts]
        if zero_p is not None and which == "p":
            parts[zero_p].zero_()
        if zero_d is not None and which in ("g", "m", "v"):
            parts[zero_d].zero_()
        return lay.scatter(parts)

    def grad():
        return fix([x[1]() for x in per], "g")
    return fix([x[0] for x in per], "p"), grad, fix([x[2] for x in per], "m"), fix([x[3] for x in per], "v")


class State:
    """p, g, m, v in guarded buffers, the tables on the device, a guarded zeroed work buffer, guarded trust and sums"""

    def __init__(self, L, lay, p, g, m, v):
        self.L, self.lay = L, lay
        self.p, self.g, self.m, self.v = (Flat(lay.n).set(t) for t in (p, g, m, v))
        self.begin_d = torch.tensor(lay.begins, dtype=torch.int64).cuda()
        self.numel_d = torch.tensor(lay.numels, dtype=torch.int64).cuda()
        self.table_d = torch.tensor([x for row in lay.table for x in row], dtype=torch.float32).cuda()
        nbytes = L.mte_lamb_work_bytes(lay.n, lay.T)
        assert nbytes >= 4 * lay.T + 16 * (lay.n // CHUNK + lay.T) and nbytes % 16 == 0
        self.work = Flat(nbytes // 4).set(torch.zeros(nbytes // 4))
        self.trust = Flat(lay.T).set(torch.full((lay.T,), -7.0))
        self.sums = torch.full((2 * lay.T + 8,), -7.0, dtype=torch.float64).cuda()

    def clone(self, lay=None):
        return State(self.L, lay or self.lay, self.p.get(), self.g.get(), self.m.get(), self.v.get())

    def moments(self, hyp_d, hyper, ctl=None, max_trust=0.0):
        _, b1, b2, eps, gscale, wd = hyper
        return self.L.mte_lamb_moments(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.lay.n, hyp_d.data_ptr(), b1, b2, eps, wd, gscale, max_trust,
                                       self.begin_d.data_ptr(), self.numel_d.data_ptr(), self.table_d.data_ptr(), self.lay.T, self.work.ptr,
                                       self.trust.ptr, self.sums.data_ptr(), None if ctl is None else ctl.data_ptr(), _st())

    def apply(self, hyp_d, hyper, ctl=None):
        _, _, _, eps, _, wd = hyper
        return self.L.mte_lamb_apply(self.p.ptr, self.m.ptr, self.v.ptr, self.lay.n, hyp_d.data_ptr(), eps, wd, self.begin_d.data_ptr(),
                                     self.numel_d.data_ptr(), self.table_d.data_ptr(), self.lay.T, self.trust.ptr,
                                     None if ctl is None else ctl.data_ptr(), _st())

    def step(self, hyp_d, hyper, ctl=None, max_trust=0.0):
        assert self.moments(hyp_d, hyper, ctl, max_trust) == OK
        assert self.apply(hyp_d, hyper, ctl) == OK
        return self

    def raws(self):
        return [x.raw.clone() for x in (self.p, self.m, self.v, self.trust, self.work)] + [self.sums.clone().view(torch.int64)]

    def check_untouched(self, before_g, padding_of):
        """after a call: guards, the gradient, the padding behind every tensor (p, m, v), the tickets and the ends of trust / sums"""
        torch.cuda.synchronize()
        outside = ~self.lay.inside.cuda()
        for buf, was in zip((self.p, self.m, self.v), padding_of):
            assert buf.guard_ok() and torch.equal(buf.raw[:self.lay.n][outside], was[:self.lay.n][outside])
        assert torch.equal(self.g.raw, before_g)
        assert self.work.guard_ok() and bool((self.work.raw[:self.lay.T] == 0).all())             # the tickets are back at zero
        assert self.trust.guard_ok() and bool((self.sums[2 * self.lay.T:] == -7.0).all())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _c_d(hyper, row):
    return 11 if _f(_f(hyper[5]) * _f(row[1])) != 0.0 else 9


def _run_and_check(L, lay, hyper, step, p0, g, m0, v0, fresh, max_trust=0.0):
    """one LAMB step from fp32 state against lamb_ref and (m, v) against mte_adamw_step_dev; -> the GPU's p, m, v (padding NaN)"""
    lr, b1, b2, eps, gscale, wd = hyper
    st = State(L, lay, p0, g, m0, v0)
    pad = [x.raw.clone() for x in (st.p, st.m, st.v)]
    g_raw = st.g.raw.clone()
    hyp = R.adam_hyper(lr, b1, b2, step).cuda()
    st.step(hyp, hyper, None, max_trust)
    st.check_untouched(g_raw, pad)
    # m, v: what the decoupled AdamW step leaves from the same inputs, bit for bit at every tensor element
    am = [Flat(lay.n).set(t) for t in (p0, m0, v0)]
    assert L.mte_adamw_step_dev(am[0].ptr, st.g.ptr, am[1].ptr, am[2].ptr, lay.n, hyp.data_ptr(), b1, b2, eps, wd, 1, gscale, _st()) == OK
    torch.cuda.synchronize()
    inside = lay.inside
    pg, mg, vg = st.p.get(), st.m.get(), st.v.get()
    assert beq(mg[inside], am[1].get()[inside]) and beq(vg[inside], am[2].get()[inside])
    z = lambda t: torch.where(inside, t, torch.zeros_like(t))                      # the reference never looks at the padding
    pr, _, _, dp, trust, sums = LR.lamb_step(z(p0), z(g), z(m0), z(v0), lr, b1, b2, eps, step, gscale, wd, lay.begins, lay.numels, lay.table,
                                             max_trust=max_trust)
    got_q = st.trust.get().double()
    got_s = st.sums[:2 * lay.T].view(-1, 2).cpu()
    worst = {"p": 0.0, "trust": 0.0, "S_d": 0.0, "S_p": 0.0}
    for t, (b, m, row) in enumerate(zip(lay.begins, lay.numels, lay.table)):
        c_d = _c_d(hyper, row)
        count = 2 * c_d + 2 if trust[t] != 1.0 else c_d
        sl = slice(b, b + m)
        err = (pg[sl].double() - pr[sl]).abs()
        bound = MARGIN * count * U * dp[sl].abs() + 2.0 ** -23 * pr[sl].abs()
        worst["p"] = max(worst["p"], float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), ("p", t, m)
        qb = MARGIN * (c_d + 1) * U * abs(trust[t])
        worst["trust"] = max(worst["trust"], abs(float(got_q[t]) - trust[t]) / qb)
        assert abs(float(got_q[t]) - trust[t]) <= qb, ("trust", t, float(got_q[t]), trust[t])
        for col, name, sb in ((0, "S_p", m * 2.0 ** -53 * sums[t][0]), (1, "S_d", MARGIN * 2 * c_d * U * sums[t][1])):
            e = abs(float(got_s[t, col]) - sums[t][col])
            worst[name] = max(worst[name], e / sb if sb > 0 else (0.0 if e == 0 else float("inf")))
            assert e <= sb, (name, t, float(got_s[t, col]), sums[t][col])
    print("lamb T=%d step=%d lr=%g: max err / bound  p %.3g  trust %.3g  S_d %.3g  S_p %.3g"
          % (lay.T, step, lr, worst["p"], worst["trust"], worst["S_d"], worst["S_p"]))
    one = _f(max_trust) if 0.0 < max_trust < 1.0 else 1.0                 # (a cap below 1 caps the rule's 1 as well)
    for t in range(lay.T):                                               # the zero-norm rule: a zero sum is exactly zero and gives exactly 1
        for col in (0, 1):
            if sums[t][col] == 0.0:
                assert float(got_s[t, col]) == 0.0 and trust[t] == one and float(got_q[t]) == one, (t, col)
    if lay.numels == A_NUMELS:
        if fresh:                                                         # (from step 2 on the all-zero tensor has moved)
            assert sums[A_ZERO_P][0] == 0.0 and sums[A_ZERO_P][1] > 0.0
        assert sums[A_ZERO_D][1] == 0.0 and sums[A_ZERO_D][0] > 0.0       # no gradient, no state, no decay: it never moves
        assert all(float(got_q[t]) == one for t in A_EXCLUDED)
        assert sum(1 for q in trust if q != 1.0) >= 10                    # the ratios are not trivially 1
    st.ref_trust = trust
    return pg, mg, vg, st


# ---- 1. against lamb_ref ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hi", [0, 1])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_lamb_steps_against_the_reference(L, layout, hi):
    """steps 1, 2, 3 from zero state (each from the fp32 state the GPU left) and step 1000 from non-zero state; bounds: module docstring"""
    lay, hyper = (LA if layout == "A" else LB), HYPERS[hi]
    p, grad, m, v = _inputs(lay, 4000 + 10 * hi + (layout == "B"), False)
    for step in (1, 2, 3):
        p, m, v, _ = _run_and_check(L, lay, hyper, step, p, grad(), m, v, step == 1)
    p, grad, m, v = _inputs(lay, 4100 + 10 * hi + (layout == "B"), True)
    _run_and_check(L, lay, hyper, 1000, p, grad(), m, v, True)


def test_max_trust_caps_the_ratio(L):
    """layout A with a cap between the free ratios of its eleven ordinary tensors (their middle): a capped tensor's ratio is exactly
    float32(max_trust), the others keep the bits of the uncapped run, and p follows the reference with the cap"""
    hyper = HYPERS[1]
    p, grad, m, v = _inputs(LA, 4150, True)
    g = grad()
    free = State(L, LA, p, g, m, v).step(R.adam_hyper(hyper[0], hyper[1], hyper[2], 1000).cuda(), hyper)
    torch.cuda.synchronize()
    q_free = free.trust.get()
    ordered = sorted(q_free[:11].tolist())
    cap = _f(0.5 * (ordered[4] + ordered[6]))
    assert ordered[4] < cap < ordered[6]
    _, _, _, st = _run_and_check(L, LA, hyper, 1000, p, g, m, v, True, max_trust=cap)
    q_cap = st.trust.get()
    assert beq(q_cap, torch.minimum(q_free, torch.tensor(cap)))
    assert int((q_free > cap).sum()) >= 5 and int((q_free < cap).sum()) >= 5 and st.ref_trust.count(cap) == int((q_free >= cap).sum())


# ---- 2. every tensor excluded: the AdamW step bit for bit ------------------------------------------------------------------------------------------
TILED_NUMELS = [64, CHUNK, 2 * CHUNK + 64, 128]                            # multiples of 64: no padding, the tensors tile the buffer


@pytest.mark.parametrize("with_ctl", [False, True])
@pytest.mark.parametrize("with_wd", [False, True])
def test_all_excluded_is_the_adamw_step_bit_for_bit(L, with_wd, with_ctl):
    """q = 1 everywhere: p, m, v equal mte_adamw_step_dev's (with ctl = {0.5, 0}: mte_adamw_step_ctl_dev's) -- at every tensor element of
    layout A, and over the WHOLE buffer, guards included, where the tensors tile it"""
    lr, b1, b2, eps, gscale, wd = HYPERS[1]
    hyper = (lr, b1, b2, eps, gscale, wd if with_wd else 0.0)
    ctl = torch.tensor([0.5, 0.0, 3.0, 0.0]).cuda() if with_ctl else None
    hyp = R.adam_hyper(lr, b1, b2, 5).cuda()
    for lay in (LA.with_table([(1.0, 1.0, 0.0)] * LA.T), Layout(TILED_NUMELS, [(1.0, 1.0, 0.0)] * 4)):
        p0, grad, m0, v0 = _inputs(lay, 4200 + with_wd, True, special=False)
        g = grad()
        st = State(L, lay, p0, g, m0, v0)
        pad, g_raw = [x.raw.clone() for x in (st.p, st.m, st.v)], st.g.raw.clone()
        st.step(hyp, hyper, ctl)
        st.check_untouched(g_raw, pad)
        am = [Flat(lay.n).set(t) for t in (p0, m0, v0)]
        args = (am[0].ptr, st.g.ptr, am[1].ptr, am[2].ptr, lay.n, hyp.data_ptr(), b1, b2, eps, hyper[5], 1, gscale)
        assert (L.mte_adamw_step_ctl_dev(*args, ctl.data_ptr(), _st()) if with_ctl else L.mte_adamw_step_dev(*args, _st())) == OK
        torch.cuda.synchronize()
        for mine, theirs in zip((st.p, st.m, st.v), am):
            if bool(lay.inside.all()):
                assert torch.equal(mine.raw, theirs.raw)
            else:
                assert beq(mine.get()[lay.inside], theirs.get()[lay.inside])
        assert bool((st.trust.get() == 1.0).all())
        assert float((st.p.get()[lay.inside] - p0[lay.inside]).abs().max()) > 0


# ---- 3. slice independence ----------------------------------------------------------------------------------------------------------------------------
def test_every_tensor_alone_gets_the_bits_it_gets_in_the_full_table(L):
    hyper = HYPERS[1]
    hyp = R.adam_hyper(hyper[0], hyper[1], hyper[2], 1000).cuda()
    p0, grad, m0, v0 = _inputs(LA, 4300, True)
    full = State(L, LA, p0, grad(), m0, v0)
    g0 = full.g.get()
    full.step(hyp, hyper)
    torch.cuda.synchronize()
    fp, fm, fv, fq = full.p.get(), full.m.get(), full.v.get(), full.trust.get()
    for t in range(LA.T):
        one = State(L, LA.sub(t), p0, g0, m0, v0)
        pad, g_raw = [x.raw.clone() for x in (one.p, one.m, one.v)], one.g.raw.clone()
        one.step(hyp, hyper)
        one.check_untouched(g_raw, pad)                                   # every other tensor counts as padding here: untouched
        sl = slice(LA.begins[t], LA.begins[t] + LA.numels[t])
        for a, b in ((one.p.get(), fp), (one.m.get(), fm), (one.v.get(), fv)):
            assert beq(a[sl], b[sl]), t
        assert beq(one.trust.get(), fq[t:t + 1]), t
        assert torch.equal(one.sums[:2].cpu().view(torch.int64), full.sums[2 * t:2 * t + 2].cpu().view(torch.int64)), t


# ---- 4. determinism and graph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["A", "B"])
def test_two_calls_are_bit_equal_and_five_replayed_steps_equal_five_eager_steps(L, layout):
    lay, hyper = (LA if layout == "A" else LB), HYPERS[1]
    lr, b1, b2 = hyper[:3]
    p0, grad, m0, v0 = _inputs(lay, 4400 + (layout == "B"), True)
    grads = [grad() for _ in range(5)]
    hypers = [R.adam_hyper(lr * (k + 1) / 5.0, b1, b2, k + 1) for k in range(5)]          # a warm-up: hyper[0] changes every step
    a, b = (State(L, lay, p0, grads[0], m0, v0) for _ in range(2))
    h0 = hypers[0].cuda()
    a.step(h0, hyper)
    b.step(h0, hyper)
    torch.cuda.synchronize()
    assert _same(a.raws(), b.raws())
    # five eager steps ...
    eager = State(L, lay, p0, grads[0], m0, v0)
    for k in range(5):
        eager.g.set(grads[k])
        eager.step(hypers[k].cuda(), hyper)
    torch.cuda.synchronize()
    # ... and the same five from ONE captured pair: the gradient and hyper are refreshed in place before each replay
    rep = State(L, lay, p0, grads[0], m0, v0)
    warm = rep.clone()                                                    # first calls outside the capture, on buffers of its own
    warm.step(h0, hyper)
    torch.cuda.synchronize()
    hyp_d = hypers[0].clone().cuda()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rep.step(hyp_d, hyper)
    for x, t in ((rep.p, p0), (rep.m, m0), (rep.v, v0)):                  # (the capture itself ran nothing, but start from the state anyway)
        x.set(t)
    for k in range(5):
        rep.g.set(grads[k])
        hyp_d.copy_(hypers[k])
        graph.replay()
    torch.cuda.synchronize()
    assert _same(eager.raws(), rep.raws())
    assert float((eager.p.get()[lay.inside] - p0[lay.inside]).abs().max()) > 0


# ---- 5. the guard -------------------------------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_changes_nothing_and_the_next_one_is_a_fresh_one(L):
    hyper = HYPERS[1]
    hyp = R.adam_hyper(hyper[0], hyper[1], hyper[2], 7).cuda()
    p0, grad, m0, v0 = _inputs(LA, 4500, True)
    g1, g2 = grad(), grad()
    st = State(L, LA, p0, g1, m0, v0)
    st.step(hyp, hyper, torch.tensor([0.5, 0.0, 1.0, 0.0]).cuda())        # one real step first: trust, sums and records hold values
    torch.cuda.synchronize()
    before = st.raws()
    st.g.set(g2)
    st.step(hyp, hyper, torch.tensor([0.25, 1.0, NAN, 1.0]).cuda())       # ctl[1] = 1: both launches return before their first load
    torch.cuda.synchronize()
    assert _same(before, st.raws())
    st.step(hyp, hyper, torch.tensor([0.25, 0.0, 1.0, 1.0]).cuda())
    held = [before[i][:LA.n].view(torch.float32).cpu() for i in range(3)]          # p, m, v as the skipped step left them
    fresh = State(L, LA, held[0], g2, held[1], held[2])
    fresh.step(hyp, hyper, torch.tensor([0.25, 0.0, 1.0, 1.0]).cuda())
    torch.cuda.synchronize()
    a, b = st.raws(), fresh.raws()
    assert _same(a[:4], b[:4]) and torch.equal(a[5], b[5])                # p, m, v, trust, sums (the records of a used work buffer differ)
    assert not torch.equal(a[0], before[0])


def test_a_nan_gradient_without_a_ctl_reaches_only_its_own_tensor(L):
    hyper = HYPERS[1]
    hyp = R.adam_hyper(hyper[0], hyper[1], hyper[2], 7).cuda()
    p0, grad, m0, v0 = _inputs(LA, 4600, True)
    g = grad()
    clean = State(L, LA, p0, g, m0, v0).step(hyp, hyper)
    t = 9                                                                 # 2 * CHUNK + 5 elements: three chunks, the ticket path
    at = LA.begins[t] + CHUNK + 17
    gn = g.clone()
    gn[at] = NAN
    bad = State(L, LA, p0, gn, m0, v0).step(hyp, hyper)
    torch.cuda.synchronize()
    sl = slice(LA.begins[t], LA.begins[t] + LA.numels[t])
    other = LA.inside.clone()
    other[sl] = False
    for x, y in ((clean.p, bad.p), (clean.m, bad.m), (clean.v, bad.v)):
        assert beq(x.get()[other], y.get()[other])
    q_clean, q_bad = clean.trust.get(), bad.trust.get()
    assert beq(torch.cat([q_clean[:t], q_clean[t + 1:]]), torch.cat([q_bad[:t], q_bad[t + 1:]]))
    pb = bad.p.get()
    assert math.isnan(float(pb[at])) and int(torch.isnan(pb[sl]).sum()) == 1          # S_d is a NaN: r = 1, the NaN arrives through d alone
    assert float(q_bad[t]) == 1.0 and float(q_clean[t]) != 1.0 and math.isnan(float(bad.sums[2 * t + 1]))


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_a_range_that_leaves_the_buffer(L):
    hyper = HYPERS[1]
    lr, b1, b2, eps, gscale, wd = hyper
    hyp = R.adam_hyper(lr, b1, b2, 7).cuda()
    p0, grad, m0, v0 = _inputs(LA, 4700, True)
    st = State(L, LA, p0, grad(), m0, v0)
    before = st.raws()
    T_ = LA.T
    mom = [st.p.ptr, st.g.ptr, st.m.ptr, st.v.ptr, LA.n, hyp.data_ptr(), b1, b2, eps, wd, gscale, 0.0, st.begin_d.data_ptr(), st.numel_d.data_ptr(),
           st.table_d.data_ptr(), T_, st.work.ptr, st.trust.ptr, st.sums.data_ptr(), None]
    for i, bad in ([(i, None) for i in (0, 1, 2, 3, 5, 12, 13, 14, 16, 17, 18)] + [(i, mom[i] + 4) for i in (0, 1, 2, 3, 16)]
                   + [(4, 0), (4, -64), (15, 0), (15, 4097), (11, -1.0), (11, NAN), (9, -0.1)]):
        args = list(mom)
        args[i] = bad
        assert L.mte_lamb_moments(*args, _st()) == ERR_ARG, i
    app = [st.p.ptr, st.m.ptr, st.v.ptr, LA.n, hyp.data_ptr(), eps, wd, st.begin_d.data_ptr(), st.numel_d.data_ptr(), st.table_d.data_ptr(), T_,
           st.trust.ptr, None]
    for i, bad in ([(i, None) for i in (0, 1, 2, 4, 7, 8, 9, 11)] + [(i, app[i] + 4) for i in (0, 1, 2)] + [(3, 0), (10, 0), (10, 4097)]):
        args = list(app)
        args[i] = bad
        assert L.mte_lamb_apply(*args, _st()) == ERR_ARG, i
    assert L.mte_lamb_work_bytes(0, 3) == 0 and L.mte_lamb_work_bytes(64, 0) == 0 and L.mte_lamb_work_bytes(64, 4097) == 0
    torch.cuda.synchronize()
    assert _same(before, st.raws())
    # tensor 6's count reaches past n and tensor 2 begins before 0: both keep p, m, v (trust 1, sums 0); the others are as ever
    ok = st.clone().step(hyp, hyper)
    st.numel_d[6] = LA.n
    st.begin_d[2] = -64
    pad, g_raw = [x.raw.clone() for x in (st.p, st.m, st.v)], st.g.raw.clone()
    st.step(hyp, hyper)
    st.check_untouched(g_raw, pad)
    for t in range(T_):
        sl = slice(LA.begins[t], LA.begins[t] + LA.numels[t])
        for mine, was, want in ((st.p, p0, ok.p), (st.m, m0, ok.m), (st.v, v0, ok.v)):
            assert beq(mine.get()[sl], (was if t in (2, 6) else want.get())[sl]), t
        if t in (2, 6):
            assert float(st.trust.get()[t]) == 1.0 and st.sums[2 * t:2 * t + 2].tolist() == [0.0, 0.0]
        else:
            assert beq(st.trust.get()[t:t + 1], ok.trust.get()[t:t + 1])


# ---- 7. the classes ---------------------------------------------------------------------------------------------------------------------------------
B1, B2, EPS, WD, LR0 = F.B1, F.B2, F.EPS, F.WD, F.LR
SHAPES = [(3,), (5, 7), (1,), (64,), (40, 33)]
CLS_SCALES = [(1.0, 0.0), (0.5, 1.0), (1.0, 1.0), (2.0, 0.5), (1.0, 1.0)]
CLS_ADAPT = [False, True, True, False, True]


def _toy(seed, n_grads):
    g = F._gen(seed)
    signs = [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0) for s in SHAPES]
    values = [s * (torch.rand(s.shape, generator=g) + 0.5) for s in signs]
    grads = [[s * (torch.rand(s.shape, generator=g) + 0.01) for s in signs] for _ in range(n_grads)]
    return values, grads


def test_fused_lamb_follows_the_reference_under_warmup_schedule_clipping_accumulation_and_ema():
    """Six optimizer steps of two micro-batches each, StepLR(2, 0.5) in between, warmup_steps = 4, clipping on, the weight EMA on, a
    state_dict() round trip into a fresh optimizer after step 3.  Every step is held to lamb_ref from the fp32 state the optimizer
    itself held before it, at the module docstring's bounds (the gradient scale float32(gscale * clip coefficient) is the float32 value
    the reference takes, the coefficient read back from the device) -- so the six steps end at that tolerance."""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedLAMB, ema_decay_pair, warmup_factor
    kwargs = dict(lr=LR0, betas=(B1, B2), eps=EPS, weight_decay=WD, warmup_steps=4, clip_grad_norm=0.5, accumulate_grad_batches=2, ema_decay=0.9,
                  adapt=CLS_ADAPT, tensor_scales=CLS_SCALES, max_trust=0.0)
    try:
        values, grads = _toy(7, 12)
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        opt = FusedLAMB(FlatParameters(params), **kwargs)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        assert not hasattr(opt, 'seg_block_class') and hasattr(opt, 'ctl')
        for k in range(1, 7):
            flat = opt.flatp
            segs = flat.segments()
            begins, numels = [s[0] for s in segs], [s[1] for s in segs]
            table = [CLS_SCALES[s[2]] + (CLS_ADAPT[s[2]],) for s in segs]
            p0, m0, v0, e0 = flat.flat.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), flat.ema.cpu()
            for q, gr in zip(params, grads[2 * k - 2]):
                q.grad.copy_(gr)
            with opt.no_sync():
                opt.accumulate()
            for q, gr in zip(params, grads[2 * k - 1]):
                q.grad.copy_(gr)
            opt.step()
            torch.cuda.synchronize()
            lr_group = LR0 * 0.5 ** ((k - 1) // 2)
            assert opt.steps == k and opt.param_groups[0]['lr'] == lr_group
            lr_k = lr_group * warmup_factor(k, 4)
            assert beq(opt.hyper.cpu(), R.adam_hyper(lr_k, B1, B2, k)) and (k >= 4 or lr_k < lr_group)
            gsum = flat.grad.cpu()                                        # the fp32 sum of the two micro-batches, as the step consumed it
            want = torch.zeros(flat.total)
            for (b, m_, slot) in segs:
                want[b:b + m_] = (grads[2 * k - 2][slot] + grads[2 * k - 1][slot]).flatten()
            assert beq(gsum, want)
            stats = opt.grad_stats()
            norm = 0.5 * float((gsum.double() ** 2).sum()) ** 0.5
            clip = min(0.5 / (norm + 1e-6), 1.0)
            assert clip < 1.0 and abs(stats['clip_coef'] - clip) <= 2.0 ** -22 * clip and not stats['skipped']
            gs = _f(_f(0.5) * _f(stats['clip_coef']))
            pr, mr, vr, dp, trust, sums = LR.lamb_step(p0, gsum, m0, v0, lr_k, B1, B2, EPS, k, gs, WD, begins, numels, table)
            pg = flat.flat.cpu()
            worst = 0.0
            c_of = [11 if CLS_SCALES[slot][1] != 0.0 else 9 for _, _, slot in segs]
            for t, (b, m_, slot) in enumerate(segs):
                c_d = c_of[t]
                count = 2 * c_d + 2 if trust[t] != 1.0 else c_d
                sl = slice(b, b + m_)
                err = (pg[sl].double() - pr[sl]).abs()
                bound = MARGIN * count * U * dp[sl].abs() + 2.0 ** -23 * pr[sl].abs()
                worst = max(worst, float((err / bound).max()))
                assert bool((err <= bound).all()), (k, t)
                assert (trust[t] == 1.0) == (not CLS_ADAPT[slot])
            ins = flat_inside(segs, flat.total)
            F._check("lamb class step %d" % k, "m", opt.exp_avg.cpu()[ins], mr[ins], F.adam_counts(True, True)["m"])
            F._check("lamb class step %d" % k, "v", opt.exp_avg_sq.cpu()[ins], vr[ins], F.adam_counts(True, True)["v"])
            print("lamb class step %d: p max err / bound = %.3g" % (k, worst))
            # the average follows the weights the step wrote: e <- d32 * e + omd32 * p, three fp32 roundings
            d32, omd32 = ema_decay_pair(k, 0.9, True)
            e_ref = d32 * e0.double() + omd32 * pg.double()
            assert opt.ema_updates == k and bool(((flat.ema.cpu().double() - e_ref).abs() <= 3 * U * (d32 * e0.abs() + omd32 * pg.abs()).double()).all())
            # trust_ratios(): names (positional without an index space), the values the step applied, one row per trained tensor
            rows = opt.trust_ratios()
            assert [r['name'] for r in rows] == [str(i) for i in range(len(SHAPES))] and [r['adapted'] for r in rows] == CLS_ADAPT
            t_of = {slot: t for t, (_, _, slot) in enumerate(segs)}
            for slot, r in enumerate(rows):
                t = t_of[slot]
                lr_t = float(np.float32(_f(lr_k)) * np.float32(CLS_SCALES[slot][0]))
                assert abs(r['trust_ratio'] - trust[t]) <= MARGIN * (c_of[t] + 1) * U * trust[t]
                assert abs(r['weight_norm'] - sums[t][0] ** 0.5) <= segs[t][1] * 2.0 ** -53 * sums[t][0] ** 0.5   # S_p: numel * 2^-53
                assert abs(r['update_norm'] - sums[t][1] ** 0.5 / lr_t) <= MARGIN * c_of[t] * U * sums[t][1] ** 0.5 / lr_t     # sqrt(S_d): c_d
            sched.step()
            if k == 3:
                # the round trip: a fresh optimizer over copies of the weights reads the file (and the scheduler's, and the average)
                sd, ssd = opt.state_dict(), sched.state_dict()
                assert {int(float(s_['step'])) for s_ in sd['state'].values()} == {3} and 'warmup_steps' not in sd['param_groups'][0]
                params2 = [torch.nn.Parameter(q.detach().clone()) for q in params]
                K.set_grad_sink(None)
                opt2 = FusedLAMB(FlatParameters(params2), **dict(kwargs, lr=0.5))
                sched2 = torch.optim.lr_scheduler.StepLR(opt2, step_size=2, gamma=0.5)
                opt2.load_state_dict(sd)
                sched2.load_state_dict(ssd)
                opt2.flatp.ema.copy_(opt.flatp.ema)
                opt2.ema_updates = opt.ema_updates
                assert opt2.steps == 3 and all(torch.equal(a, b) for a, b in zip(F._state_of(opt), F._state_of(opt2)))
                params, opt, sched = params2, opt2, sched2                # the warm-up goes on at step 4 of 4: the count came from the file
        assert opt.param_groups[0]['lr'] == LR0 / 8
    finally:
        K.set_grad_sink(None)


def flat_inside(segs, total):
    inside = torch.zeros(total, dtype=torch.bool)
    for b, m, _ in segs:
        inside[b:b + m] = True
    return inside


def test_fused_adam_with_warmup_follows_torch_adamw_at_the_same_per_step_lr():
    """FusedAdam(decoupled, warmup_steps = 4) for six steps against torch.optim.AdamW in float64 whose lr is set to lr * min(1, k / 4)
    before step k: per parameter within the sum of the single-step AdamW bounds, as
    test_classes_follow_torch_under_a_schedule_and_through_a_checkpoint holds that class without a warm-up"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    count = F.adam_counts(True, True)["p"]
    try:
        values, grads = _toy(8, 6)
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        opt = FusedAdam(FlatParameters(params), lr=LR0, betas=(B1, B2), eps=EPS, weight_decay=WD, decoupled_weight_decay=True, warmup_steps=4)
        tparams = [torch.nn.Parameter(v.double().clone()) for v in values]
        topt = torch.optim.AdamW([{'params': tparams}], lr=LR0, betas=(B1, B2), eps=EPS, weight_decay=WD)
        bounds = [torch.zeros_like(t.data) for t in tparams]
        for k in range(1, 7):
            topt.param_groups[0]['lr'] = LR0 * min(1.0, k / 4.0)
            for q, t, gr in zip(params, tparams, grads[k - 1]):
                q.grad.copy_(gr)
                t.grad = gr.double()
            before = [t.detach().clone() for t in tparams]
            opt.step()
            topt.step()
            assert opt.param_groups[0]['lr'] == LR0 and beq(opt.hyper.cpu(), R.adam_hyper(LR0 * min(1.0, k / 4.0), B1, B2, k))
            for b, b0, t in zip(bounds, before, tparams):
                b += MARGIN * count * U * (b0 - t.detach()).abs() + 2.0 ** -23 * t.detach().abs()
        torch.cuda.synchronize()
        for i, (q, t, b) in enumerate(zip(params, tparams, bounds)):
            err = (q.detach().cpu().double() - t.detach()).abs()
            print("adamw + warm-up tensor %d after 6 steps: max err / bound = %.3g" % (i, float((err / b).max())))
            assert bool((err <= b).all()), i
        # without the warm-up the first step would have moved four times as far
        assert float((params[1].detach().cpu() - values[1]).abs().max()) > 0
    finally:
        K.set_grad_sink(None)


def test_without_the_new_keys_the_step_launches_what_it_launched(L, monkeypatch):
    """FusedAdam without warmup_steps (and with it: the warm-up lives in hyper alone) calls the entry points it called; FusedLAMB calls its
    pair, behind the norm launch with a ctl -- the monkeypatched-launch pattern of test_without_tensor_scales_the_step_calls_what_it_called"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedLAMB
    names = ("mte_adam_step_dev", "mte_adamw_step_dev", "mte_adamw_step_ctl_dev", "mte_adamw_step_seg_dev", "mte_tensor_stats", "mte_grad_norm_clip",
             "mte_lamb_moments", "mte_lamb_apply", "mte_ema_update_dev", "mte_grad_accumulate")
    pair = ["mte_lamb_moments", "mte_lamb_apply"]
    cases = [(FusedAdam, dict(lr=LR0), ["mte_adam_step_dev"]),
             (FusedAdam, dict(lr=LR0, warmup_steps=4), ["mte_adam_step_dev"]),
             (FusedAdam, dict(lr=LR0, weight_decay=WD, decoupled_weight_decay=True), ["mte_adamw_step_dev"]),
             (FusedAdam, dict(lr=LR0, weight_decay=WD, decoupled_weight_decay=True, warmup_steps=4), ["mte_adamw_step_dev"]),
             (FusedAdam, dict(lr=LR0, skip_nonfinite=True), ["mte_grad_norm_clip", "mte_adamw_step_ctl_dev"]),
             (FusedLAMB, dict(lr=LR0), pair),
             (FusedLAMB, dict(lr=LR0, tensor_scales=CLS_SCALES, adapt=CLS_ADAPT, warmup_steps=4), pair),
             (FusedLAMB, dict(lr=LR0, clip_grad_norm=1.0), ["mte_grad_norm_clip"] + pair),
             (FusedLAMB, dict(lr=LR0, skip_nonfinite=True, ema_decay=0.9), ["mte_grad_norm_clip"] + pair + ["mte_ema_update_dev"])]
    try:
        K.lib.load()
        for name in names:
            getattr(K.lib, name)
        values, grads = _toy(9, 1)
        for cls, kwargs, want in cases:
            called = []
            with monkeypatch.context() as mp_:
                for name in names:
                    def spy(*a, _name=name, _real=K.lib.__dict__[name]):
                        called.append(_name)
                        return _real(*a)
                    mp_.setitem(K.lib.__dict__, name, spy)
                params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
                opt = cls(FlatParameters(params), **kwargs)
                for q, gr in zip(params, grads[0]):
                    q.grad.copy_(gr)
                opt.step()
                torch.cuda.synchronize()
                if cls is FusedLAMB:
                    opt.trust_ratios()                                    # a host read, no launch
            assert called == want, (cls.__name__, kwargs, called)
            if cls is FusedAdam:
                w = kwargs.get('warmup_steps', 0)
                # the class forms the bias corrections in double from its own (double) betas
                assert beq(opt.hyper.cpu(), torch.tensor([LR0 * (0.25 if w else 1.0), 1.0 - 0.9, (1.0 - 0.999) ** 0.5], dtype=torch.float64).float())
                assert not any(hasattr(opt, a) for a in ("adapt", "max_trust", "lamb_scales", "_lamb_tables"))
            K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


# ---- 8. the entry point and the graphed step ------------------------------------------------------------------------------------------------------
def test_train_edges_lamb_yaml_two_optimizer_steps_resume_and_the_trust_lines(tmp_path, capsys):
    """train_edges.py <the LAMB YAML> --synthetic (frame size, batch and checkpoint folder set for the test; the YAML's own accumulation of
    eight micro-batches, a log line per optimizer step, log_tensor_stats: 2): two optimizer steps and a checkpoint, then a resume for two more"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    with open(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_lamb.yaml")) as f:
        cfg = yaml.safe_load(f)
    block = cfg["model"]["optimizer"]
    assert block["name"] == "LAMB" and block["depth"] == {"lr": 0.001, "weight_decay": 0.01} and block["warmup_steps"] > 0
    assert block["lamb_exclude"] == [{"max_ndim": 1}] and cfg["arch"]["accumulate_grad_batches"] == 8
    block["log_tensor_stats"] = 2
    cfg["arch"]["log_every"] = 8
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
        return capsys.readouterr().out

    base = ["train_edges.py", path, "--synthetic", "--steps", "16", "--epochs", "1", "--save", save]
    outs = [run(base)]
    ckpt = load_checkpoint(os.path.join(save, "epoch=0.ckpt"))
    outs.append(run(base + ["--resume", os.path.join(save, "epoch=0.ckpt")]))
    ck2 = load_checkpoint(os.path.join(save, "epoch=1.ckpt"))
    for out in outs:
        assert "'steps': 16" in out and "'optimizer_steps': 2" in out
        lines = out.splitlines()
        at = [i for i, l in enumerate(lines) if l.startswith("step ")]
        assert len(at) == 2
        for i in at:
            top = lines[i + 1:i + 3]
            assert [l.split(" | ")[0] for l in top] == ["  grad top 1", "  grad top 2"], top
            ratios = [float(l.rsplit(" | trust ", 1)[1]) for l in top]
            assert all(math.isfinite(q) and q > 0.0 for q in ratios), top
    assert ckpt["epoch"] == 0 and ck2["epoch"] == 1
    for ck, steps in ((ckpt, 2), (ck2, 4)):                               # the file is torch.optim.AdamW's
        group = ck["optimizer"]["param_groups"][0]
        assert group["weight_decay"] == 0.01 and group["decoupled_weight_decay"] is True and group["lr"] == 0.001
        assert not any("lamb" in k or "warmup" in k or "trust" in k for k in group)
        assert {int(float(s_["step"])) for s_ in ck["optimizer"]["state"].values()} == {steps}
        assert all(set(s_) == {"step", "exp_avg", "exp_avg_sq"} for s_ in ck["optimizer"]["state"].values())
    moved = max(float((ck2["state_dict"][k].float() - ckpt["state_dict"][k].float()).abs().max()) for k in ckpt["state_dict"])
    assert 0 < moved < float("inf")


def test_graphed_lamb_steps_equal_eager_steps():
    """test_graphed_adamw_steps_equal_eager_steps' set-up with FusedLAMB (warm-up on, the default exclusion of the tensors of at most one
    dimension): five replayed steps follow five eager steps at that file's tolerance"""
    import random
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedLAMB
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
        flat = FlatParameters(net.parameters())
        opt = FusedLAMB(flat, lr=1e-3, weight_decay=0.01, warmup_steps=3, adapt=[p.dim() > 1 for p in flat.natural_params])
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
        rows = opt.trust_ratios()
        assert len(rows) == len(flat.natural_params) and [r['adapted'] for r in rows] == opt.adapt
        assert all(r['trust_ratio'] == 1.0 for r in rows if not r['adapted']) and any(r['trust_ratio'] != 1.0 for r in rows if r['adapted'])
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")
