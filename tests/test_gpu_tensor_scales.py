"""GPU (-m gpu): per-tensor learning-rate / weight-decay multipliers and per-tensor statistics of csrc/optim.hip.

The SEG entry points (mte_adamw_step_seg_dev, mte_sgd_step_seg_dev) are held, slice by slice and BIT FOR BIT, to the plain device-scalar
entry points (mte_adamw_step_dev / mte_sgd_step_dev and their _ctl_dev forms) launched on each slice alone with
hyper[0] = float32(lr * lr_mult) and weight_decay = float32(wd * wd_mult); those entry points are held to tests/optim_ref.py by
tests/test_gpu_optimizer_family.py and tests/test_gpu_grad_clip.py.  The classes are held to torch.optim with param groups in float64
under a StepLR schedule at that file's bounds.  mte_tensor_stats is held to exact integer sums and to the norm launch's bound.

Helpers (guarded buffers, inputs, toy parameters, operation counts) are tests/test_gpu_optimizer_family.py's own."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

import optim_ref as R
import tensor_scales_ref as T
import test_gpu_optimizer_family as F

pytestmark = pytest.mark.gpu

OK, ERR_ARG = F.OK, F.ERR_ARG
ROOT = F.ROOT
Flat, beq, _f, _st = F.Flat, F.beq, F._f, F._st
PAIRS = [(1.0, 1.0), (0.5, 1.0), (1.0, 0.0), (0.3, 0.7), (0.0, 1.0)]
WRAP_BLOCKS = 8192 * 256 // 16                                        # blocks (of 16 vectors) that one trip of the capped grid covers
# name -> (class of every 64-element block, (lr_mult, wd_mult) per class)
LAYOUTS = {
    "one_block": ([0], [PAIRS[3]]),
    "two_blocks": ([0, 1], [PAIRS[4], PAIRS[2]]),
    "five_blocks": ([0, 1, 0, 2, 1], [PAIRS[1], PAIRS[2], PAIRS[3]]),
    # the class changes exactly where the capped grid wraps (blocks 131071 | 131072) and again inside the second trip
    "grid_wrap": ([0] * WRAP_BLOCKS + [1] * 7 + [2] * 12, [PAIRS[3], PAIRS[0], PAIRS[4]]),
}
LR, B1, B2, EPS, GSCALE, WD = 3e-2, 0.5, 0.9, 1e-3, 1.0 / 3.0, 0.1    # HYPERS[1] of the family tests: nothing dyadic
STEP = 7


@pytest.fixture(scope="module")
def L():
    from mindtheedge_amd._lib import lib
    return lib.load()


@pytest.fixture(scope="module")
def inputs():
    """per layout: (p0, g, m0, v0) on the device, F._inputs' pattern (one sign per element; zeros in p, g and the state), made once"""
    assert len(LAYOUTS["grid_wrap"][0]) == 131072 + 19
    out = {}
    for i, (name, (blocks, _)) in enumerate(sorted(LAYOUTS.items())):
        n = 64 * len(blocks)
        p0, grad, m0, v0 = F._inputs(n, F._gen(7000 + i), True)
        out[name] = tuple(t.cuda() for t in (p0, grad(), m0, v0))
    return out


def _runs(blocks):
    """[(first block, end block, class)] of the maximal runs of one class: the slices"""
    runs, s = [], 0
    for b in range(1, len(blocks) + 1):
        if b == len(blocks) or blocks[b] != blocks[s]:
            runs.append((s, b, blocks[s]))
            s = b
    return runs


def _tables(blocks, pairs):
    cls = torch.tensor(blocks, dtype=torch.uint8).cuda()
    scales = torch.tensor([x for p in pairs for x in p], dtype=torch.float32).cuda()
    return cls, scales


def _ctl(mode):
    """None, or mte_grad_norm_clip's word: {coefficient 0.5, skip flag, norm, skipped steps}"""
    if mode == "null":
        return None
    return torch.tensor([0.5, 1.0 if mode == "skip" else 0.0, 3.0, 0.0], dtype=torch.float32).cuda()


def _slice_hyper(hyp, lm):
    h = hyp.clone()
    h[0] = float(np.float32(hyp[0].item()) * np.float32(lm))
    return h.cuda()


def _wd_c(wd, wm):
    return float(np.float32(wd) * np.float32(wm))


# ---- 1. per-slice identity ---------------------------------------------------------------------------------------------------------------------------
ADAM_CASES = {"adam_l2": (WD, 0), "adamw": (WD, 1), "adam": (0.0, 0)}


@pytest.mark.parametrize("mode", ["null", "coef", "skip"])
@pytest.mark.parametrize("case", sorted(ADAM_CASES))
def test_adam_seg_equals_the_plain_launch_on_every_slice(L, inputs, case, mode):
    wd, decoupled = ADAM_CASES[case]
    hyp = R.adam_hyper(LR, B1, B2, STEP)
    hyp_d = hyp.cuda()
    for name, (blocks, pairs) in LAYOUTS.items():
        n = 64 * len(blocks)
        p0, g, m0, v0 = inputs[name]
        cls, scales = _tables(blocks, pairs)
        ctl = _ctl(mode)
        seg, ref = ([Flat(n).set(t) for t in (p0, m0, v0)] for _ in range(2))
        g_keep = g.clone()
        assert L.mte_adamw_step_seg_dev(seg[0].ptr, g.data_ptr(), seg[1].ptr, seg[2].ptr, n, hyp_d.data_ptr(), B1, B2, EPS, wd, decoupled, GSCALE,
                                        cls.data_ptr(), scales.data_ptr(), len(pairs), None if ctl is None else ctl.data_ptr(), _st()) == OK
        for b0, b1, c in _runs(blocks):
            o, m = 64 * b0 * 4, 64 * (b1 - b0)
            h = _slice_hyper(hyp, pairs[c][0])
            args = (ref[0].ptr + o, g.data_ptr() + o, ref[1].ptr + o, ref[2].ptr + o, m, h.data_ptr(), B1, B2, EPS, _wd_c(wd, pairs[c][1]),
                    decoupled, GSCALE)
            if ctl is None:
                assert L.mte_adamw_step_dev(*args, _st()) == OK
            else:
                assert L.mte_adamw_step_ctl_dev(*args, ctl.data_ptr(), _st()) == OK
        torch.cuda.synchronize()
        for a, b, t0 in zip(seg, ref, (p0, m0, v0)):
            assert torch.equal(a.raw, b.raw) and a.guard_ok(), (name, case, mode)
            assert beq(a.t[:n], t0) == (mode == "skip"), (name, case, mode)      # a skipped step changes nothing; any other step does
        assert torch.equal(g.view(torch.int32), g_keep.view(torch.int32))


@pytest.mark.parametrize("mode", ["null", "coef", "skip"])
@pytest.mark.parametrize("variant", F.SGD_VARIANTS, ids=[s[0] for s in F.SGD_VARIANTS])
def test_sgd_seg_equals_the_plain_launch_on_every_slice(L, inputs, variant, mode):
    _, mu, damp, nesterov, with_wd = variant
    wd = WD if with_wd else 0.0
    hyp = R.sgd_hyper(LR, mu, damp, STEP)
    hyp_d = hyp.cuda()
    for name, (blocks, pairs) in LAYOUTS.items():
        n = 64 * len(blocks)
        p0, g, b0_, _ = inputs[name]
        cls, scales = _tables(blocks, pairs)
        ctl = _ctl(mode)
        seg, ref = ([Flat(n).set(t) for t in ((p0, b0_) if mu else (p0,))] for _ in range(2))
        g_keep = g.clone()
        assert L.mte_sgd_step_seg_dev(seg[0].ptr, g.data_ptr(), seg[1].ptr if mu else None, n, hyp_d.data_ptr(), mu, wd, nesterov, GSCALE,
                                      cls.data_ptr(), scales.data_ptr(), len(pairs), None if ctl is None else ctl.data_ptr(), _st()) == OK
        for s0, s1, c in _runs(blocks):
            o, m = 64 * s0 * 4, 64 * (s1 - s0)
            h = _slice_hyper(hyp, pairs[c][0])
            args = (ref[0].ptr + o, g.data_ptr() + o, ref[1].ptr + o if mu else None, m, h.data_ptr(), mu, _wd_c(wd, pairs[c][1]), nesterov, GSCALE)
            if ctl is None:
                assert L.mte_sgd_step_dev(*args, _st()) == OK
            else:
                assert L.mte_sgd_step_ctl_dev(*args, ctl.data_ptr(), _st()) == OK
        torch.cuda.synchronize()
        for a, b, t0 in zip(seg, ref, (p0, b0_)):
            assert torch.equal(a.raw, b.raw) and a.guard_ok(), (name, variant, mode)
            assert beq(a.t[:n], t0) == (mode == "skip"), (name, variant, mode)
        assert torch.equal(g.view(torch.int32), g_keep.view(torch.int32))


@pytest.mark.parametrize("name", ["five_blocks", "grid_wrap"])
def test_all_multipliers_one_is_the_plain_launch_over_the_whole_buffer(L, inputs, name):
    blocks, _ = LAYOUTS[name]
    n = 64 * len(blocks)
    p0, g, m0, v0 = inputs[name]
    cls, scales = _tables(blocks, [(1.0, 1.0)] * 3)
    ha, hs = R.adam_hyper(LR, B1, B2, STEP).cuda(), R.sgd_hyper(LR, 0.9, 0.1, STEP).cuda()
    for wd, decoupled in ((WD, 1), (WD, 0), (0.0, 0)):
        seg, ref = ([Flat(n).set(t) for t in (p0, m0, v0)] for _ in range(2))
        assert L.mte_adamw_step_seg_dev(seg[0].ptr, g.data_ptr(), seg[1].ptr, seg[2].ptr, n, ha.data_ptr(), B1, B2, EPS, wd, decoupled, GSCALE,
                                        cls.data_ptr(), scales.data_ptr(), 3, None, _st()) == OK
        assert L.mte_adamw_step_dev(ref[0].ptr, g.data_ptr(), ref[1].ptr, ref[2].ptr, n, ha.data_ptr(), B1, B2, EPS, wd, decoupled, GSCALE, _st()) == OK
        torch.cuda.synchronize()
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(seg, ref)) and not beq(seg[0].t[:n], p0)
    for wd in (WD, 0.0):
        seg, ref = ([Flat(n).set(t) for t in (p0, m0)] for _ in range(2))
        assert L.mte_sgd_step_seg_dev(seg[0].ptr, g.data_ptr(), seg[1].ptr, n, hs.data_ptr(), 0.9, wd, 0, GSCALE, cls.data_ptr(), scales.data_ptr(), 3,
                                      None, _st()) == OK
        assert L.mte_sgd_step_dev(ref[0].ptr, g.data_ptr(), ref[1].ptr, n, hs.data_ptr(), 0.9, wd, 0, GSCALE, _st()) == OK
        torch.cuda.synchronize()
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(seg, ref)) and not beq(seg[0].t[:n], p0)


# ---- 2. argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_a_class_byte_out_of_range(L):
    n = 128
    p, m, v = (Flat(n).set(torch.ones(n)) for _ in range(3))
    g = torch.ones(n + 64).cuda()
    hyp = R.adam_hyper(1e-4, 0.9, 0.999, 1).cuda()
    cls, scales = _tables([0, 1, 0], [(1.0, 1.0), (0.5, 0.5)])
    gp, hp, cp, sp = g.data_ptr(), hyp.data_ptr(), cls.data_ptr(), scales.data_ptr()

    def adam(p_=p.ptr, g_=gp, m_=m.ptr, v_=v.ptr, n_=n, h_=hp, wd=0.01, c_=cp, s_=sp, k=2):
        return L.mte_adamw_step_seg_dev(p_, g_, m_, v_, n_, h_, 0.9, 0.999, 1e-8, wd, 1, 1.0, c_, s_, k, None, _st())

    def sgd(p_=p.ptr, g_=gp, b_=m.ptr, n_=n, h_=hp, mu=0.9, wd=0.01, nesterov=0, c_=cp, s_=sp, k=2):
        return L.mte_sgd_step_seg_dev(p_, g_, b_, n_, h_, mu, wd, nesterov, 1.0, c_, s_, k, None, _st())

    for fn in (adam, sgd):
        for n_bad in (127, 100, 64 + 4, 0, -64):                       # n % 64 != 0; n <= 0
            assert fn(n_=n_bad) == ERR_ARG
        assert fn(c_=None) == ERR_ARG and fn(s_=None) == ERR_ARG          # null tables
        assert fn(k=0) == ERR_ARG and fn(k=17) == ERR_ARG and fn(k=-1) == ERR_ARG
        assert fn(p_=None) == ERR_ARG and fn(g_=None) == ERR_ARG and fn(h_=None) == ERR_ARG
        assert fn(wd=-0.01) == ERR_ARG and fn(wd=float("nan")) == ERR_ARG
    assert adam(m_=None) == ERR_ARG and adam(v_=None) == ERR_ARG
    assert sgd(b_=None) == ERR_ARG and sgd(mu=-0.1) == ERR_ARG and sgd(mu=0.0, nesterov=1) == ERR_ARG
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert beq(t.get(), torch.ones(n)) and t.guard_ok()

    # a map byte >= n_classes: no fault, nothing written outside n, and the block is updated as the LAST class
    n = 64 * 3
    p0, grad, m0, v0 = F._inputs(n, F._gen(77), True)
    g = grad().cuda()
    pairs = [(1.0, 1.0), (0.5, 0.25)]
    bad, scales = _tables([0, 200, 255], pairs)
    good, _ = _tables([0, 1, 1], pairs)
    got, want = ([Flat(n).set(t) for t in (p0, m0, v0)] for _ in range(2))
    for bufs, cmap in ((got, bad), (want, good)):
        assert L.mte_adamw_step_seg_dev(bufs[0].ptr, g.data_ptr(), bufs[1].ptr, bufs[2].ptr, n, hyp.data_ptr(), 0.9, 0.999, 1e-8, 0.01, 1, 1.0,
                                        cmap.data_ptr(), scales.data_ptr(), 2, None, _st()) == OK
    gs, ws = Flat(n).set(p0), Flat(n).set(p0)
    hs = R.sgd_hyper(1e-2, 0.0, 0.0, 1).cuda()
    for buf, cmap in ((gs, bad), (ws, good)):
        assert L.mte_sgd_step_seg_dev(buf.ptr, g.data_ptr(), None, n, hs.data_ptr(), 0.0, 0.01, 0, 1.0, cmap.data_ptr(), scales.data_ptr(), 2, None,
                                      _st()) == OK
    torch.cuda.synchronize()
    for a, b in list(zip(got, want)) + [(gs, ws)]:
        assert torch.equal(a.raw, b.raw) and a.guard_ok()


# ---- 3. the classes against torch.optim with param groups, under a schedule and through a checkpoint --------------------------------------------------
DYADIC = [(0.5, 1.0), (1.0, 0.0), (0.25, 0.5), (1.0, 1.0)]             # one pair per toy tensor: every lr_c and wd_c is exact in fp32
NON_DYADIC = [(0.3, 0.7), (1.0, 0.0), (0.7, 1.0), (1.0, 0.3)]
ADAM_PLAIN = ("adam", dict(lr=F.LR, betas=(F.B1, F.B2), eps=F.EPS), torch.optim.Adam, dict(lr=F.LR, betas=(F.B1, F.B2), eps=F.EPS), None)
SCHEDULE_CASES = [(c, "dyadic") for c in sorted(F.CLASS_CASES)] + [("adam_plain", "dyadic"), ("adamw", "non_dyadic")]


def _count(case, kwargs, wm_nonzero):
    """the family tests' operation count for p of a tensor whose decay is on (wm != 0 and the case has one) or off"""
    wd = bool(kwargs.get("weight_decay", 0.0)) and wm_nonzero
    if case.startswith("adam"):
        return F.adam_counts(wd, bool(kwargs.get("decoupled_weight_decay", False)))["p"]
    return F.sgd_counts(kwargs.get("momentum", 0.0), bool(kwargs.get("nesterov", False)), wd)["p"]


def _is_dyadic(x):
    return x == 0.0 or math.frexp(x)[0] == 0.5


@pytest.mark.parametrize("case,kind_of_pairs", SCHEDULE_CASES, ids=["%s-%s" % c for c in SCHEDULE_CASES])
def test_classes_follow_torch_param_groups_under_a_schedule_and_through_a_checkpoint(case, kind_of_pairs):
    """test_classes_follow_torch_under_a_schedule_and_through_a_checkpoint (tests/test_gpu_optimizer_family.py) with tensor_scales on the
    fused side and ONE PARAM GROUP PER TENSOR on the torch side (float64): its toy parameters, StepLR(2, 0.5), five steps, its bounds.

    Dyadic multipliers (0.5, 0.25, 0) and that file's dyadic LR = 2^-6: lr_c = lr * lm and wd_c = wd * wm are exact in fp32 at every
    step of the schedule, so the torch group's {lr * lm, wd * wm} are the kernel's scalars and that file's operation counts hold
    unchanged (per tensor: the count with a decay where wd_c != 0, the count without where wd_c = 0).

    The non-dyadic case.  The torch groups take lr * float32(lm) and wd * float32(wm), the products in double (the multipliers enter at
    their float32 values, as every scalar of optim_ref does).  The kernel forms lr_c = fl32(lr * lm32) and wd_c = fl32(wd * wm32): ONE
    more rounding, relative error <= u = 2^-24, per scaled scalar.  lr_c multiplies the whole update dp: +1 operation.  wd_c multiplies
    the decay term only; every term of dp has one sign for these inputs, so a relative error u in one of them is at most u in the sum
    (for L2 decay, g' rises by at most u, m and sqrt(v) by at most u in the same direction, and m / (sqrt(v) / bc2s + eps) by at most
    u): +1 operation.  So count + [lm is not a power of two] + [wd_c != 0 and wm is not a power of two], inside the same MARGIN.

    Then the checkpoint: state_dict() has the keys it always had, loads into the ONE-group torch class and into a fresh fused optimizer
    with the same tensor_scales, which continues bit-equal to the one that never stopped."""
    from mindtheedge_amd import kernels as K
    kind, kwargs, tcls, tkwargs, _ = ADAM_PLAIN if case == "adam_plain" else F.CLASS_CASES[case]
    pairs = DYADIC if kind_of_pairs == "dyadic" else NON_DYADIC
    lr0, wd0 = kwargs["lr"], kwargs.get("weight_decay", 0.0)
    counts = [_count(case, kwargs, wm != 0.0) + (0 if _is_dyadic(lm) else 1) + (0 if _is_dyadic(wm) or not wd0 else 1) for lm, wm in pairs]
    if kind_of_pairs == "dyadic":
        for lm, wm in pairs:                                              # exact in fp32: the premise of the unchanged counts
            assert T.class_scalars(lr0, wd0, lm, wm) == (lr0 * lm, wd0 * wm) and T.class_scalars(lr0 / 4, wd0, lm, wm)[0] == lr0 * lm / 4
    else:
        assert any(T.class_scalars(lr0, wd0, lm, wm) != (lr0 * _f(lm), wd0 * _f(wm)) for lm, wm in pairs)
    try:
        _, values, grads = F._toy_params()
        params, opt = F._fused(kind, values, dict(kwargs, tensor_scales=pairs))
        assert len(opt.seg_classes) == 4 and len(opt.param_groups) == 1
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        tparams = [torch.nn.Parameter(v.double().clone()) for v in values]
        topt = tcls([{'params': [t], 'lr': lr0 * _f(lm), 'weight_decay': wd0 * _f(wm)} for t, (lm, wm) in zip(tparams, pairs)], **tkwargs)
        tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=2, gamma=0.5)
        bounds = [torch.zeros_like(t.data) for t in tparams]

        def single(before, after):
            return [F.MARGIN * c * F.U * (b0 - t).abs() + 2.0 ** -23 * t.abs() for c, b0, t in zip(counts, before, after)]

        for step in range(5):
            for q, t, gr in zip(params, tparams, grads[step]):
                q.grad.copy_(gr)
                t.grad = gr.double()
            before = [t.detach().clone() for t in tparams]
            opt.step()
            topt.step()
            sched.step()
            tsched.step()
            for b, s in zip(bounds, single(before, [t.detach() for t in tparams])):
                b += s
        torch.cuda.synchronize()
        assert opt.param_groups[0]['lr'] == lr0 / 4 and opt.steps == 5
        assert [g['lr'] for g in topt.param_groups] == [lr0 * _f(lm) / 4 for lm, _ in pairs]
        for i, (q, t, b) in enumerate(zip(params, tparams, bounds)):
            err = (q.detach().cpu().double() - t.detach()).abs()
            print("%s %s tensor %d after 5 steps: max err / bound = %.3g" % (case, kind_of_pairs, i, float((err / b).max())))
            assert bool((err <= b).all()), (case, i)
        # (a multiplier that was ignored, or applied to the wrong tensor, is orders of magnitude outside these bounds)
        # ---- the checkpoint
        sd = opt.state_dict()
        _, plain = F._fused(kind, values, kwargs)
        assert set(sd) == {'state', 'param_groups'} and len(sd['param_groups']) == 1
        assert set(sd['param_groups'][0]) - {'initial_lr'} == set(plain.state_dict()['param_groups'][0]) - {'initial_lr'}
        assert {k for st in sd['state'].values() for k in st} == ({'step', 'exp_avg', 'exp_avg_sq'} if kind == "adam" else
                                                                  ({'momentum_buffer'} if kwargs.get('momentum') else set()))
        cparams = [torch.nn.Parameter(q.detach().cpu().double()) for q in params]
        copt = tcls([{'params': cparams, 'name': 'Depth'}], **{**tkwargs, 'lr': 0.5})
        copt.load_state_dict(sd)                                          # torch's own one-group class reads the file
        assert copt.param_groups[0]['lr'] == lr0 / 4 and len(copt.param_groups) == 1
        params2, opt2 = F._fused(kind, [q.detach().cpu() for q in params], dict(kwargs, lr=0.5, tensor_scales=pairs))
        opt2.load_state_dict(sd)
        assert all(torch.equal(a, b) for a, b in zip(F._state_of(opt), F._state_of(opt2)))
        for q, q2, gr in zip(params, params2, grads[5]):
            q.grad.copy_(gr)
            q2.grad.copy_(gr)
        opt.step()
        opt2.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(F._state_of(opt), F._state_of(opt2)))
    finally:
        K.set_grad_sink(None)


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------------------------------
def test_graphed_scaled_clipped_adamw_steps_equal_eager_steps_bit_for_bit():
    """test_graphed_clipped_adamw_steps_equal_eager_steps_bit_for_bit (tests/test_gpu_grad_clip.py) with tensor_scales: the norm launch and
    the SEG step captured ONCE and replayed five times with advance() before each replay and the learning rate halved every two steps, against five eager step() calls from the same state: parameters, moments and ctl bit-equal after every step -- the launch
    holds nothing that changes from step to step"""
    from mindtheedge_amd import kernels as K
    try:
        _, values, grads = F._toy_params()
        kwargs = dict(lr=F.LR, betas=(F.B1, F.B2), eps=F.EPS, weight_decay=F.WD, decoupled_weight_decay=True, clip_grad_norm=2.0,
                      skip_nonfinite=True, tensor_scales=NON_DYADIC)
        params, opt = F._fused("adam", values, kwargs)
        flat = opt.flatp
        factors = [1.0, 40.0, 1.0, 0.01, 3.0]

        def set_grads(step):
            for i, (q, gr) in enumerate(zip(params, grads[step])):
                q.grad.copy_(gr * factors[step])
                if step == 2 and i == 3:
                    q.grad.view(-1)[5] = float("inf")

        def run(do_step):
            out = []
            for step in range(5):
                opt.param_groups[0]['lr'] = F.LR * 0.5 ** (step // 2)      # StepLR(2, 0.5)'s values, set in the one group as it sets them
                set_grads(step)
                do_step()
                torch.cuda.synchronize()
                out.append(F._state_of(opt) + [opt.ctl.clone(), opt.hyper.clone()])
            return out

        snap = (F._state_of(opt), opt.steps)
        eager = run(opt.step)
        assert [bool(e[-2][1]) for e in eager] == [False, False, True, False, False] and float(eager[1][-2][0]) < 1.0
        assert float(eager[0][-1][0]) == F.LR and float(eager[4][-1][0]) == F.LR / 4          # the learning rate changed under the launches
        for b, v in zip([flat.flat] + [b for _, b in opt.state_buffers()], snap[0]):
            b.copy_(v)
        opt.steps = snap[1]
        opt.ctl.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stream = torch.cuda.current_stream().cuda_stream
            opt._norm_clip(K, 1.0, stream)
            opt._launch_seg(K, opt.param_groups[0], 1.0, (opt.seg_block_class.data_ptr(), opt.seg_class_scales.data_ptr(), len(opt.seg_classes),
                                                         opt.ctl.data_ptr()), stream)

        def replay():
            opt.advance()
            graph.replay()

        got = run(replay)
        for step in range(5):
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[step], eager[step])), step
        assert opt.steps == 5 and opt.grad_stats()['skipped_steps'] == 1
    finally:
        K.set_grad_sink(None)


def test_graphed_train_step_with_tensor_scales_follows_eager_steps():
    """GraphedTrainStep needs no change: test_graphed_adamw_steps_equal_eager_steps's set-up (tests/test_gpu_optimizer_family.py) with the
    fine-tuning recipe's multipliers and clipping on -- the whole training step captured with the norm launch and the SEG step inside --
    follows the eager steps at that test's tolerances (backward's atomics), and a tensor with lr multiplier 0 keeps its bits"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, resolve_tensor_scales
    from mindtheedge_amd.utils.graph import GraphedTrainStep
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    dev = torch.device("cuda")
    batches = [synthetic_batch(2, 64, 128, s, dev) for s in (1, 2, 3)]
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
        named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
        rules = [{"max_ndim": 1, "weight_decay_scale": 0.0}, {"pattern": r"^encoder\.", "lr_scale": 0.1},
                 {"pattern": r"^decoder\.disp1_layer\.", "lr_scale": 0.0, "weight_decay_scale": 0.0}]
        frozen = [p for n, p in named if n.startswith("decoder.disp1_layer.") and p.dim() > 1]
        scales = resolve_tensor_scales([n for n, _ in named], [tuple(p.shape) for _, p in named], rules)
        opt = FusedAdam(FlatParameters(net.parameters()), lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, clip_grad_norm=1.0,
                        skip_nonfinite=True, tensor_scales=scales)
        assert len(frozen) >= 1 and len(opt.seg_classes) == 5
        step = GraphedTrainStep(model, opt, batches[0])
        assert step.graphed, step.error
        torch.cuda.synchronize()
        assert opt.steps == 0
        snap = (opt.flatp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.steps)
        frozen0 = frozen[0].detach().clone()

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
        assert opt.steps == 3
        restore()
        random.seed(11)
        got = [float(step(b)["loss"].sum()) for b in batches]
        torch.cuda.synchronize()
        assert opt.steps == 3
        for a, b in zip(got, eager):
            assert a == pytest.approx(b, rel=5e-4), (got, eager)
        assert float((opt.flatp.flat - p_eager).abs().max()) <= 5e-3
        assert float((opt.flatp.flat - snap[0]).abs().max()) > 0
        assert torch.equal(frozen[0].detach().view(torch.int32), frozen0.view(torch.int32))    # lr x 0, decay x 0: not a bit moves
        assert math.isfinite(opt.grad_stats()['grad_norm'])
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


# ---- 5. off means off --------------------------------------------------------------------------------------------------------------------------------
def test_without_tensor_scales_the_step_calls_what_it_called(L, monkeypatch):
    """tensor_scales None (and all (1, 1)): no table attribute, neither SEG entry point nor the statistics launch is called by step(),
    and the entry points called are the ones of before: mte_adam_step_dev, mte_adamw_step_dev, mte_sgd_step_dev, the _ctl_dev forms
    behind mte_grad_norm_clip.  With scales, the SEG entry point and none of those."""
    from mindtheedge_amd import kernels as K
    steps = ("mte_adam_step_dev", "mte_adamw_step_dev", "mte_sgd_step_dev", "mte_adamw_step_ctl_dev", "mte_sgd_step_ctl_dev",
             "mte_adamw_step_seg_dev", "mte_sgd_step_seg_dev", "mte_tensor_stats", "mte_grad_norm_clip")
    cases = [("adam", dict(lr=F.LR), ["mte_adam_step_dev"], ["mte_adamw_step_seg_dev"]),
             ("adam", dict(lr=F.LR, weight_decay=F.WD, decoupled_weight_decay=True), ["mte_adamw_step_dev"], ["mte_adamw_step_seg_dev"]),
             ("sgd", dict(lr=F.LR, momentum=F.MU), ["mte_sgd_step_dev"], ["mte_sgd_step_seg_dev"]),
             ("adam", dict(lr=F.LR, skip_nonfinite=True), ["mte_grad_norm_clip", "mte_adamw_step_ctl_dev"],
              ["mte_grad_norm_clip", "mte_adamw_step_seg_dev"]),
             ("sgd", dict(lr=F.LR, clip_grad_norm=1.0), ["mte_grad_norm_clip", "mte_sgd_step_ctl_dev"], ["mte_grad_norm_clip", "mte_sgd_step_seg_dev"])]
    try:
        K.lib.load()
        for name in steps:
            getattr(K.lib, name)                                          # resolve the wrappers, so that each has an entry to replace
        _, values, grads = F._toy_params()
        for kind, kwargs, want_off, want_on in cases:
            for scales, want in ((None, want_off), ([(1.0, 1.0)] * 4, want_off), (DYADIC, want_on)):
                called = []
                with monkeypatch.context() as mp_:
                    for name in steps:
                        def spy(*a, _name=name, _real=K.lib.__dict__[name]):
                            called.append(_name)
                            return _real(*a)
                        mp_.setitem(K.lib.__dict__, name, spy)
                    params, opt = F._fused(kind, values, dict(kwargs, tensor_scales=scales))
                    has = [a for a in ("tensor_scales", "seg_classes", "seg_block_class", "seg_class_scales", "_stats_tables") if hasattr(opt, a)]
                    assert has == ([] if want is want_off else ["tensor_scales", "seg_classes", "seg_block_class", "seg_class_scales"])
                    for q, gr in zip(params, grads[0]):
                        q.grad.copy_(gr)
                    opt.step()
                    torch.cuda.synchronize()
                assert called == want, (kind, kwargs, scales, called)
                K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


# ---- 6. statistics -----------------------------------------------------------------------------------------------------------------------------------
CHUNK = 32768                                                             # csrc/optim.hip: STAT_CHUNK
STAT_NUMELS = [1, 5, 63, 64, 65, 1027, 3 * CHUNK + 1000 + 3]              # the last: three whole chunks, a ragged fourth, a 3-element tail


def _stat_layout():
    begins, total = [], 0
    for m in STAT_NUMELS:
        begins.append(total)
        total += (m + 63) // 64 * 64
    return begins, total


class _Stats:
    """one mte_tensor_stats set-up over STAT_NUMELS: g and p in guarded buffers whose padding is NaN, a guarded zeroed work buffer"""

    def __init__(self, L, values_g, values_p):
        self.L = L
        self.begins, self.n = _stat_layout()
        T_ = len(STAT_NUMELS)
        self.g, self.p = Flat(self.n), Flat(self.n)
        for buf, vals in ((self.g, values_g), (self.p, values_p)):
            host = torch.full((self.n,), float("nan"))
            for b, m, v in zip(self.begins, STAT_NUMELS, vals):
                host[b:b + m] = v
            buf.set(host)
        self.keep = (self.g.raw.clone(), self.p.raw.clone())
        nbytes = L.mte_tensor_stats_work_bytes(self.n, T_)
        assert nbytes >= 4 * T_ + 32 * (self.n // CHUNK + T_) and nbytes % 16 == 0
        self.work = Flat(nbytes // 4).set(torch.zeros(nbytes // 4))
        self.begin_d = torch.tensor(self.begins, dtype=torch.int64).cuda()
        self.numel_d = torch.tensor(STAT_NUMELS, dtype=torch.int64).cuda()
        self.out = torch.full((4 * T_ + 8,), -7.0, dtype=torch.float64).cuda()

    def call(self, with_p=True):
        rc = self.L.mte_tensor_stats(self.g.ptr, self.p.ptr if with_p else None, self.n, self.begin_d.data_ptr(), self.numel_d.data_ptr(),
                                     len(STAT_NUMELS), self.work.ptr, self.out.data_ptr(), _st())
        assert rc == OK
        return self

    def rows(self):
        torch.cuda.synchronize()
        assert bool((self.out[4 * len(STAT_NUMELS):] == -7.0).all())                        # nothing behind the last tensor's row
        assert torch.equal(self.g.raw, self.keep[0]) and torch.equal(self.p.raw, self.keep[1])   # read-only, guards included
        assert self.work.guard_ok() and bool((self.work.raw[:len(STAT_NUMELS)] == 0).all())      # the tickets are back at zero
        return self.out[:4 * len(STAT_NUMELS)].view(-1, 4).cpu()


def _ref_rows(values_g, values_p):
    rows = []
    for g, p in zip(values_g, values_p):
        g64, fin = g.double(), torch.isfinite(g)
        rows.append([float((g64 * g64).sum()), float(g64[fin].abs().max()) if bool(fin.any()) else 0.0, float((~fin).sum()),
                     float((p.double() ** 2).sum())])
    return torch.tensor(rows, dtype=torch.float64)


def test_tensor_stats_integer_inputs_are_exact_and_calls_and_replays_are_bit_equal(L):
    gen = F._gen(91)
    vg = [torch.randint(-3, 4, (m,), generator=gen).float() for m in STAT_NUMELS]
    vp = [torch.randint(-3, 4, (m,), generator=gen).float() for m in STAT_NUMELS]
    s = _Stats(L, vg, vp)
    got = s.call().rows()
    want = _ref_rows(vg, vp)
    assert torch.equal(got, want), (got, want)                            # S_g, amax_g, nonfinite = 0 and S_p: exact
    again = s.call().rows()
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    nop = s.call(with_p=False).rows()
    assert torch.equal(nop[:, :3], want[:, :3]) and bool((nop[:, 3] == 0).all())
    # under graph replay, on random inputs (the order of the additions matters there)
    vg = [torch.randn(m, generator=gen) for m in STAT_NUMELS]
    vp = [torch.randn(m, generator=gen) for m in STAT_NUMELS]
    s = _Stats(L, vg, vp)
    first = s.call().rows()
    second = s.call().rows()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.call()
    replays = []
    for _ in range(2):
        s.out.fill_(-7.0)
        graph.replay()
        replays.append(s.rows())
    for other in [second] + replays:
        assert torch.equal(first.view(torch.int64), other.view(torch.int64))
    # the project's bound for the norm launch, per tensor: |S - S_ref| <= numel * 2^-53 * S_ref
    want = _ref_rows(vg, vp)
    for t, m in enumerate(STAT_NUMELS):
        for col in (0, 3):
            err, bound = abs(float(first[t, col]) - float(want[t, col])), m * 2.0 ** -53 * float(want[t, col])
            print("tensor %d (numel %d) column %d: err / bound = %.3g" % (t, m, col, err / bound))
            assert err <= bound, (t, col)
        assert float(first[t, 1]) == float(want[t, 1]) and float(first[t, 2]) == 0.0


def test_tensor_stats_count_non_finite_elements_once_and_keep_them_to_their_tensor(L):
    gen = F._gen(92)
    vg = [torch.randn(m, generator=gen) for m in STAT_NUMELS]
    vp = [torch.randn(m, generator=gen) for m in STAT_NUMELS]
    big = STAT_NUMELS[-1]
    assert big % 4 == 3 and big > 3 * CHUNK
    # first, last (in the 3-element tail), both sides of a chunk boundary, the ragged chunk's last whole vector, the tail's first element
    spots = {0: float("inf"), CHUNK - 1: float("nan"), CHUNK: float("-inf"), big - 4: float("nan"), big - 3: float("inf"), big - 1: float("nan")}
    for i, x in spots.items():
        vg[-1][i] = x
    vg[3][63] = float("inf")                                              # and the last element of a tensor that fills its block
    vg[0][0] = float("nan")                                               # a one-element tensor that is a NaN: no finite element at all
    got = _Stats(L, vg, vp).call().rows()
    want = _ref_rows(vg, vp)
    assert got[:, 2].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, float(len(spots))] == want[:, 2].tolist()
    assert torch.equal(got[:, 1], want[:, 1]) and float(got[0, 1]) == 0.0 and float(got[-1, 1]) < 10.0       # amax ignores inf and NaN
    assert math.isnan(float(got[0, 0])) and float(got[3, 0]) == float("inf") and math.isnan(float(got[-1, 0]))
    for t in (1, 2, 4, 5):                                                # the others are finite and inside the bound
        assert abs(float(got[t, 0]) - float(want[t, 0])) <= STAT_NUMELS[t] * 2.0 ** -53 * float(want[t, 0])
    assert bool(torch.isfinite(got[:, 3]).all())                          # the weights hold no NaN: the padding was not read


def test_tensor_stats_argument_errors_and_a_range_that_leaves_the_buffer(L):
    s = _Stats(L, [torch.ones(m) for m in STAT_NUMELS], [torch.ones(m) for m in STAT_NUMELS])
    T_ = len(STAT_NUMELS)
    a = (s.g.ptr, s.p.ptr, s.n, s.begin_d.data_ptr(), s.numel_d.data_ptr(), T_, s.work.ptr, s.out.data_ptr())
    for i, bad in ((0, None), (2, 0), (3, None), (4, None), (5, 0), (5, 4097), (6, None), (7, None), (0, s.g.ptr + 4)):
        args = list(a)
        args[i] = bad
        assert L.mte_tensor_stats(*args, _st()) == ERR_ARG
    assert L.mte_tensor_stats_work_bytes(0, 3) == 0 and L.mte_tensor_stats_work_bytes(64, 0) == 0 and L.mte_tensor_stats_work_bytes(64, 4097) == 0
    torch.cuda.synchronize()
    assert bool((s.out == -7.0).all())
    # tensor 5's count reaches past n, tensor 2 begins before 0: both report zeros and read nothing; the others are as ever
    s.numel_d[5] = s.n
    s.begin_d[2] = -64
    got = s.call().rows()
    assert got[5].tolist() == [0.0] * 4 and got[2].tolist() == [0.0] * 4
    for t in (0, 1, 3, 4, 6):
        assert got[t].tolist() == [float(STAT_NUMELS[t]), 1.0, 0.0, float(STAT_NUMELS[t])]


def test_optimizer_tensor_stats_names_and_sums(L, monkeypatch):
    """FusedFlatOptimizer.tensor_stats() on a toy optimizer: reference names through set_index_space (positional without), the multipliers,
    one launch per call and none from step(), and sum_t S_g consistent with grad_stats()['grad_norm'] -- exact for integer gradients,
    inside the summed bound of the two launches otherwise"""
    from mindtheedge_amd import kernels as K
    try:
        K.lib.load()
        _, values, grads = F._toy_params()
        pairs = [(0.5, 1.0), (1.0, 0.0), (1.0, 1.0), (1.0, 1.0)]
        for scales in (None, pairs):
            params, opt = F._fused("adam", values, dict(lr=1e-3, skip_nonfinite=True, tensor_scales=scales))
            names = ["weight", "enc.a", "absent.in.this.build", "enc.b", "dec.c"]
            local = dict(zip(["weight", "enc.a", "enc.b", "dec.c"], params))
            for integer in (True, False):
                for q, gr in zip(params, grads[0]):
                    q.grad.copy_(torch.round(gr * 3) if integer else gr)
                g_host = [q.grad.detach().cpu().clone() for q in params]
                opt.step()
                assert not hasattr(opt, "_stats_tables") or integer is False               # step() launched no statistics
                stats = opt.tensor_stats()
                assert [s["name"] for s in stats] == (["0", "1", "2", "3"] if integer else ["weight", "enc.a", "enc.b", "dec.c"])
                assert [s["numel"] for s in stats] == [3, 35, 1, 64]
                assert [(s["lr_scale"], s["weight_decay_scale"]) for s in stats] == (pairs if scales else [(1.0, 1.0)] * 4)
                total, bound = 0.0, 0.0
                for s, gr, q in zip(stats, g_host, params):
                    ref = float((gr.double() ** 2).sum())
                    tol = 0.0 if integer else s["numel"] * 2.0 ** -53 * ref
                    assert abs(s["grad_sq_sum"] - ref) <= tol and s["grad_norm"] == math.sqrt(s["grad_sq_sum"])
                    assert s["grad_amax"] == float(gr.abs().max()) and s["nonfinite"] == 0
                    wref = float((q.detach().cpu().double() ** 2).sum())
                    assert abs(s["weight_norm"] ** 2 - wref) <= 4 * 2.0 ** -52 * wref + s["numel"] * 2.0 ** -53 * wref
                    total += s["grad_sq_sum"]
                    bound += tol
                S_global = float(opt._norm_work[0])                                        # the norm launch's fp64 sum of the same step
                n_all = opt.flatp.total
                assert abs(total - S_global) <= (0.0 if integer else bound + n_all * 2.0 ** -53 * S_global + 4 * 2.0 ** -53 * total)
                if integer:
                    assert opt.grad_stats()["grad_norm"] == float(np.float32(math.sqrt(total)))
                assert all(s["weight_norm"] == 0.0 for s in opt.tensor_stats(with_weights=False))
                opt.zero_grad()
                opt.set_index_space(names, local)
            K.set_grad_sink(None)
    finally:
        K.set_grad_sink(None)


# ---- 7. the entry point ------------------------------------------------------------------------------------------------------------------------------
def _train_edges(tmp_path, capsys, log_tensor_stats, resume):
    """train_edges.py <the fine-tuning YAML> --synthetic as tests/test_gpu_optimizer_family.py runs the AdamW YAML (frame size, batch and
    checkpoint folder set for the test; a log line per step): two steps and a checkpoint, with `resume` a resume for two more.
    -> (the captured output of every run, the checkpoints)"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    with open(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_finetune.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["model"]["optimizer"]["tensor_scales"] == [{"max_ndim": 1, "weight_decay_scale": 0.0}, {"pattern": r"^encoder\.", "lr_scale": 0.1}]
    cfg["model"]["optimizer"]["log_tensor_stats"] = log_tensor_stats
    cfg["arch"]["log_every"] = 1
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

    outs = [run(["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1", "--save", save])]
    ckpts = [load_checkpoint(os.path.join(save, "epoch=0.ckpt"))]
    if resume:
        outs.append(run(["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1", "--save", save, "--resume",
                         os.path.join(save, "epoch=0.ckpt")]))
        ckpts.append(load_checkpoint(os.path.join(save, "epoch=1.ckpt")))
    return outs, ckpts


def test_train_edges_finetune_yaml_two_synthetic_steps_resume_and_the_log_lines(tmp_path, capsys):
    outs, (ckpt, ck2) = _train_edges(tmp_path, capsys, 3, True)
    for out in outs:
        assert "'steps': 2" in out
        lines = out.splitlines()
        at = [i for i, l in enumerate(lines) if l.startswith("step ")]
        assert len(at) == 2
        for i in at:                                                      # after each log line: the three largest, by reference name
            top = lines[i + 1:i + 4]
            assert [l.split(" | ")[0] for l in top] == ["  grad top 1", "  grad top 2", "  grad top 3"], top
            assert all(l.split(" | ")[1].startswith(("encoder.", "decoder.")) for l in top)
            norms = [float(l.split("| norm ")[1].split(" |")[0]) for l in top]
            assert norms == sorted(norms, reverse=True) and norms[0] > 0.0
            assert all(("lr x0.1" in l) == l.split(" | ")[1].startswith("encoder.") for l in top)
        assert "grad non-finite" not in out
    assert ckpt["epoch"] == 0 and ck2["epoch"] == 1
    for ck, steps in ((ckpt, 2), (ck2, 4)):                               # the file is torch.optim.AdamW's, one group, as without the rules
        groups = ck["optimizer"]["param_groups"]
        assert len(groups) == 1 and groups[0]["weight_decay"] == 0.01 and groups[0]["lr"] == 0.0001 and groups[0]["name"] == "Depth"
        assert not any("scale" in k or "seg" in k for k in groups[0])
        assert {int(float(st["step"])) for st in ck["optimizer"]["state"].values()} == {steps}
    moved = {k: float((ck2["state_dict"][k].float() - ckpt["state_dict"][k].float()).abs().max()) for k in ckpt["state_dict"]}
    assert 0 < max(moved.values()) < 1e-2
    # Adam moves a weight by about lr per step: the encoder's largest move is about a tenth of the decoder's
    enc = max(v for k, v in moved.items() if ".encoder." in k and k.endswith("weight"))
    dec = max(v for k, v in moved.items() if ".decoder." in k and k.endswith("weight"))
    assert 0 < enc < 0.3 * dec, (enc, dec)


def test_train_edges_without_log_tensor_stats_prints_what_it_always_printed(tmp_path, capsys):
    (out,), _ = _train_edges(tmp_path, capsys, 0, False)
    lines = [l for l in out.splitlines() if l.startswith(("step ", "  grad"))]
    assert len(lines) == 2 and all(l.startswith("step ") and "grad" not in l for l in lines) and "'steps': 2" in out
