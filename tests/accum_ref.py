"""Reference for gradient accumulation (FusedFlatOptimizer(accumulate_grad_batches > 1), csrc/optim.hip::mte_grad_accumulate): the gradient
an accumulated step consumes is the SEQUENTIAL fp32 sum (((g0 + g1) + ...) + g_j) per element, every addition rounded once -- stated here
in NumPy float32 -- and the step is the plain step of tests/optim_ref.py on that sum with gscale = 1 / (world * (j + 1)).  ``self_check``
pins both on hand-computed elements; tests/test_grad_accum_cpu.py runs it."""
import numpy as np
import torch

import optim_ref as R


def sequential_sum(grads):
    """[g0, g1, ...] (float32 tensors of one shape) -> (((g0 + g1) + ...) + g_j) in float32, one rounding per addition"""
    acc = grads[0].detach().cpu().numpy().astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for g in grads[1:]:
            acc = (acc + g.detach().cpu().numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy(acc)


def group_scale(n_micro, world=1):
    """the gradient scale of a step that closes a group of n_micro micro-batches: formed in double, as the optimizer forms it"""
    return 1.0 / (world * n_micro)


def adam_step(p, grads, m, v, lr, beta1, beta2, eps, step, weight_decay=0.0, decoupled=False, world=1):
    """optim_ref.adam_step on the sequential sum of `grads`, averaged over the group"""
    return R.adam_step(p, sequential_sum(grads), m, v, lr, beta1, beta2, eps, step, group_scale(len(grads), world), weight_decay, decoupled)


def sgd_step(p, grads, buf, lr, momentum, dampening, weight_decay, nesterov, step, world=1):
    """optim_ref.sgd_step on the sequential sum of `grads`, averaged over the group"""
    return R.sgd_step(p, sequential_sum(grads), buf, lr, momentum, dampening, weight_decay, nesterov, step, group_scale(len(grads), world))


def self_check():
    """three elements whose fp32 sum depends on the order, worked by hand (u = 2^-24; ties go to the even mantissa):
         [1, u, u]         (1 + u) -> 1 (tie, even), 1 + u -> 1               : 1            (the exact sum is 1 + 2u)
         [u, u, 1]         u + u = 2u exactly, 2u + 1 = 1 + 2^-23 exactly      : 1 + 2^-23
         [2^24, 1, 1]      2^24 + 1 -> 2^24 (tie, even), again                : 2^24         (1 + 1 + 2^24 = 2^24 + 2 is representable)
       and a plain SGD step on a group of two: p = 1, lr = 0.5, gradients 1 and 2: sum 3, scale 1/2, p - 0.5 * 1.5 = 0.25."""
    u = 2.0 ** -24
    cols = [[1.0, u, 2.0 ** 24], [u, u, 1.0], [u, 1.0, 1.0]]
    got = sequential_sum([torch.tensor(c, dtype=torch.float32) for c in cols])
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -23, 2.0 ** 24], got.tolist()
    rev = sequential_sum([torch.tensor(c, dtype=torch.float32) for c in cols[::-1]])
    assert rev.tolist() == [1.0 + 2.0 ** -23, 1.0, 2.0 ** 24 + 2.0], rev.tolist()                  # another order, another sum
    assert group_scale(2) == 0.5 and group_scale(2, world=2) == 0.25 and group_scale(1) == 1.0
    p, buf, dp = sgd_step(torch.tensor([1.0]), [torch.tensor([1.0]), torch.tensor([2.0])], None, 0.5, 0.0, 0.0, 0.0, False, 1)
    assert buf is None and p.tolist() == [0.25] and dp.tolist() == [0.75]
    return True
