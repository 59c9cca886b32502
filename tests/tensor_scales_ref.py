"""Plain float64 statement of the SEG optimizer steps of csrc/optim.hip (mte_adamw_step_seg_dev, mte_sgd_step_seg_dev): per-tensor
multipliers of the learning rate and the weight decay.  It is optim_ref's step applied tensor by tensor with the per-class scalars the
kernel forms in fp32 -- lr_c = float32(lr32 * lm32), wd_c = float32(wd32 * wm32), one rounding each -- and everything after that in
float64.  wd_c = 0 is optim_ref's no-decay arithmetic.  tests/test_tensor_scales_cpu.py pins it against torch.optim.Adam / AdamW / SGD
with PARAM GROUPS in float64; the GPU tests hold the kernels, slice by slice, to the plain entry points that optim_ref already pins."""
import numpy as np

import optim_ref as R


def class_scalars(lr, weight_decay, lr_mult, wd_mult):
    """(lr_c, wd_c) as Python floats that hold float32 values: one fp32 multiplication each, of the float32 arguments"""
    lr_c = np.float32(lr) * np.float32(lr_mult)
    wd_c = np.float32(weight_decay) * np.float32(wd_mult)
    assert lr_c.dtype == np.float32 and wd_c.dtype == np.float32
    return float(lr_c), float(wd_c)


def adam_step(ps, gs, ms, vs, pairs, lr, beta1, beta2, eps, step, gscale, weight_decay=0.0, decoupled=False):
    """one SEG Adam / AdamW step over lists of tensors, pairs[i] = (lr_mult, wd_mult) of tensor i -> (ps, ms, vs, dps) as lists"""
    out = ([], [], [], [])
    for p, g, m, v, (lm, wm) in zip(ps, gs, ms, vs, pairs):
        lr_c, wd_c = class_scalars(lr, weight_decay, lm, wm)
        for o, x in zip(out, R.adam_step(p, g, m, v, lr_c, beta1, beta2, eps, step, gscale, wd_c, decoupled)):
            o.append(x)
    return out


def sgd_step(ps, gs, bufs, pairs, lr, momentum, dampening, weight_decay, nesterov, step, gscale):
    """one SEG SGD step over lists of tensors (bufs[i] may be None when momentum is 0) -> (ps, bufs, dps) as lists"""
    out = ([], [], [])
    for p, g, b, (lm, wm) in zip(ps, gs, bufs, pairs):
        lr_c, wd_c = class_scalars(lr, weight_decay, lm, wm)
        for o, x in zip(out, R.sgd_step(p, g, b, lr_c, momentum, dampening, wd_c, nesterov, step, gscale)):
            o.append(x)
    return out
