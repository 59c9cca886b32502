"""Plain float64 statements of the optimizer family of csrc/optim.hip on fp32 inputs, in the style of glue_ref.adam_step: the scalar
arguments travel to the entry points as C floats, so they enter here at their float32 values; ``gscale`` multiplies the gradient first;
everything after that is float64.  tests/test_optimizer_family_cpu.py pins these against torch.optim.Adam / AdamW / SGD in float64; the
GPU tests (tests/test_gpu_optimizer_family.py) hold the kernels to them."""
import numpy as np
import torch


def _f(s):
    return float(np.float32(s))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale, weight_decay=0.0, decoupled=False):
    """torch.optim.Adam(weight_decay) (decoupled=False: g' = g * gscale + wd * p) or torch.optim.AdamW (decoupled=True:
    p * (1 - lr * wd) first), no amsgrad.  -> (p_new, m_new, v_new, dp) with dp = p - p_new, the whole update (decay included)."""
    lr, beta1, beta2, eps, gscale, wd = _f(lr), _f(beta1), _f(beta2), _f(eps), _f(gscale), _f(weight_decay)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * gscale
    if wd != 0.0 and not decoupled:
        g = g + wd * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    dp = (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    if wd != 0.0 and decoupled:
        dp = dp + lr * wd * p                                # p * (1 - lr * wd) - step
    return p - dp, m, v, dp


def adam_hyper(lr, beta1, beta2, step):
    """what mte_adam_step_dev / mte_adamw_step_dev read from device memory: float32({lr, 1 - beta1^t, sqrt(1 - beta2^t)}), formed in
    double from the float32 betas."""
    b1, b2 = _f(beta1), _f(beta2)
    return torch.tensor([_f(lr), 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5], dtype=torch.float64).float()


def sgd_step(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, step, gscale):
    """torch.optim.SGD: g' = g * gscale + wd * p; with momentum, buf = g' at step 1 and momentum * buf + (1 - dampening) * g'
    afterwards, g'' = g' + momentum * buf under Nesterov, else buf; p -= lr * g''.  `buf` may be None when momentum is 0.
    -> (p_new, buf_new or None, dp) with dp = p - p_new."""
    lr, mu, damp, wd, gscale = _f(lr), _f(momentum), _f(dampening), _f(weight_decay), _f(gscale)
    p, g = p.double(), g.double()
    g = g * gscale
    if wd != 0.0:
        g = g + wd * p
    if mu != 0.0:
        buf = g.clone() if step == 1 else mu * buf.double() + (1.0 - damp) * g
        g = g + mu * buf if nesterov else buf
    else:
        buf = None
    dp = lr * g
    return p - dp, buf, dp


def sgd_hyper(lr, momentum, dampening, step):
    """what mte_sgd_step_dev reads from device memory: float32({lr, mu_eff, (1 - dampening)_eff}) = {lr, 0, 1} at step 1 and
    {lr, momentum, 1 - dampening} afterwards, the difference formed in double from the float32 dampening."""
    first = step == 1
    return torch.tensor([_f(lr), 0.0 if first else _f(momentum), 1.0 if first else 1.0 - _f(dampening)], dtype=torch.float64).float()
