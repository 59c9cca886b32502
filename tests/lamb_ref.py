"""Plain float64 statement of the LAMB step of csrc/optim.hip (mte_lamb_moments + mte_lamb_apply) on fp32 inputs, in the style of
tests/optim_ref.py: the scalar arguments travel to the entry points as C floats, so they enter here at their float32 values; ``gscale``
multiplies the gradient first; everything after that is float64, except the two places where the kernels round a per-tensor scalar to
float32 by definition -- lr_t = float32(lr * lr_mult), wd_t = float32(weight_decay * wd_mult) -- and the trust ratio q_t = float32(r_t).

Per tensor t = elements [begin, begin + numel) of the flat buffers, with table row {lr_mult, wd_mult, adapt}:
    g' = g * gscale;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g'
    d  = (lr_t / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))  [+ (lr_t * wd_t) * p  when wd_t != 0]     -- optim_ref.adam_step's dp, decoupled
    S_p = sum p^2,  S_d = sum d^2
    r  = lr_t * sqrt(S_p) / sqrt(S_d)  if adapt and S_p > 0 and S_d > 0  else 1;   max_trust > 0: r = min(r, max_trust)
    p  = p - q * d,  q = float32(r)
Elements outside every tensor (the padding) keep p, m and v.  tests/test_lamb_cpu.py pins this against the paper's Algorithm 2 and, with
every tensor excluded, against optim_ref.adam_step; tests/test_gpu_lamb.py holds the kernels to it."""
import numpy as np
import torch


def _f(s):
    return float(np.float32(s))


def lamb_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale, weight_decay, begins, numels, table, max_trust=0.0, round_trust=True):
    """One step over flat buffers.  table: [(lr_mult, wd_mult, adapt)] per tensor.  round_trust=False keeps q = r in float64 (the
    comparison with the paper's form, which knows no float32).
    -> (p_new, m_new, v_new, dp, trust, sums): dp = p - p_new (the applied update q * d), trust = [q_t], sums = [(S_p, S_d)]."""
    lr, beta1, beta2, eps, gscale, wd, max_trust = _f(lr), _f(beta1), _f(beta2), _f(eps), _f(gscale), _f(weight_decay), _f(max_trust)
    p, g, m, v = (t.double().clone() for t in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    dp = torch.zeros_like(p)
    trust, sums = [], []
    for b, n, (lr_mult, wd_mult, adapt) in zip(begins, numels, table):
        sl = slice(int(b), int(b) + int(n))
        lr_t = float(np.float32(lr) * np.float32(lr_mult))
        wd_t = float(np.float32(wd) * np.float32(wd_mult))
        gk = g[sl] * gscale
        m[sl] = beta1 * m[sl] + (1.0 - beta1) * gk
        v[sl] = beta2 * v[sl] + (1.0 - beta2) * gk * gk
        d = (lr_t / bc1) * (m[sl] / (v[sl].sqrt() / bc2 ** 0.5 + eps))
        if wd_t != 0.0:
            d = d + lr_t * wd_t * p[sl]
        s_p, s_d = float((p[sl] * p[sl]).sum()), float((d * d).sum())
        r = lr_t * s_p ** 0.5 / s_d ** 0.5 if (adapt and s_p > 0.0 and s_d > 0.0) else 1.0
        if max_trust > 0.0:
            r = min(r, max_trust)
        q = _f(r) if round_trust else r
        dp[sl] = q * d
        trust.append(q)
        sums.append((s_p, s_d))
    return p - dp, m, v, dp, trust, sums
