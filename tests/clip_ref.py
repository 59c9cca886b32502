"""Plain float64 statement of mte_grad_norm_clip (csrc/optim.hip) on fp32 inputs, in the style of optim_ref: the scalar arguments travel to
the entry point as C floats, so they enter here at their float32 values; everything after that is float64.

    S = sum g^2;  norm = |gscale| * sqrt(S);  coef = max_norm / (norm + 1e-6), replaced by 1 where that is > 1

which is torch.nn.utils.clip_grad_norm_'s ``clamp(max_norm / (total_norm + 1e-6), max=1.0)`` over the gradients scaled by gscale: an inf in
the gradient gives coef 0 (NaN when max_norm is inf too), a NaN gives NaN.  tests/test_grad_clip_cpu.py pins this against torch on float64
copies; the GPU tests (tests/test_gpu_grad_clip.py) hold the kernel to it."""
import numpy as np
import torch


def _f(s):
    return float(np.float32(s))


def grad_norm_clip(g, gscale, max_norm):
    """-> {'S', 'norm', 'coef'} as Python floats (float64)"""
    gscale, max_norm = _f(gscale), _f(max_norm)
    S = float((g.double().flatten() ** 2).sum())
    norm = abs(gscale) * float(np.sqrt(np.float64(S)))
    with np.errstate(invalid="ignore"):
        coef = float(np.float64(max_norm) / (np.float64(norm) + 1e-6))
    if coef > 1.0:
        coef = 1.0
    return {"S": S, "norm": norm, "coef": coef}


def ctl(g, gscale, max_norm, skip_nonfinite, skipped_before=0.0):
    """the four floats the kernel leaves: float32({coef, skip flag, norm, skipped steps})"""
    r = grad_norm_clip(g, gscale, max_norm)
    skip = bool(skip_nonfinite) and not np.isfinite(r["S"])
    with np.errstate(over="ignore"):
        return np.array([r["coef"], 1.0 if skip else 0.0, r["norm"], skipped_before + (1.0 if skip else 0.0)], dtype=np.float64).astype(np.float32)
