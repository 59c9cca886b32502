"""The fp64 statement of the GroupNorm(16)+ELU passes that the GPU tests compare with (tests/test_gpu_groupnorm.py,
tests/test_gpu_groupnorm_layout.py): torch-CPU autograd over nn.GroupNorm(16, C) + nn.ELU of Conv2D (layers01.py:32-38) and over the residual tail
with Dropout2d factors (layers01.py:62-73), and the per-(sample, group) error measure of the layout tests."""
import torch
import torch.nn.functional as F


def _reference(y1, y2, scale2, gamma, beta, dz):
    y1 = y1.double().requires_grad_(True)
    gamma, beta = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    v = y1
    if y2 is not None:
        y2 = y2.double().requires_grad_(True)
        v = y1 + y2 * scale2.double()[:, :, None, None]
    z = F.elu(F.group_norm(v, 16, gamma, beta, eps=1e-5))
    z.backward(dz.double())
    # bias gradient of the conv in front of the norm: column sums of d1 -- with a second input, of d2 (the shortcut conv's bias)
    return (z.detach(), y1.grad, None if y2 is None else y2.grad, gamma.grad, beta.grad, (y1.grad if y2 is None else y2.grad).sum(dim=(0, 2, 3)))


def _tail_reference(y1, s, scale, g1, b1, gt, bt, dz):
    y1, s = y1.double().requires_grad_(True), s.double().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in (g1, b1, gt, bt)]
    a = F.elu(F.group_norm(y1, 16, ps[0], ps[1], eps=1e-5))
    t = a + (s * scale.double()[:, :, None, None] if scale is not None else s)
    z = F.elu(F.group_norm(t, 16, ps[2], ps[3], eps=1e-5))
    z.backward(dz.double())
    return {"t": t.detach(), "z": z.detach(), "dy1": y1.grad, "ds": s.grad, "dg1": ps[0].grad, "db1": ps[1].grad, "dgt": ps[2].grad, "dbt": ps[3].grad,
            "dbias_s": s.grad.sum(dim=(0, 2, 3)), "dbias1": y1.grad.sum(dim=(0, 2, 3))}


def layout_reference(second, y1, y2, scale2, gamma, beta, dz):
    """(z, d1, d2, dgamma, dbeta, dbias) of one mte_gn_elu_fwd / _bwd pair.  second: 0 = one input; 1 = v = y1 + scale2 * y2; 2 = one input whose gradient also
    leaves scaled (the backward of the two-launch tail): d2 = scale2[b, c] * d1 and dbias = the column sums of d2 (include/mte_kernels.h, mte_gn_elu_bwd)."""
    if second == 1:
        return _reference(y1, y2, scale2, gamma, beta, dz)
    z, d1, _, dgamma, dbeta, dbias = _reference(y1, None, None, gamma, beta, dz)
    if second == 0:
        return z, d1, None, dgamma, dbeta, dbias
    d2 = d1 * scale2.double()[:, :, None, None]
    return z, d1, d2, dgamma, dbeta, d2.sum(dim=(0, 2, 3))


def slab_max(t):
    """[B, C, H, W] -> [B, 16]: max |t| over each (sample, group) slab of GroupNorm(16, C)"""
    B, C = t.shape[:2]
    return t.double().abs().reshape(B, 16, -1).amax(dim=2)


def slab_err(got, want):
    """the largest, over the (sample, group) slabs, of max |got - want| / max |want| -- both maxima over the same slab, so that a wrong small slab cannot hide
    behind a large one.  A slab whose reference is zero everywhere (a group of channels that Dropout2d removed altogether) counts 0 if `got` is zero there as
    well and infinity otherwise."""
    num, den = slab_max(got.double() - want.double()), slab_max(want)
    ratio = torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))
    return float(ratio.max())
