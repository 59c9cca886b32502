"""Plain torch-CPU / numpy statements of the layout, reduction, weight-pack and optimizer helpers of include/mte_kernels.h, written from the
header comments (not from the kernels): what each entry point must leave in memory.  Activations are NHWC tensors [B,H,W,C] here.
tests/test_glue_ref_cpu.py pins every function that is not itself a single torch op to one (F.pixel_unshuffle, torch.optim.Adam, F.conv2d
and its input gradient, sum + permute, autograd of the nearest up-sampling); tests/test_gpu_glue_kernels.py compares the HIP kernels with them."""
import numpy as np
import torch
import torch.nn.functional as F


def round8(c):
    return (c + 7) // 8 * 8


def to_dtype(x, dtype):
    """Rounding of fp32 values to the activation type (torch rounds to nearest even, as the hardware conversion does)."""
    return x.to(dtype)


# ---- layout helpers ---------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(src, Cp, flip_w, dtype):
    """mte_nchw_to_nhwc: [B,C,H,W] fp32 -> [B,H,W,Cp] in `dtype`, channels C..Cp-1 zero, optionally mirrored along W."""
    B, C, H, W = src.shape
    s = src.flip(-1) if flip_w else src
    out = torch.zeros(B, H, W, Cp, dtype=dtype)
    out[..., :C] = to_dtype(s.permute(0, 2, 3, 1), dtype)
    return out


def nearest_up2(inv):
    """[B,h,w] -> [B,2h,2w], every value repeated over its 2x2 block (mte_upsample2_f32; channel 0 of mte_upsample_inv_fwd)."""
    return inv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample_inv_fwd(inv, dtype):
    """mte_upsample_inv_fwd: the 8-channel block [B,2h,2w,8] = (nearest_up2(inv), 0, ..., 0) in `dtype`."""
    up = nearest_up2(inv)
    out = torch.zeros(up.shape + (8,), dtype=dtype)
    out[..., 0] = to_dtype(up, dtype)
    return out


def upsample_inv_bwd(d0):
    """adjoint of nearest_up2: [B,2h,2w] -> [B,h,w] sums of the 2x2 blocks, in float64."""
    B, H2, W2 = d0.shape
    return d0.double().reshape(B, H2 // 2, 2, W2 // 2, 2).sum(dim=(2, 4))


def pixel_unshuffle_nhwc(x):
    """mte_pixel_shuffle dir 0: x [B,H,W,C] -> P [B,H/2,W/2,4C] with P[b,h,w,4c + 2dy + dx] = x[b,2h+dy,2w+dx,c]."""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, 4 * C)


def pixel_shuffle_nhwc(p):
    """mte_pixel_shuffle dir 1: the inverse of pixel_unshuffle_nhwc."""
    B, H2, W2, C4 = p.shape
    C = C4 // 4
    return p.reshape(B, H2, W2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H2, 2 * W2, C)


def copy_rect(dst, src, sy, sx, dy, dx, h, w, mode):
    """mte_copy_rect on NHWC tensors, in place on `dst`: mode 0 copy, 1 add (fp32 sum, rounded once), 2 zero (src unused)."""
    if mode == 2:
        dst[:, dy:dy + h, dx:dx + w] = 0
    elif mode == 0:
        dst[:, dy:dy + h, dx:dx + w] = src[:, sy:sy + h, sx:sx + w]
    else:
        dst[:, dy:dy + h, dx:dx + w] = (dst[:, dy:dy + h, dx:dx + w].float() + src[:, sy:sy + h, sx:sx + w].float()).to(dst.dtype)
    return dst


# ---- weight packs -----------------------------------------------------------------------------------------------------------------------
def pack_fwd(w, Cin_p, dtype):
    """forward pack [Cout][taps][Cin_p]: wf[n][tap][c] = round(w[n][c][tap]), zeros for c >= Cin."""
    Cout, Cin, KH, KW = w.shape
    wf = torch.zeros(Cout, KH * KW, Cin_p, dtype=dtype)
    for n in range(Cout):
        for c in range(Cin):
            wf[n, :, c] = to_dtype(w[n, c].reshape(-1), dtype)
    return wf


def pack_bwd(wf):
    """data-gradient pack [Cin_p][taps rotated by 180 degrees][Cout]: wb[c][taps - 1 - tap][n] = wf[n][tap][c]."""
    Cout, taps, Cin_p = wf.shape
    wb = torch.zeros(Cin_p, taps, Cout, dtype=wf.dtype)
    for tap in range(taps):
        wb[:, taps - 1 - tap, :] = wf[:, tap, :].t()
    return wb


def conv_from_pack(x, pack, k):
    """y[b,n,y,x] = sum over (tap = ky*k + kx, c) of pack[n][tap][c] * xpad[b,c,y+ky,x+kx]: how the convolution kernels read a pack
    (x: [B,C,H,W] with C = pack.shape[2] channels, zero padding k//2)."""
    B, C, H, W = x.shape
    xp = F.pad(x, (k // 2,) * 4)
    cols = torch.stack([xp[:, :, ky:ky + H, kx:kx + W] for ky in range(k) for kx in range(k)], dim=1)   # [B,taps,C,H,W]
    return torch.einsum("ntc,btchw->bnhw", pack, cols)


def unpack_wgrad(stage, Cin):
    """mte_unpack_conv_wgrad: stage [parts][Cout][taps][Cin_p] -> float64 [Cout][Cin][taps] = sum over the parts, channel padding dropped."""
    parts, Cout, taps, Cin_p = stage.shape
    out = np.zeros((Cout, Cin, taps), np.float64)
    st = stage.double().numpy()
    for p in range(parts):
        for c in range(Cin):
            out[:, c, :] += st[p, :, :, c]
    return torch.from_numpy(out)


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64 on fp32 inputs.  The scalar arguments travel to the entry point as C
    floats, so they enter here at their float32 values; everything after that is float64.
    -> (p_new, m_new, v_new, dp) with dp = p - p_new, the update."""
    f = lambda s: float(np.float32(s))
    lr, beta1, beta2, eps, gscale = f(lr), f(beta1), f(beta2), f(eps), f(gscale)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * gscale
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    dp = (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    return p - dp, m, v, dp


def adam_hyper(lr, beta1, beta2, step):
    """what mte_adam_step_dev reads from device memory: float32({lr, 1 - beta1^t, sqrt(1 - beta2^t)}), formed in double from the float32 betas."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return torch.tensor([float(np.float32(lr)), 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5], dtype=torch.float64).float()


# ---- bilinear resize, silog ----------------------------------------------------------------------------------------------------------------
def resize_bilinear(x, H, W):
    """F.interpolate(mode='bilinear', align_corners=False) of [B,h,w] in float64 (differentiable)."""
    return F.interpolate(x.double()[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]


def silog(inv, depth):
    """'sparse-silog' on one scale in float64 (oracle/loss_oracle.py, pinned against the reference by tests/test_oracle_golden.py);
    differentiable in `inv`."""
    from oracle import loss_oracle as lo
    return lo.supervised_silog_loss(inv, depth.double())
