"""CPU: every reference of tests/glue_ref.py that is not a single torch op, pinned to one -- so that a reference and the HIP kernel it
judges (tests/test_gpu_glue_kernels.py) cannot share a mistake."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("shape", [(2, 8, 2, 2), (2, 16, 6, 10), (1, 40, 18, 34)])
def test_pixel_shuffle_reference_is_torch_pixel_unshuffle(shape):
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=_g(1))                     # NCHW for torch, NHWC for the reference
    want = F.pixel_unshuffle(x, 2)                                   # channel c * 4 + 2 dy + dx
    got = R.pixel_unshuffle_nhwc(x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(got, want.permute(0, 2, 3, 1))
    back = R.pixel_shuffle_nhwc(got)
    assert torch.equal(back, F.pixel_shuffle(want, 2).permute(0, 2, 3, 1))
    assert torch.equal(back, x.permute(0, 2, 3, 1))


def test_nchw_to_nhwc_reference():
    x = torch.randn(2, 3, 4, 5, generator=_g(2))
    for flip in (0, 1):
        out = R.nchw_to_nhwc(x, 16, flip, torch.bfloat16)
        src = x.flip(-1) if flip else x
        assert torch.equal(out[..., :3].permute(0, 3, 1, 2), src.to(torch.bfloat16))
        assert not out[..., 3:].any()


def test_nearest_up2_and_its_adjoint():
    inv = torch.randn(2, 3, 5, generator=_g(3), dtype=torch.float64)
    assert torch.equal(R.nearest_up2(inv), F.interpolate(inv[:, None], scale_factor=2, mode="nearest")[:, 0])
    assert torch.equal(R.upsample_inv_fwd(inv.float(), torch.float32)[..., 0], R.nearest_up2(inv.float()))
    assert not R.upsample_inv_fwd(inv.float(), torch.float32)[..., 1:].any()
    x = inv.clone().requires_grad_(True)
    d = torch.randint(-8, 9, (2, 6, 10), generator=_g(4)).double()   # integers: the block sums are exact in any order
    (R.nearest_up2(x) * d).sum().backward()
    assert torch.equal(R.upsample_inv_bwd(d), x.grad)


@pytest.mark.parametrize("hyper", [(1e-4, 0.9, 0.999, 1e-8, 1.0), (3e-2, 0.5, 0.9, 1e-3, 0.25)])
def test_adam_reference_is_torch_optim_adam(hyper):
    lr, b1, b2, eps, gscale = hyper
    f = lambda s: float(np.float32(s))                               # the reference takes its scalars at their float32 values
    p0 = torch.randn(37, generator=_g(5))
    param = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([param], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps))
    p, m, v = p0.double(), torch.zeros(37, dtype=torch.float64), torch.zeros(37, dtype=torch.float64)
    for step in range(1, 6):
        g = torch.randn(37, generator=_g(10 + step))
        g[::5] = 0.0
        param.grad = g.double() * f(gscale)
        opt.step()
        p_new, m, v, dp = R.adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale)
        assert torch.equal(p - dp, p_new)
        p = p_new
        torch.testing.assert_close(p, param.detach(), rtol=1e-13, atol=1e-15)
    h = R.adam_hyper(lr, b1, b2, 3)
    assert h.dtype == torch.float32 and float(h[0]) == f(lr)
    assert abs(float(h[1]) - (1 - f(b1) ** 3)) < 1e-7 and abs(float(h[2]) - (1 - f(b2) ** 3) ** 0.5) < 1e-7


@pytest.mark.parametrize("shape", [(8, 3, 5), (32, 65, 3), (72, 8, 1), (16, 130, 7)])
def test_pack_layouts_reproduce_conv2d_and_its_input_gradient(shape):
    Cout, Cin, k = shape
    Cin_p = R.round8(Cin)
    g = _g(6)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    x = torch.randn(2, Cin, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, Cout, 5, 6, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, padding=k // 2)
    (y * dy).sum().backward()
    wf = R.pack_fwd(w, Cin_p, torch.float64)
    assert wf.shape == (Cout, k * k, Cin_p) and not wf[:, :, Cin:].any()
    xp = F.pad(x.detach(), (0, 0, 0, 0, 0, Cin_p - Cin))             # the padded channels the kernels read
    torch.testing.assert_close(R.conv_from_pack(xp, wf, k), y.detach(), rtol=1e-12, atol=1e-12)
    wb = R.pack_bwd(wf)
    assert wb.shape == (Cin_p, k * k, Cout)
    dx = R.conv_from_pack(dy, wb, k)                                 # the data gradient is the same convolution with the other pack
    torch.testing.assert_close(dx[:, :Cin], x.grad, rtol=1e-12, atol=1e-12)
    assert not dx[:, Cin:].any()
    # rounding happens per element, before the layout change
    assert torch.equal(R.pack_fwd(w.float(), Cin_p, torch.bfloat16), R.pack_fwd(w.float().bfloat16().float(), Cin_p, torch.bfloat16))


def test_unpack_reference_is_sum_and_transpose():
    g = _g(7)
    stage = torch.randint(-8, 9, (5, 8, 9, 72), generator=g).float()
    want = stage.double().sum(0)[:, :, :65].permute(0, 2, 1)
    assert torch.equal(R.unpack_wgrad(stage, 65), want)


def test_copy_rect_reference():
    g = _g(8)
    src = torch.randint(-8, 9, (2, 4, 6, 8), generator=g).float()
    dst0 = torch.randint(-8, 9, (2, 5, 7, 8), generator=g).float()
    for mode in (0, 1, 2):
        d = R.copy_rect(dst0.clone(), src, 1, 2, 2, 3, 2, 3, mode)
        inside = d[:, 2:4, 3:6]
        want = {0: src[:, 1:3, 2:5], 1: dst0[:, 2:4, 3:6] + src[:, 1:3, 2:5], 2: torch.zeros(2, 2, 3, 8)}[mode]
        assert torch.equal(inside, want)
        d[:, 2:4, 3:6] = dst0[:, 2:4, 3:6]
        assert torch.equal(d, dst0)


def test_bilinear_reference_is_interpolate_and_silog_is_the_oracle():
    x = torch.randn(3, 5, 7, generator=_g(9))
    y = R.resize_bilinear(x, 12, 20)
    assert y.dtype == torch.float64 and y.shape == (3, 12, 20)
    assert torch.equal(y, F.interpolate(x.double()[:, None], size=(12, 20), mode="bilinear", align_corners=False)[:, 0])
    inv = torch.rand(50, generator=_g(11), dtype=torch.float64) + 0.1
    depth = 1.0 / (torch.rand(50, generator=_g(12)) + 0.1)
    depth[::4] = 0.0
    ok = depth > 0
    d = torch.log((inv[ok] + 1e-5) * 10) - torch.log(10 / depth[ok].double())
    want = 10 * torch.sqrt((d * d).mean() - 0.85 * d.mean() ** 2)
    torch.testing.assert_close(R.silog(inv, depth), want, rtol=1e-12, atol=0)
