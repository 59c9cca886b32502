"""Guard bands for tests that call the raw C ABI (tests/test_gpu_glue_kernels.py, tests/test_gpu_groupnorm_layout.py).

Every output and in/out buffer is allocated wider (extra channels per pixel on both sides of the slice, `ld > C`) and longer (a tail of
pixels / of elements behind the last one) than the kernel may touch and pre-filled with a NaN bit pattern; afterwards the band is compared
bitwise through an integer view.  A NaN that a kernel reads where it should only write shows up in the result as well."""
import torch

import glue_ref as R

_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
_SENT = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5}      # NaN bit patterns


def beq(a, b):
    """bit equality of two CPU tensors of one type"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype]))


class Band:
    """NHWC activation [B,H,W,C] as the channel slice [c0, c0 + C) of a buffer with ld = c0 + C + pad elements per pixel and `tail` further
    pixels behind the last one (default: one row, W; the GroupNorm layout tests ask for a whole sample, H * W, so that an index that is off by one
    sample or one pixel range still lands in allocated memory), everything pre-filled with the NaN pattern."""

    def __init__(self, B, H, W, C, dtype, c0=8, pad=8, tail=None):
        from mindtheedge_amd import kernels as K
        self.B, self.H, self.W, self.C, self.c0, self.dtype = B, H, W, C, c0, dtype
        self.ld = R.round8(c0 + C) + pad
        self.npix = B * H * W
        tail = W if tail is None else tail
        self.raw = torch.full((self.npix + tail, self.ld), _SENT[dtype], dtype=_INT[dtype], device="cuda")
        self.t = self.raw.view(dtype)
        self.nhwc = self.t[:self.npix].view(B, H, W, self.ld)
        self.view = K.channel_slice(self.nhwc.permute(0, 3, 1, 2), c0, c0 + C)        # logical [B,C,H,W], as the host hands it to the library
        self.ptr = self.view.data_ptr()
        if H > 1 and W > 1:
            assert K._pl(self.view) == (self.ptr, self.ld)

    def set(self, vals):
        self.nhwc[..., self.c0:self.c0 + self.C] = vals.to(self.dtype).cuda()
        return self

    def get(self):
        return self.nhwc[..., self.c0:self.c0 + self.C].cpu()

    def guard_ok(self):
        m = torch.ones_like(self.raw, dtype=torch.bool)
        m[:self.npix, self.c0:self.c0 + self.C] = False
        return bool((self.raw[m] == _SENT[self.dtype]).all())

    def untouched(self):
        return bool((self.raw == _SENT[self.dtype]).all())


class Flat:
    """n elements followed by `extra` guard elements, pre-filled with the NaN pattern"""

    def __init__(self, n, dtype=torch.float32, extra=64):
        self.n, self.dtype = n, dtype
        self.raw = torch.full((n + extra,), _SENT[dtype], dtype=_INT[dtype], device="cuda")
        self.t = self.raw.view(dtype)
        self.ptr = self.t.data_ptr()

    def set(self, vals):
        self.t[:self.n] = vals.flatten().to(self.dtype).cuda()
        return self

    def get(self):
        return self.t[:self.n].cpu()

    def guard_ok(self):
        return bool((self.raw[self.n:] == _SENT[self.dtype]).all())

    def untouched(self):
        return bool((self.raw == _SENT[self.dtype]).all())
