"""Exact references for the convolution kernels (tests/test_conv_exact_cpu.py, tests/test_gpu_conv_exact.py).  Imports without a GPU.

The method: operands that are small integers -- x, w in -3..3, output gradients in -24..24, fp32 bias in -1500..1500, old output values of that range as bf16 holds
them -- are exact in the type they are stored in,
and so is every product and every partial sum of the convolution as long as the sum of MAGNITUDES stays below 2^24 (assert_exact_in_fp32).  Then tile shape,
K order, the summation inside an MFMA and split-K slabs cannot change the fp32 value, and a kernel must give, bit for bit,
    rne(conv64 + bias)                          a plain launch
    rne(float(rne(conv64 + bias)) + old)        accumulate = 1 (two roundings: ConvArgs.accum, csrc/conv_args.hpp)
    conv64 + bias (+ old)                       fp32 outputs: out_f32, fp32 mode, weight and bias gradients
with conv64 the fp64 convolution of torch.  No tolerance anywhere, so nothing is measured."""
import functools

import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)


def _ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def int_operands(cin, cout, k, B, H, W, seed, xr=3, wr=3, gr=24, br=1500):
    """-> x [B, cin, H, W], w [cout, cin, k, k], bias [cout], dy and old [B, cout, H, W]: fp64 tensors of integers in +-xr, +-wr, +-br, +-gr, +-br; all but the
    bias (fp32 in every mode) are exact in bf16"""
    g = torch.Generator().manual_seed(seed)
    # (old is what an output buffer held before an accumulating launch: integers of that range which bf16 can hold -- above 256 not every integer is one)
    return (_ints((B, cin, H, W), xr, g), _ints((cout, cin, k, k), wr, g), _ints((cout,), br, g), _ints((B, cout, H, W), gr, g), rne(_ints((B, cout, H, W), br, g)))


def real_operands(cin, cout, k, B, H, W, seed):
    """x, w, bias uniform in [-1, 1], rounded to bf16 (exact in both compute types), as fp64"""
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.rand(s, generator=g) * 2 - 1).bfloat16().double() for s in ((B, cin, H, W), (cout, cin, k, k), (cout,)))


def conv64(x, w, bias=None):
    """the plain reference: fp64 convolution, stride 1, zero padding k // 2"""
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=w.shape[2] // 2)


def reference(x, w, bias, dy):
    """-> y, dx, dw, db in fp64: torch's convolution and its autograd"""
    x, w, b = (t.double().clone().requires_grad_(True) for t in (x, w, bias))
    y = conv64(x, w, b)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, b.grad


def tap_loop(x, w, bias):
    """the same operation stated a second time: one shifted product per filter tap and input channel"""
    B, C, H, W = x.shape
    N, _, k, _ = w.shape
    p = k // 2
    xp = torch.zeros(B, C, H + 2 * p, W + 2 * p, dtype=torch.float64)
    xp[:, :, p:p + H, p:p + W] = x
    y = bias.double().reshape(1, N, 1, 1).repeat(B, 1, H, W)
    for n in range(N):
        for c in range(C):
            for i in range(k):
                for j in range(k):
                    y[:, n] += w[n, c, i, j] * xp[:, c, i:i + H, j:j + W]
    return y


def assert_exact_in_fp32(x, w, bias=None, dy=None, old=None):
    """The precondition of the whole method: the same convolutions over ABSOLUTE values bound every partial sum a kernel can form, in any order; with |bias| and
    |old| added they must stay below 2^24, where fp32 holds every integer.  dy given: the data, weight and bias gradients too."""
    for t in (x, w, bias, dy, old):
        assert t is None or bool((t == t.round()).all()), "operands must be integers"
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.abs()
    if dy is None:
        bounds = [conv64(x.abs(), w.abs(), b)]
    else:
        bounds = list(reference(x.abs(), w.abs(), b, dy.abs()))
    if old is not None:
        bounds[0] = bounds[0] + old.abs()
    worst = max(float(t.max()) for t in bounds)
    assert worst < TWO24, "sum of magnitudes %g reaches 2^24: not exact in fp32" % worst
    return worst


def rne(t, dtype=torch.bfloat16):
    """t rounded to nearest even into `dtype`, as fp64 (torch's conversion is the rounding's definition here; fp64 -> fp32 -> bf16 rounds once for |integers| < 2^24)"""
    return t.to(torch.float32).to(dtype).double()


def truncate_bf16(t):
    """t (exact in fp32) with the low 16 bits dropped: what a kernel that truncates would store"""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def expected(conv_plus_bias, dtype, old=None):
    """what a launch must store: one rounding, or with accumulate the two roundings of the contract"""
    y = rne(conv_plus_bias, dtype)
    return y if old is None else rne(y + old, dtype)


def one_rounding(conv_plus_bias, dtype, old):
    """the accumulate result of a kernel that rounds ONCE (the mistake the two-rounding contract excludes)"""
    return rne(conv_plus_bias + old, dtype)


def strided_view(t, ld, c0, fill, dtype, device="cpu"):
    """NHWC activation with logical shape t.shape = [B, C, H, W] in channels [c0, c0 + C) of a buffer with `ld` channels per pixel, followed by a guard block of
    at least 4096 elements.  Everything outside the view holds `fill` (outputs: a finite sentinel; inputs: NaN, so that a read that crosses into a neighbour's
    channels surfaces as NaN in the result).  -> (view, whole buffer, check): check() asserts bit for bit that everything outside the view still holds `fill`."""
    B, C, H, W = t.shape
    assert 0 <= c0 and c0 + C <= ld
    pixels = B * H * W
    buf = torch.full((pixels * ld + 4096 + ld,), fill, dtype=dtype, device=device)
    view = buf.as_strided((B, C, H, W), (H * W * ld, 1, W * ld, ld), c0)
    view.copy_(t.to(dtype))
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    outside[:pixels * ld].view(pixels, ld)[:, c0:c0 + C] = False
    pattern = torch.full((1,), fill, dtype=dtype).view(bits)

    def check():
        now = buf.detach().cpu().view(bits)[outside]
        bad = int((now != pattern).sum())
        assert bad == 0, "%d elements outside the view were overwritten" % bad

    return view, buf, check


def pack_fwd(w, dtype):
    """OIHW -> the forward pack [N][taps][Cin] of mte_conv2d_igemm (tap = row-major (ky, kx)); integers: no rounding involved"""
    N, C, k, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(N, k * k, C).contiguous().to(dtype)


@functools.lru_cache(maxsize=None)
def cached(fn, *key):
    """one reference per case, shared by the tests that need it (callers do not modify what they get)"""
    return fn(*key)


# ---- 3a: layer level, default dispatch (cin, cout, k, B, H, W): one small shape per kernel family, from the lists of tests/test_gpu_conv_variants.py
LAYER_SHAPES = [
    (3, 32, 5, 1, 37, 96), (3, 16, 3, 2, 9, 32),                                                          # stem
    (65, 32, 3, 1, 9, 96), (32, 32, 3, 1, 24, 64), (48, 56, 5, 2, 9, 32), (32, 24, 7, 1, 21, 32), (32, 64, 1, 2, 8, 64),   # LDS-patch: 3x3, tall, 5x5 m16, 7x7, 1x1
    (72, 96, 3, 2, 9, 32),                                                                                # wide patch weight gradient
    (128, 128, 3, 2, 16, 64),                                                                             # nine-tap weight gradient
    (96, 256, 3, 3, 10, 52), (40, 256, 5, 1, 6, 168), (136, 264, 3, 2, 5, 80),                            # generic tiles, ragged rows and columns
    (1024, 512, 3, 1, 6, 20),                                                                             # long reduction with K split
]


# a 1x1 data gradient over 64 channels of +-24 stays mostly below 256, where bf16 holds every integer: wider gradients for that shape (the rounding must be exercised)
LAYER_RANGES = {(32, 64, 1, 2, 8, 64): dict(gr=96)}


def layer_case(shape):
    x, w, b, dy, _ = int_operands(*shape, seed=sum(shape), **LAYER_RANGES.get(shape, {}))
    return (x, w, b, dy) + reference(x, w, b, dy)


# ---- 3b: mte_conv2d_igemm through the C interface, one case per instance launch_plan (csrc/conv_igemm.hip) names.
# Every shape has a row tail (M = B H W is no multiple of the tile height), a column tail (N = 24 / 56 / 72 / 104 / 200) and, where the form allows it, an odd
# K-step count (K / 32; the one-state 8-phase loop needs Cin_p % 64 == 0, which makes it even).  `kernel`: the instance the case claims --
# conv_igemm_kernel<T, WM, WN, TM, TN, LD, RING, ..> as (form, loader, ring), conv_igemm8_kernel<BN, SM, ONE> as (form, slice-major, one-state).
# `splits`: {workspace slabs offered: K splits claimed}; tests/test_conv_exact_cpu.py proves both with the launch recorder.
TILE = {"128x32": (4, 1, 1, 1), "128x32_w2": (2, 1, 2, 1), "128x64": (2, 2, 2, 1), "128x128": (2, 2, 2, 2), "192x96": (2, 3, 3, 1), "256x128": (4, 2, 2, 2),
        "256x256_pp": (2, 4, 4, 2), "256x256_w16": (4, 4, 2, 2)}
OLD = [(6, 0), (23, 0)]                       # the four-wave tiles: no 256-row forms, no 8-phase kernels
P8 = [(23, 39), (24, 1), (6, 0)]              # 8-phase kernels on every eligible launch, tap-major
P8S = [(23, 39), (24, 1000000), (6, 0)]       # ... only where they split K


def _c(name, dt, cin_p, n, k, B, H, W, knobs, kernel, splits=None, solo=0, out_f32=0, split_only=False):
    # split_only: the launch reaches the claimed kernel only where it splits K -- the case has no variant without a workspace
    return dict(name=name, dt=dt, cin_p=cin_p, n=n, k=k, B=B, H=H, W=W, knobs=knobs, kernel=kernel, splits=splits or {}, solo=solo, out_f32=out_f32,
                split_only=split_only or knobs[:3] == P8S)


IGEMM_CASES = [
    _c("128x32-reg", "bf16", 40, 24, 5, 1, 9, 17, OLD, ("128x32", 0, 4), {2: 2, 8: 2}),
    _c("128x32-w2", "bf16", 96, 24, 5, 1, 9, 17, OLD, ("128x32_w2", 2, 4), {2: 2, 8: 4}),
    _c("128x64-ld2", "bf16", 96, 56, 5, 2, 9, 11, OLD, ("128x64", 2, 4), {2: 2, 8: 4}),
    _c("128x64-ld1", "bf16", 40, 56, 5, 2, 9, 11, OLD, ("128x64", 1, 4), {2: 2, 8: 2}),
    _c("128x64-ld0", "bf16", 96, 56, 5, 2, 9, 11, OLD + [(0, 0)], ("128x64", 0, 4), {2: 2, 8: 4}),
    _c("128x128-ld2", "bf16", 96, 104, 5, 2, 9, 11, OLD, ("128x128", 2, 4), {2: 2, 8: 4}),
    _c("128x128-ld1", "bf16", 40, 72, 5, 2, 9, 11, OLD, ("128x128", 1, 4), {2: 2, 8: 2}),
    _c("128x128-ld0", "bf16", 96, 200, 5, 2, 9, 11, OLD + [(0, 0)], ("128x128", 0, 4), {2: 2, 8: 4}),
    _c("192x96", "bf16", 96, 72, 3, 1, 13, 17, [(6, 3), (23, 0), (7, 1)], ("192x96", 2, 4)),
    _c("256x128-ring4", "bf16", 96, 104, 3, 2, 13, 11, [(6, 1), (23, 0), (7, 1)], ("256x128", 2, 4)),
    _c("256x128-ring3", "bf16", 96, 104, 3, 2, 13, 11, [(6, 1), (23, 0), (7, 1)], ("256x128", 2, 3), solo=1),
    _c("256x128-ring6", "bf16", 96, 104, 3, 2, 13, 11, [(6, 1), (23, 0), (7, 1), (15, 1)], ("256x128", 2, 6)),
    _c("256x256-pp", "bf16", 96, 200, 3, 2, 13, 11, [(6, 2), (23, 0), (7, 1), (21, 1)], ("256x256_pp", 2, 4)),
    _c("256x256-w16", "bf16", 96, 200, 3, 2, 13, 11, [(6, 2), (23, 0), (7, 1), (21, 0)], ("256x256_w16", 2, 4)),
    # the 16-wave loop under split-K is planned for 20 and more 256 x 256 tiles with a reduction of 128 and more K-steps: the smallest such launch (M N K = 2.9e9,
    # beyond the 5e8 of the other cases; its fp64 reference still takes a fraction of a second)
    _c("256x256-w16-split", "bf16", 480, 136, 3, 5, 7, 139, [(6, 2), (23, 0)], ("256x256_w16", 2, 4), {8: 8}, split_only=True),
    _c("p8-256x256-two", "bf16", 96, 200, 3, 2, 13, 11, P8, ("p8", 256, False, False)),
    _c("p8-256x256-one", "bf16", 64, 200, 3, 2, 13, 11, P8, ("p8", 256, False, True)),
    _c("p8-256x256-slice", "bf16", 64, 200, 3, 2, 13, 11, [(23, 7), (24, 1), (6, 0)], ("p8", 256, True, False)),
    _c("p8-256x128-two", "bf16", 96, 104, 3, 2, 13, 11, P8, ("p8", 128, False, False)),
    _c("p8-256x128-one", "bf16", 64, 104, 3, 2, 13, 11, P8, ("p8", 128, False, True)),
    _c("p8-256x128-slice", "bf16", 64, 104, 3, 2, 13, 11, [(23, 7), (24, 1), (6, 0)], ("p8", 128, True, False)),
    _c("p8-256x128-split-two", "bf16", 160, 200, 3, 2, 13, 11, P8S, ("p8", 128, False, False), {2: 2, 8: 2}),
    _c("p8-256x128-split-one", "bf16", 128, 200, 3, 2, 13, 11, P8S, ("p8", 128, False, True), {2: 2, 8: 2}),
    _c("p8-256x256-split-two", "bf16", 160, 200, 3, 2, 13, 11, P8S + [(29, 0)], ("p8", 256, False, False), {2: 2, 8: 2}),
    _c("p8-256x256-split-one", "bf16", 128, 200, 3, 2, 13, 11, P8S + [(29, 0)], ("p8", 256, False, True), {2: 2, 8: 2}),
    # fp32 outputs (out_f32 = 1): never split, never a 256-row form; the LDS-DMA forms leave through the register epilogue
    _c("f32out-128x32-reg", "bf16", 96, 24, 3, 1, 9, 17, [], ("128x32", 0, 4), out_f32=1),
    _c("f32out-128x64-ld2", "bf16", 96, 56, 3, 2, 9, 11, [], ("128x64", 2, 4), out_f32=1),
    _c("f32out-128x128-ld2", "bf16", 96, 200, 3, 2, 9, 11, [], ("128x128", 2, 4), out_f32=1),
    _c("f32out-128x128-ld1", "bf16", 40, 104, 3, 2, 9, 11, [], ("128x128", 1, 4), out_f32=1),
    _c("f32out-fp32-128x32-reg", "fp32", 40, 24, 3, 1, 9, 17, [], ("128x32", 0, 4), out_f32=1),
    _c("f32out-fp32-128x64-ld2", "fp32", 48, 56, 3, 2, 9, 11, [], ("128x64", 2, 4), out_f32=1),
    _c("f32out-fp32-128x128-ld2", "fp32", 48, 200, 3, 2, 9, 11, [], ("128x128", 2, 4), out_f32=1),
    _c("f32out-fp32-128x128-ld0", "fp32", 40, 104, 3, 2, 9, 11, [(0, 0)], ("128x128", 0, 4), out_f32=1),
]
LDX_EXTRA, LDY_EXTRA, C0 = 16, 24, 8           # the strided variants: x in channels [8, 8 + Cin_p) of Cin_p + 16, y in [8, 8 + N) of N + 24


def igemm_case(name):
    c = next(c for c in IGEMM_CASES if c["name"] == name)
    x, w, b, _, old = int_operands(c["cin_p"], c["n"], c["k"], c["B"], c["H"], c["W"], seed=len(name) + c["cin_p"] + c["n"])
    return c, x, w, b, old, conv64(x, w)


def kernel_name(c):
    """the instance a case claims, as the launch recorder prints it"""
    kern = c["kernel"]
    if kern[0] == "p8":
        return "conv_igemm8_kernel<%d, %s, %s>" % (kern[1], "true" if kern[2] else "false", "true" if kern[3] else "false")
    return "conv_igemm_kernel<%s, %d, %d, %d, %d, %d, %d, " % (("bf16" if c["dt"] == "bf16" else "float",) + TILE[kern[0]] + kern[1:])


# ---- 3c: LDS-patch and stem forward through the C interface (cin_p, n, k, B, H, W): one shape per form plan_patch (csrc/patch_plan.hpp) distinguishes
PATCH_CASES = [
    (32, 64, 1, 2, 9, 32),       # 1x1, first form, two output tiles, ragged 8-row tiles
    (32, 32, 1, 1, 20, 32),      # 1x1, first form, tall: 16 + 4 rows
    (64, 64, 3, 1, 9, 32),       # 3x3, first form (two tiles, <= 64 inputs)
    (72, 32, 3, 1, 20, 32),      # 3x3, second form, tall, three slices with a channel tail
    (32, 24, 3, 1, 9, 64),       # 3x3, second form, 8-row tiles (H < 16), N <= 32 with a column tail
    (96, 64, 3, 1, 11, 32),      # 3x3, second form, two output tiles
    (48, 56, 5, 1, 9, 32),       # 5x5, two tiles, column tail
    (32, 32, 5, 1, 20, 32),      # 5x5, tall
    (40, 32, 5, 1, 20, 32),      # 5x5, more than one slice: 8-row tiles
    (32, 24, 7, 1, 21, 32),      # 7x7, tall: 16 + 5 rows
    (64, 32, 7, 1, 9, 32),       # 7x7, two slices, 8-row tiles
]
STEM_CASES = [(8, 32, 5, 1, 19, 32), (8, 16, 3, 2, 9, 32), (8, 24, 7, 1, 11, 64)]
GN_CASES = [(32, 32, 3, 1, 20, 32), (64, 64, 3, 1, 9, 32), (32, 64, 5, 1, 11, 32), (32, 16, 7, 1, 21, 32)]      # N % 16 == 0; small ranges, see gn_case


def patch_case(shape):
    x, w, b, _, old = int_operands(*shape, seed=7 + sum(shape))
    return x, w, b, old, conv64(x, w)


def gn_case(shape):
    """operands whose stored values stay small: a tile's fp32 sums of values AND of squares must be exact (gn_sums asserts it)"""
    x, w, b, _, old = int_operands(*shape, seed=11 + sum(shape), xr=2, wr=1, br=12)
    return x, w, b, old, conv64(x, w)


def gn_sums(stored):
    """-> [B][16][2] fp64: sum and sum of squares of the stored values per GroupNorm(16) group.  Asserts the precondition under which a kernel's fp32 per-tile
    sums are exact in any order: integers, and the sums of magnitudes and of squares over a whole sample's group (so over any tile of it) stay below 2^24."""
    B, N = stored.shape[:2]
    v = stored.double().reshape(B, 16, -1)
    assert bool((v == v.round()).all()) and float(v.abs().sum(2).max()) < TWO24 and float((v * v).sum(2).max()) < TWO24
    return torch.stack([v.sum(2), (v * v).sum(2)], dim=2)


# ---- 3d: weight gradients (cin, cout, k, B, H, W, patch kernels on?, compute type) and the family plan_wgrad / plan_patch give each
WGRAD_CASES = [
    (32, 32, 3, 1, 48, 32, False, "bf16"),       # register-staged conv_wgrad_kernel<bf16, 1, 4, 1, 1>, several splits added into slab 0
    (64, 64, 3, 1, 12, 40, False, "fp32"),       # register-staged, fp32
    (64, 64, 5, 1, 12, 40, False, "bf16"),       # LDS-DMA 4-wave 64 x 128, flattened pixels (W = 40)
    (72, 96, 3, 2, 9, 40, False, "bf16"),        # LDS-DMA 4-wave 128 x 128, channel tails
    (128, 256, 3, 2, 9, 40, False, "bf16"),      # LDS-DMA 8-wave 256 x 128
    (256, 128, 1, 3, 7, 24, False, "bf16"),      # LDS-DMA 8-wave 128 x 256
    (256, 256, 1, 1, 24, 32, False, "bf16"),     # LDS-DMA 16-wave 256 x 256, row-aligned blocks
    (128, 128, 3, 2, 16, 64, True, "bf16"),      # nine-tap, 1 x 32 K-steps
    (64, 128, 3, 1, 6, 48, True, "bf16"),        # nine-tap, 2 x 16 K-steps
    (32, 32, 7, 1, 16, 64, True, "bf16"),        # LDS-patch, one slice
    (65, 32, 3, 1, 9, 96, True, "bf16"),         # LDS-patch, three slices in one workgroup
    (48, 56, 5, 2, 9, 32, True, "bf16"),         # LDS-patch, two output tiles
    (72, 96, 3, 2, 9, 32, True, "bf16"),         # wide LDS-patch (65..128 outputs)
    (3, 32, 5, 1, 19, 32, True, "bf16"),         # stem
    (3, 16, 3, 2, 9, 32, True, "bf16"),          # stem
]


def wgrad_case(shape):
    x, w, b, dy, _ = int_operands(*shape, seed=13 + sum(shape))
    _, _, dw, db = reference(x, w, b, dy)
    return x, w, dy, dw, db


# ---- 3e: one real-valued case per family, K <= 288 (cin_p, n, k, B, H, W)
REAL_CASES = {"igemm": (32, 72, 3, 2, 9, 17), "patch": (32, 32, 3, 1, 20, 32), "stem": (8, 32, 5, 1, 19, 32)}


def real_case(family):
    shape = REAL_CASES[family]
    x, w, b = real_operands(*shape, seed=17 + sum(shape))
    return x, w, b, conv64(x, w, b), conv64(x.abs(), w.abs(), b.abs())


def real_bound(r, S, K):
    """|got - r| <= 2^-8 |r| + (1 + 2^-8) K 2^-23 S: one bf16 rounding (half an ulp, relative 2^-8) of an fp32 sum that is off by at most one fp32 ulp
    (2^-23 relative to the running magnitude, which S bounds) per addition, in any order -- also with a truncating accumulator"""
    return 2.0 ** -8 * r.abs() + (1 + 2.0 ** -8) * K * 2.0 ** -23 * S
