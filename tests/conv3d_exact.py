"""Exact references for the conv3d pack / unpack kernels (tests/test_conv3d_exact_cpu.py, tests/test_gpu_conv3d_exact.py).  Imports without a GPU.

The method of tests/conv_exact.py, for csrc/pack3d.hip and the fold helpers of csrc/pack_fold.hip: x and dy are integers in -3..3 (exact in bf16), the fp32 bias b3 in
-1500..1500, the fp32 weights w3 [4,1,3,3,3] in -1023..1023.  The matrix-core forms split a weight into hi = bf16(w) and lo = bf16(w - hi); below 2^16 both are exact
and hi + lo == w, but about half of such weights have lo != 0, so a form that drops lo stores something else.  Every product and every partial sum is an integer, and
fp32 holds it in any order -- tile shape, taps in K, banded operands, depth slabs, the float atomics of dwb -- while the same operation over MAGNITUDES stays below
2^24 (assert_exact_in_fp32, with |hi| + |lo| for the weights).  Then a launch must store, bit for bit,
    rne(ref64)      bf16 activations: y and dx
    ref64           fp32 mode, and dwb[112] = (dw3, db3) in every mode
with ref64 from torch in fp64 (pack_ref, unpack_ref and their autograd).  No tolerance anywhere, so nothing is measured."""
import torch
import torch.nn.functional as F

from conv_exact import C0, LDX_EXTRA, LDY_EXTRA, TWO24, cached, rne, strided_view, truncate_bf16  # noqa: F401  (re-exported: the tests use them through this module)


def _ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def packing(x):
    """space-to-depth of the layer (layers01.py): packed channel 4c + 2 dy + dx"""
    b, c, h, w = x.shape
    return x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, 4 * c, h // 2, w // 2)


def pack_ref(x, w3, b3):
    """packing(x, 2) -> conv3d(1 -> 4, pad 1) over (packed channel, H/2, W/2) -> view [B, 16C, H/2, W/2], channel f 4C + d"""
    y = F.conv3d(packing(x).unsqueeze(1), w3, b3, padding=1)
    b, f, d, h, w = y.shape
    return y.reshape(b, f * d, h, w)


def unpack_ref(x, w3, b3):
    """conv3d(1 -> 4, pad 1) over (C, H, W) -> view [B, 4C, H, W], channel f C + c -> pixel_shuffle(2)"""
    y = F.conv3d(x.unsqueeze(1), w3, b3, padding=1)
    b, f, d, h, w = y.shape
    return F.pixel_shuffle(y.reshape(b, f * d, h, w), 2)


def _grads(fn, x, w3, b3, dy):
    x, w3, b3 = (t.double().clone().requires_grad_(True) for t in (x, w3, b3))
    y = fn(x, w3, b3)
    y.backward(dy.double())
    return y.detach(), x.grad, w3.grad, b3.grad


def reference(op, x, w3, b3, dy):
    """-> y, dx, dw3, db3 in fp64: torch's conv3d and its autograd"""
    return _grads(pack_ref if op == "pack" else unpack_ref, x, w3, b3, dy)


# ---- the same operations stated a second time: 27 shifted products per feature, the index formulas of the header of csrc/pack3d.hip written out.
# The flags state the MISTAKES the cases must be able to show (tests/test_conv3d_exact_cpu.py): swap = the dy / dx sub-pixel bits exchanged, dfirst = the channel
# order d 4 + f in place of f 4C + d (unpack: q = c 4 + f in place of f C + c).
def _taps(vol, w3, b3):
    """vol [B, D, H, W] -> the four features [B, D, H, W] of conv3d(1 -> 4, 3x3x3, zero pad 1), one shifted product per tap"""
    B, D, H, W = vol.shape
    vp = F.pad(vol, (1, 1, 1, 1, 1, 1))
    out = []
    for f in range(4):
        t = b3[f] + torch.zeros_like(vol)
        for kd in range(3):
            for kh in range(3):
                for kw in range(3):
                    t = t + w3[f, 0, kd, kh, kw] * vp[:, kd:kd + D, kh:kh + H, kw:kw + W]
        out.append(t)
    return out


def pack_taps(x, w3, b3, swap=False, dfirst=False):
    B, C, H, W = x.shape
    parts = [None] * 4
    for dy in range(2):
        for dx in range(2):
            parts[(2 * dx + dy) if swap else (2 * dy + dx)] = x[:, :, dy::2, dx::2]
    P = torch.stack(parts, 2).reshape(B, 4 * C, H // 2, W // 2)                  # packed channel d = 4c + 2 dy + dx
    T = _taps(P, w3, b3)
    if dfirst:
        return torch.stack(T, 2).reshape(B, 16 * C, H // 2, W // 2)              # (the mistake) channel d 4 + f
    return torch.cat(T, 1)                                                       # output channel f 4C + d


def unpack_taps(x, w3, b3, swap=False, dfirst=False):
    B, C, H, W = x.shape
    T = _taps(x, w3, b3)
    Q = torch.stack(T, 2).reshape(B, 4 * C, H, W) if dfirst else torch.cat(T, 1)      # q = f C + c
    rows = []
    for i in range(2):                                                           # out[b, q >> 2, 2h + ((q & 3) >> 1), 2w + (q & 1)] = Q[b, q, h, w]
        cols = [Q[:, (2 * j + i if swap else 2 * i + j)::4] for j in range(2)]
        rows.append(torch.stack(cols, 4).reshape(B, C, H, 2 * W))
    return torch.stack(rows, 3).reshape(B, C, 2 * H, 2 * W)


def taps_reference(op, x, w3, b3, dy, **flags):
    fn = pack_taps if op == "pack" else unpack_taps
    return _grads(lambda a, b, c: fn(a, b, c, **flags), x, w3, b3, dy)


def mistaken_dwb(op, x, w3, b3, dy, swap=False, dfirst=False):
    """dwb[112] = (dw3, db3) under the same two mistakes, from torch's reference alone (cheap enough for the large cases): each mistake is a fixed permutation
    of the sub-pixels of x (pack) or dy (unpack), or of the channels of dy, in front of the right operation"""
    B, C, H, W = x.shape
    if swap and op == "pack":
        x = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 5, 4, 3).reshape(B, C, H, W)
    if swap and op == "unpack":
        dy = dy.reshape(B, C, H, 2, W, 2).permute(0, 1, 2, 5, 4, 3).reshape(B, C, 2 * H, 2 * W)
    if dfirst and op == "pack":
        dy = dy.reshape(B, 4 * C, 4, H // 2, W // 2).transpose(1, 2).reshape(B, 16 * C, H // 2, W // 2)
    if dfirst and op == "unpack":
        dy = F.pixel_shuffle(F.pixel_unshuffle(dy, 2).reshape(B, C, 4, H, W).transpose(1, 2).reshape(B, 4 * C, H, W), 2)
    _, _, dw3, db3 = reference(op, x, w3, b3, dy)
    return torch.cat([dw3.reshape(108), db3])


def hi_lo(w):
    """the two bf16 parts the matrix-core forms make of an fp32 weight"""
    hi = rne(w)
    return hi, rne(w - hi)


def assert_exact_in_fp32(op, x, w3, b3, dy):
    """The precondition of the whole method: the operation and its three gradients over ABSOLUTE values bound every partial sum a kernel can form, in any order.
    The weights count as |hi| + |lo| (which can exceed |w|: hi may round away from zero); hi + lo must be w.  All of it stays below 2^24, where fp32 holds every
    integer.  -> the worst sum"""
    for t in (x, w3, b3, dy):
        assert bool((t == t.round()).all()), "operands must be integers"
    hi, lo = hi_lo(w3)
    assert torch.equal(hi + lo, w3.double()), "a weight is not the sum of two bf16 values"
    assert torch.equal(rne(x), x.double()) and torch.equal(rne(dy), dy.double()), "activations must be exact in bf16"
    worst = max(float(t.max()) for t in reference(op, x.abs(), hi.abs() + lo.abs(), b3.abs(), dy.abs()))
    assert worst < TWO24, "sum of magnitudes %g reaches 2^24: not exact in fp32" % worst
    return worst


def int_operands(op, C, B, H, W, r=3):
    """-> x [B, C, H, W], w3 [4, 1, 3, 3, 3], b3 [4], dy (pack: [B, 16C, H/2, W/2]; unpack: [B, C, 2H, 2W]) as fp64 integers; x and dy in +-r"""
    g = torch.Generator().manual_seed(1000 * C + 100 * B + 10 * H + W + (7 if op == "pack" else 0))
    oshape = (B, 16 * C, H // 2, W // 2) if op == "pack" else (B, C, 2 * H, 2 * W)
    return _ints((B, C, H, W), r, g), _ints((4, 1, 3, 3, 3), 1023, g), _ints((4,), 1500, g), _ints(oshape, r, g)


def shape_case(op, C, B, H, W, r=3):
    """-> x, w3, b3, dy, y, dx, dw3, db3; one per shape, shared by every case and variant on it (through `cached`; callers do not modify what they get)"""
    x, w3, b3, dy = int_operands(op, C, B, H, W, r)
    return (x, w3, b3, dy) + reference(op, x, w3, b3, dy)


def one_weight_case(op, C, B, H, W, r=3):
    """-> y, dx under the contract of the P3_ONE_BF16_WEIGHT forms (csrc/p3_plan.hpp, include/mte_kernels.h): every conv3d weight is rounded ONCE to bf16, to
    nearest even, and everything after that is exact as in the other forms -- so such a launch must store, bit for bit, what the reference gives for rne(w3)"""
    x, w3, b3, dy = int_operands(op, C, B, H, W, r)
    return reference(op, x, rne(w3), b3, dy)[:2]


def expected_y_dx(c):
    """what a data launch of case c must store, before the rounding to the activation type: (y, dx) in fp64"""
    return cached(one_weight_case, *case_key(c)) if c["one"] else cached(shape_case, *case_key(c))[4:6]


# ---- the tiles of csrc/p3_plan.hpp, restated (the recorder proves that a case's launch has the tile the table says: tests/test_conv3d_exact_cpu.py)
def p3_tile(C, small=True):
    i = (32, 64, 128, 256, 1 << 30).index(next(c for c in (32, 64, 128, 256, 1 << 30) if C <= c))
    return ((4, 16), (4, 8), (2, 8), (2, 4), (2, 2))[i] if small else ((8, 16), (4, 16), (4, 8), (2, 8), (2, 4))[i]


def up_tile(C, halved=False):
    i = (32, 64, 128, 256, 1 << 30).index(next(c for c in (32, 64, 128, 256, 1 << 30) if C <= c))
    th, tw = ((16, 32), (8, 32), (8, 16), (4, 16), (4, 8))[i]
    return (th // 2 if halved and th >= 4 else th, tw)


def up4_tile(C):
    return (8, 16) if C <= 32 else (4, 16) if C <= 64 else (4, 8)


BF16, F32 = "bf16", "fp32"
MAIN = (32, 64, 128, 256, 512)                 # the C classes with LDS and matrix-core forms; 8 and 16 are taken too
CASES = []


def _add(op, what, dt, C, shape, knobs, kernel, tile=None, r=3, big=False):
    """op: pack | unpack; what: fwd | bwd_data | bwd_weight; shape = (B, H, W) of the UN-packed side tensor; knobs: the values of mte_debug_set(1, .) the case
    sets (none: the product's dispatch); kernel: the instance it claims, as the launch recorder prints it; tile: the (TH, TW) the shape is one row and one column
    beyond, over the packed volume for pack; big: the tile count exceeds the grid cap"""
    B, H, W = shape
    name = "%s_%s-%s-C%d-%dx%dx%d%s" % (op, what, dt, C, B, H, W, "".join("-k%d" % k for k in knobs))
    assert all(c["name"] != name for c in CASES), name
    one = kernel.endswith("false>") and "bwd_weight" not in kernel         # HILO = false: the P3_ONE_BF16_WEIGHT forms, see one_weight_case
    CASES.append(dict(name=name, op=op, what=what, dt=dt, C=C, B=B, H=H, W=W, knobs=tuple(knobs), kernel=kernel, tile=tile, r=r, big=big, one=one))


def _beyond(op, tile, B=2):
    """one row and one column more than a whole tile: two tile rows and two tile columns, the second of each one pixel wide"""
    th, tw = tile
    return (B, 2 * (th + 1), 2 * (tw + 1)) if op == "pack" else (B, th + 1, tw + 1)


def _gather_shape(op, C):
    """no tiles: more than one block of 256 threads, and no whole number of them"""
    if op == "pack":
        return (3, 12, 18) if C <= 32 else (2, 6, 10)
    return (3, 7, 13) if C <= 32 else (2, 3, 5)


def _build():
    # ---- pack forward: taps in K (2 x 16, depth slabs of 128: 16 of them at C = 512), LDS stencil (p3_tile small and large), gather
    for C in MAIN:
        _add("pack", "fwd", BF16, C, _beyond("pack", (2, 16)), (), "pack3d_fwd_tr_kernel<2, 4>", (2, 16))
        _add("pack", "fwd", BF16, C, _beyond("pack", p3_tile(C)), (347,), "pack3d_fwd_lds_kernel", p3_tile(C))
        _add("pack", "fwd", BF16, C, _beyond("pack", p3_tile(C, False)), (347, 100), "pack3d_fwd_lds_kernel", p3_tile(C, False))
        _add("pack", "bwd_data", BF16, C, _beyond("pack", (4, 16)), (), "pack3d_bwd_data_mfma_kernel<true>", (4, 16))
        _add("pack", "bwd_data", BF16, C, _beyond("pack", (4, 16)), (555,), "pack3d_bwd_data_mfma_kernel<false>", (4, 16))
        _add("pack", "bwd_data", BF16, C, _beyond("pack", p3_tile(C)), (411,), "pack3d_bwd_data_lds_kernel", p3_tile(C))
        _add("pack", "bwd_data", BF16, C, _beyond("pack", p3_tile(C, False)), (411, 100), "pack3d_bwd_data_lds_kernel", p3_tile(C, False))
    for C in (8, 16) + MAIN:
        for what, stem in (("fwd", "pack3d_fwd_kernel"), ("bwd_data", "pack3d_bwd_data_kernel"), ("bwd_weight", "pack3d_bwd_weight_kernel")):
            cpt = 4 if C <= 256 else 8
            if C in (8, 64, 256, 512):
                _add("pack", what, BF16, C, _gather_shape("pack", C), (0,), "%s<bf16, %d>" % (stem, cpt))
            if C in (8, 32, 256, 512):
                _add("pack", what, F32, C, _gather_shape("pack", C), (), "%s<float, %d>" % (stem, cpt))
        if C <= 16:                                                            # the product's kernels for these: the LDS stencils
            _add("pack", "fwd", BF16, C, _beyond("pack", p3_tile(C)), (), "pack3d_fwd_lds_kernel", p3_tile(C))
            _add("pack", "bwd_data", BF16, C, _beyond("pack", p3_tile(C)), (), "pack3d_bwd_data_lds_kernel", p3_tile(C))
        # weight gradients: matrix cores (the product's) and fp32 VALU, small and large tiles
        for small in (True, False):
            extra = () if small else (100,)
            _add("pack", "bwd_weight", BF16, C, _beyond("pack", p3_tile(C, small)), extra, "conv3d_bwd_weight_mfma_kernel<false>", p3_tile(C, small))
            _add("pack", "bwd_weight", BF16, C, _beyond("pack", p3_tile(C, small)), (200,) + extra, "pack3d_bwd_weight_lds_kernel", p3_tile(C, small))
    # the matrix-core weight gradient with 4 waves in place of 8 (mte_debug_set(1, 1000 + threads); the kernel is built for at most 512 threads, and a value
    # of 2000 and more is another knob)
    _add("pack", "bwd_weight", BF16, 64, _beyond("pack", p3_tile(64)), (1256,), "conv3d_bwd_weight_mfma_kernel<false>", p3_tile(64))
    _add("unpack", "bwd_weight", BF16, 64, _beyond("unpack", up_tile(64, True)), (1256,), "conv3d_bwd_weight_mfma_kernel<true>", up_tile(64, True))

    # ---- unpack forward: taps in K (256 / C x 16, in 1 / 2 / 4 output passes), banded (8 or 4 x 16, persistent), gather
    for C in (32, 64, 128, 256):
        for passes, knobs in ((1, (3001,)), (2, (3002,)), (4, ())):
            _add("unpack", "fwd", BF16, C, _beyond("unpack", (256 // C, 16)), knobs, "unpack3d_fwd_tr_kernel<%d, %d, %d>" % (C, 256 // C, passes), (256 // C, 16))
    for C in (32, 64):
        band = (8 if C == 32 else 4, 16)
        for knob, hilo in ((315, "true"), (331, "false")):
            _add("unpack", "fwd", BF16, C, _beyond("unpack", band), (knob,), "unpack3d_fwd_mfma_kernel<%d, %s>" % (C, hilo), band)
            for wgs in (8, 1024):                                              # 20 tiles dealt to 8 workgroups (a workgroup walks 2 or 3, double-buffered) and to 1024
                _add("unpack", "fwd", BF16, C, _beyond("unpack", band, B=5), (knob, 2000 + wgs), "unpack3d_fwd_mfma_kernel<%d, %s>" % (C, hilo), band)
        # unpack backward data: LDS-DMA (C = 32; 4 waves, 2 waves, one-value weights), banded, four planes, plane by plane
        for knob, hilo in ((301, "true"), (317, "false")) if C == 32 else ((None, "true"), (555, "false")):
            _add("unpack", "bwd_data", BF16, C, _beyond("unpack", band), () if knob is None else (knob,), "unpack3d_bwd_data_mfma_kernel<%d, %s>" % (C, hilo), band)
    for knobs, inst in (((), "4, true"), ((555,), "4, false"), ((303,), "2, true")):
        _add("unpack", "bwd_data", BF16, 32, _beyond("unpack", (8, 16)), knobs, "unpack3d_bwd_data_dma32_kernel<%s>" % inst, (8, 16))
    for C in (32, 64, 128):
        _add("unpack", "bwd_data", BF16, C, _beyond("unpack", up4_tile(C)), () if C == 128 else (300,), "unpack3d_bwd_data_lds4_kernel", up4_tile(C))
    for C in MAIN:
        _add("unpack", "bwd_data", BF16, C, _beyond("unpack", up_tile(C)), () if C >= 256 else (1,), "unpack3d_bwd_data_lds_kernel", up_tile(C))
        for small in (True, False):
            extra = () if small else (100,)
            t = up_tile(C, small)
            _add("unpack", "bwd_weight", BF16, C, _beyond("unpack", t), extra, "conv3d_bwd_weight_mfma_kernel<true>", t)
            _add("unpack", "bwd_weight", BF16, C, _beyond("unpack", t), (200,) + extra, "unpack3d_bwd_weight_lds_kernel", t)
    for what in ("fwd", "bwd_data", "bwd_weight"):
        for C, knobs in ((8, ()), (16, ()), (64, (0,))) + (((512, ()), (32, (307,))) if what == "fwd" else ()):
            _add("unpack", what, BF16, C, _gather_shape("unpack", C), knobs, "unpack3d_%s_kernel<bf16>" % what)
        for C in (8, 64, 512):
            _add("unpack", what, F32, C, _gather_shape("unpack", C), (), "unpack3d_%s_kernel<float>" % what)

    # ---- one-pixel and 2 x 2 images (pack: of the packed volume), the product's dispatch, B = 1 and B > 1
    for C in (32, 64):
        for op, what, kernel in (("pack", "fwd", "pack3d_fwd_tr_kernel<2, 4>"), ("pack", "bwd_data", "pack3d_bwd_data_mfma_kernel<true>"),
                                 ("pack", "bwd_weight", "conv3d_bwd_weight_mfma_kernel<false>"),
                                 ("unpack", "fwd", "unpack3d_fwd_tr_kernel<%d, %d, 4>" % (C, 256 // C)),
                                 ("unpack", "bwd_data", "unpack3d_bwd_data_dma32_kernel<4, true>" if C == 32 else "unpack3d_bwd_data_mfma_kernel<64, true>"),
                                 ("unpack", "bwd_weight", "conv3d_bwd_weight_mfma_kernel<true>")):
            for B, n in ((1, 1), (3, 2)):
                _add(op, what, BF16, C, (B, 2 * n, 2 * n) if op == "pack" else (B, n, n), (), kernel)

    # ---- weight gradients beyond the grid cap: every sample is four tiles (one whole, three ragged), so 200 samples are 800 tiles for the cap of 512 and 400
    # samples 1600 for the cap of 1024 -- more than half of the workgroups walk two tiles
    _add("pack", "bwd_weight", BF16, 32, _beyond("pack", p3_tile(32), B=200), (), "conv3d_bwd_weight_mfma_kernel<false>", p3_tile(32), big=True)
    _add("pack", "bwd_weight", BF16, 32, _beyond("pack", p3_tile(32), B=200), (200,), "pack3d_bwd_weight_lds_kernel", p3_tile(32), big=True)
    _add("unpack", "bwd_weight", BF16, 32, _beyond("unpack", up_tile(32, True), B=200), (), "conv3d_bwd_weight_mfma_kernel<true>", up_tile(32, True), big=True)
    _add("unpack", "bwd_weight", BF16, 32, _beyond("unpack", up_tile(32, True), B=400), (200,), "unpack3d_bwd_weight_lds_kernel", up_tile(32, True), big=True)
    _add("unpack", "bwd_weight", BF16, 32, _beyond("unpack", up_tile(32), B=200), (200, 100), "unpack3d_bwd_weight_lds_kernel", up_tile(32), big=True)
    # the same at C = 512, where a pack tile is 2 x 2 packed pixels of 2048 depths: 800 tiles, 3.7 M volume elements, x and dy in -1..1
    _add("pack", "bwd_weight", BF16, 512, _beyond("pack", p3_tile(512), B=200), (), "conv3d_bwd_weight_mfma_kernel<false>", p3_tile(512), r=1, big=True)
    # the gather weight gradients walk their work under a capped grid too (256 x 1024 threads for pack, 256 x 2048 for unpack): C = 8, 1.1 times the cap, so a
    # tenth of the threads take a second item.  4.6 M volume elements, x and dy in -1..1.  These are the product's kernels in fp32 mode and for unpack C = 8.
    _add("pack", "bwd_weight", F32, 8, (3, 300, 642), (), "pack3d_bwd_weight_kernel<float, 4>", r=1, big=True)
    _add("unpack", "bwd_weight", BF16, 8, (3, 300, 641), (), "unpack3d_bwd_weight_kernel<bf16>", r=1, big=True)


_build()


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


def case_key(c):
    return (c["op"], c["C"], c["B"], c["H"], c["W"], c["r"])


def is_product(c):
    """no knob set: the launch is what the product's dispatch gives the shape"""
    return not c["knobs"]


def strides(c, strided):
    """-> (ldx, ldo): pixel strides of the un-packed side and of the feature side (pack: 16C channels; unpack: C).  strided: an input sits in channels
    [C0, C0 + its own) of a buffer LDX_EXTRA wider, the output in a buffer LDY_EXTRA wider"""
    C, feat = c["C"], 16 * c["C"] if c["op"] == "pack" else c["C"]
    if not strided:
        return C, feat
    if c["what"] == "fwd":
        return C + LDX_EXTRA, feat + LDY_EXTRA
    if c["what"] == "bwd_data":
        return C + LDY_EXTRA, feat + LDX_EXTRA
    return C + LDX_EXTRA, feat + LDX_EXTRA


# ---- 3a: layer level, default dispatch (op, C, B, H, W): every C class, ragged tiles, B > 1
LAYER_SHAPES = [("pack", 8, 2, 10, 34), ("pack", 16, 2, 8, 12), ("pack", 32, 2, 10, 34), ("pack", 64, 3, 6, 34), ("pack", 128, 2, 10, 18), ("pack", 256, 1, 6, 34),
                ("pack", 512, 2, 6, 10),
                ("unpack", 8, 2, 7, 13), ("unpack", 16, 2, 5, 9), ("unpack", 32, 2, 9, 17), ("unpack", 64, 2, 5, 19), ("unpack", 128, 2, 3, 17),
                ("unpack", 256, 3, 2, 17), ("unpack", 512, 1, 5, 9)]
SKIP = 32                                      # channels of the skip connection behind the unpack layer's own in the decoder's concat buffer


# ---- 3d: the fold helpers (Co, D, k): W' [Co][D][k+2][k+2], b' [Co] from W [Co][4D][k][k], K3 [4][1][3][3][3], b [Co], b3 [4] -- csrc/pack_fold.hip
FOLD_CASES = [(32, 64, 3), (32, 64, 5), (32, 128, 3), (32, 128, 5)]
FOLD_RANGES = dict(W=2, K3=15, b=1500, b3=100, g=3)      # small enough for the sums below (fold_precondition); g: dW', db' and what dW and dk3b held before


def fold_ref(W, K3, b, b3):
    """W'[co][c][u] = sum_{f, kd, dh, dw} W[co][f D + c - kd + 1][u - (dh, dw)] K3[f][kd][dh][dw];  b'[co] = b[co] + sum_f b3[f] sum_{d, t} W[co][f D + d][t]"""
    Co, D4, k, _ = W.shape
    D = D4 // 4
    Wf = torch.zeros(Co, D, k + 2, k + 2, dtype=torch.float64)
    Wv = F.pad(W.reshape(Co, 4, D, k, k), (0, 0, 0, 0, 1, 1))                    # depth -1 and D: zero
    for f in range(4):
        for kd in range(3):
            for dh in range(3):
                for dw in range(3):
                    Wf[:, :, dh:dh + k, dw:dw + k] = Wf[:, :, dh:dh + k, dw:dw + k] + Wv[:, f, 2 - kd:2 - kd + D] * K3[f, 0, kd, dh, dw]
    return Wf, b + (W.reshape(Co, 4, -1).sum(2) * b3.reshape(1, 4)).sum(1)


def fold_operands(Co, D, k):
    """-> W, K3, b, b3, dW', db', old dW, old dk3b[112]: fp64 integers"""
    g = torch.Generator().manual_seed(Co + 10 * D + k)
    R = FOLD_RANGES
    return (_ints((Co, 4 * D, k, k), R["W"], g), _ints((4, 1, 3, 3, 3), R["K3"], g), _ints((Co,), R["b"], g), _ints((4,), R["b3"], g),
            _ints((Co, D, k + 2, k + 2), R["g"], g), _ints((Co,), R["g"], g), _ints((Co, 4 * D, k, k), R["g"], g), _ints((112,), R["g"], g))


def fold_case(Co, D, k):
    """-> operands, W', b', and the transpose by autograd of fold_ref: dW, dk3b = (dK3, db3) WITHOUT what the buffers held before"""
    ops = fold_operands(Co, D, k)
    W, K3, b, b3 = (t.clone().requires_grad_(True) for t in ops[:4])
    Wf, bf = fold_ref(W, K3, b, b3)
    ((Wf * ops[4]).sum() + (bf * ops[5]).sum()).backward()
    return ops, Wf.detach(), bf.detach(), W.grad, torch.cat([K3.grad.reshape(108), b3.grad])


def fold_precondition(Co, D, k):
    """every sum of the fold and of its transpose over magnitudes, the old buffer contents included, stays below 2^24"""
    ops = [t.abs() for t in fold_operands(Co, D, k)]
    W, K3, b, b3 = (t.clone().requires_grad_(True) for t in ops[:4])
    Wf, bf = fold_ref(W, K3, b, b3)
    ((Wf * ops[4]).sum() + (bf * ops[5]).sum()).backward()
    worst = max(float(Wf.detach().max()), float(bf.detach().max()), float((W.grad + ops[6]).max()), float((torch.cat([K3.grad.reshape(108), b3.grad]) + ops[7]).max()))
    assert worst < TWO24, "sum of magnitudes %g reaches 2^24: not exact in fp32" % worst
    return worst


# ---- 3e: real-valued operands, one case per form family: (case of the table whose launch it repeats, A, e) for the coefficient A 2^-23 + e of real_bound.
# A: the additions the form makes per output -- 27 taps onto the bias for a forward, 4 x 27 for a data gradient (108 terms cannot be bounded with 27), twice that
# where the hi and the lo products are added separately.  e: what is allowed for the weights the form multiplies with in place of w -- 0 for fp32 weights, 2^-18
# for hi + lo, 2^-9 for one bf16 value.  These e are NOT worst cases of the roundings (bf16 rounds to within 2^-8 relative, so one weight can be off by 2^-8 |w|
# and hi + lo by 2^-16 |w|); they hold for sums over 27 or 108 random weights, and real_precondition proves from the operands of each case, on the CPU and
# before anything is launched, that they hold for that case.
REAL_CASES = {
    "pack-fwd-valu": ("pack_fwd-bf16-C32-2x10x34-k347", 27, 0.0),
    "pack-fwd-gather": ("pack_fwd-bf16-C64-2x6x10-k0", 27, 0.0),
    "pack-fwd-taps-k": ("pack_fwd-bf16-C32-2x6x34", 54, 2.0 ** -18),
    "unpack-fwd-gather": ("unpack_fwd-bf16-C32-3x7x13-k307", 27, 0.0),
    "unpack-fwd-taps-k": ("unpack_fwd-bf16-C64-2x5x17", 54, 2.0 ** -18),
    "unpack-fwd-banded": ("unpack_fwd-bf16-C32-2x9x17-k315", 54, 2.0 ** -18),
    "unpack-fwd-banded-one": ("unpack_fwd-bf16-C32-2x9x17-k331", 27, 2.0 ** -9),
    "pack-bwd-valu": ("pack_bwd_data-bf16-C32-2x10x34-k411", 108, 0.0),
    "pack-bwd-banded": ("pack_bwd_data-bf16-C32-2x10x34", 216, 2.0 ** -18),
    "pack-bwd-banded-one": ("pack_bwd_data-bf16-C32-2x10x34-k555", 108, 2.0 ** -9),
    "unpack-bwd-valu": ("unpack_bwd_data-bf16-C32-2x9x17-k300", 108, 0.0),
    "unpack-bwd-dma": ("unpack_bwd_data-bf16-C32-2x9x17", 216, 2.0 ** -18),
    "unpack-bwd-banded": ("unpack_bwd_data-bf16-C64-2x5x17", 216, 2.0 ** -18),
    "unpack-bwd-banded-one": ("unpack_bwd_data-bf16-C64-2x5x17-k555", 108, 2.0 ** -9),
}


def real_case(family):
    """x and dy uniform in [-1, 1] rounded to bf16, w3 and b3 uniform in [-1, 1] as fp32 holds them -> c, x, w3, b3, dy, r, S: r the fp64 result of the case's
    entry point (y, or dx), S the same over magnitudes"""
    c = case_named(REAL_CASES[family][0])
    g = torch.Generator().manual_seed(len(family) + c["C"])
    u = lambda shape: torch.rand(shape, generator=g) * 2 - 1                     # noqa: E731
    x, _, _, dy = int_operands(c["op"], c["C"], c["B"], c["H"], c["W"])
    x, dy = u(x.shape).bfloat16().double(), u(dy.shape).bfloat16().double()
    w3, b3 = u((4, 1, 3, 3, 3)).double(), u((4,)).double()
    i = 0 if c["what"] == "fwd" else 1
    return c, x, w3, b3, dy, reference(c["op"], x, w3, b3, dy)[i], reference(c["op"], x.abs(), w3.abs(), b3.abs(), dy.abs())[i]


def form_weights(w3, e_w):
    """the bf16 / fp32 values a form multiplies with in place of w3: [w], [hi, lo] or [hi]"""
    hi, lo = hi_lo(w3)
    return [w3.double()] if e_w == 0.0 else [hi, lo] if e_w == 2.0 ** -18 else [hi]


def real_precondition(family):
    """What makes real_bound a derived bound for this case, checked from its operands alone: with the weights w^ the form multiplies (form_weights), per output
        A 2^-23 S^ + E <= (A 2^-23 + e) S
    S^: the operation over the magnitudes the form adds (|hi| + |lo| for a hi + lo form), E: the operation over |x| (or |dy|) and |w - sum(w^)| -- the exact
    bound of what the form's weights change.  -> the largest ratio of the two sides"""
    _, A, e_w = REAL_CASES[family]
    c, x, w3, b3, dy, r, S = cached(real_case, family)
    parts = form_weights(w3, e_w)
    i = 0 if c["what"] == "fwd" else 1
    S_form = reference(c["op"], x.abs(), sum(p.abs() for p in parts), b3.abs(), dy.abs())[i]
    E = reference(c["op"], x.abs(), (w3 - sum(parts)).abs(), torch.zeros(4), dy.abs())[i]
    ratio = float(((A * 2.0 ** -23 * S_form + E) / ((A * 2.0 ** -23 + e_w) * S)).max())
    assert ratio <= 1.0, "%s: the weights' error and the summation term exceed the coefficient by a factor %g" % (family, ratio)
    return ratio


def real_bound(r, S, additions, e_w):
    """|got - r| <= 2^-8 |r| + (1 + 2^-8) (A 2^-23 + e) S.  got is one bf16 rounding (to within 2^-8 relative) of an fp32 sum s, so |got - r| <= 2^-8 |s| + |s - r|
    <= 2^-8 |r| + (1 + 2^-8) |s - r|.  s is off from the exact sum over the form's own weights by at most one fp32 ulp of the running magnitude per addition,
    in any order, also with a truncating accumulator: A 2^-23 S^; that sum is off from r by at most E.  real_precondition shows A 2^-23 S^ + E <= (A 2^-23 + e) S
    for the case.  For a forward the coefficient is never above the 27 2^-23 + {0, 2^-17, 2^-9} written for the three weight forms (54 2^-23 + 2^-18 =
    86 2^-23 < 27 2^-23 + 2^-17 = 91 2^-23); for a data gradient it counts the 108 terms that sum has."""
    return 2.0 ** -8 * r.abs() + (1 + 2.0 ** -8) * (additions * 2.0 ** -23 + e_w) * S
