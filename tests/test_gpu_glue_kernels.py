"""GPU (-m gpu): the layout, reduction, weight-pack and Adam helpers of heads_misc.hip, pack_fold.hip and the tail of conv_igemm.hip, each
called through the raw C ABI and compared with the plain statements of tests/glue_ref.py (pinned to torch ops by tests/test_glue_ref_cpu.py).

Method 1 -- guard band (tests/guard_band.py).  Every output and in/out buffer is allocated wider (extra channels per pixel on both sides of the slice, `ld > C`)
and longer (one extra row of pixels / a tail of elements) than the kernel may touch and pre-filled with a NaN bit pattern; afterwards the
band is compared bitwise through an integer view.  A NaN that a kernel reads where it should only write shows up in the result as well.

Method 2 -- exact arithmetic.  Kernels that copy, permute or add get small integers (or multiples of 1/8), chosen so that every partial sum
is representable: the result does not depend on summation order, atomics or split counts, and the criterion is bit equality.  The three
kernels that multiply by non-dyadic values (Adam, bilinear resize, silog) are held to bounds derived from their fp32 operation counts."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
from guard_band import Band, Flat, beq, _SENT, _INT  # noqa: F401  (the guard-band helpers, shared with test_gpu_groupnorm_layout.py)

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [BF16, F32]


@pytest.fixture(scope="module")
def L():
    """the raw ctypes handle: entry points return their codes instead of raising"""
    from mindtheedge_amd._lib import lib
    return lib.load()


def _dt(dtype):
    from mindtheedge_amd import kernels as K
    return K._dt(torch.empty(0, dtype=dtype))


def _st():
    from mindtheedge_amd import kernels as K
    return K._stream()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, g, lim=8):
    """integers in [-lim, lim] as fp32.  |v| <= 8 is exact in bf16 (8 significant bits hold every integer up to 256) and in fp32."""
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def sync():
    torch.cuda.synchronize()


# ---- 1. mte_nchw_to_nhwc ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3, 8, 11])
def test_nchw_to_nhwc(L, C, dtype):
    g = _gen(100 + C)
    for Cp in (R.round8(C), R.round8(C) + 8):
        for H, W in ((1, 1), (3, 5), (4, 33)):
            full = torch.randn(3, C, H, W, generator=g)                  # the image is the head of a longer buffer: nothing the kernel could
            src, src_d = full[:2], full.cuda()                            # read by mistake lies outside an allocation
            for flip in (0, 1):
                for c0, pad in ((0, 0), (8, 8)):                      # ldd = Cp and ldd = Cp + 16
                    dst = Band(2, H, W, Cp, dtype, c0=c0, pad=pad)
                    assert dst.ld == Cp + c0 + pad
                    assert L.mte_nchw_to_nhwc(src_d.data_ptr(), dst.ptr, dst.ld, 2, C, H, W, Cp, flip, _dt(dtype), _st()) == OK
                    sync()
                    case = (C, Cp, H, W, flip, dst.ld)
                    assert beq(dst.get(), R.nchw_to_nhwc(src, Cp, flip, dtype)), case       # real channels = src.to(dtype), pad = +0
                    assert dst.guard_ok(), case


def test_nchw_to_nhwc_rejects_bad_padding(L):
    src = torch.randn(2, 11, 3, 5).cuda()
    dst = Band(2, 3, 5, 16, BF16)
    for C, Cp in ((11, 8), (3, 12)):                                  # Cp < C; Cp not a multiple of 8
        assert L.mte_nchw_to_nhwc(src.data_ptr(), dst.ptr, dst.ld, 2, C, 3, 5, Cp, 0, _dt(BF16), _st()) == ERR_ARG
    sync()
    assert dst.untouched()


# ---- 2. mte_upsample_inv_fwd / _bwd, mte_upsample2_f32 ------------------------------------------------------------------------------------------
HW_UP = [(1, 1), (3, 5), (7, 33)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", HW_UP)
def test_upsample_inv_fwd(L, hw, dtype):
    h, w = hw
    inv = torch.randn(2, h, w, generator=_gen(200 + h))
    dst = Band(2, 2 * h, 2 * w, 8, dtype, c0=0, pad=8)               # ld = 16: channels 8..15 belong to a neighbour
    assert dst.ld == 16
    assert L.mte_upsample_inv_fwd(inv.cuda().data_ptr(), dst.ptr, dst.ld, 2, h, w, _dt(dtype), _st()) == OK
    sync()
    assert beq(dst.get(), R.upsample_inv_fwd(inv, dtype))           # channel 0 = nearest_up2 rounded to the type, channels 1..7 = +0
    assert dst.guard_ok()
    dst2 = Band(2, 2 * h, 2 * w, 8, dtype, c0=8, pad=0)              # the block at a non-zero channel offset
    assert L.mte_upsample_inv_fwd(inv.cuda().data_ptr(), dst2.ptr, dst2.ld, 2, h, w, _dt(dtype), _st()) == OK
    sync()
    assert beq(dst2.get(), R.upsample_inv_fwd(inv, dtype)) and dst2.guard_ok()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", HW_UP)
def test_upsample_inv_bwd(L, hw, dtype):
    h, w = hw
    g = _gen(210 + h)
    # |v| <= 8: a block sum is at most 32, plus an old value of at most 8: integers below 2^24, exact in fp32 in any order
    d = _ints((2, 2 * h, 2 * w, 8), g)
    old = _ints((2, h, w), g)
    src = Band(2, 2 * h, 2 * w, 8, dtype, c0=8, pad=8).set(d)        # strided source: channel 0 of the slice is element 8 of a 24-wide pixel
    want = R.upsample_inv_bwd(d[..., 0])
    out = Flat(2 * h * w)                                             # NaN on entry: accumulate = 0 must not read it
    assert L.mte_upsample_inv_bwd(src.ptr, src.ld, out.ptr, 2, h, w, 0, _dt(dtype), _st()) == OK
    sync()
    assert beq(out.get(), want.float().flatten()) and out.guard_ok()
    acc = Flat(2 * h * w).set(old)
    assert L.mte_upsample_inv_bwd(src.ptr, src.ld, acc.ptr, 2, h, w, 1, _dt(dtype), _st()) == OK
    sync()
    assert beq(acc.get(), (want + old.double()).float().flatten()) and acc.guard_ok()
    assert src.guard_ok()


@pytest.mark.parametrize("hw", HW_UP)
def test_upsample2_f32(L, hw):
    h, w = hw
    inv = torch.randn(2, h, w, generator=_gen(220 + h))
    out = Flat(2 * 4 * h * w)
    assert L.mte_upsample2_f32(inv.cuda().data_ptr(), out.ptr, 2, h, w, _st()) == OK
    sync()
    assert beq(out.get(), inv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).flatten()) and out.guard_ok()


# ---- 3. mte_copy_channels, mte_add_channels ------------------------------------------------------------------------------------------------
def _three_views(npix, C, dtype, g):
    """a, b, out with lda, ldb, ldo all different and all larger than C, slices at non-zero channel offsets"""
    a = Band(1, 1, npix, C, dtype, c0=8, pad=8, tail=3)
    b = Band(1, 1, npix, C, dtype, c0=16, pad=8, tail=3)
    o = Band(1, 1, npix, C, dtype, c0=8, pad=24, tail=3)
    assert len({a.ld, b.ld, o.ld}) == 3 and min(a.ld, b.ld, o.ld) > C
    # |v| <= 8: a + b is an integer of at most 16, exact in bf16 and fp32
    va, vb = _ints((1, 1, npix, C), g), _ints((1, 1, npix, C), g)
    return a.set(va), b.set(vb), o, va, vb


def _copy_add_case(L, npix, C, dtype, g, copy=True):
    a, b, o, va, vb = _three_views(npix, C, dtype, g)
    case = (npix, C, dtype)
    if copy:
        assert L.mte_copy_channels(a.ptr, a.ld, o.ptr, o.ld, npix, C, _dt(dtype), _st()) == OK
        sync()
        assert beq(o.get(), va.to(dtype)) and o.guard_ok(), case
        o = Band(1, 1, npix, C, dtype, c0=8, pad=24, tail=3)
    # the call of kernels.ForkFn.backward: two gradient views summed into a third buffer
    assert L.mte_add_channels(a.ptr, a.ld, b.ptr, b.ld, o.ptr, o.ld, npix, C, _dt(dtype), _st()) == OK
    sync()
    assert beq(o.get(), (va + vb).to(dtype)) and o.guard_ok(), case
    assert beq(a.get(), va.to(dtype)) and beq(b.get(), vb.to(dtype)), case              # the inputs are only read
    # out = a in place (same pointer and stride): every 16-byte chunk is read before it is written by the same thread
    assert L.mte_add_channels(a.ptr, a.ld, b.ptr, b.ld, a.ptr, a.ld, npix, C, _dt(dtype), _st()) == OK
    sync()
    assert beq(a.get(), (va + vb).to(dtype)) and a.guard_ok() and b.guard_ok(), case


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_and_add_channels(L, dtype):
    g = _gen(300)
    for C in (8, 24, 72):
        for npix in (1, 37):
            _copy_add_case(L, npix, C, dtype, g)
    if dtype == F32:
        for C in (4, 12):                                             # fp32 sums take any multiple of 4 channels (one 16-byte chunk)
            for npix in (1, 37):
                _copy_add_case(L, npix, C, dtype, g, copy=False)


def test_copy_and_add_channels_past_the_grid_cap(L):
    """bf16, C = 256, 66000 pixels: 66000 * 32 = 2,112,000 chunks > 8192 * 256 threads, so some threads take a second trip"""
    assert 66000 * (256 // 8) > 8192 * 256
    _copy_add_case(L, 66000, 256, BF16, _gen(301))
    torch.cuda.empty_cache()


# ---- 4. mte_split_record ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(0, 5), (5, 0), (1, 1), (288, 32), (20000, 7), (0, 0)])
def test_split_record(L, n0, n1):
    assert 20000 + 7 > 64 * 256                                       # the last pair is past the 64-block cap
    src = torch.randn(max(n0 + n1, 1), generator=_gen(400 + n0))
    G = 8
    buf = Flat(G + n0 + G + n1, extra=G)                              # [guard | dst0 | guard | dst1 | guard]
    d0, d1 = buf.ptr + 4 * G, buf.ptr + 4 * (G + n0 + G)
    assert L.mte_split_record(src.cuda().data_ptr(), d0, n0, d1, n1, _st()) == OK
    sync()
    if n0 + n1 == 0:
        assert buf.untouched()
        return
    got = buf.get()
    assert beq(got[G:G + n0], src[:n0]) and beq(got[2 * G + n0:], src[n0:n0 + n1])
    m = torch.ones(buf.raw.numel(), dtype=torch.bool)
    m[G:G + n0] = False
    m[2 * G + n0:2 * G + n0 + n1] = False
    assert bool((buf.raw.cpu()[m] == _SENT[F32]).all())


# ---- 5. mte_colsum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum(L, dtype):
    g = _gen(500)
    nmax = 2048 if dtype == BF16 else 1024                            # 256 16-byte chunks per row
    cases = [(M, N) for N in (8, 24, 72, 200, nmax) for M in (1, 31, 1000)] + [(40000, 8)]
    for M, N in cases:
        # |v| <= 8, M <= 40000: |sum| <= 320000 < 2^24, every partial sum is an integer fp32 holds exactly -- in registers, LDS and global atomics alike
        y = _ints((1, 1, M, N), g)
        src = Band(1, 1, M, N, dtype, c0=8, pad=8, tail=2).set(y)
        out = Flat(N)                                                 # garbage on entry: the call zeroes it
        assert L.mte_colsum(src.ptr, src.ld, M, N, out.ptr, _dt(dtype), _st()) == OK
        sync()
        assert beq(out.get(), y.double().sum(dim=(0, 1, 2)).float()), (M, N)
        assert out.guard_ok() and src.guard_ok(), (M, N)


def test_colsum_past_the_block_cap(L):
    """The launcher wants one block per 32 * (256 / chunks per row) rows and stops at 1024 blocks, so the grid-stride loop only wraps above
    1024 * 32 * 256 chunks = 134 MB of input whatever the shape: bf16, N = 2048 (one row per thread row), M = 33000 > 32768."""
    M, N = 33000, 2048
    assert (M + 31) // 32 > 1024
    # |v| <= 8, M = 33000: |sum| <= 264000 < 2^24: exact in fp32 in any order
    y = torch.randint(-8, 9, (M, N), generator=_gen(510), dtype=torch.int8)
    src = Band(1, 1, M, N, BF16, c0=8, pad=8, tail=2)
    src.nhwc[0, 0, :, 8:8 + N] = y.cuda().to(BF16)
    out = Flat(N)
    assert L.mte_colsum(src.ptr, src.ld, M, N, out.ptr, _dt(BF16), _st()) == OK
    sync()
    assert beq(out.get(), y.sum(0, dtype=torch.int64).float())
    assert out.guard_ok() and src.guard_ok()
    del src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum_rejects_one_chunk_too_many(L, dtype):
    N = (2048 if dtype == BF16 else 1024) + 8
    src = Band(1, 1, 2, N, dtype, c0=0, pad=0).set(torch.zeros(1, 1, 2, N))
    out = Flat(N)
    assert L.mte_colsum(src.ptr, src.ld, 2, N, out.ptr, _dt(dtype), _st()) == ERR_UNSUPPORTED
    sync()
    assert out.untouched()


# ---- 6. mte_unpack_conv_wgrad --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 3, 8, 5), (40, 65, 72, 3), (16, 8, 8, 1), (8, 70, 72, 7)])
def test_unpack_conv_wgrad(L, shape):
    Cout, Cin, Cin_p, k = shape
    taps, g = k * k, _gen(600 + Cin)
    elems = Cout * taps * Cin_p
    for parts in (1, 2, 32, 33, 64, 65, 100, 513):
        # |v| <= 8, parts <= 513: |sum| <= 4104 < 2^24: exact in fp32 whatever the grouping of the two-level sum
        stage = _ints((parts, Cout, taps, Cin_p), g)
        stage[..., Cin:] = 7.0                                        # garbage in the channel padding: it must be dropped, not summed into a neighbour
        scratch = 32 if parts > 32 else 0                             # the header: a stage of more than 32 parts carries 32 scratch slabs behind them
        buf = Flat((parts + scratch) * elems, extra=elems)            # + one guard slab
        buf.t[:parts * elems] = stage.flatten().cuda()                # the scratch slabs keep the NaN pattern: they must be written before they are read
        out = Flat(Cout * Cin * taps)
        assert L.mte_unpack_conv_wgrad(buf.ptr, parts, out.ptr, Cout, Cin, k, k, Cin_p, _st()) == OK
        sync()
        want = R.unpack_wgrad(stage, Cin)                             # [Cout][Cin][taps] = OIHW
        assert beq(out.get(), want.float().flatten()), (shape, parts)
        assert out.guard_ok() and buf.guard_ok(), (shape, parts)      # (the stage itself is scratch: no statement about its content)
        del buf


# ---- 7. mte_pack_conv_weights, _bwd, one job of _multi ---------------------------------------------------------------------------------------------
class PackJob(ctypes.Structure):                                       # mte_pack_job of include/mte_kernels.h
    _fields_ = [("w", ctypes.c_void_p), ("wf", ctypes.c_void_p), ("wb", ctypes.c_void_p), ("pf", ctypes.c_void_p), ("pb", ctypes.c_void_p),
                ("Cout", ctypes.c_int), ("Cin", ctypes.c_int), ("taps", ctypes.c_int), ("Cin_p", ctypes.c_int),
                ("end_f", ctypes.c_int), ("end_b", ctypes.c_int), ("end_pf", ctypes.c_int), ("end_pb", ctypes.c_int)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(8, 3, 5), (32, 65, 3), (72, 8, 1), (16, 130, 7)])
def test_pack_conv_weights(L, shape, dtype):
    Cout, Cin, k = shape
    Cin_p, taps = R.round8(Cin), k * k
    w = torch.randn(Cout, Cin, k, k, generator=_gen(700 + Cin))
    w_d = w.cuda()
    n = Cout * taps * Cin_p
    want_f = R.pack_fwd(w, Cin_p, dtype)                              # wf[n][tap][c] = round(w[n][c][tap]), zeros for c >= Cin
    want_b = R.pack_bwd(want_f)                                       # wb[c][taps - 1 - tap][n] = wf[n][tap][c]
    wf, wb = Flat(n, dtype), Flat(n, dtype)
    assert L.mte_pack_conv_weights(w_d.data_ptr(), wf.ptr, wb.ptr, Cout, Cin, k, k, Cin_p, Cout, _dt(dtype), _st()) == OK
    sync()
    assert beq(wf.get(), want_f.flatten()) and wf.guard_ok()
    assert beq(wb.get(), want_b.flatten()) and wb.guard_ok()
    wf1 = Flat(n, dtype)                                              # forward pack alone (null wbwd)
    assert L.mte_pack_conv_weights(w_d.data_ptr(), wf1.ptr, None, Cout, Cin, k, k, Cin_p, Cout, _dt(dtype), _st()) == OK
    wb2 = Flat(n, dtype)                                              # the data-gradient pack derived from the forward pack
    assert L.mte_pack_conv_weights_bwd(wf.ptr, wb2.ptr, Cout, k, k, Cin_p, _dt(dtype), _st()) == OK
    sync()
    assert beq(wf1.get(), want_f.flatten()) and wf1.guard_ok()
    assert beq(wb2.get(), wb.get()) and wb2.guard_ok()
    wf3, wb3 = Flat(n, dtype), Flat(n, dtype)                         # one job through the multi-tensor form
    job = (PackJob * 1)()
    job[0].w, job[0].wf, job[0].wb, job[0].pf, job[0].pb = w_d.data_ptr(), wf3.ptr, wb3.ptr, None, None
    job[0].Cout, job[0].Cin, job[0].taps, job[0].Cin_p = Cout, Cin, taps, Cin_p
    assert L.mte_pack_conv_weights_multi(ctypes.addressof(job), 1, _dt(dtype), _st()) == OK
    sync()
    assert beq(wf3.get(), want_f.flatten()) and wf3.guard_ok()
    assert beq(wb3.get(), want_b.flatten()) and wb3.guard_ok()


def test_pack_conv_weights_rejects_padded_cout_with_a_backward_pack(L):
    w = torch.randn(8, 3, 3, 3).cuda()
    wf, wb = Flat(8 * 9 * 8, BF16), Flat(8 * 9 * 16, BF16)
    assert L.mte_pack_conv_weights(w.data_ptr(), wf.ptr, wb.ptr, 8, 3, 3, 3, 8, 16, _dt(BF16), _st()) == ERR_ARG
    sync()
    assert wf.untouched() and wb.untouched()


# ---- 8. mte_pixel_shuffle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 16, 40])
def test_pixel_shuffle(L, C, dtype):
    g = _gen(800 + C)
    for H, W in ((2, 2), (6, 10), (18, 34)):
        x = torch.randn(2, H, W, C, generator=g).to(dtype)
        want = F.pixel_unshuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)          # depth d = 4 c + 2 dy + dx
        assert beq(R.pixel_unshuffle_nhwc(x), want)
        src = Band(2, H, W, C, dtype, c0=8, pad=8).set(x)
        packed = Band(2, H // 2, W // 2, 4 * C, dtype, c0=16, pad=8)
        assert L.mte_pixel_shuffle(src.ptr, src.ld, packed.ptr, packed.ld, 2, H, W, C, 0, _dt(dtype), _st()) == OK
        sync()
        assert beq(packed.get(), want) and packed.guard_ok(), (H, W)
        back = Band(2, H, W, C, dtype, c0=8, pad=16)
        assert L.mte_pixel_shuffle(packed.ptr, packed.ld, back.ptr, back.ld, 2, H, W, C, 1, _dt(dtype), _st()) == OK
        sync()
        assert beq(back.get(), F.pixel_shuffle(want.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)) and back.guard_ok(), (H, W)
        assert beq(back.get(), x), (H, W)                                                # the round trip is the identity


def test_pixel_shuffle_rejects_odd_sizes(L):
    src = Band(2, 6, 6, 16, BF16).set(torch.zeros(2, 6, 6, 16))
    dst = Band(2, 3, 3, 64, BF16)
    for H, W, C in ((5, 6, 16), (6, 5, 16), (6, 6, 12)):
        for d in (0, 1):
            assert L.mte_pixel_shuffle(src.ptr, src.ld, dst.ptr, dst.ld, 2, H, W, C, d, _dt(BF16), _st()) == ERR_ARG
    sync()
    assert dst.untouched()


# ---- 9. mte_copy_rect, mte_copy_rects ----------------------------------------------------------------------------------------------------------------
class RectOp(ctypes.Structure):                                        # mte_rect_op of include/mte_kernels.h
    _fields_ = [("src", ctypes.c_void_p), ("lds_", ctypes.c_long), ("Hs", ctypes.c_int), ("Ws", ctypes.c_int), ("sy", ctypes.c_int),
                ("sx", ctypes.c_int), ("dst", ctypes.c_void_p), ("ldd", ctypes.c_long), ("Hd", ctypes.c_int), ("Wd", ctypes.c_int),
                ("dy", ctypes.c_int), ("dx", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("mode", ctypes.c_int)]


RECTS = [  # Hs, Ws, Hd, Wd, (sy, sx, dy, dx, h, w)
    (5, 7, 5, 7, (0, 0, 0, 0, 5, 7)),          # the whole tensor
    (5, 7, 5, 7, (1, 0, 3, 0, 2, 7)),          # a full-width band
    (5, 7, 6, 9, (2, 3, 4, 5, 1, 1)),          # one pixel, tensors of different size
    (5, 7, 6, 9, (0, 0, 4, 6, 2, 3)),          # top left     -> bottom right
    (5, 7, 6, 9, (0, 4, 4, 0, 2, 3)),          # top right    -> bottom left
    (5, 7, 6, 9, (3, 0, 0, 6, 2, 3)),          # bottom left  -> top right
    (5, 7, 6, 9, (3, 4, 0, 0, 2, 3)),          # bottom right -> top left
    (5, 7, 6, 9, (1, 1, 1, 2, 4, 6)),
]


def _rect_tensors(Hs, Ws, Hd, Wd, C, dtype, g):
    # |v| <= 8: mode 1 forms dst + src, an integer of at most 16: exact in bf16 and fp32
    s, d = _ints((2, Hs, Ws, C), g), _ints((2, Hd, Wd, C), g)
    return Band(2, Hs, Ws, C, dtype, c0=8, pad=8).set(s), Band(2, Hd, Wd, C, dtype, c0=16, pad=8).set(d), s.to(dtype), d.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_rect(L, dtype):
    g, C = _gen(900), 16
    for Hs, Ws, Hd, Wd, (sy, sx, dy, dx, h, w) in RECTS:
        for mode in (0, 1, 2):
            src, dst, s, d = _rect_tensors(Hs, Ws, Hd, Wd, C, dtype, g)
            if mode == 2:                                             # zero fill: null source, its geometry unused
                rc = L.mte_copy_rect(None, 0, 0, 0, 0, 0, dst.ptr, dst.ld, Hd, Wd, dy, dx, 2, h, w, C, 2, _dt(dtype), _st())
            else:
                rc = L.mte_copy_rect(src.ptr, src.ld, Hs, Ws, sy, sx, dst.ptr, dst.ld, Hd, Wd, dy, dx, 2, h, w, C, mode, _dt(dtype), _st())
            assert rc == OK
            sync()
            case = (Hs, Ws, Hd, Wd, sy, sx, dy, dx, h, w, mode)
            assert beq(dst.get(), R.copy_rect(d.clone(), s, sy, sx, dy, dx, h, w, mode)), case       # rectangle AND everything around it
            assert dst.guard_ok() and src.guard_ok() and beq(src.get(), s), case


def _fill_op(o, src, dst, Hs, Ws, Hd, Wd, rect, mode):
    sy, sx, dy, dx, h, w = rect
    o.dst, o.ldd, o.Hd, o.Wd, o.dy, o.dx, o.h, o.w, o.mode = dst.ptr, dst.ld, Hd, Wd, dy, dx, h, w, mode
    if mode != 2:
        o.src, o.lds_, o.Hs, o.Ws, o.sy, o.sx = src.ptr, src.ld, Hs, Ws, sy, sx


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_rects(L, dtype):
    g, C = _gen(910), 16
    for picks in ([2], list(range(8))):                               # n = 1; n = 8 with areas from one pixel to the whole tensor (the grid follows the largest)
        ops = (RectOp * len(picks))()
        items = []
        for o, i in zip(ops, picks):
            Hs, Ws, Hd, Wd, rect = RECTS[i]
            mode = i % 3
            src, dst, s, d = _rect_tensors(Hs, Ws, Hd, Wd, C, dtype, g)                   # every operation has its own destination
            _fill_op(o, src, dst, Hs, Ws, Hd, Wd, rect, mode)
            items.append((src, dst, s, d, rect, mode))
        assert L.mte_copy_rects(ctypes.addressof(ops), len(picks), 2, C, _dt(dtype), _st()) == OK
        sync()
        for src, dst, s, d, rect, mode in items:
            assert beq(dst.get(), R.copy_rect(d.clone(), s, *rect, mode)), (rect, mode)
            assert dst.guard_ok() and src.guard_ok() and beq(src.get(), s), (rect, mode)
    # one destination: zero a rectangle, then add into it in a second call
    Hs, Ws, Hd, Wd, rect = RECTS[7]
    src, dst, s, d = _rect_tensors(Hs, Ws, Hd, Wd, C, dtype, g)
    for mode in (2, 1):
        ops = (RectOp * 1)()
        _fill_op(ops[0], src, dst, Hs, Ws, Hd, Wd, rect, mode)
        assert L.mte_copy_rects(ctypes.addressof(ops), 1, 2, C, _dt(dtype), _st()) == OK
    sync()
    assert beq(dst.get(), R.copy_rect(d.clone(), s, *rect, 0)) and dst.guard_ok()         # 0 + src = src exactly


def test_copy_rect_argument_errors(L):
    g, C, dt = _gen(920), 16, _dt(BF16)
    src, dst, s, d = _rect_tensors(5, 7, 6, 9, C, BF16, g)
    bad = [(0, 0, 5, 0, 2, 3), (0, 0, 0, 7, 2, 3),                    # leaves the destination (dy + h > Hd; dx + w > Wd)
           (4, 0, 0, 0, 2, 3), (0, 5, 0, 0, 2, 3),                    # leaves the source
           (0, 0, 0, 0, 0, 3)]                                        # h = 0
    for sy, sx, dy, dx, h, w in bad:
        assert L.mte_copy_rect(src.ptr, src.ld, 5, 7, sy, sx, dst.ptr, dst.ld, 6, 9, dy, dx, 2, h, w, C, 0, dt, _st()) == ERR_ARG
        ops = (RectOp * 1)()
        _fill_op(ops[0], src, dst, 5, 7, 6, 9, (sy, sx, dy, dx, h, w), 0)
        assert L.mte_copy_rects(ctypes.addressof(ops), 1, 2, C, dt, _st()) == ERR_ARG
    ops = (RectOp * 9)()
    for o in ops:
        _fill_op(o, src, dst, 5, 7, 6, 9, (0, 0, 0, 0, 1, 1), 0)
    assert L.mte_copy_rects(ctypes.addressof(ops), 0, 2, C, dt, _st()) == ERR_ARG
    assert L.mte_copy_rects(ctypes.addressof(ops), 9, 2, C, dt, _st()) == ERR_ARG
    sync()
    assert beq(dst.get(), d) and dst.guard_ok()


# ---- 10. mte_adam_step, mte_adam_step_dev -------------------------------------------------------------------------------------------------------
HYPERS = [(1e-4, 0.9, 0.999, 1e-8, 1.0), (3e-2, 0.5, 0.9, 1e-3, 0.25)]  # lr, beta1, beta2, eps, gscale
ADAM_BIG = 4 * 8192 * 256 + 3                                          # every thread of the capped grid holds one vector, then a 3-element tail
ADAM_WRAP = 4 * (8192 * 256 + 300) + 3                                 # 300 vectors more: a second trip through the vector loop


def _adam_call(L, n, hyper, step, p0, g, m0, v0):
    """one mte_adam_step and one mte_adam_step_dev from the same fp32 state.  Bounds, per element, from the kernel's ten fp32 operations
    (g * gscale; three for m; four for v; sqrt, divide, add for the denominator; divide, multiply, subtract for p -- each within 2^-24
    relative, sqrt and divide correctly rounded) against the float64 reference on the SAME fp32 inputs:
      m, v: at most four roundings on top of the rounded g * gscale: < 5 * 2^-24 * 2 = 6e-7 <= 2e-6 relative -- for m this needs
            beta1 * m and (1 - beta1) * g of one sign (no cancellation), which the inputs below guarantee;
      p:    the update carries m (1.8e-7), the denominator (v's error halved by the sqrt, three more operations, the rounded bias
            corrections: 4.5e-7) and three more operations: < 1e-6 <= 2e-6 of the update; the final subtraction rounds once: 2^-24 |p| <= 2^-23 |p_ref|."""
    lr, b1, b2, eps, gscale = hyper
    extra = 67                                                        # elements after position n of a longer buffer
    bufs = [[Flat(n, extra=extra).set(t) for t in (p0, m0, v0)] for _ in range(2)]
    g_d = g.cuda()
    (p, m, v), (pd, md, vd) = bufs
    assert L.mte_adam_step(p.ptr, g_d.data_ptr(), m.ptr, v.ptr, n, lr, b1, b2, eps, step, gscale, _st()) == OK
    hyp = R.adam_hyper(lr, b1, b2, step).cuda()
    assert L.mte_adam_step_dev(pd.ptr, g_d.data_ptr(), md.ptr, vd.ptr, n, hyp.data_ptr(), b1, b2, eps, gscale, _st()) == OK
    sync()
    for a, b in ((p, pd), (m, md), (v, vd)):
        assert torch.equal(a.raw, b.raw)                              # the device-scalar form: bit for bit, guard included
        assert a.guard_ok()
    assert beq(g_d.cpu(), g)
    pr, mr, vr, dp = R.adam_step(p0, g, m0, v0, lr, b1, b2, eps, step, gscale)
    pg, mg, vg = p.get(), m.get(), v.get()
    for name, got, ref in (("m", mg, mr), ("v", vg, vr)):
        err = (got.double() - ref).abs()
        print("adam n=%d step=%d %s: max err / |ref| = %.3g" % (n, step, name, float((err / ref.abs().clamp(min=1e-300)).max())))
        assert bool((err <= 2e-6 * ref.abs()).all()), name
    err = (pg.double() - pr).abs()
    bound = 2e-6 * dp.abs() + 2.0 ** -23 * pr.abs()
    print("adam n=%d step=%d p: max err / bound = %.3g" % (n, step, float((err / bound.clamp(min=1e-300)).max())))
    assert bool((err <= bound).all())
    return pg, mg, vg


def _adam_inputs(n, g, nonzero_state):
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)   # one sign per element for its gradients and its first moment: no cancellation in m
    p0 = torch.randn(n, generator=g)

    def grad():
        x = sign * (torch.rand(n, generator=g) + 0.01)
        x[2::3] = 0.0                                                 # exact zeros
        return x
    if not nonzero_state:
        return p0, grad, torch.zeros(n), torch.zeros(n)
    m0 = sign * (torch.rand(n, generator=g) + 0.01) * 0.1
    v0 = (torch.rand(n, generator=g) + 0.01) * 0.01
    v0[2::6] = 0.0                                                    # with a zero gradient there: v stays 0, the denominator is eps alone
    return p0, grad, m0, v0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1027])
def test_adam_step(L, n):
    for hi, hyper in enumerate(HYPERS):
        g = _gen(1000 + 10 * n + hi)
        p, grad, m, v = _adam_inputs(n, g, False)
        for step in (1, 2, 3):                                        # from zero state; the zero gradients meet v = 0
            p, m, v = _adam_call(L, n, hyper, step, p, grad(), m, v)
        p, grad, m, v = _adam_inputs(n, g, True)
        _adam_call(L, n, hyper, 1000, p, grad(), m, v)


@pytest.mark.parametrize("n", [ADAM_BIG, ADAM_WRAP])
def test_adam_step_past_the_grid_cap(L, n):
    assert (ADAM_BIG >> 2) == 8192 * 256 and (ADAM_WRAP >> 2) > 8192 * 256 and n % 4 == 3
    g = _gen(1100)
    p, grad, m, v = _adam_inputs(n, g, False)
    _adam_call(L, n, HYPERS[0], 1, p, grad(), m, v)
    p, grad, m, v = _adam_inputs(n, g, True)
    _adam_call(L, n, HYPERS[1], 1000, p, grad(), m, v)
    torch.cuda.empty_cache()


def test_adam_step_argument_errors(L):
    p, m, v = (Flat(8).set(torch.ones(8)) for _ in range(3))
    g = torch.ones(8).cuda()
    hyp = R.adam_hyper(1e-4, 0.9, 0.999, 1).cuda()
    assert L.mte_adam_step(p.ptr, g.data_ptr(), m.ptr, v.ptr, 8, 1e-4, 0.9, 0.999, 1e-8, 0, 1.0, _st()) == ERR_ARG       # step = 0
    assert L.mte_adam_step(p.ptr, g.data_ptr(), m.ptr, v.ptr, 0, 1e-4, 0.9, 0.999, 1e-8, 1, 1.0, _st()) == ERR_ARG       # n = 0
    assert L.mte_adam_step_dev(p.ptr, g.data_ptr(), m.ptr, v.ptr, 0, hyp.data_ptr(), 0.9, 0.999, 1e-8, 1.0, _st()) == ERR_ARG
    sync()
    for t in (p, m, v):
        assert beq(t.get(), torch.ones(8)) and t.guard_ok()


# ---- 11. mte_resize_bilinear_fwd / _bwd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 6, 8, 12), (5, 7, 12, 20), (12, 20, 5, 7), (1, 1, 3, 4), (3, 4, 3, 4), (7, 5, 7, 11)])
def test_resize_bilinear(L, shape):
    h, w, H, W = shape
    B, g = 3, _gen(1200 + h)
    x = torch.randn(B, h, w, generator=g)
    dy = torch.randn(B, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    yr = R.resize_bilinear(xr, H, W)
    (yr * dy.double()).sum().backward()
    y = Flat(B * H * W)
    assert L.mte_resize_bilinear_fwd(x.cuda().data_ptr(), y.ptr, B, h, w, H, W, _st()) == OK
    dx = Flat(B * h * w)                                              # garbage on entry: the call zeroes it
    assert L.mte_resize_bilinear_bwd(dy.cuda().data_ptr(), dx.ptr, B, h, w, H, W, _st()) == OK
    sync()
    assert y.guard_ok() and dx.guard_ok()
    yg, dxg = y.get().view(B, H, W).double(), dx.get().view(B, h, w).double()
    # forward: the source coordinate (< 20) carries at most ~2.4e-6 of fp32 error and multiplies a neighbour difference of at most 2 max|x|; four product
    # roundings on top: 1e-5 max|x|
    err = float((yg - yr.detach()).abs().max())
    print("bilinear %s fwd: err %.3g, bound %.3g" % (shape, err, 1e-5 * float(x.abs().max())))
    assert err <= 1e-5 * float(x.abs().max())
    # backward: a source pixel sums one such term from each destination pixel it feeds: the same bound times the largest fan-in
    basis = torch.eye(h * w, dtype=torch.float64).view(h * w, h, w)
    fan_in = int((R.resize_bilinear(basis, H, W) != 0).flatten(1).sum(1).max())
    err = float((dxg - xr.grad).abs().max())
    print("bilinear %s bwd: err %.3g, bound %.3g (fan-in %d)" % (shape, err, 1e-5 * fan_in * float(dy.abs().max()), fan_in))
    assert err <= 1e-5 * fan_in * float(dy.abs().max())
    # adjoint identity <R x, g> = <x, R^T g> on what the two kernels returned
    lhs, rhs = float((yg * dy.double()).sum()), float((x.double() * dxg).sum())
    print("bilinear %s adjoint: %.10g vs %.10g" % (shape, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


# ---- 12. mte_silog_fwd / _bwd -----------------------------------------------------------------------------------------------------------------------
def _silog_inputs(n, g):
    depth = 1.0 / (torch.rand(n, generator=g) * 0.9 + 0.05)
    inv = (1.0 / depth) * torch.exp(torch.rand(n, generator=g) - 0.5)        # the log ratio spreads over [-0.5, 0.5]: S = E[d^2] - 0.85 E[d]^2 is well away from 0
    if n == 1:
        inv = inv * 2.0                                               # one pixel: S = 0.15 d^2, keep d away from 0
    else:
        depth[1::3] = 0.0                                             # invalid pixels
    return inv, depth


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_silog(L, n):
    g = _gen(1300 + n)
    inv, depth = _silog_inputs(n, g)
    ir = inv.double().requires_grad_(True)
    ref = R.silog(ir, depth)
    ref.backward()
    ref, dref = float(ref.detach()), ir.grad
    inv_d, depth_d = inv.cuda(), depth.cuda()
    sums, aux, this = Flat(3, torch.float64, extra=4), Flat(2), Flat(1)
    # plain call: loss_this and aux only
    assert L.mte_silog_fwd(inv_d.data_ptr(), depth_d.data_ptr(), n, sums.ptr, 1.0, None, this.ptr, aux.ptr, _st()) == OK
    sync()
    loss = float(this.get()[0])
    print("silog n=%d: loss %.8g ref %.8g rel %.3g" % (n, loss, ref, abs(loss - ref) / abs(ref)))
    assert abs(loss - ref) <= 1e-5 * abs(ref)                         # the project's bar for this scalar
    assert sums.guard_ok() and aux.guard_ok() and this.guard_ok()
    # a path the Python host never takes: loss_acc += out_scale * loss with out_scale != 1 (two fp32 operations on top of loss_this)
    acc, this2, aux2 = Flat(1).set(torch.tensor([3.0])), Flat(1), Flat(2)
    assert L.mte_silog_fwd(inv_d.data_ptr(), depth_d.data_ptr(), n, sums.ptr, 0.5, acc.ptr, this2.ptr, aux2.ptr, _st()) == OK
    sync()
    assert beq(this2.get(), this.get()) and beq(aux2.get(), aux.get())
    assert beq(acc.get(), torch.tensor([3.0]) + torch.tensor([0.5]) * this.get()) and acc.guard_ok()
    # backward, overwrite: dinv within 2e-4 of its maximum (the project's bar for this gradient), exact zeros on the invalid pixels
    dinv = Flat(n)
    assert L.mte_silog_bwd(inv_d.data_ptr(), depth_d.data_ptr(), aux.ptr, None, dinv.ptr, n, 0, _st()) == OK
    # accumulate = 1 onto a non-zero dinv with an upstream gradient of 0.5
    old = torch.randn(n, generator=g)
    dacc, gout = Flat(n).set(old), torch.tensor([0.5]).cuda()
    assert L.mte_silog_bwd(inv_d.data_ptr(), depth_d.data_ptr(), aux.ptr, gout.data_ptr(), dacc.ptr, n, 1, _st()) == OK
    sync()
    got, gacc = dinv.get(), dacc.get()
    dmax = float(dref.abs().max())
    err = float((got.double() - dref).abs().max())
    print("silog n=%d: dinv err / max = %.3g" % (n, err / dmax))
    assert err <= 2e-4 * dmax and dinv.guard_ok()
    masked = depth <= 0
    assert not got[masked].any()
    want = old.double() + 0.5 * dref
    assert bool(((gacc.double() - want).abs() <= 2e-4 * 0.5 * dmax + 2.0 ** -23 * want.abs()).all()) and dacc.guard_ok()      # + one fp32 addition
    assert beq(gacc[masked], old[masked])


def test_silog_without_a_valid_pixel_is_nan(L):
    n = 257
    inv, _ = _silog_inputs(n, _gen(1390))
    depth = torch.zeros(n)
    sums, aux, this = Flat(3, torch.float64, extra=4), Flat(2), Flat(1)
    assert L.mte_silog_fwd(inv.cuda().data_ptr(), depth.cuda().data_ptr(), n, sums.ptr, 1.0, None, this.ptr, aux.ptr, _st()) == OK
    sync()
    assert bool(torch.isnan(this.get()).all())
    assert sums.guard_ok() and aux.guard_ok() and this.guard_ok()
