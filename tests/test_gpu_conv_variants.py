"""GPU (-m gpu): the specialised conv kernels must agree with the generic implicit GEMM on identical bf16 inputs
(same products, fp32 accumulation, only the summation order differs), and the generic kernel in fp32 mode must agree
with torch's CPU fp32 convolution.  Shapes cover every (k, C_in, C_out) class of the PackNetSAN01 high-resolution
layers, ragged heights (H % 8 != 0), channel-padded inputs and the split-K path.

Tests that force a kernel variant take the ``devlib`` fixture: they run on libmte_hip_dev.so, the -DMTE_DEV build of the same
sources -- the shipped libmte_hip.so does not export mte_debug_set (tests/test_cabi.py)."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture
def devlib():
    from mindtheedge_amd._lib import dev_library
    with dev_library() as lib:
        yield lib

SHAPES = [  # cin, cout, k, B, H, W
    (32, 32, 7, 2, 16, 64), (512, 32, 5, 1, 12, 32), (3, 32, 5, 2, 20, 64), (65, 32, 3, 1, 9, 96), (64, 64, 3, 2, 16, 32),
    (32, 64, 1, 2, 8, 64), (97, 64, 3, 1, 24, 32), (1024, 64, 3, 1, 8, 32), (64, 32, 3, 2, 10, 32), (16, 16, 3, 1, 8, 32),
    (32, 64, 3, 1, 7, 64),
    # round 3: 65..128 output channels, 3x3 -- the wide LDS-patch WEIGHT gradient (forward / data gradient stay on the implicit GEMM)
    # round 3: the 8-input-channel stem kernels (csrc/conv_stem.hip): reduction over (tap, channel), ragged heights, k = 3 / 5 / 7
    (3, 32, 5, 1, 37, 96), (3, 16, 3, 2, 9, 32), (3, 32, 7, 1, 16, 32), (8, 24, 5, 2, 16, 64),
    (128, 128, 3, 2, 16, 64), (200, 128, 3, 1, 12, 32), (64, 128, 3, 2, 8, 64), (256, 128, 3, 1, 13, 32), (72, 96, 3, 2, 9, 32), (64, 72, 3, 1, 6, 96),
    # round 3: the second form of the LDS-patch forward -- tall (16-row) tiles with a ragged last tile, one / two / three slices, 5x5 and 7x7
    (32, 32, 3, 1, 24, 64), (72, 32, 3, 1, 20, 32), (32, 32, 5, 1, 40, 64), (40, 32, 5, 1, 20, 32), (32, 24, 7, 1, 21, 32), (136, 64, 3, 1, 11, 64),
    # round 6: the 5x5 / 7x7 second form on v_mfma_f32_16x16x32_bf16 -- two 32-channel output tiles, several slices, ragged rows, channel tails
    (256, 64, 5, 1, 12, 64), (48, 56, 5, 2, 9, 32), (128, 32, 7, 1, 18, 32),
]


def _run(cin, cout, k, B, H, W, patch, dtype="bf16"):
    from mindtheedge_amd import kernels as K
    K.set_compute_dtype(dtype)
    K.use_patch_kernels(patch)
    try:
        g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + k)
        w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda().requires_grad_(True)
        b = (torch.rand(cout, generator=g) - 0.5).cuda().requires_grad_(True)
        x = (torch.rand(B, cin, H, W, generator=g) * 2 - 1)
        G = (torch.rand(B, cout, H, W, generator=g) * 2 - 1)
        xa = K.image_to_act(x.cuda()).detach().requires_grad_(True)
        pack = K.WeightPack()
        y = K.ConvFn.apply(xa, w, b, pack)
        (y.float() * G.cuda()).sum().backward()
        torch.cuda.synchronize()
        return dict(y=y.float().cpu(), dx=xa.grad.float().cpu()[:, :cin], dw=w.grad.cpu(), db=b.grad.cpu(), x=x, G=G,
                    w=w.detach().cpu(), b=b.detach().cpu())
    finally:
        K.use_patch_kernels(True)
        K.set_compute_dtype("bf16")


@pytest.mark.parametrize("shape", SHAPES)
def test_patch_kernels_match_generic_igemm(shape):
    a = _run(*shape, patch=True)
    r = _run(*shape, patch=False)
    assert rel_err(a["y"], r["y"]) < 8e-3          # both round the same fp32 sums to bf16: at most 1 bf16 ulp apart
    assert rel_err(a["dx"], r["dx"]) < 8e-3
    assert rel_err(a["dw"], r["dw"]) < 2e-4        # fp32 outputs: summation order only
    assert rel_err(a["db"], r["db"]) < 1e-5


PATCH_M16_SHAPES = [(32, 32, 7, 2, 16, 64), (128, 32, 7, 1, 18, 32), (256, 64, 5, 1, 12, 64), (48, 56, 5, 2, 9, 32), (64, 64, 3, 2, 16, 32), (32, 64, 1, 2, 8, 64),
                    (72, 32, 3, 1, 20, 32), (136, 64, 3, 1, 11, 64), (65, 32, 3, 1, 9, 96), (64, 32, 3, 2, 10, 32)]


@pytest.mark.parametrize("shape", PATCH_M16_SHAPES)
def test_patch_forward_mfma_shapes_agree(shape, devlib):
    """round 6: every LDS-patch forward form runs on v_mfma_f32_16x16x32_bf16; the 32x32x16 forms of rounds 1-5 live on in the development library (knobs
    11 = 500 / 600 / 700).  Same products, fp32 sums in another order inside the instruction: outputs and data gradients within one bf16 rounding."""
    cin, cout, k, B, H, W = shape

    def run(m16):
        for base in (500, 600, 700):
            devlib.mte_debug_set(11, base + m16)
        try:
            return _run(cin, cout, k, B, H, W, patch=True)
        finally:
            for base in (500, 600, 700):
                devlib.mte_debug_set(11, base + 1)

    a, r = run(1), run(0)
    assert rel_err(a["y"], r["y"]) < 8e-3
    assert rel_err(a["dx"], r["dx"]) < 8e-3


@pytest.mark.parametrize("shape", SHAPES[:6] + [(512, 512, 3, 2, 4, 8), (256, 8, 3, 1, 6, 10)])
def test_generic_igemm_fp32_matches_torch_cpu(shape):
    r = _run(*shape, patch=False, dtype="fp32")
    x = r["x"].clone().requires_grad_(True)
    w = r["w"].clone().requires_grad_(True)
    b = r["b"].clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, b, padding=shape[2] // 2)
    (y * r["G"]).sum().backward()
    assert rel_err(r["y"], y) < 2e-5
    assert rel_err(r["dx"], x.grad) < 2e-5
    assert rel_err(r["dw"], w.grad) < 5e-5
    assert rel_err(r["db"], b.grad) < 2e-5


WGRAD_SHAPES = [  # cin, cout, k, B, H, W — row-aligned blocks (W % 32 == 0, ragged W >= 160), flattened pixels, partial tiles
    (128, 128, 3, 2, 16, 64), (72, 96, 3, 2, 9, 40), (256, 64, 3, 1, 12, 32), (64, 128, 1, 3, 7, 24), (40, 256, 5, 1, 6, 168),
    (512, 512, 3, 1, 8, 20), (136, 264, 3, 2, 5, 80), (64, 64, 7, 1, 9, 48), (256, 256, 3, 2, 12, 32), (128, 256, 3, 2, 9, 40),
    (256, 128, 3, 1, 6, 168), (512, 256, 1, 2, 10, 24),
]


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_dma_wgrad_matches_register_staged_wgrad(shape, devlib):
    """The LDS-DMA ring weight-gradient kernel (swizzled tiles) against the register-staged one (padded tiles): identical
    bf16 products, fp32 accumulation, only the order of the pixel reduction differs."""
    from mindtheedge_amd import kernels as K
    try:
        a = _run(*shape, patch=False)
        K.lib.mte_debug_set(8, 0)                      # 4-wave 128x128 tiles only
        big = _run(*shape, patch=False)
        K.lib.mte_debug_set(4, 0)
        r = _run(*shape, patch=False)
    finally:
        K.lib.mte_debug_set(33, 0)                     # every weight-gradient knob back to its default (WgradKnobs{}, csrc/wgrad_plan.hpp)
    assert rel_err(a["dw"], r["dw"]) < 2e-4
    assert rel_err(big["dw"], r["dw"]) < 2e-4
    assert torch.equal(a["y"], r["y"])                 # (the forward kernel is the same in all three runs and bit-reproducible)


@pytest.mark.parametrize("shape", [(64, 128, 3, 2, 24, 40), (96, 256, 3, 3, 10, 52), (32, 128, 5, 1, 30, 33), (128, 384, 1, 2, 16, 48)])
def test_igemm_256x128_tiles_match_128x128_tiles(shape, devlib):
    """The 8-wave 256x128-tile and 16-wave 256x256-tile instantiations of the implicit GEMM against the 4-wave 128x128 one: same K order, same fp32
    accumulation chain per output, so forward and data gradient must be bit-identical."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W = shape

    def run(big):
        K.lib.mte_debug_set(6, big); K.lib.mte_debug_set(23, 0)      # (the older tile forms are the subject: 8-phase kernels off)
        K.lib.mte_debug_set(7, 1)
        orig, K._splitk_workspace = K._splitk_workspace, lambda *a: (None, 0)
        try:
            g = torch.Generator().manual_seed(3 + cin + cout)
            w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
            b = (torch.rand(cout, generator=g) - 0.5).cuda()
            xa = K.image_to_act(torch.rand(B, cin, H, W, generator=g).cuda() * 2 - 1)
            dy = K.image_to_act(torch.rand(B, cout, H, W, generator=g).cuda() * 2 - 1)
            pack = K.WeightPack()
            wf, wb = pack.get(w, xa.dtype, True)
            y = K.conv_forward(xa, wf, b, cout, k, k)
            dx = K.conv_forward(dy, wb, None, K.round8(cin), k, k) if K.round8(cin) % 128 == 0 else None
            torch.cuda.synchronize()
            return y.float().cpu(), None if dx is None else dx.float().cpu()
        finally:
            K._splitk_workspace = orig
            K.lib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)

    K.use_patch_kernels(False)
    try:
        yb, db = run(0)
        for big in (1, 2):                                          # 1: 256x128 only; 2: 256x256 where C_out % 256 == 0
            ya, da = run(big)
            assert torch.equal(ya, yb)
            if da is not None:
                assert torch.equal(da, db)
    finally:
        K.use_patch_kernels(True)


@pytest.mark.parametrize("shape", [(256, 256, 3, 8, 48, 160), (64, 256, 5, 2, 96, 320), (96, 512, 3, 3, 10, 52), (128, 256, 1, 8, 48, 160),
                                   (32, 256, 1, 2, 16, 48), (64, 512, 1, 1, 24, 40), (96, 256, 1, 2, 10, 52)])      # (the last three: 1, 2 and 3 K-steps)
def test_igemm_pingpong_loop_matches_one_barrier_loop(shape, devlib):
    """The 8-wave ping-pong form of the 256x256 tile (two wave groups half a K-step apart, round 3) against the 16-wave one-barrier form and
    the 4-wave 128x128 tiles: same K order and fp32 accumulation chain per output, so all three are bit-identical -- repeated, because a
    stale ring slot or a fragment read that overtakes its DMA would show on some launches only (tools/igemm_race_stress.py screens longer)."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W = shape
    g = torch.Generator().manual_seed(11 + cin + cout)
    w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
    b = (torch.rand(cout, generator=g) - 0.5).cuda()
    xa = K.image_to_act(torch.rand(B, cin, H, W, generator=g).cuda() * 2 - 1)
    pack = K.WeightPack()
    wf, _ = pack.get(w, xa.dtype, False)
    orig, K._splitk_workspace = K._splitk_workspace, lambda *a: (None, 0)
    K.use_patch_kernels(False)

    def run(big, pp):
        K.lib.mte_debug_set(6, big); K.lib.mte_debug_set(23, 0)      # (the older tile forms are the subject: 8-phase kernels off)
        K.lib.mte_debug_set(7, 1)
        K.lib.mte_debug_set(21, pp)
        y = K.conv_forward(xa, wf, b, cout, k, k)
        torch.cuda.synchronize()
        return y
    try:
        ref = run(0, 0).clone()
        for rep in range(6):
            assert torch.equal(run(2, 1), ref), "ping-pong loop, repetition %d" % rep
            assert torch.equal(run(2, 0), ref), "16-wave loop, repetition %d" % rep
    finally:
        K._splitk_workspace = orig
        K.use_patch_kernels(True)
        K.lib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)


@pytest.mark.parametrize("shape", [(512, 256, 3, 4, 32, 40), (1024, 512, 3, 2, 40, 64)])
def test_big_tile_split_k_matches_small_tiles(shape, devlib):
    """Few output tiles + a long reduction (the pack4/pack5.conv regime): 256x256 tiles with the K range split over
    workgroups (one slab per split + finish kernel) against the 128x128 split-K path -- same bf16 products, different
    summation order.  Each path is bit-reproducible run to run (slabs are added in split order, no atomics)."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W = shape
    K.use_patch_kernels(False)
    try:
        outs = []
        for big in (2, 0, 2, 0):
            K.lib.mte_debug_set(6, big); K.lib.mte_debug_set(23, 0)      # (the older tile forms are the subject: 8-phase kernels off)
            g = torch.Generator().manual_seed(11 + cin)
            w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
            b = (torch.rand(cout, generator=g) - 0.5).cuda()
            xa = K.image_to_act(torch.rand(B, cin, H, W, generator=g).cuda() * 2 - 1)
            wf, _ = K.WeightPack().get(w, xa.dtype, False)
            outs.append(K.conv_forward(xa, wf, b, cout, k, k).float().cpu())
        assert rel_err(outs[0], outs[1]) < 8e-3
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
        assert float(outs[0].abs().mean()) > 0.1                 # (not trivially zero)
    finally:
        K.lib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)
        K.use_patch_kernels(True)


@pytest.mark.parametrize("shape", [(32, 72, 3, 2, 24, 40), (64, 88, 3, 1, 30, 33), (96, 96, 1, 2, 16, 48), (32, 72, 3, 1, 17, 31)])
def test_igemm_192x96_tiles_match_128x128_tiles(shape, devlib):
    """The 6-wave 192x96-tile instantiation (65..96 output columns: the 72-channel decoder concat as data-gradient N)
    against the 4-wave 128x128 one: same K order and accumulation chain per output -> bit-identical, with and without
    accumulation into the destination."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W = shape

    def run(big):
        K.lib.mte_debug_set(6, big); K.lib.mte_debug_set(23, 0)      # (the older tile forms are the subject: 8-phase kernels off)
        K.lib.mte_debug_set(7, 1)
        orig, K._splitk_workspace = K._splitk_workspace, lambda *a: (None, 0)
        try:
            g = torch.Generator().manual_seed(5 + cin + cout)
            w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
            b = (torch.rand(cout, generator=g) - 0.5).cuda()
            xa = K.image_to_act(torch.rand(B, cin, H, W, generator=g).cuda() * 2 - 1)
            wf, _ = K.WeightPack().get(w, xa.dtype, False)
            y = K.conv_forward(xa, wf, b, cout, k, k)
            acc = K.conv_forward(xa, wf, None, cout, k, k, out=y.clone(memory_format=torch.preserve_format), accumulate=True)
            torch.cuda.synchronize()
            return y.float().cpu(), acc.float().cpu()
        finally:
            K._splitk_workspace = orig
            K.lib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)

    K.use_patch_kernels(False)
    try:
        y0, a0 = run(0)
        y3, a3 = run(3)
        assert torch.equal(y3, y0) and torch.equal(a3, a0)
        assert float(y0.abs().mean()) > 0.05
    finally:
        K.use_patch_kernels(True)


IGEMM8_SHAPES = [  # cin, cout, k, B, H, W, channels per input pixel (None = cin): odd K-step counts, column / row tails, 64 / 96 / 160-channel taps
    (64, 256, 3, 2, 24, 40, None), (96, 256, 3, 3, 10, 52, None), (32, 384, 5, 1, 17, 33, None), (128, 384, 1, 2, 16, 48, None),
    (256, 256, 3, 2, 48, 80, None), (64, 200, 3, 2, 40, 64, 96), (128, 128, 3, 2, 48, 96, None), (96, 128, 3, 1, 33, 47, None),
    (512, 104, 3, 1, 24, 80, None), (160, 136, 3, 1, 31, 45, 200), (32, 128, 7, 1, 64, 96, None), (1024, 512, 3, 1, 12, 40, None),
]


@pytest.mark.parametrize("order", ["tap-major", "slice-major"])
@pytest.mark.parametrize("shape", IGEMM8_SHAPES)
def test_eight_phase_igemm_against_the_128x128_tile(devlib, shape, order):
    """round 4 (csrc/conv_igemm8.hip): the 8-phase kernels -- 256 x 256 and 256 x 128 tiles -- forced onto small and awkward shapes (development knob
    23 = 7, 24 = 1), repeatedly (a stale LDS slot or a fragment read that overtakes its DMA shows on some repetitions only), with and without
    accumulation into the output and through a channel-slice output.
      tap-major (knob bit 5: the K order of every other tile form): the same K-steps in the same order -> the 4-wave 128 x 128 kernel BIT FOR BIT;
      slice-major (round 5, a DEVELOPMENT option -- the shipped default is tap-major, knob 23 = 51, and the product library returns MTE_ERR_UNSUPPORTED for
      ConvArgs.kslice; 64-channel slice outer, taps inner, where Cin_p % 64 == 0): bit-identical from run to run, and to the
      128 x 128 kernel within one bf16 rounding of the output (another order of the same fp32 sum); shapes whose channels do not allow it run tap-major.
    Split-K (another grouping of the fp32 sums): bitwise against itself, one bf16 rounding against the unsplit result."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W, ldx = shape
    K.set_compute_dtype("bf16")
    K.use_patch_kernels(False)
    saved = K._splitk_workspace
    exact = order == "tap-major" or K.round8(cin) % 64 != 0
    try:
        g = torch.Generator().manual_seed(3 + cin + cout)
        w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
        b = (torch.rand(cout, generator=g) - 0.5).cuda()
        buf = K.new_act(B, ldx or cin, H, W)
        buf.copy_((torch.rand(B, ldx or cin, H, W, generator=g) * 2 - 1).cuda())
        x = K.channel_slice(buf, 0, cin) if ldx else buf
        wf, _ = K.WeightPack().get(w, x.dtype, True)
        y0 = K.new_act(B, cout + 8, H, W)
        y0.copy_(torch.randn(B, cout + 8, H, W, generator=g).cuda())

        def run(v8, split, accumulate):
            devlib.mte_debug_set(23, v8); devlib.mte_debug_set(24, 1000000 if split else 1); devlib.mte_debug_set(6, 0)
            K._splitk_workspace = (lambda M, N, dev: (torch.empty((8 * M * N,), dtype=torch.float32, device=dev), 8 * M * N)) if split else (lambda *a: (None, 0))
            out = y0.clone()
            K.conv_forward(x, wf, b, cout, k, k, out=K.channel_slice(out, 0, cout), accumulate=accumulate)
            torch.cuda.synchronize()
            return out

        def one_rounding(a_, ref_, old=None):
            # |d| <= one bf16 ulp of the result; with accumulation (old = the values added onto) the convolution is rounded BEFORE the sum, so an ulp
            # of the convolution's own size (ref - old) can come on top -- far larger than the result's where the two nearly cancel
            d = (a_.float() - ref_.float()).abs()
            size = ref_.float().abs() if old is None else ref_.float().abs() + (ref_.float() - old.float()).abs()
            return float((d - size * 2.0 ** -7).max()) <= 1e-3

        v8 = 7 | (32 if order == "tap-major" else 0)                     # (23 = 0 below: the older tile forms; the test restores the product's 51)
        for accumulate in (False, True):
            ref = run(0, False, accumulate)
            first = run(v8, False, accumulate)
            for rep in range(3):
                assert torch.equal(run(v8, False, accumulate), first), (shape, accumulate, rep)
            if exact:
                assert torch.equal(first, ref), (shape, accumulate)
            else:
                # (accumulate: conv + bias is rounded to bf16, then the sum with the old value is -- two roundings that can each fall the other way)
                assert one_rounding(first[:, :cout], ref[:, :cout], y0[:, :cout] if accumulate else None), (shape, accumulate)
            assert torch.equal(first[:, cout:], y0[:, cout:])                   # nothing written past the slice
        first = run(v8, True, False)
        assert torch.equal(run(v8, True, False), first)
        assert one_rounding(first, run(0, False, False))
    finally:
        K._splitk_workspace = saved
        devlib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)
        K.use_patch_kernels(True)


@pytest.mark.parametrize("shape", [s_ for s_ in IGEMM8_SHAPES if ((s_[0] + 7) // 8 * 8) % 64 == 0])
def test_eight_phase_one_tap_state_loop_matches_the_two_state_loop(devlib, shape):
    """round-5 advisor: the shipped default of conv_igemm8_kernel where Cin_p % 64 == 0 is the ONE form (both K-halves of a K-tile from one tap state,
    IgemmKnobs.igemm8_one = 1) -- it had no on / off test of its own.  Development knob 28 = 0 runs the general two-state loop on the same launch: the same K-steps in
    the same order, so the outputs must be bit-identical -- unsplit, accumulating, and under split-K (where the ONE form also needs an even K-step count per
    split: the launcher's own rule decides, the test only flips the knob)."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W, ldx = shape
    K.set_compute_dtype("bf16")
    K.use_patch_kernels(False)
    saved = K._splitk_workspace
    try:
        g = torch.Generator().manual_seed(5 + cin + cout)
        w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
        b = (torch.rand(cout, generator=g) - 0.5).cuda()
        buf = K.new_act(B, ldx or cin, H, W)
        buf.copy_((torch.rand(B, ldx or cin, H, W, generator=g) * 2 - 1).cuda())
        x = K.channel_slice(buf, 0, cin) if ldx else buf
        wf, _ = K.WeightPack().get(w, x.dtype, True)
        y0 = K.new_act(B, cout, H, W)
        y0.copy_(torch.randn(B, cout, H, W, generator=g).cuda())
        devlib.mte_debug_set(23, 7 | 32); devlib.mte_debug_set(6, 0)

        def run(one, split, accumulate):
            devlib.mte_debug_set(28, one); devlib.mte_debug_set(24, 1000000 if split else 1)
            K._splitk_workspace = (lambda M, N, dev: (torch.empty((8 * M * N,), dtype=torch.float32, device=dev), 8 * M * N)) if split else (lambda *a: (None, 0))
            out = y0.clone()
            K.conv_forward(x, wf, b, cout, k, k, out=out, accumulate=accumulate)
            torch.cuda.synchronize()
            return out

        for split, accumulate in ((False, False), (False, True), (True, False)):
            assert torch.equal(run(1, split, accumulate), run(0, split, accumulate)), (shape, split, accumulate)
    finally:
        K._splitk_workspace = saved
        devlib.mte_debug_set(33, 0)                     # every implicit-GEMM knob back to its default (IgemmKnobs{}, csrc/conv_plan.hpp)
        K.use_patch_kernels(True)


# ---- round 5: the nine-tap 3x3 weight gradient (csrc/conv_wgrad9.hip) behind mte_conv2d_wgrad
WGRAD9_SHAPES = [  # cin, cout, B, H, W, input as a channel slice of a wider buffer?
    (128, 128, 2, 16, 64, False),      # one tile, 1 x 32 K-steps
    (256, 256, 2, 12, 32, False),      # 2 x 4 tiles, one K-step per image row: every patch column block touches both borders
    (128, 256, 2, 8, 80, False),       # 80-pixel rows: 2 x 16 K-steps (the 24x80 layers' form)
    (512, 512, 1, 8, 48, False),       # 2 x 16 K-steps, 4 x 8 tiles, few K-steps per split
    (192, 128, 1, 6, 160, True),       # three input tiles out of a 256-channel buffer (a decoder concat slice)
    (64, 384, 3, 10, 32, False),       # three output tiles, three images
    (256, 128, 1, 5, 64, True),        # odd height
    (64, 128, 8, 24, 80, False),       # many pixel splits (one tile: splits = the CU count, capped by the stage)
    (2048, 128, 16, 3, 160, False),    # the folded pack layers' form (round 5: taken over from the LDS-patch kernel): three rows, every K-step at a border
    (128, 128, 1, 1, 32, False),       # one row: top and bottom border in the same K-step
]


@pytest.mark.parametrize("shape", WGRAD9_SHAPES)
def test_nine_tap_wgrad_matches_the_per_tap_kernel_and_fp64(shape, devlib):
    """mte_conv2d_wgrad's nine-tap kernel against the generic per-tap kernel (development knob 26 = 0) on identical bf16 operands -- fp32
    accumulation, only the order of the pixel sum differs -- against an fp64 convolution gradient of the same rounded operands, and twice
    bit for bit (plain stores into per-split slabs, fixed-order sums)."""
    from mindtheedge_amd import kernels as K
    cin, cout, B, H, W, sliced = shape
    K.set_compute_dtype("bf16")
    K.use_patch_kernels(False)
    try:
        g = torch.Generator().manual_seed(cin + 3 * cout + W)
        xf = (torch.rand(B, cin, H, W, generator=g) * 2 - 1).bfloat16().float()
        gf = (torch.rand(B, cout, H, W, generator=g) * 2 - 1).bfloat16().float()
        w = torch.zeros(cout, cin, 3, 3, device="cuda")
        if sliced:
            buf = K.new_act(B, cin + 64, H, W, torch.bfloat16)
            buf.zero_()
            x = K.channel_slice(buf, 32, 32 + cin)
            x.copy_(xf.cuda())
        else:
            x = K.as_act(xf.cuda(), torch.bfloat16)
        dy = K.as_act(gf.cuda(), torch.bfloat16)
        assert devlib.mte_debug_set(26, 1) is None
        a, _ = K._conv_wgrad(x, dy, w, False, None, None)
        a2, _ = K._conv_wgrad(x, dy, w, False, None, None)
        devlib.mte_debug_set(26, 0)
        r, _ = K._conv_wgrad(x, dy, w, False, None, None)
        torch.cuda.synchronize()
        assert torch.equal(a, a2)
        assert rel_err(a.cpu(), r.cpu()) < 2e-4
        xd = xf.double().requires_grad_(False)
        wd = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(xd, wd, None, padding=1)
        (y * gf.double()).sum().backward()
        assert rel_err(a.cpu(), wd.grad) < 2e-5, rel_err(a.cpu(), wd.grad)
    finally:
        devlib.mte_debug_set(33, 0)                    # every weight-gradient knob back to its default (WgradKnobs{}, csrc/wgrad_plan.hpp)
        K.use_patch_kernels(True)


GN_IN_CONV_SHAPES = [
    # cin, cout, k, B, H, W, accumulate
    (32, 32, 7, 2, 16, 64, False),     # tall second form (16-row tiles)
    (32, 64, 3, 1, 24, 32, False),     # first form, two 32-channel output blocks
    (96, 64, 3, 2, 12, 64, False),     # second form, two output blocks, ragged last tile row (12 = 8 + 4)
    (64, 32, 3, 1, 40, 32, False),     # tall 3x3, 40 = 2 x 16 + 8 rows
    (32, 32, 3, 1, 9, 32, False),      # H < 16: 8-row tiles, one row in the second tile
    (128, 32, 7, 1, 16, 32, False),    # 7x7 with four input slices (8-row tiles)
    (32, 64, 5, 2, 8, 96, False),
    (32, 64, 3, 1, 24, 32, True),      # accumulating launches: the statistics of the SUMS that are stored
    (96, 32, 3, 2, 20, 64, True),
    (32, 16, 3, 1, 16, 32, False),     # 16 outputs: one channel per group
]


@pytest.mark.parametrize("shape", GN_IN_CONV_SHAPES)
def test_patch_forward_leaves_the_groupnorm_statistics_of_what_it_stores(shape):
    """mte_conv2d_patch_fwd_gn (round 5; reference layers01.py:35-38, Conv2d -> GroupNorm(16)): the per-tile records written in the store loop, added by
    mte_gn_stats_from_records, against the stand-alone statistics pass (mte_gn_stats) over the same output -- every kernel form, ragged tile rows, accumulating
    launches; the convolution output itself must not change by a bit, and two runs must agree bit for bit."""
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W, accumulate = shape
    K.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(cin + cout + k + H)
    x = K.image_to_act((torch.rand(B, cin, H, W, generator=g) * 2 - 1).cuda())
    w = ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5).cuda()
    b = (torch.rand(cout, generator=g) - 0.5).cuda()
    old = K.image_to_act((torch.rand(B, cout, H, W, generator=g) * 2 - 1).cuda()) if accumulate else None
    pack = K.WeightPack()
    wf, _ = pack.get(w, x.dtype, False)
    st = torch.cuda.current_stream().cuda_stream

    def run(records):
        out = old.clone() if accumulate else None
        recs = [] if records else None
        y = K.conv_forward(x, wf, b, cout, k, k, out=out, pack=pack, w=w, accumulate=accumulate, gn_records=recs)
        stats = K.gn_stats_buffer(B, x.device)
        if records:
            assert len(recs) == 1
            K.lib.mte_gn_stats_from_records(recs[0][0].data_ptr(), recs[0][1], stats.data_ptr(), B, st)
        else:
            p, l = K._pl(y)
            K.lib.mte_gn_stats(p, l, 0, 0, 0, stats.data_ptr(), B, H * W, cout, K.DT_BF16, st)
        torch.cuda.synchronize()
        return y, stats[:32 * B].clone().cpu()

    y0, ref = run(False)
    y1, got = run(True)
    assert torch.equal(y0, y1)                                                 # the store loop stores what it stored before
    v = y1.float().double()
    exact = torch.stack([v.reshape(B, 16, -1).sum(2), (v * v).reshape(B, 16, -1).sum(2)], dim=2).reshape(-1).cpu()   # (NCHW view: groups of cout/16 channels)
    scale = exact.abs().max()
    assert float((got - exact).abs().max()) <= 2e-6 * float(scale) + 2 * float((ref - exact).abs().max())
    y2, again = run(True)
    assert torch.equal(got, again)


@pytest.mark.parametrize("cin,cout,k,B,H,W", [(256, 256, 3, 2, 24, 64), (64, 64, 3, 1, 32, 64), (32, 32, 7, 1, 16, 64), (128, 128, 3, 1, 16, 96)])
def test_weight_gradient_launch_width_follows_the_schedule_and_not_the_result(cin, cout, k, B, H, W):
    """MTE_OPT_WGRAD_SHARES_CHIP (round 5): beside the data-gradient chain the MFMA weight-gradient kernels aim for half a chip of workgroups, alone for one per
    CU.  The width only changes how many pixel splits there are: the gradients must agree to fp32 summation order, and each setting must reproduce itself bit
    for bit (plain stores + fixed-order part sums: no atomics)."""
    from mindtheedge_amd import kernels as K
    K.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(cin + cout + k + W)
    x = K.image_to_act((torch.rand(B, cin, H, W, generator=g) * 2 - 1).cuda())
    dy = K.image_to_act((torch.rand(B, cout, H, W, generator=g) * 2 - 1).cuda())
    w = torch.zeros(cout, cin, k, k, device="cuda")
    out = {}
    try:
        for shared in (True, False, True, False):
            K.use_wgrad_side_stream(shared)
            dw, _ = K._conv_wgrad(x, dy, w, False, None, None)
            torch.cuda.synchronize()
            if shared in out:
                assert torch.equal(out[shared], dw.cpu())
            out[shared] = dw.cpu()
    finally:
        K.use_wgrad_side_stream(True)
    ref = torch.nn.grad.conv2d_weight(x.float().double().contiguous(), (cout, cin, k, k), dy.float().double().contiguous(), padding=k // 2).cpu()
    scale = float(ref.abs().max())
    for shared in (True, False):
        assert float((out[shared].double() - ref).abs().max()) < 2e-5 * scale


# The smallest shapes that still reach more than one pixel split, and the form plan_wgrad (csrc/wgrad_plan.hpp) gives each -- tests/wgrad_launch_table.json has
# these lines, recorded on the CPU.  `most`: the pixel splits the shape gets where the stage has room (slab-writing families), 0 = the register-staged family.
WGRAD_STAGE_SHAPES = [  # cin, cout, k, dtype, B, H, W, most
    (128, 128, 3, "bf16", 1, 24, 32, 2),       # nine-tap (conv_wgrad9_kernel<1>), 24 K-steps: two splits of 12 where the cap allows
    (64, 64, 5, "bf16", 1, 48, 32, 3),         # LDS-DMA 64 x 128 tile (conv_wgrad_dma_kernel<2, 2, 1, 2, true>), 48 pixel blocks: up to three splits of 16
    (256, 256, 1, "bf16", 1, 48, 32, 3),       # LDS-DMA 16-wave 256 x 256 tile (conv_wgrad_dma_kernel<4, 4, 2, 2, true>): up to three splits
    (32, 32, 3, "bf16", 1, 48, 32, 0),         # register-staged (conv_wgrad_kernel<bf16, 1, 4, 1, 1, true>): clears slab 0 itself and adds three splits into it
    (64, 64, 3, "fp32", 1, 48, 32, 0),         # register-staged (conv_wgrad_kernel<float, 2, 2, 1, 2, true>): the same
]


@pytest.mark.parametrize("stage_parts", [1, 2, 3])
@pytest.mark.parametrize("shape", WGRAD_STAGE_SHAPES)
def test_weight_gradient_writes_no_slab_beyond_its_stage(shape, stage_parts):
    """mte_conv2d_wgrad through the C interface with a stage of `stage_parts` slabs: it reports 1 .. stage_parts slabs, leaves everything behind them alone (a
    NaN-filled slab more than it was given, and the unused ones), the slabs it reports add up to the fp64 weight gradient of the same rounded operands, and the
    slab-writing families (plain stores) reproduce themselves bit for bit.  The register-staged family ignores the cap: one slab, cleared by the launch itself."""
    import ctypes
    from mindtheedge_amd import kernels as K
    cin, cout, k, dtype, B, H, W, most = shape
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(cin + 7 * cout + k + stage_parts)
    xf = (torch.rand(B, cin, H, W, generator=g) * 2 - 1).bfloat16().float()
    gf = (torch.rand(B, cout, H, W, generator=g) * 2 - 1).bfloat16().float()
    x, dy = K.as_act(xf.cuda(), tdt), K.as_act(gf.cuda(), tdt)
    (xp, ldx), (dyp, lddy) = K._pl(x), K._pl(dy)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        stage = torch.full((stage_parts + 1, cout, k * k, cin), float("nan"), dtype=torch.float32, device="cuda")
        parts = ctypes.c_int(-1)
        # (the binding raises MteError, naming the code, on any return but MTE_OK)
        assert K.lib.mte_conv2d_wgrad(xp, ldx, dyp, lddy, stage.data_ptr(), stage_parts, ctypes.byref(parts), B, H, W, cin, cout, k, k, K._dt(x), st) is None
        torch.cuda.synchronize()
        return stage.cpu(), parts.value

    stage, parts = run()
    assert 1 <= parts <= stage_parts
    assert parts == (min(stage_parts, most) if most else 1)
    assert bool(torch.isnan(stage[parts:]).all())
    dw = stage[:parts].double().sum(0).reshape(cout, k, k, cin).permute(0, 3, 1, 2)             # [N][tap][Cin_p] -> OIHW
    ref = torch.nn.grad.conv2d_weight(xf.double(), (cout, cin, k, k), gf.double(), padding=k // 2)
    assert float((dw - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    if most:
        again, parts2 = run()
        assert parts2 == parts and torch.equal(again[:parts], stage[:parts])


@pytest.mark.parametrize("C,cout,k,B,H2,W2", [(32, 32, 7, 2, 24, 64), (32, 32, 7, 1, 13, 40), (64, 64, 5, 2, 16, 48), (8, 32, 3, 1, 9, 33), (64, 40, 5, 1, 8, 24)])
def test_unshuffled_data_gradient_equals_igemm_then_pixel_shuffle(C, cout, k, B, H2, W2):
    """round 6: mte_conv2d_igemm_unshuffle writes the folded pack layer's data gradient straight into the un-shuffled tensor; bit-identical to the two launches it
    replaces (mte_conv2d_igemm into a packed [B, 4C, H/2, W/2] gradient, then mte_pixel_shuffle), with and without accumulation into the destination"""
    from mindtheedge_amd import kernels as K
    K.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(C + cout + k)
    coutp = K.round8(cout)
    dy = K.image_to_act((torch.rand(B, coutp, H2, W2, generator=g) * 2 - 1).cuda())
    Wf = ((torch.rand(cout, 4 * C, k, k, generator=g) - 0.5) * 0.2).cuda()
    pack = K.WeightPack()
    _, wb = pack.get(Wf, dy.dtype, True)
    dyp, lddy = K._pl(dy)
    for accumulate in (0, 1):
        base = K.image_to_act((torch.rand(B, C, 2 * H2, 2 * W2, generator=g) * 2 - 1).cuda())
        # reference: packed gradient, then the shuffle (accumulating: shuffle into a scratch tensor and add in fp32 with one rounding, as the epilogue does)
        dP = K.new_act(B, 4 * C, H2, W2)
        pp, ldp = K._pl(dP)
        K.lib.mte_conv2d_igemm(dyp, lddy, wb.data_ptr(), 0, pp, ldp, 0, B, H2, W2, coutp, 4 * C, k, k, K._dt(dy), 0, 0, 0, K._stream())
        ref = K.new_act(B, C, 2 * H2, 2 * W2)
        rp, ldr = K._pl(ref)
        K.lib.mte_pixel_shuffle(pp, ldp, rp, ldr, B, 2 * H2, 2 * W2, C, 1, K._dt(dy), K._stream())
        want = ref.float()
        if accumulate:
            want = (want + base.float()).to(torch.bfloat16).float()
        got = base.clone() if accumulate else K.new_act(B, C, 2 * H2, 2 * W2).fill_(7.0)
        got = K.as_act(got, torch.bfloat16)
        gp, ldg = K._pl(got)
        from mindtheedge_amd import _lib as L
        rc = L.lib.load().mte_conv2d_igemm_unshuffle(dyp, lddy, wb.data_ptr(), gp, ldg, B, H2, W2, coutp, 4 * C, k, k, K._dt(dy), accumulate, K._stream())
        if coutp % 32:
            assert rc == -3, rc                                  # (no LDS-DMA loader: nothing staged in LDS -- the caller keeps the two-launch path)
            return
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert torch.equal(got.float()[:, :C].cpu(), want[:, :C].cpu()), accumulate
