"""GPU (-m gpu): csrc/pack_border.hip -- the exact border of the folded pack layers from the one-pixel ring.  Each kernel alone against its fp64 reference
(tests/pack_border_ref.py) in both activation types, then the layer against the unfolded formulation on its border pixels and corners.

Bounds.  fp32 mode: 1e-5 of the largest reference value (fp32 sums of at most a few thousand terms).  bf16 mode: integer-valued operands whose results stay
below 2^8 are exact in every format involved, so the kernels must reproduce the fp64 value bit for bit (the convention of tests/test_gpu_conv3d_exact.py);
with bf16-representable random operands a bf16 result lies within one rounding of the fp64 value: |got - ref| <= 2^-8 |ref| (half an ulp, at most) plus the
fp32 accumulation slack of 1e-5 of the largest value."""

import pytest
import torch

import pack_border_ref as R

pytestmark = pytest.mark.gpu

# (C, Co, k, B, H, W) of the un-packed input: D = 4C packed depths, H2 x W2 = H/2 x W/2.  The third case has 16C = 512 channels (many 16-byte chunk
# columns) and W2 + 2 = 34 ring positions (no multiple of a tile)
CASES = [(8, 8, 3, 2, 14, 20), (8, 8, 5, 2, 22, 24), (32, 16, 5, 2, 24, 64)]
DTYPES = ["fp32", "bf16"]


def _lib():
    from mindtheedge_amd import kernels as K
    return K.lib


def _td(dtype):
    return torch.float32 if dtype == "fp32" else torch.bfloat16


def _dt(dtype):
    return 1 if dtype == "fp32" else 0


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _floats(g, dtype, *shape):
    """random values in (-1, 1) that the activation type represents exactly"""
    return (torch.rand(*shape, generator=g) * 2 - 1).to(_td(dtype)).double()


def _dev(t, td):
    return t.to(td).cuda().contiguous()


def _check(got, ref, dtype, exact, out_is_act, what):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = (got - ref).abs()
    top = float(ref.abs().max())
    if exact:
        assert float(diff.max()) == 0.0, (what, float(diff.max()), top)
    elif dtype == "bf16" and out_is_act:
        bad = diff > ref.abs() * 2.0 ** -8 + 1e-5 * top
        assert not bool(bad.any()), (what, float(diff.max()), top)
    else:
        assert float(diff.max()) <= 1e-5 * top, (what, float(diff.max()), top)


def _geom(case):
    C, Co, k, B, H, W = case
    return C, Co, k, B, H // 2, W // 2, 4 * C


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("ints", [True, False])
def test_ring_stencil(case, dtype, ints):
    C, Co, k, B, H2, W2, D = _geom(case)
    L, td, g = _lib(), _td(dtype), _gen(1)
    if ints:      # |U| <= 9 * 3, |dx + dP| <= 3 + 72 * 2, sums of dK3 far below 2^24
        P, K3 = _ints(g, -3, 3, B, H2, W2, D), _ints(g, -1, 1, 4, 3, 3, 3)
        dRr, dRc, dx0 = _ints(g, -2, 2, 2 * B, W2 + 2, 4 * D), _ints(g, -2, 2, 2 * B, H2, 4 * D), _ints(g, -3, 3, B, 2 * H2, 2 * W2, C)
    else:
        P, K3 = _floats(g, dtype, B, H2, W2, D), torch.rand(4, 3, 3, 3, generator=g).double() - 0.5
        dRr, dRc, dx0 = _floats(g, dtype, 2 * B, W2 + 2, 4 * D), _floats(g, dtype, 2 * B, H2, 4 * D), _floats(g, dtype, B, 2 * H2, 2 * W2, C)
        K3 = K3.float().double()
    Pd, K3d = _dev(P, td), _dev(K3, torch.float32)
    Rr, Rc = torch.empty(2 * B, W2 + 2, 4 * D, dtype=td, device="cuda"), torch.empty(2 * B, H2, 4 * D, dtype=td, device="cuda")
    L.mte_pack_ring_fwd(Pd.data_ptr(), D, K3d.data_ptr(), Rr.data_ptr(), Rc.data_ptr(), B, H2, W2, D, _dt(dtype), _st())
    wr, wc = R.ring_fwd(P, K3)
    _check(Rr, wr, dtype, ints, True, "R_rows")
    _check(Rc, wc, dtype, ints, True, "R_cols")
    # data gradient, accumulated into dx
    gr, gc, dx = _dev(dRr, td), _dev(dRc, td), _dev(dx0, td)
    L.mte_pack_ring_bwd_data(gr.data_ptr(), gc.data_ptr(), K3d.data_ptr(), dx.data_ptr(), C, B, H2, W2, D, _dt(dtype), _st())
    add = R.unshuffle(R.ring_bwd_data(dRr, dRc, K3, (B, H2, W2, D)))
    _check(dx, dx0 + add, dtype, ints, True, "dx")
    inner = (dx.double().cpu() - dx0)[:, 2:-2, 2:-2]
    assert float(inner.abs().max()) == 0.0                       # only the two outermost rows / columns of dx are touched
    # conv3d weight gradient, added to dk3
    base = torch.arange(108, dtype=torch.float64) - 50 if ints else torch.zeros(108, dtype=torch.float64)
    dk3 = _dev(base, torch.float32)
    work = torch.empty(int(L.mte_pack_ring_work_elems()), dtype=torch.float32, device="cuda")
    L.mte_pack_ring_bwd_weight(gr.data_ptr(), gc.data_ptr(), Pd.data_ptr(), D, dk3.data_ptr(), work.data_ptr(), B, H2, W2, D, _dt(dtype), _st())
    _check(dk3, base + R.ring_bwd_weight(dRr, dRc, P).flatten(), dtype, ints, False, "dk3")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("ints", [True, False])
def test_ring_weights_and_scatter(case, ints):
    C, Co, k, B, H2, W2, D = _geom(case)
    L, g = _lib(), _gen(2)
    pad, nc, N = k // 2, 2 * (k // 2) + 1, 2 * (k // 2) * Co
    if ints:
        W, b3 = _ints(g, -3, 3, Co, 4 * D, k, k), _ints(g, -2, 2, 4)
        dWr, dWc, dD = _ints(g, -9, 9, N, 4 * D, 1, k), _ints(g, -9, 9, N, 4 * D, k, 1), _ints(g, -9, 9, nc * nc, Co)
    else:
        W, b3 = (torch.rand(Co, 4 * D, k, k, generator=g) - 0.5).double(), (torch.rand(4, generator=g) - 0.5).double()
        dWr, dWc, dD = [(torch.rand(*s, generator=g) - 0.5).double() for s in ((N, 4 * D, 1, k), (N, 4 * D, k, 1), (nc * nc, Co))]
    dD.view(nc, nc, Co)[pad, pad] = 0
    Wd, b3d = _dev(W, torch.float32), _dev(b3, torch.float32)
    Wr, Wc = torch.empty(N, 4 * D, 1, k, device="cuda"), torch.empty(N, 4 * D, k, 1, device="cuda")
    Dt = torch.empty(nc * nc, Co, device="cuda")
    L.mte_pack_border_weights(Wd.data_ptr(), b3d.data_ptr(), Wr.data_ptr(), Wc.data_ptr(), Dt.data_ptr(), Co, D, k, _st())
    rWr, rWc, rDt = R.border_weights(W, b3)
    _check(Wr, rWr, "fp32", True, False, "Wr")
    _check(Wc, rWc, "fp32", True, False, "Wc")
    _check(Dt, rDt, "fp32", ints, False, "Dt")
    # scatter: the class sums arrive as PB_CLASS_SPLITS partial rows per class
    splits = int(L.mte_pack_border_class_sums_elems(Co, k)) // (nc * nc * Co)
    part = torch.zeros(nc * nc, splits, Co, dtype=torch.float64)
    part[:, 0], part[:, splits - 1] = dD - 1, torch.ones_like(dD)
    part.view(nc, nc, splits, Co)[pad, pad] = 0
    dW = torch.empty(Co, 4 * D, k, k, device="cuda")
    base = torch.arange(112, dtype=torch.float64)
    dk3b = _dev(base, torch.float32)
    work = torch.empty(int(L.mte_pack_border_scatter_work_elems(Co, k)), dtype=torch.float32, device="cuda")
    dWrd, dWcd, partd = _dev(dWr, torch.float32), _dev(dWc, torch.float32), _dev(part, torch.float32)
    L.mte_pack_border_scatter(dWrd.data_ptr(), dWcd.data_ptr(), partd.data_ptr(), Wd.data_ptr(), b3d.data_ptr(), dW.data_ptr(), dk3b.data_ptr(),
                              work.data_ptr(), Co, D, k, _st())
    rdW, rdb3 = R.border_scatter(dWr, dWc, dD, W, b3)
    _check(dW, rdW, "fp32", ints, False, "dW")
    want = base.clone()
    want[108:] += rdb3
    _check(dk3b, want, "fp32", ints, False, "dk3b")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("ints", [True, False])
def test_border_apply_and_gather(case, dtype, ints):
    C, Co, k, B, H2, W2, D = _geom(case)
    L, td, g = _lib(), _td(dtype), _gen(3)
    pad, nc, N = k // 2, 2 * (k // 2) + 1, 2 * (k // 2) * Co
    if ints:      # |y + 2 corr + Dt| <= 3 + 3 * 20
        y, cr, cc = _ints(g, -3, 3, B, H2, W2, Co), _ints(g, -20, 20, 2 * B, W2 + 2, N), _ints(g, -20, 20, 2 * B, H2, N)
        Dt, dy = _ints(g, -20, 20, nc * nc, Co), _ints(g, -3, 3, B, H2, W2, Co)
    else:
        y, dy = _floats(g, dtype, B, H2, W2, Co), _floats(g, dtype, B, H2, W2, Co)
        cr, cc, Dt = [(torch.rand(*s, generator=g) - 0.5).double() for s in ((2 * B, W2 + 2, N), (2 * B, H2, N), (nc * nc, Co))]
    Dt.view(nc, nc, Co)[pad, pad] = 0
    yd = _dev(y, td)
    crd, ccd, Dtd = _dev(cr, torch.float32), _dev(cc, torch.float32), _dev(Dt, torch.float32)
    L.mte_pack_border_apply(yd.data_ptr(), Co, crd.data_ptr(), ccd.data_ptr(), Dtd.data_ptr(), B, H2, W2, Co, k, _dt(dtype), _st())
    _check(yd, R.border_apply(y, cr, cc, Dt, k), dtype, ints, True, "y")
    assert torch.equal(yd[:, pad:H2 - pad, pad:W2 - pad].double().cpu(), y[:, pad:H2 - pad, pad:W2 - pad])          # the interior is not touched
    # gather (a copy: exact in either type) and the class sums
    dyd = _dev(dy, td)
    Gr = torch.full((2 * B, W2 + 2, N), 7.0, dtype=td, device="cuda")
    Gc = torch.full((2 * B, H2, N), 7.0, dtype=td, device="cuda")
    L.mte_pack_border_gather(dyd.data_ptr(), Co, Gr.data_ptr(), Gc.data_ptr(), B, H2, W2, Co, k, _dt(dtype), _st())
    rGr, rGc, rdD = R.border_gather(dy, k)
    _check(Gr, rGr, dtype, True, True, "G_rows")
    _check(Gc, rGc, dtype, True, True, "G_cols")
    n = int(L.mte_pack_border_class_sums_elems(Co, k))
    part = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    L.mte_pack_border_class_sums(dyd.data_ptr(), Co, part.data_ptr(), B, H2, W2, Co, k, _dt(dtype), _st())
    _check(part.view(nc * nc, -1, Co).double().sum(1), rdD, dtype, ints, False, "dD")


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------------------
LAYER_FP32 = [(16, 5, 2, 28, 36), (32, 3, 1, 16, 24), (32, 5, 1, 24, 64), (64, 3, 2, 14, 20)]          # the shapes of tests/test_gpu_pack_fold.py
LAYER_BF16 = [(32, 5, 1, 24, 64), (64, 3, 2, 14, 20)]
_layer_runs = {}


def _layer(C, k, B, H, W, fold, dtype):
    """one forward + backward of tests/test_gpu_pack_fold.py's layer run (shared by the tests below, never modified)"""
    key = (C, k, B, H, W, fold, dtype)
    if key not in _layer_runs:
        import test_gpu_pack_fold as TPF
        _layer_runs[key] = TPF._run(C, k, B, H, W, fold, dtype)[0]
    return _layer_runs[key]


def _regions(t, band):
    """the border pixels (within `band` of an edge) and the four band x band corners of an NCHW tensor, as flat selections"""
    H, W = t.shape[2], t.shape[3]
    m = torch.zeros(H, W, dtype=torch.bool)
    m[:band], m[H - band:], m[:, :band], m[:, W - band:] = True, True, True, True
    out = {"border": t[:, :, m]}
    for name, (ys, xs) in {"tl": (slice(0, band), slice(0, band)), "tr": (slice(0, band), slice(W - band, W)),
                           "bl": (slice(H - band, H), slice(0, band)), "br": (slice(H - band, H), slice(W - band, W))}.items():
        out["corner " + name] = t[:, :, ys, xs]
    return out


def _compare_layer(C, k, B, H, W, dtype, rel, absolute):
    from conftest import rel_err
    a, r = _layer(C, k, B, H, W, True, dtype), _layer(C, k, B, H, W, False, "fp32")
    pad = k // 2
    for key in r:
        err = rel_err(a[key], r[key])
        print("%s %s: rel %.3e" % (dtype, key, err))
        assert err < rel or float((a[key] - r[key]).abs().max()) < absolute, (key, err)
    # a failure at the border must not hide in a whole-tensor norm: y within pad of an edge, dx within the 2 (pad + 1) input pixels under the ring's reach
    for key, band in (("y", pad), ("dx", 2 * (pad + 1))):
        ra, rr = _regions(a[key], band), _regions(r[key], band)
        for name in rr:
            err = rel_err(ra[name], rr[name])
            print("%s %s %s: rel %.3e" % (dtype, key, name, err))
            assert err < rel or float((ra[name] - rr[name]).abs().max()) < absolute, (key, name, err)


@pytest.mark.parametrize("C,k,B,H,W", LAYER_FP32)
def test_layer_border_equals_unfolded_fp32(C, k, B, H, W):
    _compare_layer(C, k, B, H, W, "fp32", 3e-4, 1e-4)


@pytest.mark.parametrize("C,k,B,H,W", LAYER_BF16)
def test_layer_border_equals_unfolded_bf16(C, k, B, H, W):
    _compare_layer(C, k, B, H, W, "bf16", 6e-2, 1e-1)


@pytest.mark.parametrize("C,k,B,H,W", LAYER_BF16)
def test_layer_is_bit_reproducible(C, k, B, H, W):
    """Two calls give bit-identical y, dx and dW -- from the same dy.  The layer's dy comes out of the GroupNorm backward, whose channel sums are float
    atomics (csrc/norm_act.hip, gn_elu_bwd_reduce_kernel; older than the folded layers and not part of them): measured over 8 repeats of the 64-channel case,
    3 had ONE element of dy off by 1.2e-7, after which 1885 elements of the ring weight gradient differed by 1.2e-7 and 3461 of dW by up to 1.9e-6, while with
    equal dy every intermediate (ring lines, gathered gradient, both weight-gradient GEMMs) and every output was bit-identical.  So the second call takes the
    first call's dy behind the GroupNorm backward; everything of the folded layer itself -- forward, border kernels, GEMMs, scatter, unfold -- runs twice."""
    from mindtheedge_amd import kernels as K
    import test_gpu_pack_fold as TPF
    orig, kept = K._gn_backward, []

    def first(*a, **kw):
        r = orig(*a, **kw)
        kept.append(r[0].clone())
        return r

    def second(*a, **kw):
        r = orig(*a, **kw)
        assert r[0].shape == kept[0].shape and float((r[0].float() - kept[0].float()).abs().max()) < 1e-5      # the same gradient up to the atomics' order
        r[0].copy_(kept[0])
        return r

    try:
        K._gn_backward = first
        a = TPF._run(C, k, B, H, W, True, "bf16")[0]
        K._gn_backward = second
        b = TPF._run(C, k, B, H, W, True, "bf16")[0]
    finally:
        K._gn_backward = orig
    assert len(kept) == 1
    for key in ("y", "dx", "g.conv.conv_base.weight"):
        assert torch.equal(a[key], b[key]), key
