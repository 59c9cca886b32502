"""GPU (-m gpu): csrc/pack_border_gemm.hip -- the forward ring terms of a folded pack layer as one grouped split-K launch (mte_pack_border_gemm_fwd) and the
apply that adds its slabs (mte_pack_border_apply_slabs), against the fp64 references of tests/pack_border_ref.py and against the two mte_conv2d_igemm launches
they replace.  Conventions of tests/test_gpu_pack_border.py.

Only the columns (far, j, co) of line-batch (far', b) with far == far' are produced (mte_pack_border_apply reads no others); the tests compare those and require
the rest of the workspace, and a guard band behind it, to keep the value they were filled with.

Bounds.  Integer operands in [-2, 2]: every product is at most 4 and K <= 2560, so every partial sum and every total is an integer below 2^14, exact in fp32
in any order -- the slabs added in order must equal the fp64 reference and the unsplit launches bit for bit.  bf16-representable random operands in (-1, 1):
the fp32 ring terms carry the accumulation slack of the file above, 1e-5 of the largest reference value (fp32 sums of at most a few thousand terms); y after
the apply is a bf16 result, within one rounding of the fp64 value: |got - ref| <= 2^-8 |ref| plus that slack."""

import ctypes
import os

import pytest
import torch

import pack_border_ref as R

pytestmark = pytest.mark.gpu

# (C, Co, k, B, H, W) of the un-packed input: C16 = 16 C channels per ring line, H2 x W2 = H/2 x W/2
CASES = [(8, 8, 3, 1, 8, 12),              # lines shorter than a tile; K = 384 is too short to split: one slice, the workspace is the result
         (8, 8, 5, 3, 22, 24),             # odd B; pad = 2: two distances per edge
         (32, 16, 5, 2, 24, 64),           # 34 ring positions (no tile multiple); K = 2560; splits without being forced
         (24, 24, 3, 2, 20, 260)]          # M over one tile with a ragged last tile; pad * Co = 24 (no multiple of 32); 36 K-steps in 5 slices
FORCED = [0, 2, 5]                         # slices asked of the plan (0: its own choice); tiny shapes would otherwise not split
GUARD = 64


def _K():
    from mindtheedge_amd import kernels as K
    return K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _geom(case):
    C, Co, k, B, H, W = case
    return C, Co, k, B, H // 2, W // 2, 16 * C, k // 2, 2 * (k // 2) * Co


_inputs = {}


def _problem(case, ints):
    """operands (fp64, exactly representable in bf16), their device copies and the fp64 ring terms -- made once per (case, kind), never modified"""
    key = (case, ints)
    if key not in _inputs:
        C, Co, k, B, H2, W2, C16, pad, N = _geom(case)
        g = torch.Generator().manual_seed(11 + 7 * len(_inputs))
        if ints:
            mk = lambda *s: torch.randint(-2, 3, s, generator=g).double()
        else:
            mk = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(torch.bfloat16).double()
        Rr, Rc, Wr, Wc = mk(2 * B, W2 + 2, C16), mk(2 * B, H2, C16), mk(N, C16, 1, k), mk(N, C16, k, 1)
        cr, cc = R.ring_gemms(Rr, Rc, Wr, Wc)
        bf = lambda t: t.to(torch.bfloat16).cuda().contiguous()
        dev = {"Rr": bf(Rr), "Rc": bf(Rc),
               "wr": bf(Wr[:, :, 0, :].permute(0, 2, 1)), "wc": bf(Wc[:, :, :, 0].permute(0, 2, 1))}           # forward packs [N][k][C16]
        _inputs[key] = (dev, cr, cc)
    return _inputs[key]


def _own(t, B, pad, Co):
    """the far == far' columns of ring terms [..., 2B, n, N] as [..., 2, B, n, pad * Co]"""
    Ng = pad * Co
    v = t.reshape(t.shape[:-3] + (2, B) + t.shape[-2:])
    return torch.stack([v[..., 0, :, :, :Ng], v[..., 1, :, :, Ng:]], dim=-4)


def _cross(t, B, pad, Co):
    Ng = pad * Co
    v = t.reshape(t.shape[:-3] + (2, B) + t.shape[-2:])
    return torch.stack([v[..., 0, :, :, Ng:], v[..., 1, :, :, :Ng]], dim=-4)


def _launch(case, dev, force, fill=7.0):
    """-> (slabs of the rows [splits, 2B, W2+2, N], slabs of the columns [splits, 2B, H2, N], the whole workspace with its guard band, splits)"""
    C, Co, k, B, H2, W2, C16, pad, N = _geom(case)
    L = _K().lib
    splits = ctypes.c_int(0)
    n = int(L.mte_pack_border_gemm_ws_elems(B, H2, W2, C16, Co, k, 0, force, ctypes.byref(splits)))
    s = splits.value
    assert n == s * 2 * B * (W2 + 2 + H2) * N and s >= 1
    ws = torch.full((n + GUARD,), fill, dtype=torch.float32, device="cuda")
    L.mte_pack_border_gemm_fwd(dev["Rr"].data_ptr(), dev["Rc"].data_ptr(), dev["wr"].data_ptr(), dev["wc"].data_ptr(), ws.data_ptr(), n,
                               B, H2, W2, C16, Co, k, 0, force, _st())
    nr = s * 2 * B * (W2 + 2) * N
    return ws[:nr].view(s, 2 * B, W2 + 2, N), ws[nr:n].view(s, 2 * B, H2, N), ws, s


def _sum_in_order(slabs):
    acc = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        acc += slabs[s]
    return acc


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("case", CASES)
def test_terms_are_exact_on_integers(case, force):
    C, Co, k, B, H2, W2, C16, pad, N = _geom(case)
    K = _K()
    dev, cr, cc = _problem(case, True)
    sr, sc, ws, s = _launch(case, dev, force)
    if force > 1:
        assert 1 < s <= force                  # (a slice is a whole number of two-K-step stages: 12 K-steps asked for 5 slices give 3)
    if case == CASES[3]:
        assert s == (force or s) and (k * C16 // 32) % 5 != 0
    if case == CASES[0] and force == 0:
        assert s == 1
    if case == CASES[2] and force == 0:
        assert s > 1
    got_r, got_c = _sum_in_order(sr), _sum_in_order(sc)
    for got, ref, what in ((got_r, cr, "rows"), (got_c, cc, "columns")):
        d = (_own(got, B, pad, Co).double().cpu() - _own(ref, B, pad, Co)).abs()
        assert float(d.max()) == 0.0, (what, s, float(d.max()))
    # nothing else is written: the cross blocks of every slab and the guard band keep their fill
    assert bool((_cross(sr, B, pad, Co) == 7.0).all()) and bool((_cross(sc, B, pad, Co) == 7.0).all())
    assert bool((ws[-GUARD:] == 7.0).all())
    # ... and the launches it replaces give the same numbers
    old_r = K._ring_gemm(dev["Rr"].view(2 * B, 1, W2 + 2, C16).permute(0, 3, 1, 2), dev["wr"], N, 1, k, True, K._CONV_SOLO)
    old_c = K._ring_gemm(dev["Rc"].view(2 * B, H2, 1, C16).permute(0, 3, 1, 2), dev["wc"], N, k, 1, True, K._CONV_SOLO)
    assert torch.equal(_own(got_r, B, pad, Co), _own(old_r.view(2 * B, W2 + 2, N), B, pad, Co))
    assert torch.equal(_own(got_c, B, pad, Co), _own(old_c.view(2 * B, H2, N), B, pad, Co))


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("case", CASES)
def test_slabs_and_fused_apply(case, force):
    C, Co, k, B, H2, W2, C16, pad, N = _geom(case)
    L = _K().lib
    dev, cr, cc = _problem(case, False)
    sr, sc, ws, s = _launch(case, dev, force, fill=float("nan"))          # an element read that was never written poisons y
    top = max(float(cr.abs().max()), float(cc.abs().max()))
    for slabs, ref, what in ((sr, cr, "rows"), (sc, cc, "columns")):
        d = (_own(slabs.double().sum(0), B, pad, Co).cpu() - _own(ref, B, pad, Co)).abs()
        print("%s %s slices %d: max |terms - fp64| %.3e of %.3e" % (case, what, s, float(d.max()), top))
        assert float(d.max()) <= 1e-5 * top, (what, float(d.max()), top)
    g = torch.Generator().manual_seed(5)
    nc = 2 * pad + 1
    y = (torch.rand(B, H2, W2, Co, generator=g) * 2 - 1).to(torch.bfloat16).double()
    Dt = (torch.rand(nc * nc, Co, generator=g) - 0.5).float().double()
    Dt.view(nc, nc, Co)[pad, pad] = 0
    yd, Dtd = y.to(torch.bfloat16).cuda().contiguous(), Dt.float().cuda()
    L.mte_pack_border_apply_slabs(yd.data_ptr(), Co, ws.data_ptr(), s, Dtd.data_ptr(), B, H2, W2, Co, k, 0, _st())
    ref = R.border_apply(y, cr, cc, Dt, k)
    got = yd.double().cpu()
    diff = (got - ref).abs()
    print("%s slices %d: max |y - fp64| %.3e, largest |y| %.3e" % (case, s, float(diff.max()), float(ref.abs().max())))
    bad = diff > ref.abs() * 2.0 ** -8 + 1e-5 * float(ref.abs().max())
    assert not bool(bad.any()), (float(diff.max()), float(ref.abs().max()))
    assert torch.equal(got[:, pad:H2 - pad, pad:W2 - pad], y[:, pad:H2 - pad, pad:W2 - pad])                 # the interior is not touched
    # the same y from the summed terms through mte_pack_border_apply: the fused sum adds the slabs in the same order
    y2 = y.to(torch.bfloat16).cuda().contiguous()
    tr, tc = _sum_in_order(sr).contiguous(), _sum_in_order(sc).contiguous()
    tr[torch.isnan(tr)] = 0
    tc[torch.isnan(tc)] = 0
    L.mte_pack_border_apply(y2.data_ptr(), Co, tr.data_ptr(), tc.data_ptr(), Dtd.data_ptr(), B, H2, W2, Co, k, 0, _st())
    assert torch.equal(yd, y2)


@pytest.mark.parametrize("case", CASES[2:])
def test_repeated_calls_are_bit_equal(case):
    C, Co, k, B, H2, W2, C16, pad, N = _geom(case)
    dev, _, _ = _problem(case, False)
    first = None
    for _ in range(8):
        sr, sc, _, s = _launch(case, dev, 5)
        got = (_own(sr, B, pad, Co).clone(), _own(sc, B, pad, Co).clone())
        if first is None:
            first = got
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def test_unsupported_shapes_are_refused_not_launched():
    L = _K().lib
    from mindtheedge_amd import _lib
    raw = _lib.lib.load()
    splits = ctypes.c_int(0)
    assert int(L.mte_pack_border_gemm_ws_elems(2, 12, 32, 512, 16, 5, 1, 0, ctypes.byref(splits))) == -3          # fp32
    assert int(L.mte_pack_border_gemm_ws_elems(2, 12, 32, 512, 12, 5, 0, 0, ctypes.byref(splits))) == -3          # Co % 8
    t = torch.zeros(64, device="cuda")
    assert raw.mte_pack_border_gemm_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 64, 2, 12, 32, 512, 16, 5, 1, 0, _st()) == -3
    assert raw.mte_pack_border_gemm_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 64, 2, 12, 32, 512, 16, 5, 0, 0, _st()) == -1      # workspace too small


@pytest.mark.parametrize("C,k,B,H,W", [(32, 5, 1, 24, 64), (64, 3, 2, 14, 20)])          # the bf16 layer shapes of tests/test_gpu_pack_border.py
def test_layer_takes_the_grouped_launch(C, k, B, H, W):
    """PackFoldedConvGnEluFn in bf16 runs the grouped launch (its plan is cached as taken), and its output equals the output of the same build on the two
    mte_conv2d_igemm launches up to the last bit of a bf16 rounding.  The two differ only in the fp32 summation order of the ring terms (1e-5 of a term, far
    below half a bf16 ulp), so a border pixel of y moves by at most one bf16 ulp, 2^-8 |y|; GroupNorm divides by the standard deviation of y, which the layer's
    fixture keeps within a factor of a few of max |y|, and the result is rounded to bf16 once more: |dz| <= 2^-6 max |z| with a factor of two to spare.
    Equality with the unfolded formulation, forward and backward, is tests/test_gpu_pack_border.py's (unchanged)."""
    K = _K()
    import test_gpu_pack_fold as TPF
    K._ring_plan.clear()
    a = TPF._run(C, k, B, H, W, True, "bf16")[0]
    key = (B, H // 2, W // 2, 16 * C, C, k, 0)
    assert K._ring_plan.get(key) is not None and K._ring_plan[key][0] > 0
    os.environ["MTE_NO_GROUPED_RING"] = "1"
    try:
        K._ring_plan.clear()
        b = TPF._run(C, k, B, H, W, True, "bf16")[0]
        assert K._ring_plan.get(key, 0) is None
    finally:
        del os.environ["MTE_NO_GROUPED_RING"]
        K._ring_plan.clear()
    d = float((a["y"] - b["y"]).abs().max())
    print("layer %s: max |z grouped - z two launches| %.3e of %.3e" % ((C, k, B, H, W), d, float(b["y"].abs().max())))
    assert d <= 2.0 ** -6 * float(b["y"].abs().max())
