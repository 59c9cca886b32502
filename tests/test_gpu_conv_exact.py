"""GPU (-m gpu): the convolution kernels bit for bit against the fp64 convolution of torch, on integer operands whose fp32 arithmetic is exact in any order
(tests/conv_exact.py: the method, the case tables and the references; tests/test_conv_exact_cpu.py: the preconditions of every case and, with the launch
recorder, the kernel instance every mte_conv2d_igemm case below launches -- this file only has to run them).  torch.equal everywhere but in the last test:
    a. K.ConvFn layers in default dispatch, bf16 and fp32 mode, LDS-patch kernels on and off: y, dx rounded once, dw, db exact;
    b. mte_conv2d_igemm through the C interface, one case per tile form / loader / ring / 8-phase loop: plain, accumulate (TWO roundings: ConvArgs.accum), no bias,
       channel-slice input (NaN neighbours) and output (canaries), split-K into a NaN-filled workspace with a sentinel behind it, fp32 output;
    c. mte_conv2d_patch_fwd, mte_conv2d_stem_fwd, and the GroupNorm records of mte_conv2d_patch_fwd_gn;
    d. weight and bias gradients of every family of csrc/wgrad_plan.hpp and csrc/patch_plan.hpp;
    e. one real-valued case per family against a derived bound (integers cannot show a lost low-order operand bit)."""
import ctypes

import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
NAN = float("nan")
CANARY = 0.40625                         # exact in bf16 and no integer: no expected output equals it, so an element a launch skipped shows as well


@pytest.fixture
def devlib():
    from mindtheedge_amd._lib import dev_library
    with dev_library() as lib:
        yield lib


@pytest.fixture(autouse=True)
def stop_after_a_device_fault():
    """a launch that faulted leaves the context unusable: end the session there instead of running the remaining cases into it"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                  # noqa: BLE001
        pytest.exit("device fault, nothing more is launched: %s" % e, returncode=3)


def _same(got, want, what):
    got = got.detach().cpu().double()
    bad = int((got != want).sum()) if got.shape == want.shape else -1
    assert bad == 0, "%s: %d of %d elements differ from the exact reference" % (what, bad, want.numel())


def _checked(fn, key):
    """the case, after its precondition (before anything is launched): every partial sum stays below 2^24"""
    case = X.cached(fn, key)
    X.cached(_precondition, fn, key)
    return case


def _precondition(fn, key):
    case = X.cached(fn, key)
    if fn is X.layer_case:
        X.assert_exact_in_fp32(*case[:4])
    elif fn is X.wgrad_case:
        X.assert_exact_in_fp32(case[0], case[1], None, case[2])
    elif fn is X.igemm_case:
        X.assert_exact_in_fp32(case[1], case[2], case[3], old=case[4])
    else:
        X.assert_exact_in_fp32(case[0], case[1], case[2], old=case[3])
    return True


# ---- a. layer level, default dispatch
@pytest.mark.parametrize("patch", [True, False], ids=["patch", "generic"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", X.LAYER_SHAPES, ids=str)
def test_layer_is_exact(shape, dtype, patch):
    from mindtheedge_amd import kernels as K
    x, w, b, dy, y, dx, dw, db = _checked(X.layer_case, shape)
    cin = shape[0]
    K.set_compute_dtype(dtype)
    K.use_patch_kernels(patch)
    try:
        wg, bg = w.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)
        xa = K.image_to_act(x.float().cuda()).detach().requires_grad_(True)
        got = K.ConvFn.apply(xa, wg, bg, K.WeightPack())
        got.backward(K.as_act(dy.float().cuda(), DT[dtype]))
        torch.cuda.synchronize()
        _same(got, X.rne(y, DT[dtype]), "y")
        _same(xa.grad[:, :cin], X.rne(dx, DT[dtype]), "dx")
        _same(wg.grad, dw, "dw")
        _same(bg.grad, db, "db")
    finally:
        K.use_patch_kernels(True)
        K.set_compute_dtype("bf16")


# ---- b. mte_conv2d_igemm, one case per instance
def _igemm_variants(c):
    out = []
    if not c["split_only"]:
        out += ["plain", "acc", "nobias", "strided"] + ([] if c["out_f32"] else ["strided_acc"])
    for slabs in c["splits"]:
        out += ["split%d" % slabs, "split%d_acc" % slabs]
    return out


@pytest.mark.parametrize("name,variant", [(c["name"], v) for c in X.IGEMM_CASES for v in _igemm_variants(c)])
def test_igemm_instance_is_exact(devlib, name, variant):
    from mindtheedge_amd import kernels as K
    c, x, w, b, old, y64 = _checked(X.igemm_case, name)
    T = DT[c["dt"]]
    OT = torch.float32 if c["out_f32"] else T                      # ldy counts elements of the output type
    acc, strided, slabs = variant.endswith("acc"), variant.startswith("strided"), int(variant[5]) if variant.startswith("split") else 0
    cin_p, N, k, B, H, W = c["cin_p"], c["n"], c["k"], c["B"], c["H"], c["W"]
    M = B * H * W
    bias = None if variant == "nobias" else b.float().cuda()
    cpb = y64 if bias is None else y64 + b.reshape(1, -1, 1, 1)
    want = X.expected(cpb, OT, old if acc else None)
    xv, _, x_check = X.strided_view(x, cin_p + (X.LDX_EXTRA if strided else 0), X.C0 if strided else 0, NAN, T, "cuda")
    yv, _, y_check = X.strided_view(old if acc else torch.full_like(old, CANARY), N + (X.LDY_EXTRA if strided else 0), X.C0 if strided else 0, CANARY, OT, "cuda")
    wf = X.pack_fwd(w, T).cuda()
    ws = None
    if slabs:                                                      # "the workspace needs no clearing": NaN inside, a sentinel behind what was offered
        ws = torch.full((slabs * M * N + 4096,), NAN, dtype=torch.float32, device="cuda")
        ws[slabs * M * N:] = CANARY
    try:
        for key, value in c["knobs"]:
            devlib.mte_debug_set(key, value)
        devlib.mte_conv2d_igemm(xv.data_ptr(), xv.stride(3), wf.data_ptr(), K._ptr(bias), yv.data_ptr(), yv.stride(3), c["out_f32"], B, H, W, cin_p, N, k, k,
                                K._dt(xv), K._ptr(ws), slabs * M * N, (1 if acc else 0) | (2 if c["solo"] else 0), K._stream())
        torch.cuda.synchronize()
    finally:
        devlib.mte_debug_set(33, 0)                                # every knob back to its default
    _same(yv, want, "%s %s" % (name, variant))
    y_check()
    x_check()
    if slabs:
        assert bool((ws[slabs * M * N:] == CANARY).all()), "written behind workspace_elems"


# ---- c. LDS-patch and stem forward
def _patch_pack(K, w, cin_p, N, k):
    wf = X.pack_fwd(w, torch.bfloat16).cuda()
    n = int(K.lib.mte_conv2d_patch_pack_elems(cin_p, N, k, k))
    wp = torch.empty((n,), dtype=torch.bfloat16, device="cuda")
    K.lib.mte_conv2d_patch_repack(wf.data_ptr(), wp.data_ptr(), cin_p, N, k, k, K._stream())
    return wp


@pytest.mark.parametrize("variant", ["plain", "acc", "nobias", "strided", "strided_acc"])
@pytest.mark.parametrize("shape", X.PATCH_CASES, ids=str)
def test_patch_forward_is_exact(shape, variant):
    from mindtheedge_amd import kernels as K
    x, w, b, old, y64 = _checked(X.patch_case, shape)
    cin_p, N, k, B, H, W = shape
    assert K.lib.mte_conv2d_patch_supported(W, cin_p, N, k, k, K.DT_BF16) == 1
    acc, strided = variant.endswith("acc"), variant.startswith("strided")
    bias = None if variant == "nobias" else b.float().cuda()
    cpb = y64 if bias is None else y64 + b.reshape(1, -1, 1, 1)
    xv, _, x_check = X.strided_view(x, cin_p + (X.LDX_EXTRA if strided else 0), X.C0 if strided else 0, NAN, torch.bfloat16, "cuda")
    yv, _, y_check = X.strided_view(old if acc else torch.full_like(old, CANARY), N + (X.LDY_EXTRA if strided else 0), X.C0 if strided else 0, CANARY,
                                    torch.bfloat16, "cuda")
    wp = _patch_pack(K, w, cin_p, N, k)
    K.lib.mte_conv2d_patch_fwd(xv.data_ptr(), xv.stride(3), wp.data_ptr(), K._ptr(bias), yv.data_ptr(), yv.stride(3), B, H, W, cin_p, N, k, k, 1 if acc else 0,
                               K._stream())
    torch.cuda.synchronize()
    _same(yv, X.expected(cpb, torch.bfloat16, old if acc else None), "%s %s" % (shape, variant))
    y_check()
    x_check()


@pytest.mark.parametrize("variant", ["plain", "nobias", "strided"])
@pytest.mark.parametrize("shape", X.STEM_CASES, ids=str)
def test_stem_forward_is_exact(shape, variant):
    from mindtheedge_amd import kernels as K
    x, w, b, old, y64 = _checked(X.patch_case, shape)
    cin_p, N, k, B, H, W = shape
    assert cin_p == 8 and K.lib.mte_conv2d_stem_supported(W, cin_p, N, k, k, K.DT_BF16) == 1
    strided = variant == "strided"
    bias = None if variant == "nobias" else b.float().cuda()
    cpb = y64 if bias is None else y64 + b.reshape(1, -1, 1, 1)
    xv, _, x_check = X.strided_view(x, 8 + (X.LDX_EXTRA if strided else 0), X.C0 if strided else 0, NAN, torch.bfloat16, "cuda")
    yv, _, y_check = X.strided_view(torch.full_like(old, CANARY), N + (X.LDY_EXTRA if strided else 0), X.C0 if strided else 0, CANARY, torch.bfloat16, "cuda")
    wf = X.pack_fwd(w, torch.bfloat16).cuda()                      # (the generic forward pack [N][taps][8])
    K.lib.mte_conv2d_stem_fwd(xv.data_ptr(), xv.stride(3), wf.data_ptr(), K._ptr(bias), yv.data_ptr(), yv.stride(3), B, H, W, N, k, k, K._stream())
    torch.cuda.synchronize()
    _same(yv, X.expected(cpb, torch.bfloat16), "%s %s" % (shape, variant))
    y_check()
    x_check()


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "acc"])
@pytest.mark.parametrize("shape", X.GN_CASES, ids=str)
def test_patch_forward_groupnorm_records_are_exact(shape, acc):
    """mte_conv2d_patch_fwd_gn stores the y of mte_conv2d_patch_fwd, and its per-tile records add up to the fp64 sums of the stored values -- exactly: the values
    are integers and a tile's fp32 sums stay below 2^24 (X.gn_sums asserts it)"""
    from mindtheedge_amd import kernels as K
    x, w, b, old, y64 = _checked(X.gn_case, shape)
    cin_p, N, k, B, H, W = shape
    want = X.expected(y64 + b.reshape(1, -1, 1, 1), torch.bfloat16, old if acc else None)
    sums = X.gn_sums(want)
    xv, _, _ = X.strided_view(x, cin_p, 0, NAN, torch.bfloat16, "cuda")
    wp = _patch_pack(K, w, cin_p, N, k)
    bias = b.float().cuda()
    n = int(K.lib.mte_conv2d_patch_fwd_gn_elems(B, H, W))
    rec = torch.full((n + 4096,), NAN, dtype=torch.float32, device="cuda")
    rec[n:] = CANARY
    tiles = ctypes.c_int(0)
    ys = []
    for gn in (False, True):
        yv, _, y_check = X.strided_view(old if acc else torch.full_like(old, CANARY), N, 0, CANARY, torch.bfloat16, "cuda")
        if gn:
            K.lib.mte_conv2d_patch_fwd_gn(xv.data_ptr(), cin_p, wp.data_ptr(), bias.data_ptr(), yv.data_ptr(), N, B, H, W, cin_p, N, k, k, acc, rec.data_ptr(), n,
                                          ctypes.byref(tiles), K._stream())
        else:
            K.lib.mte_conv2d_patch_fwd(xv.data_ptr(), cin_p, wp.data_ptr(), bias.data_ptr(), yv.data_ptr(), N, B, H, W, cin_p, N, k, k, acc, K._stream())
        torch.cuda.synchronize()
        y_check()
        ys.append(yv.cpu())
    assert torch.equal(ys[0], ys[1])
    _same(ys[1], want, "y")
    assert 0 < B * tiles.value * 32 <= n and bool((rec[n:] == CANARY).all())
    got = rec[:B * tiles.value * 32].cpu().double().reshape(B, tiles.value, 16, 2).sum(1)
    assert torch.equal(got, sums)


# ---- d. weight and bias gradients
@pytest.mark.parametrize("shape", X.WGRAD_CASES, ids=str)
def test_weight_gradient_is_exact(shape):
    from mindtheedge_amd import kernels as K
    cin, cout, k, B, H, W, patch, dtype = shape
    x, w, dy, dw, db = _checked(X.wgrad_case, shape[:6])
    K.set_compute_dtype(dtype)
    K.use_patch_kernels(patch)
    try:
        xa = K.image_to_act(x.float().cuda())
        dya = K.as_act(dy.float().cuda(), DT[dtype])
        gw, gb = K._conv_wgrad(xa, dya, torch.zeros(cout, cin, k, k, device="cuda"), True, None, None)
        torch.cuda.synchronize()
        _same(gw, dw, "dw")
        _same(gb, db, "db")
    finally:
        K.use_patch_kernels(True)
        K.set_compute_dtype("bf16")


# ---- e. real-valued operands, one case per family
@pytest.mark.parametrize("family", sorted(X.REAL_CASES))
def test_real_valued_case_is_within_one_rounding(family):
    """operands uniform in [-1, 1], rounded to bf16; per element |got - r| <= 2^-8 |r| + (1 + 2^-8) K 2^-23 S (X.real_bound: derived, not measured)"""
    from mindtheedge_amd import kernels as K
    cin_p, N, k, B, H, W = X.REAL_CASES[family]
    x, w, b, r, S = X.cached(X.real_case, family)
    xv, _, x_check = X.strided_view(x, cin_p, 0, NAN, torch.bfloat16, "cuda")
    yv, _, y_check = X.strided_view(torch.full_like(r, CANARY), N, 0, CANARY, torch.bfloat16, "cuda")
    wf = X.pack_fwd(w, torch.bfloat16).cuda()
    bias = b.float().cuda()
    if family == "igemm":
        K.lib.mte_conv2d_igemm(xv.data_ptr(), cin_p, wf.data_ptr(), bias.data_ptr(), yv.data_ptr(), N, 0, B, H, W, cin_p, N, k, k, K.DT_BF16, 0, 0, 0, K._stream())
    elif family == "patch":
        wp = _patch_pack(K, w, cin_p, N, k)
        K.lib.mte_conv2d_patch_fwd(xv.data_ptr(), cin_p, wp.data_ptr(), bias.data_ptr(), yv.data_ptr(), N, B, H, W, cin_p, N, k, k, 0, K._stream())
    else:
        K.lib.mte_conv2d_stem_fwd(xv.data_ptr(), cin_p, wf.data_ptr(), bias.data_ptr(), yv.data_ptr(), N, B, H, W, N, k, k, K._stream())
    torch.cuda.synchronize()
    y_check()
    x_check()
    excess = (yv.cpu().double() - r).abs() - X.real_bound(r, S, cin_p * k * k)
    assert float(excess.max()) <= 0, "%d elements beyond the bound, worst by %g" % (int((excess > 0).sum()), float(excess.max()))
