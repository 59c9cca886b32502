"""GPU (-m gpu): the conv3d pack / unpack kernels and the fold helpers bit for bit against torch's fp64 conv3d, on integer operands whose fp32 arithmetic is exact
in any order (tests/conv3d_exact.py: the method, the case table and the references; tests/test_conv3d_exact_cpu.py: the precondition and the discriminating power of
every case and, with the launch recorder, the kernel instance and tile every case below launches -- this file only has to run them).  torch.equal everywhere but
in the last test:
    a. K.Pack3dFn and K.Unpack3dFn in default dispatch, bf16 and fp32 mode: y and dx rounded once, dw3 and db3 exact; the unpack also into a channel slice of a
       wider, canary-filled activation, as the decoder calls it;
    b. the four data entry points through the C interface, one case per instance / C class / tile shape (the P3_ONE_BF16_WEIGHT forms against the reference on
       weights rounded once to bf16: their contract, exact like the rest): plain, and with the input in a channel slice between NaN
       neighbours and the output in a slice of a canary-filled buffer with a guard block behind it; the persistent unpack forward with 8 and 1024 workgroups;
    c. the two weight-gradient entry points, every form, also with more tiles than workgroups: dwb[112] inside a NaN-prefilled buffer between canaries;
    d. mte_fold_pack_weights and mte_unfold_pack_wgrad (accumulate 0 and 1) against the fold reference;
    e. one real-valued case per form family against a derived bound (integers cannot show a lost low-order bit of a real weight).
A case that sets no knob runs on the product library, the others on the development build."""
import contextlib

import pytest
import torch

import conv3d_exact as X

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
NAN = float("nan")
CANARY = 0.40625                         # exact in bf16 and no integer: no expected output equals it, so an element a launch skipped shows as well


@contextlib.contextmanager
def _library(knobs):
    """the library a case runs on: the product's where it sets no knob, else the development build with mte_debug_set(1, .) of each value"""
    from mindtheedge_amd import kernels as K
    if not knobs:
        yield K.lib
        return
    from mindtheedge_amd._lib import dev_library
    with dev_library() as lib:
        try:
            for value in knobs:
                lib.mte_debug_set(1, value)
            yield lib
            torch.cuda.synchronize()
        finally:
            lib.mte_debug_set(33, 0)                               # every knob back to its default


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


def _checked(key):
    """the shape's operands and references, after the precondition (before anything is launched): every partial sum stays below 2^24"""
    X.cached(_precondition, key)
    return X.cached(X.shape_case, *key)


def _precondition(key):
    x, w3, b3, dy = X.cached(X.shape_case, *key)[:4]
    return X.assert_exact_in_fp32(key[0], x, w3, b3, dy)


def _entry(lib, c):
    return getattr(lib, "mte_%s3d_%s" % (c["op"], c["what"]))


def _dwb():
    """dwb[112] in a NaN-prefilled buffer (the entry point clears it itself) with canaries in front of it and behind it -> buffer, dwb, check"""
    buf = torch.full((64 + 112 + 64,), CANARY, dtype=torch.float32, device="cuda")
    buf[64:176] = NAN

    def check():
        assert bool((buf[:64] == CANARY).all()) and bool((buf[176:] == CANARY).all()), "written outside dwb[112]"

    return buf, buf[64:176], check


# ---- a. layer level, default dispatch
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", X.LAYER_SHAPES, ids=str)
def test_layer_is_exact(shape, dtype):
    from mindtheedge_amd import kernels as K
    op, C, B, H, W = shape
    x, w3, b3, dy, y, dx, dw3, db3 = _checked(shape + (3,))
    K.set_compute_dtype(dtype)
    try:
        for sliced in (False, True) if op == "unpack" else (False,):
            wg, bg = w3.float().cuda().requires_grad_(True), b3.float().cuda().requires_grad_(True)
            xa = K.image_to_act(x.float().cuda()).detach().requires_grad_(True)
            if op == "pack":
                got = K.Pack3dFn.apply(xa, wg, bg)
            elif not sliced:
                got = K.Unpack3dFn.apply(xa, wg, bg, None)
            else:                                                  # the decoder's call: the result goes into the first C channels of the concat buffer
                wide = K.new_act(B, C + X.SKIP, 2 * H, 2 * W, DT[dtype])
                wide.fill_(CANARY)
                got = K.Unpack3dFn.apply(xa, wg, bg, K.channel_slice(wide, 0, C))
            got.backward(K.as_act(dy.float().cuda(), DT[dtype]))
            torch.cuda.synchronize()
            _same(got, X.rne(y, DT[dtype]), "y")
            _same(xa.grad, X.rne(dx, DT[dtype]), "dx")
            _same(wg.grad, dw3, "dw3")
            _same(bg.grad, db3, "db3")
            if sliced:
                assert got.data_ptr() == wide.data_ptr() and torch.equal(wide[:, :C], got)
                skip = wide[:, C:].cpu()
                assert torch.equal(skip, torch.full_like(skip, CANARY)), "the skip channels behind the unpack layer's own were written"
    finally:
        K.set_compute_dtype("bf16")


# ---- b. the four data entry points, one case per instance, C class and tile shape
@pytest.mark.parametrize("variant", ["plain", "strided"])
@pytest.mark.parametrize("name", [c["name"] for c in X.CASES if c["what"] != "bwd_weight"])
def test_data_entry_point_is_exact(name, variant):
    from mindtheedge_amd import kernels as K
    c = X.case_named(name)
    x, w3, b3, dy = _checked(X.case_key(c))[:4]
    y, dx = X.expected_y_dx(c)                                     # (the one-bf16-weight forms: under their contract, the reference on rne(w3))
    T = DT[c["dt"]]
    strided = variant == "strided"
    ldx, ldo = X.strides(c, strided)
    c0 = X.C0 if strided else 0
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    w, b = w3.float().cuda().contiguous(), b3.float().cuda()
    if c["what"] == "fwd":
        src, _, src_check = X.strided_view(x, ldx, c0, NAN, T, "cuda")
        dst, _, dst_check = X.strided_view(torch.full_like(y, CANARY), ldo, c0, CANARY, T, "cuda")
        want = y
    else:
        src, _, src_check = X.strided_view(dy, ldo, c0, NAN, T, "cuda")
        dst, _, dst_check = X.strided_view(torch.full_like(x, CANARY), ldx, c0, CANARY, T, "cuda")
        want = dx
    with _library(c["knobs"]) as lib:
        if c["what"] == "fwd":
            _entry(lib, c)(src.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), dst.data_ptr(), ldo, B, H, W, C, K._dt(src), K._stream())
        else:
            _entry(lib, c)(src.data_ptr(), ldo, w.data_ptr(), dst.data_ptr(), ldx, B, H, W, C, K._dt(src), K._stream())
        torch.cuda.synchronize()
    _same(dst, X.rne(want, T), "%s %s" % (name, variant))
    dst_check()
    src_check()


# ---- c. the two weight-gradient entry points
@pytest.mark.parametrize("name,variant", [(c["name"], v) for c in X.CASES if c["what"] == "bwd_weight" for v in (("plain",) if c["big"] else ("plain", "strided"))])
def test_weight_gradient_entry_point_is_exact(name, variant):
    from mindtheedge_amd import kernels as K
    c = X.case_named(name)
    x, w3, b3, dy, _, _, dw3, db3 = _checked(X.case_key(c))
    T = DT[c["dt"]]
    strided = variant == "strided"
    ldx, ldo = X.strides(c, strided)
    c0 = X.C0 if strided else 0
    xv, _, x_check = X.strided_view(x, ldx, c0, NAN, T, "cuda")
    dv, _, d_check = X.strided_view(dy, ldo, c0, NAN, T, "cuda")
    buf, dwb, dwb_check = _dwb()
    with _library(c["knobs"]) as lib:
        _entry(lib, c)(xv.data_ptr(), ldx, dv.data_ptr(), ldo, dwb.data_ptr(), c["B"], c["H"], c["W"], c["C"], K._dt(xv), K._stream())
        torch.cuda.synchronize()
    _same(dwb, torch.cat([dw3.reshape(108), db3]), "%s %s" % (name, variant))
    dwb_check()
    x_check()
    d_check()


# ---- d. the fold helpers
def _guarded(t, fill=None):
    """t (or `fill` in its shape) as fp32 on the device, with a canary block behind it -> tensor, check"""
    n = t.numel()
    buf = torch.full((n + 1024,), CANARY, dtype=torch.float32, device="cuda")
    if fill is None:
        buf[:n] = t.reshape(-1).float().cuda()
    else:
        buf[:n] = fill

    def check():
        assert bool((buf[n:] == CANARY).all()), "written behind the buffer"

    return buf[:n].view(t.shape), check


@pytest.mark.parametrize("shape", X.FOLD_CASES, ids=str)
def test_fold_pack_weights_is_exact(shape):
    from mindtheedge_amd import kernels as K
    Co, D, k = shape
    X.cached(X.fold_precondition, *shape)
    (W, K3, b, b3, _, _, _, _), Wf, bf, _, _ = X.cached(X.fold_case, *shape)
    ins = [t.float().cuda().contiguous() for t in (W, K3, b, b3)]
    gWf, wf_check = _guarded(Wf, NAN)
    gbf, bf_check = _guarded(bf, NAN)
    K.lib.mte_fold_pack_weights(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), gWf.data_ptr(), gbf.data_ptr(), Co, D, k, K._stream())
    torch.cuda.synchronize()
    _same(gWf, Wf, "W'")
    _same(gbf, bf, "b'")
    wf_check()
    bf_check()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", X.FOLD_CASES, ids=str)
def test_unfold_pack_wgrad_is_exact(shape, accumulate):
    """dW is overwritten, or added to what the buffer held (accumulate = 1); dk3b[112] = (dK3, db3) is added to in both"""
    from mindtheedge_amd import kernels as K
    Co, D, k = shape
    X.cached(X.fold_precondition, *shape)
    (W, K3, b, b3, dWf, dbf, oldW, old3), _, _, dW, dk3b = X.cached(X.fold_case, *shape)
    ins = [t.float().cuda().contiguous() for t in (dWf, dbf, W, K3, b3)]
    gdW, dw_check = _guarded(oldW) if accumulate else _guarded(oldW, NAN)
    g3, d3_check = _guarded(old3)
    K.lib.mte_unfold_pack_wgrad(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), gdW.data_ptr(), g3.data_ptr(),
                                Co, D, k, accumulate, K._stream())
    torch.cuda.synchronize()
    _same(gdW, dW + oldW if accumulate else dW, "dW")
    _same(g3, dk3b + old3, "dk3b")
    dw_check()
    d3_check()


# ---- e. real-valued operands, one case per form family
@pytest.mark.parametrize("family", sorted(X.REAL_CASES))
def test_real_valued_case_is_within_one_rounding(family):
    """x and dy uniform in [-1, 1] rounded to bf16, w3 and b3 uniform in [-1, 1] in fp32.  Per element
        |got - r| <= 2^-8 |r| + (1 + 2^-8) (A 2^-23 + e) S
    with r the fp64 result and S the same operation over magnitudes.  Derived, not measured.  The stored value is one bf16 rounding (to within 2^-8 relative) of
    an fp32 sum s, so |got - r| <= 2^-8 |s| + |s - r| <= 2^-8 |r| + (1 + 2^-8) |s - r|.  s is off from the exact sum over the weights w^ the form multiplies
    with by at most one fp32 ulp of the running magnitude per addition -- A of them, in any order, also with an accumulator that truncates: A 2^-23 S^, S^ the
    operation over the magnitudes the form adds -- and that sum is off from r by at most E, the operation over |x| and |w - w^|.  A = 27 for a forward on fp32
    weights (27 taps onto the bias), 4 x 27 for a data gradient (its sum has 108 terms), twice that for a hi + lo form, which adds the lo products separately.
    e = 0 for the fp32-VALU and gather forms, 2^-18 for hi + lo, 2^-9 for the P3_ONE_BF16_WEIGHT forms.  These e are no worst cases of a single weight's
    rounding (2^-16 and 2^-8); they hold over sums of 27 or 108 weights, and X.real_precondition proves A 2^-23 S^ + E <= (A 2^-23 + e) S from the operands of
    the case before it is launched (and tests/test_conv3d_exact_cpu.py without a GPU).  For the forwards the coefficient is at or below
    27 2^-23 + {0, 2^-17, 2^-9}."""
    from mindtheedge_amd import kernels as K
    _, additions, e_w = X.REAL_CASES[family]
    X.cached(X.real_precondition, family)
    c, x, w3, b3, dy, r, S = X.cached(X.real_case, family)
    ldx, ldo = X.strides(c, False)
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    w, b = w3.float().cuda().contiguous(), b3.float().cuda()
    src, _, src_check = X.strided_view(x if c["what"] == "fwd" else dy, ldx if c["what"] == "fwd" else ldo, 0, NAN, torch.bfloat16, "cuda")
    dst, _, dst_check = X.strided_view(torch.full_like(r, CANARY), ldo if c["what"] == "fwd" else ldx, 0, CANARY, torch.bfloat16, "cuda")
    with _library(c["knobs"]) as lib:
        if c["what"] == "fwd":
            _entry(lib, c)(src.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), dst.data_ptr(), ldo, B, H, W, C, K.DT_BF16, K._stream())
        else:
            _entry(lib, c)(src.data_ptr(), ldo, w.data_ptr(), dst.data_ptr(), ldx, B, H, W, C, K.DT_BF16, K._stream())
        torch.cuda.synchronize()
    dst_check()
    src_check()
    excess = (dst.cpu().double() - r).abs() - X.real_bound(r, S, additions, e_w)
    assert float(excess.max()) <= 0, "%d elements beyond the bound, worst by %g" % (int((excess > 0).sum()), float(excess.max()))
