"""The exact method for the conv3d pack / unpack kernels (tests/conv3d_exact.py), checked without a GPU: the torch reference against the 27-tap loop written from
the index formulas of csrc/pack3d.hip, the precondition and the discriminating power of every case tests/test_gpu_conv3d_exact.py runs, the fold reference, and --
with the launch recorder (tests/conv_launch_recorder.py --p3) -- the kernel instance and the tile every case launches.  These are conditions on the INPUTS, not
measurements of the kernels: a case that misses one gets other ranges or another shape, never another bound."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv3d_exact as X
import conv_launch_recorder as R

SMALL = sorted({X.case_key(c) for c in X.CASES if not c["big"]} | {s + (3,) for s in X.LAYER_SHAPES})
EVERY = sorted({X.case_key(c) for c in X.CASES} | {s + (3,) for s in X.LAYER_SHAPES})


def _changed(a, b):
    return float((a != b).double().mean())


@pytest.mark.parametrize("key", SMALL, ids=str)
def test_reference_agrees_with_the_tap_loop_and_the_case_is_discriminating(key):
    op = key[0]
    x, w3, b3, dy, y, dx, dw3, db3 = X.cached(X.shape_case, *key)
    ty, tdx, tdw, tdb = X.taps_reference(op, x, w3, b3, dy)
    assert torch.equal(y, ty) and torch.equal(dx, tdx) and torch.equal(dw3, tdw) and torch.equal(db3, tdb)       # integers: fp64 is exact in any order
    # what a launch stores in bf16 mode, against what each mistake would store: more than a tenth of the elements must differ
    sy, sdx = X.rne(y), X.rne(dx)
    assert _changed(X.truncate_bf16(y), sy) > 0.10 and _changed(X.truncate_bf16(dx), sdx) > 0.10                # truncation in place of rne
    hi = X.hi_lo(w3)[0]
    hy, hdx, _, _ = X.reference(op, x, hi, b3, dy)
    assert _changed(X.rne(hy), sy) > 0.10 and _changed(X.rne(hdx), sdx) > 0.10                                  # the weights' lo parts lost
    assert _changed(X.rne(X.reference(op, x, w3, torch.zeros(4), dy)[0]), sy) > 0.10                            # a dropped bias
    dwb = torch.cat([dw3.reshape(108), db3])
    for flags in (dict(swap=True), dict(dfirst=True)):                                                          # the sub-pixel bits swapped; channel order d 4 + f
        my, mdx, mdw, mdb = X.taps_reference(op, x, w3, b3, dy, **flags)
        assert _changed(X.rne(my), sy) > 0.10 and _changed(X.rne(mdx), sdx) > 0.10, flags
        assert _changed(torch.cat([mdw.reshape(108), mdb]), dwb) > 0.10, flags
        assert torch.equal(X.mistaken_dwb(op, x, w3, b3, dy, **flags), torch.cat([mdw.reshape(108), mdb]))       # (what the large cases are checked with, below)


@pytest.mark.parametrize("key", sorted({X.case_key(c) for c in X.CASES if c["big"]}), ids=str)
def test_large_weight_gradient_cases_are_discriminating(key):
    """the cases beyond a grid cap store dwb[112] in fp32: nothing is rounded and the weights do not enter, so the two layout mistakes are what they can show"""
    x, w3, b3, dy, _, _, dw3, db3 = X.cached(X.shape_case, *key)
    dwb = torch.cat([dw3.reshape(108), db3])
    for flags in (dict(swap=True), dict(dfirst=True)):
        assert _changed(X.mistaken_dwb(key[0], x, w3, b3, dy, **flags), dwb) > 0.10, flags


@pytest.mark.parametrize("key", EVERY, ids=str)
def test_every_case_passes_the_precondition(key):
    x, w3, b3, dy, y, dx, dw3, db3 = X.cached(X.shape_case, *key)
    worst = X.assert_exact_in_fp32(key[0], x, w3, b3, dy)
    assert worst >= float(dw3.abs().max()) > 0
    assert int((X.hi_lo(w3)[1] != 0).sum()) >= 27                                # a fair share of the weights has a lo part


def test_the_table_covers_what_it_must():
    C = X.CASES
    assert {c["C"] for c in C} == {8, 16, 32, 64, 128, 256, 512}
    for op in ("pack", "unpack"):
        for what in ("fwd", "bwd_data", "bwd_weight"):
            mine = [c for c in C if c["op"] == op and c["what"] == what]
            n = 2 if op == "pack" else 1
            assert any(c["H"] == c["W"] == n for c in mine) and any(c["H"] == c["W"] == 2 * n and c["B"] > 1 for c in mine), (op, what)
    assert any(c["op"] == "pack" and c["what"] == "fwd" and c["C"] == 512 and c["kernel"] == "pack3d_fwd_tr_kernel<2, 4>" for c in C)      # 16 depth slabs
    assert sorted({c["kernel"] for c in C if c["big"]}) == ["conv3d_bwd_weight_mfma_kernel<false>", "conv3d_bwd_weight_mfma_kernel<true>",
                                                             "pack3d_bwd_weight_kernel<float, 4>", "pack3d_bwd_weight_lds_kernel",
                                                             "unpack3d_bwd_weight_kernel<bf16>", "unpack3d_bwd_weight_lds_kernel"]
    assert all(not c["big"] or c["what"] == "bwd_weight" for c in C)
    # the forms that multiply with ONE bf16 value per weight are checked against the reference on rounded weights: exactly the HILO = false instances
    assert {c["kernel"] for c in C if c["one"]} == {"pack3d_bwd_data_mfma_kernel<false>", "unpack3d_bwd_data_mfma_kernel<32, false>",
                                                    "unpack3d_bwd_data_mfma_kernel<64, false>", "unpack3d_bwd_data_dma32_kernel<4, false>",
                                                    "unpack3d_fwd_mfma_kernel<32, false>", "unpack3d_fwd_mfma_kernel<64, false>"}
    assert all(c["knobs"] and (c["knobs"][0] - 300) & 16 for c in C if c["one"]) and not any(c["one"] for c in C if X.is_product(c))
    for family, (name, additions, e_w) in X.REAL_CASES.items():
        c = X.case_named(name)
        assert c["what"] != "bwd_weight" and additions in ((27, 54) if c["what"] == "fwd" else (108, 216)) and e_w in (0.0, 2.0 ** -18, 2.0 ** -9), family
        if c["what"] == "fwd":                                                   # never above the bound written for the forward's three weight forms
            assert additions * 2.0 ** -23 + e_w <= 27 * 2.0 ** -23 + {0.0: 0.0, 2.0 ** -18: 2.0 ** -17, 2.0 ** -9: 2.0 ** -9}[e_w], family


@pytest.mark.parametrize("family", sorted(X.REAL_CASES))
def test_real_valued_bound_holds_for_the_operands_of_its_case(family):
    """the coefficient of X.real_bound covers the summation error and what the form's weights change, for this case's operands (X.real_precondition); and the
    summation term stays well below the one bf16 rounding of a typical output, so that the bound still tells a wrong weight from a right one"""
    assert X.real_precondition(family) <= 1.0
    _, A, e_w = X.REAL_CASES[family]
    c, x, w3, b3, dy, r, S = X.cached(X.real_case, family)
    assert float((A * 2.0 ** -23 * S).max()) < 2.0 ** -8 * float(r.abs().mean())


# ---- the fold helpers
@pytest.mark.parametrize("shape", X.FOLD_CASES, ids=str)
def test_fold_reference_is_the_two_convolutions_away_from_the_border(shape):
    """conv2d(pad(P), W') + b' == conv2d(pad(conv3d(P)), W) + b at pixels more than k/2 + 1 from the border, exactly (integers in fp64); and the sums of the fold
    and of its transpose stay below 2^24"""
    Co, D, k = shape
    X.fold_precondition(*shape)
    (W, K3, b, b3, gWf, gbf, oldW, old3), Wf, bf, dW, dk3b = X.cached(X.fold_case, *shape)
    assert bool((Wf == Wf.round()).all()) and bool((bf == bf.round()).all())
    m = k // 2 + 1
    n = 2 * m + 3
    P = torch.randint(-3, 4, (2, D, n, n), generator=torch.Generator().manual_seed(k)).double()
    T = F.conv3d(P.unsqueeze(1), K3, b3, padding=1).reshape(2, 4 * D, n, n)
    two = F.conv2d(T, W, b, padding=k // 2)
    one = F.conv2d(P, Wf, bf, padding=m)
    assert torch.equal(one[:, :, m:n - m, m:n - m], two[:, :, m:n - m, m:n - m]) and not torch.equal(one, two)
    # the transpose, restated from the comments of unfold_dw_kernel: dW = sum dW'[co][d + kd - 1][t + (dh, dw)] K3[f][kd][dh][dw] + db'[co] b3[f]
    gp = F.pad(gWf, (0, 0, 0, 0, 1, 1))
    want = torch.zeros_like(W).reshape(Co, 4, D, k, k)
    for f in range(4):
        want[:, f] += gbf.reshape(Co, 1, 1, 1) * b3[f]
        for kd in range(3):
            for dh in range(3):
                for dw in range(3):
                    want[:, f] += gp[:, kd:kd + D, dh:dh + k, dw:dw + k] * K3[f, 0, kd, dh, dw]
    assert torch.equal(want.reshape(W.shape), dW)
    assert float(dk3b.abs().min()) > 0


# ---- which instance and which tile every case launches: the recorder
def _lines(c):
    dt = R.BF16 if c["dt"] == "bf16" else R.F32
    return [R.p3_case("%s_%s" % (c["op"], c["what"]), dt, c["B"], c["H"], c["W"], c["C"], *X.strides(c, strided), knobs=list(c["knobs"]) or None)
            for strided in (False, True)]


def _named_in_the_launch_switch():
    with open(os.path.join(R.CSRC, "pack3d.hip")) as f:
        src = f.read()
    body = src[src.index("int launch_p3plan("):src.index("#ifdef MTE_DEV", src.index("int launch_p3plan("))]
    return [re.sub(r"\bbf16_t\b", "bf16", m) for m in re.findall(r"launch_(?:tiled|gather)<(\w+(?:<[^>]*>)?)>\(pl, a, st\)", body)]


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_every_case_launches_the_instance_it_claims(tmp_path, dev):
    cases = [c for c in X.CASES if dev or X.is_product(c)]
    exe = R.build(str(tmp_path), dev=dev, p3=True)
    rows = [(c, line) for c in cases for line in _lines(c)]
    got = [json.loads(ln) for ln in R.run(exe, [line for _, line in rows])]
    seen = set()
    for (c, line), g in zip(rows, got):
        assert g["rc"] == 0, (c["name"], g)
        launches = list(g["launches"])
        if c["what"] == "bwd_weight":
            assert launches.pop(0) == {"clear": "dwb", "bytes": 448}, (c["name"], g)
        assert len(launches) == 1 and launches[0]["k"] == c["kernel"], (c["name"], line, launches)
        k = launches[0]
        if c["tile"]:                                                          # one row and one column beyond a whole tile
            th, tw = c["tile"]
            h, w = (c["H"] // 2, c["W"] // 2) if c["op"] == "pack" else (c["H"], c["W"])
            assert (k["TH"], k["TW"], k["tiles_h"], k["tiles_w"]) == (th, tw, 2, 2) and (h, w) == (th + 1, tw + 1), (c["name"], k)
        if c["big"]:                                                           # a workgroup walks at least two tiles
            if "ntiles" in k:
                assert k["ntiles"] >= k["grid"] + k["grid"] // 2, (c["name"], k)
            else:                                                              # the gather forms: more items than threads, a thread takes a second one
                assert k["grid"] * k["block"] < k["total"] < 2 * k["grid"] * k["block"] and k["grid_y"] == 3, (c["name"], k)
        if c["knobs"] == (1256,):
            assert k["block"] == 256, (c["name"], k)
        if c["kernel"].startswith("unpack3d_fwd_mfma_kernel") and len(c["knobs"]) == 2:
            assert k["grid"] == min(k["ntiles"], c["knobs"][1] - 2000) and k["ntiles"] == 20, (c["name"], k)
        seen.add(k["k"])
    named = _named_in_the_launch_switch()
    assert len(named) == len(set(named)) == 52
    if dev:
        assert seen == set(named), (sorted(set(named) - seen), sorted(seen - set(named)))
    else:                                                                      # the cases without knobs are the product's: the same instance without the knobs' code
        assert seen == {c["kernel"] for c in X.CASES if X.is_product(c)} and len(seen) >= 20
