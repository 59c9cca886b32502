"""CPU: the ring formulation of the folded pack layers' border (csrc/pack_border.hip) in fp64 -- the identity
y_fold + ring correction = conv2d(pad(conv3d(X))), every gradient by autograd on the same composition, the explicit references of the
backward kernels against autograd, and the index arithmetic of csrc/pack_border_plan.hpp compiled alone with g++."""
import itertools
import os
import subprocess

import pytest
import torch

import pack_border_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mindtheedge_amd", "csrc")
BOUND = 1e-10          # relative, of the largest reference value (fp64 sums of a few thousand terms: ~1e-13)
CASES = [(k, D, hw) for k in (3, 5) for D in (8, 12) for hw in ((3, 3), (4, 5), (6, 7))]


def _inputs(k, D, hw, B=2, Co=3, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * k + D)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    return r(B, hw[0], hw[1], D), r(4, 3, 3, 3), r(4), r(Co, 4 * D, k, k), r(Co)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("k,D,hw", CASES)
def test_ring_identity_and_gradients(k, D, hw):
    args = [t.requires_grad_(True) for t in _inputs(k, D, hw)]
    assert float(args[2].detach().abs().min()) > 0                         # b3 != 0
    ref = R.layer_reference(*args)
    got = R.layer_ring(*args)
    assert _rel(got, ref) < BOUND
    if min(hw) > k // 2 + 1:                                       # the folded form alone IS wrong at the border (the test would pass trivially otherwise)
        assert _rel(R.layer_folded(*args), ref) > 1e-3
    G = torch.rand(ref.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 2 - 1
    g_ref = torch.autograd.grad((ref * G).sum(), args)
    g_got = torch.autograd.grad((got * G).sum(), args)
    for a, b in zip(g_got, g_ref):
        assert _rel(a, b) < BOUND


@pytest.mark.parametrize("k,D,hw", CASES)
def test_ring_stencil_by_taps(k, D, hw):
    P, K3, _, _, _ = _inputs(k, D, hw)
    P.requires_grad_(True)
    K3.requires_grad_(True)
    Rr, Rc = R.ring_fwd(P, K3)
    Tr, Tc = R.ring_fwd_taps(P, K3)
    assert _rel(Tr, Rr) < BOUND and _rel(Tc, Rc) < BOUND
    # U is exactly zero beyond the ring: conv3d of the image grown by two pixels has no data part on its outermost frame
    U2 = R.conv3d_on(P, K3, torch.zeros(4, dtype=torch.float64), 2)
    assert float(U2[:, :, 0].abs().max()) == 0 and float(U2[:, :, :, 0].abs().max()) == 0
    g = torch.Generator().manual_seed(4)
    dRr, dRc = torch.rand(Rr.shape, generator=g, dtype=torch.float64) - 0.5, torch.rand(Rc.shape, generator=g, dtype=torch.float64) - 0.5
    dP, dK3 = torch.autograd.grad((Rr * dRr).sum() + (Rc * dRc).sum(), (P, K3))
    assert _rel(R.ring_bwd_data(dRr, dRc, K3.detach(), P.shape), dP) < BOUND
    assert _rel(R.ring_bwd_weight(dRr, dRc, P.detach()), dK3) < BOUND
    x = R.unshuffle(P.detach())
    assert x.shape == (P.shape[0], 2 * hw[0], 2 * hw[1], D // 4)
    assert float(x[0, 3, 2, 1]) == float(P[0, 1, 1, 4 * 1 + 2 * 1 + 0])


@pytest.mark.parametrize("k,D,hw", [(3, 8, (4, 5)), (3, 12, (6, 7)), (5, 8, (4, 5)), (5, 12, (6, 7))])
def test_backward_pieces_equal_autograd(k, D, hw):
    """gather -> GEMM gradients -> ring backward / scatter, chained by hand, against autograd of the forward composition (shapes the kernels take)"""
    P, K3, b3, W, _ = [t.requires_grad_(True) for t in _inputs(k, D, hw)]
    Rr, Rc = R.ring_fwd(P, K3)
    Wr, Wc, Dt = R.border_weights(W, b3)
    cr, cc = R.ring_gemms(Rr, Rc, Wr, Wc)
    y0 = torch.zeros(P.shape[0], hw[0], hw[1], W.shape[0], dtype=torch.float64)
    out = R.border_apply(y0, cr, cc, Dt, k)
    dy = torch.rand(out.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2 - 1
    gP, gK3, gb3, gW = torch.autograd.grad((out * dy).sum(), (P, K3, b3, W), retain_graph=True)
    Gr, Gc, dD = R.border_gather(dy, k)
    dcr, dcc, dDt = torch.autograd.grad((out * dy).sum(), (cr, cc, Dt), retain_graph=True)
    assert _rel(Gr, dcr) < BOUND and _rel(Gc, dcc) < BOUND and _rel(dD, dDt) < BOUND
    dRr, dRc, dWr, dWc = torch.autograd.grad((cr * Gr).sum() + (cc * Gc).sum(), (Rr, Rc, Wr, Wc), retain_graph=True)
    assert _rel(R.ring_bwd_data(dRr, dRc, K3.detach(), P.shape), gP) < BOUND
    assert _rel(R.ring_bwd_weight(dRr, dRc, P.detach()), gK3) < BOUND
    dW, db3 = R.border_scatter(dWr, dWc, dD, W.detach(), b3.detach())
    assert _rel(dW, gW) < BOUND and _rel(db3, gb3) < BOUND


PLAN_MAIN = r"""
#include <cstdio>
#include "pack_border_plan.hpp"
int main() {
    const int ks[2] = {3, 5};
    for (int k : ks) {
        const int pad = k / 2;
        for (int far = 0; far < 2; ++far) for (int j = 0; j < pad; ++j) {
            int f2, j2; const int t = pb_tap(far, j, pad);
            printf("tap %d %d %d %d %d\n", k, far, j, t, pb_tap_owner(t, pad, &f2, &j2) && f2 == far && j2 == j);
        }
        { int f2, j2; printf("centre %d %d\n", k, (int)pb_tap_owner(pad, pad, &f2, &j2)); }
        for (int c = 0; c <= 2 * pad; ++c) for (int t = 0; t < k; ++t) printf("out %d %d %d %d\n", k, c, t, (int)pb_tap_outside(c, t, pad));
        const int hs[4] = {pad + 1, 2 * pad, 2 * pad + 1, 9}, ws[2] = {2 * pad, 11};
        for (int H2 : hs) for (int W2 : ws) {
            printf("ok %d %d %d %d\n", k, H2, W2, (int)pb_shape_ok(H2, W2, k));
            if (!pb_shape_ok(H2, W2, k)) continue;
            for (int r = 0; r < H2; ++r) printf("cls %d %d %d %d\n", k, H2, r, pb_class(r, H2, pad));
            for (int c = 0; c <= 2 * pad; ++c) printf("clsrange %d %d %d %d %d\n", k, H2, c, pb_class_first(c, H2, pad), pb_class_count(c, H2, pad));
            const long n = pb_border_count(H2, W2, pad);
            for (long i = 0; i < n; ++i) { int r, x; pb_border_pixel(i, H2, W2, pad, &r, &x); printf("pix %d %d %d %ld %d %d\n", k, H2, W2, i, r, x); }
            for (int e = 0; e < 4; ++e) for (int i = 0; i < pb_edge_len(e, H2, W2); ++i) for (int a = 0; a < 3; ++a) {
                int h, w, al, off; const bool v = pb_edge_src(e, i, a, H2, W2, &h, &w);
                const bool on = v && pb_edge_of_pixel(e, h, w, H2, W2, &al, &off) && al + off - a == i;
                printf("src %d %d %d %d %d %d %d %d %d\n", H2, W2, e, i, a, (int)v, v ? h : -1, v ? w : -1, v ? (int)on : 1);
            }
        }
    }
    for (int e = 0; e < 4; ++e) for (int f = 0; f < 4; ++f) for (int kd = 0; kd < 3; ++kd) for (int a = 0; a < 3; ++a) printf("k3 %d %d %d %d %d\n", e, f, kd, a, pb_k3_index(e, f, kd, a));
    return 0;
}
"""


def test_plan_header_index_arithmetic(tmp_path):
    """csrc/pack_border_plan.hpp with plain g++ against the Python arithmetic of pack_border_ref: taps, classes (including the smallest image whose top and
    bottom classes touch, H2 = 2 pad -- and H2 = pad + 1, which is that image for k = 3 and refused for k = 5), border pixels, ring sources, K3 taps."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", exe], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    by = lambda tag: [[int(v) for v in r[1:]] for r in rows if r[0] == tag]
    assert len(by("tap")) == 2 * (1 + 2)
    for k, far, j, t, back in by("tap"):
        assert t == R.tap(far, j, k // 2) and back == 1
    assert all(v == 0 for _, v in by("centre"))
    for k, c, t, o in by("out"):
        assert bool(o) == R.tap_outside(c, t, k // 2)
    oks = {(k, H2, W2): o for k, H2, W2, o in by("ok")}
    for (k, H2, W2), o in oks.items():
        assert bool(o) == (H2 >= 2 * (k // 2) and W2 >= 2 * (k // 2))
    assert oks[(3, 2, 2)] == 1 and oks[(5, 3, 4)] == 0 and oks[(5, 4, 4)] == 1
    for k, H2, r, c in by("cls"):
        assert c == R.class_of(r, H2, k // 2)
    cls = {}
    for k, H2, r, c in by("cls"):
        cls.setdefault((k, H2, c), set()).add(r)
    for k, H2, c, first, count in by("clsrange"):
        assert sorted(cls.get((k, H2, c), ())) == list(range(first, first + count))
    pix = {}
    for k, H2, W2, i, r, x in by("pix"):
        pix.setdefault((k, H2, W2), {})[i] = (r, x)            # (k = 3 lists H2 = pad + 1 = 2 pad twice)
    for (k, H2, W2), rows_ in pix.items():
        got = [rows_[i] for i in range(len(rows_))]
        pad = k // 2
        want = {(r, x) for r, x in itertools.product(range(H2), range(W2)) if min(r, x, H2 - 1 - r, W2 - 1 - x) < pad}
        assert len(got) == len(set(got)) and set(got) == want                      # each border pixel exactly once
    for H2, W2, e, i, a, v, h, w, on in by("src"):
        if e < 2:
            hh, ww = (0 if e == 0 else H2 - 1), i + a - 2
            valid = 0 <= ww < W2
        else:
            hh, ww = i + a - 1, (0 if e == 2 else W2 - 1)
            valid = 0 <= hh < H2
        assert bool(v) == valid and on == 1
        if valid:
            assert (h, w) == (hh, ww)
    for e, f, kd, a, ix in by("k3"):
        dh, dw = (R.k3_fixed(e), a) if e < 2 else (a, R.k3_fixed(e))
        assert ix == ((f * 3 + kd) * 3 + dh) * 3 + dw
