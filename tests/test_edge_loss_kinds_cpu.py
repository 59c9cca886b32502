"""CPU: the edge-loss choices beyond 'cross_entropy' (GradLoss 'cross_entropy_dice', 'attention_loss[_dice]',
'spatially_adaptive[_dice]'; grad_loss.py:139-156, attention_loss.py:21-49).  The CPU restatement (tests/edge_kinds_oracle.py)
against the reference's golden vectors, the type-string parsing of GradLoss, and the C-ABI entry points in the shipped library."""
import os
import subprocess

import pytest
import torch

import edge_kinds_oracle as eko
from conftest import load_golden, rel_err

WEIGHT = 10.0
NEW_SYMBOLS = ("mte_edge_loss_kind_work_elems", "mte_edge_loss_kind_fwd", "mte_edge_loss_kind_bwd")
# case -> (input, label, mask, normal, is_grad, is_sigmoid): tests/golden/make_golden_edge_kinds.py
CASES = {
    "nomask": ("depth", "edge", None, "normal", True, True),
    "binmask": ("depth", "edge", "mask_bin", "normal", True, True),
    "softmask": ("depth", "edge", "mask_soft", "normal", True, True),
    "nonormal": ("depth", "edge", None, None, True, True),
    "dee": ("prob", "edge", None, None, False, False),
    "sparse": ("depth", "sparse", None, "normal", True, True),
    "half": ("depth_half", "edge", None, "normal", True, True),
    "sat": ("depth_sat", "edge", None, "normal", True, True),
}


def _oracle_case(t, inp, case):
    x, e, m, n, is_grad, is_sigmoid = CASES[case]
    xin = inp[x].clone().requires_grad_(True)
    loss, g = eko.grad_loss(t, xin, inp[e], None if m is None else inp[m], is_grad, is_sigmoid, 4.0, None if n is None else inp[n],
                            weight=WEIGHT)
    (dx,) = torch.autograd.grad(loss, xin)
    return loss, g, dx


@pytest.mark.parametrize("t", eko.ACCEPTED)
def test_restatement_matches_reference_vectors(t):
    inp = load_golden("loss_edge_kinds_inputs")
    ref = load_golden("loss_edge_kinds_" + t)
    for case in CASES:
        loss, g, dx = _oracle_case(t, inp, case)
        assert torch.isfinite(loss) and torch.isfinite(dx).all(), case
        assert rel_err(loss.reshape(1), ref["loss_" + case].reshape(1)) <= 1e-6, (case, float(loss), float(ref["loss_" + case]))
        assert rel_err(g, ref["g_" + case]) <= 1e-6, case
        assert rel_err(dx, ref["dx_" + case]) <= 1e-6, case


def test_restatement_matches_reference_model_vectors():
    ref = load_golden("loss_edge_kinds_model")
    invs = [ref["inv%d" % s].clone().requires_grad_(True) for s in range(4)]
    batch = {k: v for k, v in ref.items() if k.startswith("edge") or k.startswith("normal")}
    loss = eko.edge_loss_all_scales("spatially_adaptive_dice", invs, batch, None, WEIGHT)
    dinv = torch.autograd.grad(loss, invs)
    assert rel_err(loss.reshape(1), ref["loss"].reshape(1)) <= 1e-6
    for s in range(4):
        assert rel_err(dinv[s], ref["dinv%d" % s]) <= 1e-6, s


def test_box_alpha_edges():
    """all-negative windows take 0.5; a lone positive lowers alpha by exactly 1/225 in its window; binary sums are exact."""
    t = torch.zeros(1, 1, 20, 30)
    t[0, 0, 0, 0] = 1.0
    a = eko.box_alpha(t)
    assert float(a[0, 0, 19, 29]) == 0.5
    assert float(a[0, 0, 7, 7]) == float(torch.tensor(1.0) - torch.tensor(1.0) / 225)
    assert float(a[0, 0, 8, 8]) == 0.5


def test_type_strings_parse():
    from mindtheedge_amd.losses.grad_loss import GradLoss, parse_edge_loss_type
    for t in eko.ACCEPTED + ("cross_entropy",):
        head = GradLoss(t, True, [], WEIGHT, 1.0)
        assert (head.loss_kind, head.dice) == eko.parse(t), t
    assert parse_edge_loss_type("cross_entropy_dice") == (0, True)
    assert parse_edge_loss_type("attention_loss") == (1, False)
    assert parse_edge_loss_type("spatially_adaptive_dice") == (2, True)
    assert parse_edge_loss_type("cross_entropy_spatially_adaptive") == (2, False)       # the last base loss named wins
    for t in eko.REJECTED:
        with pytest.raises(NotImplementedError):
            GradLoss(t)
    with pytest.raises(NotImplementedError):
        GradLoss("attention_loss", True, [(1, 2, 3)])


def test_shipped_library_exports_the_kind_entry_points():
    from mindtheedge_amd import _build, _lib
    path = _build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T mte" in l}
    protos = _lib.parse_header()
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in protos, name
    assert "mte_edge_loss_kind_work_elems" in _lib.QUERIES
    assert os.path.exists(path)
