"""CPU: the supervised losses of SupervisedLoss beyond 'sparse-silog' on one scale ({sparse-,}{l1,mse,berhu,silog,abs_rel} over up to four
scales; supervised_loss.py:13-216) and the nearest upsample of upsample_depth_maps.  The CPU restatement (tests/supervised_oracle.py)
against the reference's golden vectors, the method parsing and construction of SupervisedLoss, and the C-ABI entry points in the shipped
library."""
import os
import subprocess

import pytest
import torch

import supervised_oracle as so
from conftest import load_golden, rel_err

NEW_SYMBOLS = ("mte_supervised_loss_work_elems", "mte_supervised_loss_fwd", "mte_supervised_loss_bwd",
               "mte_upsample_nearest_fwd", "mte_upsample_nearest_bwd")
SETS = ("base", "ragged")
NS = (1, 2, 4)


def golden_name(method):
    return "loss_supervised_" + method.replace("-", "_")


def close(a, b, tol):
    """rel_err over the finite entries; NaN / inf must sit at the same places with the same values"""
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    if not torch.equal(fa, fb) or not torch.equal(a[~fa].nan_to_num(0.0, 1.0, -1.0), b[~fb].nan_to_num(0.0, 1.0, -1.0)):
        return False
    return fa.sum() == 0 or rel_err(a[fa], b[fb]) <= tol


@pytest.mark.parametrize("method", so.ACCEPTED)
def test_restatement_matches_reference_vectors(method):
    inp = load_golden("loss_supervised_inputs")
    ref = load_golden(golden_name(method))
    for name in SETS:
        for n in NS:
            invs = [inp["%s.inv%d" % (name, s)].clone().requires_grad_(True) for s in range(4)]
            loss = so.supervised_loss(method, n, invs, inp[name + ".depth"])
            grads = torch.autograd.grad(loss, invs[:n])
            key = "%s.n%d" % (name, n)
            assert close(loss.reshape(1), ref[key + ".loss"].reshape(1), 1e-6), (key, float(loss), float(ref[key + ".loss"]))
            for s in range(n):
                assert close(grads[s], ref["%s.dinv%d" % (key, s)], 1e-6), (key, s)


def test_restatement_matches_reference_model_vectors():
    """the supervised half of the model fixtures: sparse-l1 on four scales, at the predicted sizes and upsampled"""
    ref = load_golden("loss_supervised_model")
    invs = [ref["inv%d" % s] for s in range(4)]
    depth = ref["batch.depth"]
    for tag, maps in (("plain", invs), ("up", so.upsample(invs))):
        loss = so.supervised_loss("sparse-l1", 4, maps, depth)
        assert rel_err(loss.reshape(1), ref[tag + ".supervised_loss"].reshape(1)) <= 1e-6, tag


def test_nearest_upsample_restatement_is_a_block_copy():
    x = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 1, 3, 5)
    up = so.upsample([torch.zeros(2, 1, 12, 20), x])[1]
    assert torch.equal(up, x.repeat_interleave(4, 2).repeat_interleave(4, 3))


def test_methods_parse_like_the_reference():
    from mindtheedge_amd.losses.supervised_loss import parse_supervised_method
    for method in so.ACCEPTED:
        suffix, sparse = so.parse(method)
        assert parse_supervised_method(method) == (so.SUFFIXES.index(suffix), sparse), method
    assert parse_supervised_method("sparse-l1") == (0, True)
    assert parse_supervised_method("abs_rel") == (4, False)
    assert parse_supervised_method("anything-berhu") == (2, False)
    with pytest.raises(ValueError):
        parse_supervised_method("sparse-l2")


def test_supervised_loss_constructs_for_every_accepted_method():
    """every method the reference accepts, on 1..4 scales and with progressive scaling (no effect, as upstream)"""
    from mindtheedge_amd.losses.supervised_loss import SupervisedLoss
    for method in so.ACCEPTED:
        for n in (1, 2, 3, 4):
            sup = SupervisedLoss(supervised_method=method, supervised_num_scales=n)
            assert sup.n == n and sup.logs == {"supervised_num_scales": n}
        sup = SupervisedLoss(supervised_method=method, supervised_num_scales=4, progressive_scaling=0.5)
        assert sup.n == 4
    assert SupervisedLoss().supervised_method == "sparse-l1" and SupervisedLoss().n == 4        # the reference's defaults


def test_supervised_loss_rejects_dense_berhu_and_unknown_suffixes():
    from mindtheedge_amd.losses.supervised_loss import SupervisedLoss
    with pytest.raises(NotImplementedError, match="torch.cat"):
        SupervisedLoss(supervised_method="berhu")
    with pytest.raises(ValueError):
        SupervisedLoss(supervised_method="sparse-huber")
    with pytest.raises(NotImplementedError):
        SupervisedLoss(supervised_method="sparse-l1", supervised_num_scales=5)


def test_default_config_builds_its_model():
    """utils/config.py's defaults (sparse-l1 over four scales) build SemiSupEdgeModel, with and without upsample_depth_maps"""
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.utils.config import default_config
    loss = dict(default_config().model.loss)
    for up in (False, True):
        kw = {k: v for k, v in loss.items() if k not in ("supervised_loss_weight",)}
        kw["upsample_depth_maps"] = up
        m = SemiSupEdgeModel(supervised_loss_weight=1.0, **kw)
        assert m._supervised_loss.supervised_method == "sparse-l1" and m._supervised_loss.n == 4
        assert m.upsample_depth_maps is up


def test_shipped_library_exports_the_supervised_entry_points():
    from mindtheedge_amd import _build, _lib
    path = _build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T mte" in l}
    protos = _lib.parse_header()
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in protos, name
    assert "mte_supervised_loss_work_elems" in _lib.QUERIES
    assert os.path.exists(path)
