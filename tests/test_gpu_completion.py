"""GPU (-m gpu): depth completion training -- the two-branch one-launch loss (kernels.DepthLossesPairFn -> mte_edge_loss_pair_fwd / _bwd,
the <2> instantiation of csrc/edge_fast.hpp), the two completion models, one training step and the entry point.

Pair path: the depth-edge loss of four scales + the silog loss of scale 0 for TWO sets of predictions against one set of labels, against
  * the float64 oracle (oracle/loss_oracle.py), losses 1e-4 and gradients 2e-4 of the largest gradient of a map (the single launch's bars);
  * two single launches (kernels.DepthLossesFn), bit for bit: both are instantiations of one template with the same order of every sum;
  * itself: swapping the branches swaps the outputs bit for bit, a branch does not see the other one, repeated runs are bit-equal.
Shapes: one tile; a 4 x 8 lowest scale (one partial tile); a partial last tile column with three consecutive tiles per workgroup; several
tile rows with a partial lowest scale; B = 8, i.e. 64 (branch, scale, sample) images in the finish; B = 21 and 22, the last batch whose sums
the finish stages in LDS and the first it reads straight from memory (one tile per image).
Fallback: a width that is no multiple of 4 and a batch without normals answer MTE_ERR_UNSUPPORTED and run as two single launches."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFX = ["", "_1", "_2", "_3"]
WEIGHT, POS_TO_NEG, THRESH = 10.0, 1.0, 4.0
SHAPES = [(2, 64, 128), (1, 32, 64), (3, 96, 224), (2, 160, 320), (8, 32, 64), (21, 32, 64), (22, 32, 64)]


@functools.lru_cache(maxsize=None)
def _maps(B, H, W, with_normals=True):
    """as _maps of test_gpu_edge_loss_fused.py, with a second, independent set of predictions"""
    g = torch.Generator().manual_seed(1000 * B + H + W)
    r = lambda *s: torch.rand(*s, generator=g)
    a, b, batch = [], [], {}
    for s in range(4):
        h, w = H >> s, W >> s
        a.append(0.05 + 1.9 * r(B, 1, h, w))
        b.append(0.05 + 1.9 * r(B, 1, h, w))
        batch["edge" + SFX[s]] = (r(B, 1, h, w) < 0.08).float() * r(B, 1, h, w)
        if with_normals:
            batch["normal" + SFX[s]] = (r(B, 1, h, w) * 2 - 1) * math.pi
    batch["depth"] = (r(B, 1, H, W) < 0.1).float() * (1.0 + 79.0 * r(B, 1, H, W))
    return a, b, batch


def _gout(n_out):
    """upstream gradients, different for every output, so that a mixed-up coefficient or branch shows"""
    return torch.tensor([[1.0 + 0.25 * k for k in range(n_out)], [0.5 + 0.125 * k for k in range(n_out)]])


@functools.lru_cache(maxsize=None)
def _oracle(B, H, W, with_gt, with_normals=True):
    """float64: losses [2, 4 (+1)] and the gradients of sum(gout * losses) with respect to the eight maps.  Computed once per case."""
    from oracle import loss_oracle as lo
    a, b, batch = _maps(B, H, W, with_normals)
    bd = {k: v.double() for k, v in batch.items()}
    rows, grads = [], []
    gout = _gout(5 if with_gt else 4).double()
    for br, invs in enumerate((a, b)):
        invs = [i.double().requires_grad_(True) for i in invs]
        row = [lo.grad_loss(lo.inv2depth(invs[s]), bd["edge" + SFX[s]], None, True, True, THRESH, bd.get("normal" + SFX[s]),
                            weight=WEIGHT, pos_to_neg=POS_TO_NEG)[0] for s in range(4)]
        if with_gt:
            row.append(lo.supervised_silog_loss(invs[0], bd["depth"]))
        row = torch.stack(row)
        (row * gout[br]).sum().backward()
        rows.append(row.detach())
        grads += [i.grad for i in invs]
    return torch.stack(rows), grads


def _dev(ts):
    return [t.cuda().contiguous() for t in ts]


def _pair(a, b, batch, with_gt):
    """-> losses [2, 4 (+1)] and the eight gradients of sum(gout * losses), on the host"""
    from mindtheedge_amd import kernels as K
    preds = [t.requires_grad_(True) for t in _dev(a) + _dev(b)]
    edges = _dev([batch["edge" + s] for s in SFX])
    normals = [batch["normal" + s].cuda() if "normal" + s in batch else None for s in SFX]
    gt = batch["depth"].cuda() if with_gt else None
    losses = K.DepthLossesPairFn.apply(WEIGHT, POS_TO_NEG, THRESH, gt, edges, normals, *preds)
    (losses * _gout(losses.shape[1]).cuda()).sum().backward()
    torch.cuda.synchronize()
    return losses.detach().cpu(), [p.grad.cpu() for p in preds]


def _single(invs, batch, with_gt, gout_row):
    from mindtheedge_amd import kernels as K
    preds = [t.requires_grad_(True) for t in _dev(invs)]
    edges = _dev([batch["edge" + s] for s in SFX])
    normals = [batch["normal" + s].cuda() if "normal" + s in batch else None for s in SFX]
    gt = batch["depth"].cuda() if with_gt else None
    losses = K.DepthLossesFn.apply(WEIGHT, POS_TO_NEG, THRESH, True, None, gt, edges, normals, *preds)
    (losses * gout_row.cuda()).sum().backward()
    torch.cuda.synchronize()
    return losses.detach().cpu(), [p.grad.cpu() for p in preds]


def _check(losses, grads, want_losses, want_grads, tol, gtol):
    print("losses", losses.tolist(), "want", want_losses.tolist())
    assert tuple(losses.shape) == tuple(want_losses.shape)
    for got, want in zip(losses.flatten().tolist(), want_losses.flatten().tolist()):
        assert got == pytest.approx(want, rel=tol)
    for i, (g, w) in enumerate(zip(grads, want_grads)):
        err = float((g.double() - w.double()).abs().max() / w.double().abs().max().clamp(min=1e-30))
        print("gradient", i, "error", err)
        assert err <= gtol, (i, err)


def _raw_scales(a, b, edges, normals, dpreds=None):
    from mindtheedge_amd.kernels_loss import _EdgePairScale
    arr = (_EdgePairScale * 4)()
    for s, o in enumerate(arr):
        o.pred[0], o.pred[1] = a[s].data_ptr(), b[s].data_ptr()
        if dpreds is not None:
            o.dpred[0], o.dpred[1] = dpreds[s].data_ptr(), dpreds[4 + s].data_ptr()
        o.edge, o.normal = edges[s].data_ptr(), (None if normals[s] is None else normals[s].data_ptr())
        o.H, o.W = a[s].shape[-2], a[s].shape[-1]
    return arr


# ---------------- the pair path -------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gt", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_matches_the_float64_oracle(shape, with_gt):
    a, b, batch = _maps(*shape)
    want_losses, want_grads = _oracle(*shape, with_gt)
    losses, grads = _pair(a, b, batch, with_gt)
    _check(losses, grads, want_losses, want_grads, 1e-4, 2e-4)


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_matches_two_single_launches(shape):
    a, b, batch = _maps(*shape)
    losses, grads = _pair(a, b, batch, True)
    gout = _gout(5)
    for br, invs in enumerate((a, b)):
        one, one_grads = _single(invs, batch, True, gout[br])
        _check(losses[br], grads[4 * br:4 * br + 4], one, one_grads, 2e-6, 2e-5)
        assert torch.equal(losses[br], one), br
        for s, (x, y) in enumerate(zip(grads[4 * br:4 * br + 4], one_grads)):
            assert torch.equal(x, y), (br, s)


def test_branches_are_independent_and_swap_exactly():
    a, b, batch = _maps(3, 96, 224)
    losses, grads = _pair(a, b, batch, True)
    # swapped inputs (and swapped upstream gradients): swapped outputs, bit for bit
    from mindtheedge_amd import kernels as K
    preds = [t.requires_grad_(True) for t in _dev(b) + _dev(a)]
    edges = _dev([batch["edge" + s] for s in SFX])
    normals = _dev([batch["normal" + s] for s in SFX])
    sw = K.DepthLossesPairFn.apply(WEIGHT, POS_TO_NEG, THRESH, batch["depth"].cuda(), edges, normals, *preds)
    (sw * _gout(5).flip(0).cuda()).sum().backward()
    assert torch.equal(sw.detach().cpu(), losses.flip(0))
    for i in range(8):
        assert torch.equal(preds[i].grad.cpu(), grads[(i + 4) % 8]), i
    # another input on one branch leaves the other branch's numbers alone
    other = [0.05 + 1.9 * torch.rand(t.shape, generator=torch.Generator().manual_seed(77 + i)) for i, t in enumerate(b)]
    l2, g2 = _pair(a, other, batch, True)
    assert torch.equal(l2[0], losses[0]) and not torch.equal(l2[1], losses[1])
    assert all(torch.equal(x, y) for x, y in zip(g2[:4], grads[:4]))
    l3, g3 = _pair(other, b, batch, True)
    assert torch.equal(l3[1], losses[1]) and all(torch.equal(x, y) for x, y in zip(g3[4:], grads[4:]))


def test_pair_is_bit_reproducible():
    a, b, batch = _maps(2, 160, 320)
    losses, grads = _pair(a, b, batch, True)
    noise = torch.cuda.Stream()
    na = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    nb = torch.empty_like(na)
    for rep in range(3):
        if rep == 1:
            with torch.cuda.stream(noise):
                nb.copy_(na)
        l, g = _pair(a, b, batch, True)
        assert torch.equal(l, losses)
        assert all(torch.equal(x, y) for x, y in zip(g, grads))
    torch.cuda.synchronize()


def test_library_clears_the_pair_workspace_unless_told_otherwise():
    """MTE_OPT_LOSS_PREZEROED off: `work` may hold anything, NaN included; on: the caller's zeros are trusted.  Same bits either way."""
    from mindtheedge_amd import kernels as K
    B = 2
    a, b, batch = _maps(B, 64, 128)
    a, b = _dev(a), _dev(b)
    edges, normals = _dev([batch["edge" + s] for s in SFX]), _dev([batch["normal" + s] for s in SFX])
    gt = batch["depth"].cuda().contiguous()
    arr = _raw_scales(a, b, edges, normals)
    n = K.lib.mte_edge_loss_pair_work_elems(ctypes.addressof(arr), 4, B)
    assert n > 0
    results = []
    try:
        for prezeroed, fill in ((0, 123.0), (0, float("nan")), (1, 0.0)):
            K.lib.set_option(1, prezeroed)
            work = torch.full((n,), fill, dtype=torch.float64, device="cuda")
            losses = torch.empty((2, 4), dtype=torch.float32, device="cuda")
            coef = torch.empty((2 * 4 * (2 * B + 1),), dtype=torch.float32, device="cuda")
            sil = torch.empty((2,), dtype=torch.float32, device="cuda")
            aux = torch.empty((4,), dtype=torch.float32, device="cuda")
            K.lib.mte_edge_loss_pair_fwd(ctypes.addressof(arr), 4, B, THRESH, WEIGHT, POS_TO_NEG, gt.data_ptr(), work.data_ptr(), losses.data_ptr(),
                                         coef.data_ptr(), sil.data_ptr(), aux.data_ptr(), K._stream())
            torch.cuda.synchronize()
            results.append((losses.clone(), coef.clone(), sil.clone(), aux.clone()))
    finally:
        K.lib.set_option(1, 1 if K._arena.enabled else 0)
    for r in results[1:]:
        for x, y in zip(results[0], r):
            assert torch.equal(x, y)
    assert all(bool(torch.isfinite(t).all()) for t in results[0])


# ---------------- the fallback --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,with_normals", [((2, 72, 100), True), ((2, 64, 128), False)])
def test_outside_the_training_configuration_two_single_launches(shape, with_normals):
    from mindtheedge_amd import _lib as L
    from mindtheedge_amd import kernels as K
    B = shape[0]
    a, b, batch = _maps(*shape, with_normals)
    da, db = _dev(a), _dev(b)
    edges = _dev([batch["edge" + s] for s in SFX])
    normals = [batch["normal" + s].cuda().contiguous() if with_normals else None for s in SFX]
    dpreds = [torch.full_like(t, 7.0) for t in da + db]
    arr = _raw_scales(da, db, edges, normals, dpreds)
    n = K.lib.mte_edge_loss_pair_work_elems(ctypes.addressof(arr), 4, B)
    work = torch.zeros((max(n, 1),), dtype=torch.float64, device="cuda")
    losses = torch.full((2, 4), 7.0, device="cuda")
    coef = torch.zeros((2 * 4 * (2 * B + 1),), device="cuda")
    raw = L.lib.load()
    assert raw.mte_edge_loss_pair_fwd(ctypes.addressof(arr), 4, B, THRESH, WEIGHT, POS_TO_NEG, None, work.data_ptr(), losses.data_ptr(),
                                      coef.data_ptr(), None, None, K._stream()) == -3
    assert raw.mte_edge_loss_pair_bwd(ctypes.addressof(arr), 4, B, THRESH, coef.data_ptr(), None, None, None, None, K._stream()) == -3
    torch.cuda.synchronize()
    assert bool((losses == 7.0).all()) and all(bool((d == 7.0).all()) for d in dpreds)        # nothing was launched
    want_losses, want_grads = _oracle(*shape, True, with_normals)
    got_losses, got_grads = _pair(a, b, batch, True)
    _check(got_losses, got_grads, want_losses, want_grads, 1e-4, 2e-4)


# ---------------- the models ----------------------------------------------------------------------------------------

class _StubNet(torch.nn.Module):
    """the two passes of the network as fixed leaves (tests/golden/make_golden_completion.py)"""
    with_san = True

    def __init__(self, inv, inv_rgbd, depth_loss):
        super().__init__()
        self.inv, self.inv_rgbd, self.depth_loss = inv, inv_rgbd, depth_loss

    def forward(self, rgb, input_depth=None, **kw):
        assert input_depth is not None
        return {"inv_depths": list(self.inv), "inv_depths_rgbd": list(self.inv_rgbd), "depth_loss": self.depth_loss * 1.0}


def _golden_model(name, fuse=True):
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.utils.load import load_class
    g = load_golden("completion_2x32x64")
    batch = {k[6:]: v.cuda() for k, v in g.items() if k.startswith("batch.")}
    inv = [g["inv%d" % s].cuda().requires_grad_(True) for s in range(4)]
    inv_rgbd = [g["inv_rgbd%d" % s].cuda().requires_grad_(True) for s in range(4)]
    depth_loss = g["depth_loss"].cuda().requires_grad_(True)
    kw = dict(supervised_loss_weight=1.0, weight_rgbd=float(g["weight_rgbd"]), supervised_method="sparse-silog", supervised_num_scales=1,
              upsample_depth_maps=False, flip_lr_prob=0.0, edges_depth_edge_loss_all_scales=True)
    if name == "SemiSupEdgeCompletionModel":
        kw["depth_edges_loss_weight"] = float(g["depth_edges_loss_weight"])
    model = load_class(name, "models")(**kw)
    model.add_depth_net(_StubNet(inv, inv_rgbd, depth_loss))
    if name == "SemiSupEdgeCompletionModel":
        model.add_edge_loss(GradLoss("cross_entropy", True, [], float(g["head_weight"]), float(g["pos_to_neg"])))
        model.fuse_losses = fuse
    model.train()
    out = model(batch)
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    return g, out, inv, inv_rgbd, depth_loss


# The golden numbers are the reference's float32 arithmetic.  Its distance from the float64 oracle is bounded by the oracle-against-golden
# bars (1e-4 losses, 2e-3 gradients; tests/test_completion_cpu.py), the kernels' by the bars above (1e-4, 2e-4): the sum of the two.
GOLDEN_TOL, GOLDEN_GTOL = 2e-4, 2.2e-3


@pytest.mark.parametrize("fuse", [True, False])
def test_edge_completion_model_matches_the_reference(fuse):
    g, out, inv, inv_rgbd, depth_loss = _golden_model("SemiSupEdgeCompletionModel", fuse)
    assert rel_err(out["loss"].cpu(), g["edge.loss"]) < GOLDEN_TOL
    assert set(out["metrics"]) == {"edge_loss", "edge_lidar_loss", "supervised_loss"}
    for m in ("edge_loss", "edge_lidar_loss", "supervised_loss"):
        assert rel_err(out["metrics"][m].cpu(), g["edge." + m]) < GOLDEN_TOL, m
    for s in range(4):
        assert rel_err(inv[s].grad.cpu(), g["edge.grad_inv%d" % s]) < GOLDEN_GTOL, s
        assert rel_err(inv_rgbd[s].grad.cpu(), g["edge.grad_inv_rgbd%d" % s]) < GOLDEN_GTOL, s
    assert float(depth_loss.grad) == 1.0
    assert "inv_depths_rgbd" in out and "depth_loss" in out


def test_edge_completion_model_fused_path_matches_the_per_scale_path():
    _, fused, fi, fr, _ = _golden_model("SemiSupEdgeCompletionModel", True)
    _, per, pi, pr, _ = _golden_model("SemiSupEdgeCompletionModel", False)
    assert float(fused["loss"].detach()) == pytest.approx(float(per["loss"].detach()), rel=2e-6)
    for m in ("edge_loss", "edge_lidar_loss", "supervised_loss"):
        assert float(fused["metrics"][m]) == pytest.approx(float(per["metrics"][m]), rel=2e-6), m
    for x, y in zip(fi + fr, pi + pr):
        assert float((x.grad - y.grad).abs().max() / y.grad.abs().max()) <= 2e-5


def test_completion_model_matches_the_reference():
    g, out, inv, inv_rgbd, depth_loss = _golden_model("SemiSupCompletionModel")
    assert rel_err(out["loss"].cpu(), g["plain.loss"]) < GOLDEN_TOL
    assert rel_err(out["metrics"]["supervised_loss"].cpu(), g["plain.supervised_loss"]) < GOLDEN_TOL
    assert rel_err(inv[0].grad.cpu(), g["plain.grad_inv0"]) < GOLDEN_GTOL and rel_err(inv_rgbd[0].grad.cpu(), g["plain.grad_inv_rgbd0"]) < GOLDEN_GTOL
    assert all(t.grad is None for t in inv[1:] + inv_rgbd[1:]) and float(depth_loss.grad) == 1.0


# ---------------- one training step, the entry point ------------------------------------------------------------------

def test_two_optimizer_steps_move_the_sparse_branch_and_validation_reports_both_predictions():
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    over = {"model": {"name": "SemiSupEdgeCompletionModel",
                      "loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                               "depth_edges_loss_weight": 1.0, "edges_depth_edge_loss_all_scales": True},
                      "depth_net": {"dropout": 0.5}},
            "datasets": {"augmentation": {"image_shape": (64, 128)}, "train": {"batch_size": 2}}}
    try:
        torch.manual_seed(11)
        wrap = ModelWrapper(load_config(None, over)).cuda()
        assert wrap.depth_net.with_san and type(wrap.model).__name__ == "SemiSupEdgeCompletionModel"
        from test_gpu_san import _randomise
        _randomise(wrap.depth_net.mconvs, seed=3)             # as the sparse-branch gradient tests: every tensor of the branch carries a gradient
        optimizer, _ = wrap.configure_optimizers()
        watch = {n: p.detach().clone() for n, p in wrap.depth_net.named_parameters()
                 if n in ("weight", "bias") or n.startswith("mconvs.")}
        assert "weight" in watch and "bias" in watch and sum(n.startswith("mconvs.") for n in watch) >= 10
        wrap.train()
        dev = torch.device("cuda", torch.cuda.current_device())
        for step in range(2):
            batch = synthetic_batch(2, 64, 128, seed=40 + step, device=dev, lidar=True)
            optimizer.zero_grad()
            out = wrap.training_step(batch)
            out["loss"].backward()
            optimizer.step()
            assert bool(torch.isfinite(out["loss"]).all()) and float(out["loss"].sum()) > 0
            assert {"edge_loss", "edge_lidar_loss", "supervised_loss"} <= set(out["metrics"])
            assert all(bool(torch.isfinite(v).all()) for v in out["metrics"].values())
        now = dict(wrap.depth_net.named_parameters())
        moved = {n: float((now[n].detach() - w).abs().max()) for n, w in watch.items()}
        assert moved["weight"] > 0 and moved["bias"] > 0
        still = [n for n, m in moved.items() if n.startswith("mconvs.") and m == 0.0]
        assert not still, still
        wrap.eval()
        batch = synthetic_batch(1, 64, 128, seed=50, device=dev, lidar=True)
        batch["edge"] = (batch["edge"] > 0).float()
        metrics = wrap.evaluate_depth(dict(batch))["metrics"]
        assert "edges" in metrics and "edges_input" in metrics and tuple(metrics["edges_input"].shape) == tuple(metrics["edges"].shape) == (9,)
        assert bool(torch.isfinite(metrics["edges_input"]).all())
        summary = wrap.validation_epoch_end([{"idx": None, **metrics}])
        assert "edges_input-f1_0" in summary and "edges-f1_0" in summary and "depth-abs_rel" in summary
        # a batch without the LiDAR input reports what it reported before
        batch.pop("input_depth")
        assert "edges_input" not in wrap.evaluate_depth(dict(batch))["metrics"]
    finally:
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")


def test_train_edges_completion_two_steps(tmp_path, capsys):
    """the shipped completion config through the entry point (the DEE test of test_gpu_entry_points.py, for the completion model)"""
    import importlib
    import yaml
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.models.model_checkpoint import load_checkpoint
    with open(os.path.join(ROOT, "configs", "train_packnet_san_completion_with_edges.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["datasets"]["augmentation"]["image_shape"] = [64, 128]
    cfg["datasets"]["train"]["batch_size"] = 2
    cfg.setdefault("checkpoint", {})["filepath"] = ""
    cfgp = os.path.join(tmp_path, "cfg.yaml")
    with open(cfgp, "w") as f:
        yaml.safe_dump(cfg, f)
    save = os.path.join(tmp_path, "completion")
    old = sys.argv
    sys.argv = ["train_edges.py", cfgp, "--synthetic", "--synthetic-lidar", "--steps", "2", "--epochs", "1", "--save", save]
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        importlib.import_module("train_edges").main()
    finally:
        sys.argv = old
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")
    hist = eval(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(hist) == 1 and hist[0]["steps"] == 2 and np.isfinite(hist[0]["avg_loss"]) and hist[0]["avg_loss"] > 0
    ckpt = load_checkpoint(os.path.join(save, "epoch=0.ckpt"))
    assert len([k for k in ckpt["state_dict"] if ".mconvs." in k]) >= 70
    assert {int(float(st["step"])) for st in ckpt["optimizer"]["state"].values()} == {2}
