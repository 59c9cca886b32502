"""GPU (-m gpu): SupervisedLoss over up to four scales with every method the reference accepts, and upsample_depth_maps, on the kernels
of csrc/supervised_loss.hip: the reference's golden vectors, the CPU restatement on ragged shapes and non-integer nearest ratios, the
empty-mask and BerHu edge cases, the nearest upsample against torch, run-to-run bit equality, the model-level losses, a graph-replayed
training step and the training entry point."""
import os
import random

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

import supervised_oracle as so
from conftest import load_golden, rel_err
from test_supervised_loss_cpu import NS, SETS, close, golden_name

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _mid(method):
    suffix, sparse = so.parse(method)
    return so.SUFFIXES.index(suffix), sparse


def _run(method, n, invs, depth):
    """the kernel (K.SupervisedLossFn) -> loss, [d loss / d inv_s for s < n]"""
    from mindtheedge_amd import kernels as K
    mid, sparse = _mid(method)
    xs = [t.to(DEV).clone().requires_grad_(True) for t in invs[:n]]
    loss = K.SupervisedLossFn.apply(mid, sparse, depth.to(DEV), *xs)
    grads = torch.autograd.grad(loss, xs)
    return loss.detach().cpu(), [g.cpu() for g in grads]


def _oracle(method, n, invs, depth):
    xs = [t.clone().requires_grad_(True) for t in invs[:n]]
    loss = so.supervised_loss(method, n, xs, depth)
    return loss.detach(), list(torch.autograd.grad(loss, xs))


def _masked_out(depth, shape):
    return so.nearest(so.depth2inv(depth), shape) <= 0


@pytest.mark.parametrize("method", so.ACCEPTED)
def test_matches_reference_vectors(method):
    inp = load_golden("loss_supervised_inputs")
    ref = load_golden(golden_name(method))
    sparse = so.parse(method)[1]
    for name in SETS:
        invs = [inp["%s.inv%d" % (name, s)] for s in range(4)]
        depth = inp[name + ".depth"]
        for n in NS:
            key = "%s.n%d" % (name, n)
            loss, grads = _run(method, n, invs, depth)
            assert close(loss.reshape(1), ref[key + ".loss"].reshape(1), 1e-5), (key, float(loss), float(ref[key + ".loss"]))
            for s in range(n):
                want = ref["%s.dinv%d" % (key, s)]
                assert close(grads[s], want, 1e-5), (key, s, rel_err(grads[s], want))
                if sparse:
                    out = _masked_out(depth, invs[s].shape[-2:])
                    assert out.any() and (grads[s][out] == 0).all(), (key, s)


def test_supervised_loss_module_routes():
    """SupervisedLoss: 'sparse-silog' on one scale at the ground truth's size keeps SilogFn, everything else takes the new kernel
    (also 'sparse-silog' with a ground truth of another size, which used to raise)"""
    from mindtheedge_amd.losses.supervised_loss import SupervisedLoss
    inp = load_golden("loss_supervised_inputs")
    invs = [inp["base.inv%d" % s].to(DEV) for s in range(4)]
    depth = inp["base.depth"].to(DEV)
    for method, n in (("sparse-l1", 4), ("abs_rel", 2), ("sparse-berhu", 4), ("sparse-silog", 4)):
        ref = load_golden(golden_name(method))
        out = SupervisedLoss(supervised_method=method, supervised_num_scales=n)(invs, depth)
        assert close(out["loss"].cpu(), ref["base.n%d.loss" % n].reshape(1), 1e-5), method
    sup = SupervisedLoss(supervised_method="sparse-silog", supervised_num_scales=1)
    ref = load_golden(golden_name("sparse-silog"))
    assert rel_err(sup(invs, depth)["loss"].cpu(), ref["base.n1.loss"].reshape(1)) < 1e-4
    big = F.interpolate(inp["base.depth"], scale_factor=2, mode="nearest").to(DEV)        # nearest of it at 32 x 64 is the same gt
    assert rel_err(sup(invs, big)["loss"].cpu(), ref["base.n1.loss"].reshape(1)) < 1e-5


@pytest.mark.parametrize("case", [
    ((3, 37, 101), [(37, 101), (19, 51), (10, 26), (5, 13)]),       # W % 4 != 0, ratios 37/19, 101/51, ...
    ((2, 20, 30), [(37, 61), (19, 31), (9, 15), (4, 8)]),           # ground truth SMALLER than the predictions
    ((1, 96, 320), [(96, 320), (48, 160), (24, 80), (12, 40)]),     # many workgroups, 16-byte path
    ((2, 5, 7), [(5, 7), (3, 4), (2, 2), (1, 1)]),                  # tiny
])
def test_ragged_shapes_match_restatement(case):
    (B, hd, wd), sizes = case
    gen = torch.Generator().manual_seed(hd * 1000 + wd)
    depth = (torch.rand(B, 1, hd, wd, generator=gen) < 0.6).float() * (1 + 40 * torch.rand(B, 1, hd, wd, generator=gen))
    depth[0, 0, 0, 0] = 2.0                                         # at least one valid pixel on every scale
    invs = [0.02 + torch.rand(B, 1, h, w, generator=gen) for h, w in sizes]
    for method in ("sparse-l1", "mse", "sparse-berhu", "sparse-silog", "abs_rel", "sparse-abs_rel"):
        for n in (1, 3, 4):
            loss, grads = _run(method, n, invs, depth)
            lr_, gr = _oracle(method, n, invs, depth)
            assert close(loss.reshape(1), lr_.reshape(1), 1e-5), (method, n, float(loss), float(lr_))
            for s in range(n):
                assert close(grads[s], gr[s], 1e-5), (method, n, s, rel_err(grads[s], gr[s]))


def test_empty_sparse_scale_gives_nan_and_zero_gradient():
    B, H, W = 2, 16, 24
    invs = [torch.rand(B, 1, H >> s, W >> s) + 0.1 for s in range(4)]
    for method in ("sparse-l1", "sparse-mse", "sparse-silog", "sparse-abs_rel", "sparse-berhu"):
        loss, grads = _run(method, 4, invs, torch.zeros(B, 1, H, W))
        assert torch.isnan(loss), method
        assert all(torch.equal(g, torch.zeros_like(g)) for g in grads), method
    # one empty scale among valid ones: NaN loss, zero gradient on that scale only, the others' gradients unchanged
    depth = torch.zeros(B, 1, H, W)
    depth[:, :, 1::2, 1::2] = 5.0                                   # never the nearest source of the halvings (even indices)
    loss, grads = _run("sparse-l1", 2, invs, depth)
    assert torch.isnan(loss) and torch.equal(grads[1], torch.zeros_like(grads[1]))
    _, g0 = _run("sparse-l1", 1, invs, depth)
    assert rel_err(grads[0], g0[0] / 2) <= 1e-6 and (grads[0] != 0).any()


def test_berhu_with_nonpositive_max_counts_every_pixel_twice():
    B, H, W = 2, 16, 24
    gen = torch.Generator().manual_seed(1)
    depth = 1 + torch.rand(B, 1, H, W, generator=gen)              # gt inverse depth in (0.5, 1]
    invs = [0.1 * torch.rand(B, 1, H >> s, W >> s, generator=gen) for s in range(2)]     # x - y < 0 everywhere
    loss, grads = _run("sparse-berhu", 2, invs, depth)
    lr_, gr = _oracle("sparse-berhu", 2, invs, depth)
    want = 0
    for s in range(2):
        d = (invs[s] + 1e-5 - so.nearest(so.depth2inv(depth), invs[s].shape[-2:])).abs().double()
        want = want + (d.sum() + (d * d).sum()) / (2 * d.numel())
    assert abs(float(loss) - float(want) / 2) <= 1e-5 * abs(float(want) / 2)
    assert rel_err(loss.reshape(1), lr_.reshape(1)) <= 1e-5
    for s in range(2):
        assert rel_err(grads[s], gr[s]) <= 1e-5


@pytest.mark.parametrize("case", [
    (2, (24, 40), [(6, 10), (3, 10), (12, 20)]),                   # ratios 4, (8, 4), 2
    (3, (21, 27), [(7, 9), (3, 9)]),                               # ratio 3: a float scale that is not a power of two
    (2, (10, 15), [(5, 5), (2, 3), (1, 1)]),                       # different ratios per axis, odd widths
    (8, (384, 1280), [(192, 640), (96, 320), (48, 160)]),          # the T8 halvings of upsample_depth_maps
])
def test_nearest_upsample_matches_torch(case):
    from mindtheedge_amd import kernels as K
    B, (H, W), sizes = case
    gen = torch.Generator().manual_seed(H * 100 + W)
    maps = [torch.rand(B, 1, h, w, generator=gen) for h, w in sizes]
    xs = [m.to(DEV).requires_grad_(True) for m in maps]
    ys = K.NearestUpsampleFn.apply(H, W, *xs)
    gys = [torch.randn(B, 1, H, W, generator=gen) for _ in maps]
    gx = torch.autograd.grad(ys, xs, [g.to(DEV) for g in gys])
    for m, y, g, d in zip(maps, ys, gys, gx):
        mr = m.clone().requires_grad_(True)
        yr = F.interpolate(mr, size=(H, W), mode="nearest")
        assert torch.equal(y.detach().cpu(), yr.detach())
        (dr,) = torch.autograd.grad(yr, mr, g)
        assert rel_err(d.cpu(), dr) <= 1e-6


def test_nearest_upsample_rejects_non_integer_ratios():
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd._lib import MteError
    with pytest.raises(MteError):
        K.NearestUpsampleFn.apply(20, 30, torch.rand(1, 1, 7, 10, device=DEV))


def test_two_runs_are_bit_identical_at_t8_shapes():
    B, H, W = 8, 384, 1280
    gen = torch.Generator().manual_seed(5)
    depth = ((torch.rand(B, 1, H, W, generator=gen) < 0.05).float() * (1 + 79 * torch.rand(B, 1, H, W, generator=gen))).to(DEV)
    invs = [(0.02 + torch.rand(B, 1, H >> s, W >> s, generator=gen)).to(DEV) for s in range(4)]
    for method in ("sparse-l1", "sparse-berhu", "sparse-silog", "abs_rel"):
        runs = [_run(method, 4, invs, depth) for _ in range(2)]
        assert torch.isfinite(runs[0][0]), method
        assert torch.equal(runs[0][0], runs[1][0]), method
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), method


class _StubNet(nn.Module):
    """a depth network that returns fixed inverse-depth maps"""

    def __init__(self, invs):
        super().__init__()
        self.invs = invs

    def forward(self, rgb=None, **kwargs):
        return {"inv_depths": list(self.invs)}


def _head(t="cross_entropy", weight=10.0):
    from mindtheedge_amd.losses.grad_loss import GradLoss
    return GradLoss(t, True, [], weight, 1.0)


@pytest.mark.parametrize("tag", ["plain", "up"])
def test_semisup_model_matches_reference(tag):
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    ref = load_golden("loss_supervised_model")
    invs = [ref["inv%d" % s].to(DEV).requires_grad_(True) for s in range(4)]
    batch = {k[len("batch."):]: v.to(DEV) for k, v in ref.items() if k.startswith("batch.")}
    m = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-l1", supervised_num_scales=4,
                         edges_depth_edge_loss_all_scales=True, upsample_depth_maps=(tag == "up"), flip_lr_prob=0.0)
    m.add_depth_net(_StubNet(invs))
    m.add_edge_loss(_head())
    m.train()
    out = m(dict(batch))
    if tag == "up":
        assert all(tuple(t.shape[-2:]) == tuple(invs[0].shape[-2:]) for t in out["inv_depths"])
    grads = torch.autograd.grad(out["loss"].sum(), invs)
    assert rel_err(out["metrics"]["supervised_loss"].cpu().reshape(1), ref[tag + ".supervised_loss"].reshape(1)) <= 1e-5
    assert rel_err(out["metrics"]["edge_loss"].cpu().reshape(1), ref[tag + ".edge_loss"].reshape(1)) <= 1e-5
    assert rel_err(out["loss"].detach().cpu().reshape(1), ref[tag + ".loss"].reshape(1)) <= 1e-5
    for s in range(4):
        assert rel_err(grads[s].cpu(), ref["%s.dinv%d" % (tag, s)]) <= 1e-4, (s, rel_err(grads[s].cpu(), ref["%s.dinv%d" % (tag, s)]))


@pytest.mark.parametrize("method", ["sparse-berhu", "sparse-l1"])
def test_graphed_step_with_upsampled_maps_equals_eager_steps(method):
    """Same state, same batches, same flip draws: replayed steps against eager steps with four-scale supervision on upsampled maps.  The
    first step agrees to 1e-5; later steps to 5e-4, as in test_gpu_graph_train.py: the weight-gradient tails add with fp32 atomics, and
    Adam at lr 1e-3 amplifies that order noise step by step."""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    from mindtheedge_amd.utils.graph import GraphedTrainStep
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    batches = [synthetic_batch(2, 64, 128, s, DEV) for s in (1, 2, 3)]
    try:
        K.set_compute_dtype("fp32")
        K.set_grad_sink(None)
        torch.manual_seed(3)
        net = PackNetSAN01(dropout=None, version="1A").cuda()
        model = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method=method,
                                 supervised_num_scales=4, edges_depth_edge_loss_all_scales=True, upsample_depth_maps=True,
                                 flip_lr_prob=0.5)
        model.add_depth_net(net)
        model.add_edge_loss(_head())
        model.train()
        opt = FusedAdam(FlatParameters(net.parameters()), lr=1e-3)
        step = GraphedTrainStep(model, opt, batches[0])
        assert step.graphed, step.error
        torch.cuda.synchronize()
        snap = (opt.flatp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.steps)

        def restore():
            opt.flatp.flat.copy_(snap[0]); opt.exp_avg.copy_(snap[1]); opt.exp_avg_sq.copy_(snap[2]); opt.steps = snap[3]
            K.bump_weights_epoch()
            K.prefetch_weight_packs()
            K.join_side_stream()
            torch.cuda.synchronize()

        restore()
        random.seed(11)
        eager = []
        static = step.batch
        for b in batches:
            flip = model.draw_flip()
            step.batch = b
            eager.append(float(step._eager(flip)["loss"].sum()))
        step.batch = static
        model._pinned_flip = None
        restore()
        random.seed(11)
        got = [float(step(b)["loss"].sum()) for b in batches]
        torch.cuda.synchronize()
        assert all(torch.isfinite(torch.tensor(got)))
        assert got[0] == pytest.approx(eager[0], rel=1e-5), (got, eager)
        for a, b in zip(got, eager):
            assert a == pytest.approx(b, rel=5e-4), (got, eager)
    finally:
        K.set_compute_dtype("bf16")


def test_train_edges_synthetic_with_sparse_l1_four_scales_upsampled(tmp_path, capsys):
    import importlib
    import sys
    import numpy as np
    with open(os.path.join(ROOT, "configs", "train_packnet_san_with_edges.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["datasets"]["augmentation"]["image_shape"] = [64, 128]
    cfg["datasets"]["train"]["batch_size"] = 2
    cfg.setdefault("model", {}).setdefault("depth_net", {})["checkpoint_path"] = ""
    cfg.setdefault("checkpoint", {})["filepath"] = ""
    cfg["model"]["loss"].update(supervised_method="sparse-l1", supervised_num_scales=4, upsample_depth_maps=True)
    path = os.path.join(tmp_path, "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    old = sys.argv
    sys.argv = ["train_edges.py", path, "--synthetic", "--steps", "2", "--epochs", "1"]
    try:
        importlib.import_module("train_edges").main()
    finally:
        sys.argv = old
        from mindtheedge_amd import kernels as K
        K.set_grad_sink(None)
        K.set_compute_dtype("bf16")
    out = capsys.readouterr().out
    assert "'steps': 2" in out
    hist = eval(out.strip().splitlines()[-1])
    assert len(hist) == 1 and np.isfinite(hist[0]["avg_loss"]) and hist[0]["avg_loss"] > 0
