"""CPU: gradient-norm clipping and the non-finite step guard, the parts that need no GPU.
1. tests/clip_ref.py (the float64 statement the GPU tests hold mte_grad_norm_clip to) against torch.nn.utils.clip_grad_norm_ on float64
   copies split into several tensors.
2. Configuration routing: model.optimizer.clip_grad_norm / skip_nonfinite_steps reach FusedAdam / FusedSGD; the defaults build an
   optimizer without a `ctl`; neither key enters the optimizer's param_groups or its state_dict()."""
import math

import numpy as np
import pytest
import torch

import clip_ref as C


def _split(g, sizes):
    out, o = [], 0
    for s in sizes:
        out.append(g[o:o + s])
        o += s
    assert o == g.numel()
    return out


# ---- 1. the reference is torch's rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.25, 1.0 / 3.0])
@pytest.mark.parametrize("max_norm", [0.5, 7.0, 1e6, float("inf")])
@pytest.mark.parametrize("n", [1, 7, 1027, 10000])
def test_clip_ref_is_torch_clip_grad_norm(n, max_norm, gscale):
    """norm and coefficient against clip_grad_norm_ on float64 copies of the scaled gradient, split into several tensors: 1e-12 relative.
    Both sides are fp64 sums of at most 1e4 non-negative terms in different orders (n * 2^-53 = 1.1e-12 at the largest n, relative to a
    sum without cancellation; the square root halves it).  The coefficient is read off the clipped tensors: grad_after / grad_before."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(100 + n))
    r = C.grad_norm_clip(g, gscale, max_norm)
    gs = float(np.float32(gscale))
    sizes = [n] if n < 4 else [n // 3, 1, n - n // 3 - 1]
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in sizes]
    for p, part in zip(params, _split(g.double() * gs, sizes)):
        p.grad = part.clone()
    before = [p.grad.clone() for p in params]
    total = float(torch.nn.utils.clip_grad_norm_(params, float(np.float32(max_norm))))
    assert abs(r["norm"] - total) <= 1e-12 * total
    big = max(range(len(params)), key=lambda i: float(before[i].abs().max()))
    j = int(before[big].abs().argmax())
    coef = float(params[big].grad[j] / before[big][j])
    assert abs(r["coef"] - coef) <= 1e-12 * coef                         # (the product and the quotient read back round twice more: 2^-52)
    assert r["coef"] <= 1.0 and (r["coef"] == 1.0) == (total + 1e-6 <= float(np.float32(max_norm)))
    if math.isinf(max_norm):
        assert r["coef"] == 1.0


@pytest.mark.parametrize("bad,max_norm", [(float("inf"), 2.0), (float("-inf"), 2.0), (float("nan"), 2.0), (float("inf"), float("inf")),
                                          (float("nan"), float("inf"))])
def test_clip_ref_non_finite_is_torch(bad, max_norm):
    """an inf in the gradient gives coefficient 0 (NaN when max_norm is inf as well), a NaN gives NaN, as torch"""
    g = torch.ones(9)
    g[4] = bad
    r = C.grad_norm_clip(g, 1.0, max_norm)
    p = torch.nn.Parameter(torch.zeros(9, dtype=torch.float64))
    p.grad = g.double().clone()
    total = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    coef = float(p.grad[0])                                               # 1.0 * coefficient
    assert (math.isnan(total) and math.isnan(r["norm"])) or total == r["norm"]
    assert (math.isnan(coef) and math.isnan(r["coef"])) or coef == r["coef"]
    if math.isinf(bad) and not math.isinf(max_norm):
        assert r["coef"] == 0.0
    else:
        assert math.isnan(r["coef"])
    assert not np.isfinite(r["S"])
    assert C.ctl(g, 1.0, max_norm, True, 2.0)[1] == 1.0 and C.ctl(g, 1.0, max_norm, True, 2.0)[3] == 3.0
    assert C.ctl(g, 1.0, max_norm, False, 2.0)[1] == 0.0 and C.ctl(g, 1.0, max_norm, False, 2.0)[3] == 2.0


# ---- 2. configuration routing ------------------------------------------------------------------------------------------------------------------------
def _wrapper(optimizer):
    """a CPU ModelWrapper as tests/test_optimizer_family_cpu.py builds one"""
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    cfg = {"model": {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                              "edges_depth_edge_loss_all_scales": True, "flip_lr_prob": 0.0},
                     "depth_net": {"dropout": 0.0}, "optimizer": optimizer}}
    return ModelWrapper(load_config(None, cfg))


def test_config_defaults_are_off():
    from mindtheedge_amd.utils.config import default_config, load_config
    for cfg in (default_config(), load_config(None, {"model": {"optimizer": {"name": "SGD"}}})):
        assert cfg.model.optimizer.clip_grad_norm == 0.0 and cfg.model.optimizer.skip_nonfinite_steps is False
        assert "clip_grad_norm" not in cfg.model.optimizer.depth and "skip_nonfinite_steps" not in cfg.model.optimizer.depth


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
def test_default_config_builds_an_optimizer_without_ctl(name):
    opt, _ = _wrapper({"name": name, "depth": {"lr": 1e-4}}).configure_optimizers()
    assert opt.clip_grad_norm == 0.0 and opt.skip_nonfinite is False
    assert getattr(opt, "ctl", None) is None and getattr(opt, "_norm_work", None) is None


@pytest.mark.parametrize("name,block", [("Adam", {"clip_grad_norm": 10.0}), ("AdamW", {"skip_nonfinite_steps": True}),
                                        ("SGD", {"clip_grad_norm": 0.5, "skip_nonfinite_steps": True})])
def test_the_keys_reach_the_fused_optimizers_and_stay_out_of_the_checkpoint(name, block):
    from mindtheedge_amd.trainers.data_parallel import FusedAdam, FusedSGD
    depth = {"lr": 1e-4, "weight_decay": 1e-4, **({"momentum": 0.9} if name == "SGD" else {})}
    opt, _ = _wrapper({"name": name, "depth": depth, **block}).configure_optimizers()
    assert type(opt) is (FusedSGD if name == "SGD" else FusedAdam)
    assert opt.clip_grad_norm == block.get("clip_grad_norm", 0.0) and opt.skip_nonfinite is block.get("skip_nonfinite_steps", False)
    assert opt.ctl.shape == (4,) and opt.ctl.dtype == torch.float32 and not bool(opt.ctl.any())
    tcls = getattr(torch.optim, name)
    t = tcls([{'params': [torch.nn.Parameter(torch.zeros(2))], 'name': 'Depth'}], lr=1e-4)
    torch.optim.lr_scheduler.StepLR(t, step_size=10)
    live, saved = opt.param_groups[0], opt.state_dict()['param_groups'][0]
    assert set(live) == set(t.param_groups[0]) and set(saved) == set(t.state_dict()['param_groups'][0])
    for group in (live, saved):
        assert not any("clip" in k or "nonfinite" in k for k in group)
    assert opt.param_groups[0]["weight_decay"] == 1e-4 and opt.param_groups[0]["lr"] == 1e-4


def test_the_shipped_clip_yaml_switches_both_on():
    import os
    from mindtheedge_amd.utils.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "train_packnet_san_kitti_with_edges_clip.yaml"))
    assert cfg.model.optimizer.clip_grad_norm == 10.0 and cfg.model.optimizer.skip_nonfinite_steps is True
    assert cfg.model.optimizer.name == "AdamW" and dict(cfg.model.optimizer.depth) == {"lr": 0.0001, "weight_decay": 0.01}


@pytest.mark.parametrize("bad", [-1.0, -1e-9, float("nan")])
def test_a_negative_clip_grad_norm_raises(bad):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            cls(FlatParameters([torch.nn.Parameter(torch.ones(5))]), clip_grad_norm=bad)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _wrapper({"name": "Adam", "depth": {"lr": 1e-4}, "clip_grad_norm": bad}).configure_optimizers()


def test_clipping_optimizers_have_no_cpu_step_either():
    """no CPU fallback: the clipped step on host buffers raises like the plain one"""
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    for cls in (FusedAdam, FusedSGD):
        opt = cls(FlatParameters([torch.nn.Parameter(torch.ones(5))]), clip_grad_norm=1.0, skip_nonfinite=True)
        with pytest.raises(MteError):
            opt.step()
