"""CPU: the weight EMA's reference (tests/ema_ref.py) against its closed form, the decay schedule, the configuration and constructor
defaults, and load_network's choice between a file's raw and averaged weights.

Closed form.  For constant weights p the exact recursion e_t = d_t e_(t-1) + (1 - d_t) p gives e_t = p + (e0 - p) * prod d_i.  The float32
recursion rounds three times per update (two products, one sum), each by at most 2^-24 relative to a value no larger than
max(|e0|, |p|) (the average stays between e0 and p); later updates only shrink an earlier error (d_t < 1).  omd32 = float32(1 - d32)
differs from 1 - d32 by at most 2^-25 relative to 1 - d32 <= 1, a fourth error of the same size, so the bound t * 2^-22 * max(|e0|, |p|)
(four times 2^-24 per update) covers it."""
import math
import os

import numpy as np
import pytest
import torch

import ema_ref as E


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_run_follows_the_closed_form_for_constant_weights(decay, warmup):
    rng = np.random.default_rng(7)
    n, T = 513, 200
    e0 = rng.standard_normal(n).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    worst = 0.0
    for t in (1, 2, 9, 50, T):
        got = E.run(e0, [p] * t, decay, warmup).astype(np.float64)
        prod = 1.0
        for i in range(1, t + 1):
            prod *= float(E.decay_pair(i, decay, warmup)[0])
        want = p.astype(np.float64) + (e0.astype(np.float64) - p.astype(np.float64)) * prod
        bound = t * 2.0 ** -22 * np.maximum(np.abs(e0), np.abs(p)).astype(np.float64)
        err = np.abs(got - want)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (decay, warmup, t)
    print("closed form, decay %g warmup %s: worst error / bound = %.3g" % (decay, warmup, worst))


def test_a_skipped_step_leaves_the_average_and_advances_t():
    rng = np.random.default_rng(3)
    e0 = rng.standard_normal(17).astype(np.float32)
    snaps = [rng.standard_normal(17).astype(np.float32) for _ in range(4)]
    got = E.run(e0, snaps, 0.9, True, skipped=(3,))
    want = e0
    for t in (1, 2, 4):
        want = E.update(want, snaps[t - 1], *E.decay_pair(t, 0.9, True))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not np.array_equal(got, E.run(e0, snaps, 0.9, True))


def test_the_decay_schedule():
    d1, omd1 = E.decay_pair(1, 0.999, True)
    assert d1 == np.float32(2.0 / 11.0) and omd1 == np.float32(1.0 - float(np.float32(2.0 / 11.0)))
    assert isinstance(d1, np.float32) and isinstance(omd1, np.float32)
    top = np.float32(0.999)
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990: the warm-up meets the decay exactly there and the decay holds afterwards
    assert (1.0 + 8989) / (10.0 + 8989) < 0.999 and (1.0 + 8990) / (10.0 + 8990) >= 0.999
    assert E.decay_pair(8989, 0.999, True)[0] < top
    first = min(t for t in range(8900, 9100) if (1.0 + t) / (10.0 + t) >= 0.999)
    assert first == 8990
    for t in (8990, 8991, 10 ** 4, 10 ** 6):
        assert E.decay_pair(t, 0.999, True) == (top, np.float32(1.0 - float(top)))
    last = 0.0
    for t in range(1, 8990):
        d = (1.0 + t) / (10.0 + t)
        assert last < d < 0.999
        last = d
    for t in (1, 5, 10 ** 6):
        assert E.decay_pair(t, 0.999, False) == (top, np.float32(1.0 - float(top)))


def test_the_optimizer_forms_the_reference_pair():
    from mindtheedge_amd.trainers.data_parallel import ema_decay_pair
    for decay in (0.9, 0.999, 0.5):
        for warmup in (True, False):
            for t in (1, 2, 3, 7, 80, 8989, 8990, 8991, 10 ** 6):
                d, omd = ema_decay_pair(t, decay, warmup)
                rd, romd = E.decay_pair(t, decay, warmup)
                assert np.float32(d) == rd and float(np.float32(d)) == d
                assert np.float32(omd) == romd and float(np.float32(omd)) == omd


def test_config_defaults_are_off():
    from mindtheedge_amd.utils.config import load_config
    cfg = load_config(None, {})
    opt = cfg.model.optimizer
    assert opt.ema_decay == 0.0 and opt.ema_warmup is True and opt.ema_validate is True
    assert cfg.model.checkpoint_ema is False and cfg.model.depth_net.checkpoint_ema is False
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "train_packnet_san_kitti_with_edges_ema.yaml")) as f:
        shipped = yaml.safe_load(f)
    assert shipped["model"]["optimizer"]["ema_decay"] == 0.999 and shipped["checkpoint"]["save_top_k"] == 3
    assert load_config(None, shipped).model.optimizer.ema_decay == 0.999
    # the keys sit beside `name`, not under `depth`: filter_args never hands them to torch.optim
    from mindtheedge_amd.utils.load import filter_args
    assert not any(k.startswith("ema") for k in filter_args(torch.optim.Adam, cfg.model.optimizer.depth))


def _params():
    return [torch.nn.Parameter(torch.arange(5.0)), torch.nn.Parameter(torch.ones(3, 4))]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_constructor_rejects_bad_decays_and_the_default_has_no_buffer(kind):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    build = (lambda f, **kw: FusedAdam(f, lr=1e-3, **kw)) if kind == "adam" else (lambda f, **kw: FusedSGD(f, lr=1e-2, momentum=0.9, **kw))
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            build(FlatParameters(_params()), ema_decay=bad)
    for extra in ({}, dict(ema_decay=0), dict(ema_decay=0.0, ema_warmup=False)):
        opt = build(FlatParameters(_params()), **extra)
        assert not hasattr(opt.flatp, "ema") and not hasattr(opt, "ema_scal") and opt.ema_decay == 0.0 and opt.hyper.numel() == 3
        assert set(opt.state_dict()) == {"state", "param_groups"}
        with pytest.raises(RuntimeError, match="ema_decay"):
            with opt.ema_weights():
                pass
    flat = FlatParameters(_params())
    opt = build(flat, ema_decay=0.99, ema_warmup=False)
    assert flat.ema.shape == flat.flat.shape and flat.ema.data_ptr() != flat.flat.data_ptr()
    assert torch.equal(flat.ema.view(torch.int32), flat.flat.view(torch.int32))
    assert opt.ema_state() == {"decay": 0.99, "warmup": False, "num_updates": 0} and opt.hyper.numel() == 3 and opt.ema_scal.numel() == 2
    assert not any("ema" in k for k in opt.state_dict()["param_groups"][0]) and set(opt.state_dict()) == {"state", "param_groups"}


def test_load_ema_fills_the_average_through_the_index_space():
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    flat = FlatParameters(net.parameters())
    opt = FusedAdam(flat, ema_decay=0.9)
    names = [n for n, _ in net.named_parameters()]
    opt.set_index_space(names, dict(net.named_parameters()))
    before = flat.flat.clone()
    named = {n: torch.full_like(p, float(i + 1)) for i, (n, p) in enumerate(net.named_parameters()) if n != "1.bias"}
    opt.load_ema(named, 41)
    assert opt.ema_state()["num_updates"] == 41 and torch.equal(flat.flat, before)
    got = {id(p): v for p, v in zip(flat.params, (opt.ema_named()[id(p)] for p in flat.params))}
    for i, (n, p) in enumerate(net.named_parameters()):
        want = named.get(n, p.data)                                     # a tensor the dictionary does not name keeps the weights' copy
        assert torch.equal(got[id(p)], want), n
    with pytest.raises(ValueError, match="shape"):
        opt.load_ema({"0.weight": torch.zeros(2, 2)}, 0)


def test_ema_weights_on_host_buffers_swaps_and_restores_and_refuses_an_open_group():
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedSGD
    params = _params()
    flat = FlatParameters(params)
    opt = FusedSGD(flat, lr=1e-2, ema_decay=0.9, accumulate_grad_batches=2)
    flat.ema.mul_(3.0)
    raw, avg = flat.flat.clone(), flat.ema.clone()
    with opt.ema_weights():
        assert torch.equal(flat.flat, avg) and torch.equal(flat.ema, raw) and torch.equal(params[0].data, 3.0 * torch.arange(5.0))
    assert torch.equal(flat.flat, raw) and torch.equal(flat.ema, avg) and torch.equal(params[0].data, torch.arange(5.0))
    opt._pending = 1
    with pytest.raises(RuntimeError, match="accumulation group"):
        with opt.ema_weights():
            pass
    assert torch.equal(flat.flat, raw) and torch.equal(flat.ema, avg)


def test_load_network_picks_the_raw_or_the_averaged_weights(tmp_path):
    from mindtheedge_amd.utils.load import load_network
    net = torch.nn.Linear(3, 2)
    raw = {"model.depth_net.weight": torch.full((2, 3), 1.0), "model.depth_net.bias": torch.full((2,), 2.0)}
    avg = {"model.depth_net.weight": torch.full((2, 3), 5.0), "model.depth_net.bias": torch.full((2,), 6.0)}
    both, plain = os.path.join(tmp_path, "both.ckpt"), os.path.join(tmp_path, "plain.ckpt")
    torch.save({"state_dict": raw, "state_dict_ema": avg, "ema": {"decay": 0.9, "warmup": True, "num_updates": 3}}, both)
    torch.save({"state_dict": raw}, plain)
    load_network(net, both, ["depth_net"], ema=True)
    assert float(net.weight.data[0, 0]) == 5.0 and float(net.bias.data[0]) == 6.0
    load_network(net, both, ["depth_net"], ema=False)
    assert float(net.weight.data[0, 0]) == 1.0 and float(net.bias.data[0]) == 2.0
    load_network(net, both, ["depth_net"])
    assert float(net.weight.data[0, 0]) == 1.0
    with pytest.raises(KeyError, match="state_dict_ema"):
        load_network(net, plain, ["depth_net"], ema=True)
    load_network(net, plain, ["depth_net"])
    assert float(net.weight.data[0, 0]) == 1.0 and math.isclose(float(net.bias.data[1]), 2.0)
