"""CPU: the optimizer choices of config.model.optimizer (reference models/model_wrapper.py:142-180: getattr(torch.optim, name) with the
keys of config.model.optimizer.depth that the class accepts).

1. tests/optim_ref.py -- the float64 statements the GPU tests hold csrc/optim.hip to -- against a different implementation:
   torch.optim.Adam / AdamW / SGD on float64 CPU tensors over five steps, 1e-12 relative (float64 round-off).
2. ModelWrapper.configure_optimizers builds the fused optimizer of that name with the config's keys; what is not built raises."""
import itertools

import numpy as np
import pytest
import torch

import optim_ref as R

HYPERS = [(1e-4, 0.9, 0.999, 1e-8, 1.0), (3e-2, 0.5, 0.9, 1e-3, 1.0 / 3.0)]  # lr, beta1, beta2, eps, gscale
STEPS, N, TOL = 5, 257, 1e-12


def _f(s):
    return float(np.float32(s))


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(N, generator=g)
    grads = [torch.randn(N, generator=g) for _ in range(STEPS)]
    for x in grads:
        x[2::3] = 0.0
    return p0, grads


def _close(got, want, what):
    err = (got - want).abs()
    rel = float((err / want.abs().clamp(min=1e-300)).max())
    print("%s: max err / |torch| = %.3g" % (what, rel))
    assert bool((err <= TOL * want.abs()).all()), what


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("hi", [0, 1])
def test_adam_reference_is_torch_adam_and_adamw(hi, wd, decoupled):
    lr, b1, b2, eps, gscale = HYPERS[hi]
    p0, grads = _inputs(10 + hi)
    tp = torch.nn.Parameter(p0.double().clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=_f(lr), betas=(_f(b1), _f(b2)), eps=_f(eps), weight_decay=_f(wd))
    p, m, v = p0, torch.zeros(N), torch.zeros(N)
    for step, g in enumerate(grads, 1):
        tp.grad = g.double() * _f(gscale)
        opt.step()
        p, m, v, _ = R.adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale, wd, decoupled)
        st = opt.state[tp]
        _close(p, tp.detach(), "p step %d" % step)
        _close(m, st['exp_avg'], "m step %d" % step)
        _close(v, st['exp_avg_sq'], "v step %d" % step)
    assert p.dtype == torch.float64
    hyp = R.adam_hyper(lr, b1, b2, 3)
    assert hyp.dtype == torch.float32 and float(hyp[0]) == _f(lr) and float(hyp[1]) == _f(1.0 - _f(b1) ** 3)


SGD_CASES = [(mu, damp, nest) for mu, damp, nest in itertools.product([0.0, 0.9], [0.0, 0.1], [False, True])
             if not nest or (mu > 0 and damp == 0)]      # torch: Nesterov needs a momentum and zero dampening


@pytest.mark.parametrize("mu,damp,nest", SGD_CASES)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_sgd_reference_is_torch_sgd(wd, mu, damp, nest):
    lr, gscale = 3e-2, 1.0 / 3.0
    p0, grads = _inputs(20)
    tp = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([tp], lr=_f(lr), momentum=_f(mu), dampening=_f(damp), weight_decay=_f(wd), nesterov=nest)
    p, buf = p0, (torch.zeros(N) if mu else None)
    for step, g in enumerate(grads, 1):
        tp.grad = g.double() * _f(gscale)
        opt.step()
        p, buf, _ = R.sgd_step(p, g, buf, lr, mu, damp, wd, nest, step, gscale)
        _close(p, tp.detach(), "p step %d" % step)
        if mu:
            _close(buf, opt.state[tp]['momentum_buffer'], "buf step %d" % step)
        else:
            assert buf is None and 'momentum_buffer' not in opt.state_dict()['state'].get(0, {})
    assert R.sgd_hyper(lr, mu, damp, 1).tolist() == [_f(lr), 0.0, 1.0]
    assert R.sgd_hyper(lr, mu, damp, 2).tolist() == [_f(lr), _f(mu), _f(1.0 - _f(damp))]


# ---- configure_optimizers ---------------------------------------------------------------------------------------------------------------------
def _wrapper(optimizer):
    """a CPU ModelWrapper as tests/test_checkpoint_format.py builds one, with another model.optimizer block"""
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    cfg = {"model": {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                              "edges_depth_edge_loss_all_scales": True, "flip_lr_prob": 0.0},
                     "depth_net": {"dropout": 0.0}, "optimizer": optimizer}}
    return ModelWrapper(load_config(None, cfg))


def _torch_keys(cls, **kw):
    """group keys of the torch class over a dummy parameter with a StepLR attached (the scheduler adds 'initial_lr'), plus 'name'"""
    opt = cls([{'params': [torch.nn.Parameter(torch.zeros(2))], 'name': 'Depth'}], **kw)
    torch.optim.lr_scheduler.StepLR(opt, step_size=10)
    return set(opt.param_groups[0]), set(opt.state_dict()['param_groups'][0])


@pytest.mark.parametrize("name,decoupled", [("Adam", False), ("AdamW", True)])
def test_configure_optimizers_adam_with_weight_decay(name, decoupled):
    from mindtheedge_amd.trainers.data_parallel import FusedAdam
    w = _wrapper({"name": name, "depth": {"lr": 1e-4, "weight_decay": 1e-4}})
    opt, _ = w.configure_optimizers()
    assert type(opt) is FusedAdam
    live, saved = opt.param_groups[0], opt.state_dict()['param_groups'][0]
    for group in (live, saved):
        assert group['weight_decay'] == 1e-4 and group['decoupled_weight_decay'] is decoupled
        assert group['lr'] == 1e-4 and tuple(group['betas']) == (0.9, 0.999) and group['eps'] == 1e-8 and group['name'] == 'Depth'
        assert group['amsgrad'] is False and group['maximize'] is False
    want_live, want_saved = _torch_keys(getattr(torch.optim, name))
    assert set(live) == want_live and set(saved) == want_saved
    assert saved['params'] == list(range(288)) and opt.state_dict()['state'] == {}


def test_configure_optimizers_adamw_takes_the_configs_default_weight_decay():
    """as upstream: the config's weight_decay (default 0.0) reaches AdamW, not torch's own default of 0.01"""
    opt, _ = _wrapper({"name": "AdamW", "depth": {"lr": 1e-4}}).configure_optimizers()
    assert opt.param_groups[0]['weight_decay'] == 0.0 and opt.param_groups[0]['decoupled_weight_decay'] is True


def test_configure_optimizers_sgd_with_momentum():
    from mindtheedge_amd.trainers.data_parallel import FusedSGD
    w = _wrapper({"name": "SGD", "depth": {"lr": 1e-2, "momentum": 0.9, "nesterov": True, "weight_decay": 1e-4, "betas": [0.5, 0.9]}})
    opt, sched = w.configure_optimizers()
    assert type(opt) is FusedSGD and isinstance(sched, torch.optim.lr_scheduler.StepLR)
    live, saved = opt.param_groups[0], opt.state_dict()['param_groups'][0]
    for group in (live, saved):
        assert group['momentum'] == 0.9 and group['nesterov'] is True and group['dampening'] == 0 and group['weight_decay'] == 1e-4
        assert group['lr'] == 1e-2 and group['name'] == 'Depth' and 'betas' not in group       # betas: no key of torch.optim.SGD
    want_live, want_saved = _torch_keys(torch.optim.SGD, lr=1e-2)
    assert set(live) == want_live and set(saved) == want_saved
    assert opt.state_dict()['state'] == {} and opt.momentum_buffer.numel() == opt.flatp.flat.numel()


@pytest.mark.parametrize("optimizer", [{"name": "RMSprop", "depth": {"lr": 1e-4}},
                                       {"name": "Adam", "depth": {"lr": 1e-4, "amsgrad": True}},
                                       {"name": "AdamW", "depth": {"lr": 1e-4, "maximize": True}},
                                       {"name": "SGD", "depth": {"lr": 1e-4, "maximize": True}}])
def test_what_is_not_built_raises(optimizer):
    w = _wrapper(optimizer)
    with pytest.raises(NotImplementedError, match="Adam.*AdamW.*SGD"):
        w.configure_optimizers()


def test_fused_optimizers_have_no_cpu_step():
    """no CPU fallback: a step on host buffers raises, for every class and variant"""
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    for build in (lambda f: FusedAdam(f), lambda f: FusedAdam(f, weight_decay=0.01), lambda f: FusedAdam(f, weight_decay=0.01, decoupled_weight_decay=True),
                  lambda f: FusedSGD(f), lambda f: FusedSGD(f, momentum=0.9)):
        opt = build(FlatParameters([torch.nn.Parameter(torch.ones(5))]))
        with pytest.raises(MteError):
            opt.step()


def _same_state(a, b, keys):
    sa, sb = a.state_dict()['state'], b.state_dict()['state']
    return set(sa) == set(sb) and all(set(sa[i]) == set(keys) and torch.equal(sa[i][k], sb[i][k]) for i in sa for k in keys)


def test_state_dict_layouts_load_into_torch_and_back():
    """each class writes the layout of its torch class (state filled by hand here: the step itself needs the GPU) and reads it back, also from
    a torch-written file whose group names other hyper-parameters"""
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedSGD
    shapes = [(3,), (5, 7), (1,), (64,)]
    params = lambda: [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    g = torch.Generator().manual_seed(3)

    sgd = FusedSGD(FlatParameters(params()), lr=1e-2, momentum=0.9, weight_decay=1e-3)
    assert sgd.state_dict()['state'] == {}
    sgd.momentum_buffer.copy_(torch.randn(sgd.momentum_buffer.shape, generator=g))
    sgd.steps = 4
    sd = sgd.state_dict()
    assert set(sd['state']) == {0, 1, 2, 3} and set(sd['state'][1]) == {'momentum_buffer'} and sd['state'][1]['momentum_buffer'].shape == (5, 7)
    ref = torch.optim.SGD([{'params': params(), 'name': 'Depth'}], lr=0.5)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]['momentum'] == 0.9 and ref.param_groups[0]['weight_decay'] == 1e-3 and ref.param_groups[0]['lr'] == 1e-2
    fresh = FusedSGD(FlatParameters(params()), lr=0.5)                 # momentum 0: no buffer until the file asks for one
    assert fresh.momentum_buffer is None and fresh.state_dict()['state'] == {}
    fresh.load_state_dict(ref.state_dict())
    assert fresh.steps == 1 and _same_state(fresh, sgd, ['momentum_buffer'])
    assert fresh.param_groups[0]['momentum'] == 0.9 and fresh.param_groups[0]['weight_decay'] == 1e-3 and fresh.param_groups[0]['lr'] == 1e-2
    assert FusedSGD(FlatParameters(params()), lr=0.5).state_dict()['param_groups'][0]['momentum'] == 0

    adam = FusedAdam(FlatParameters(params()), lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)
    adam.exp_avg.copy_(torch.randn(adam.exp_avg.shape, generator=g))
    adam.exp_avg_sq.copy_(torch.rand(adam.exp_avg_sq.shape, generator=g))
    adam.steps = 7
    ref = torch.optim.AdamW([{'params': params(), 'name': 'Depth'}])
    ref.load_state_dict(adam.state_dict())
    assert ref.param_groups[0]['weight_decay'] == 0.01 and ref.param_groups[0]['decoupled_weight_decay'] is True
    fresh = FusedAdam(FlatParameters(params()))
    fresh.load_state_dict(ref.state_dict())
    assert fresh.steps == 7 and _same_state(fresh, adam, ['step', 'exp_avg', 'exp_avg_sq'])
    assert fresh.param_groups[0]['weight_decay'] == 0.01 and fresh.param_groups[0]['decoupled_weight_decay'] is True
    # the flat layout of earlier builds keeps loading
    legacy = FusedAdam(FlatParameters(params()))
    legacy.load_state_dict({'steps': 7, 'exp_avg': adam.exp_avg.clone(), 'exp_avg_sq': adam.exp_avg_sq.clone()})
    assert legacy.steps == 7 and _same_state(legacy, adam, ['step', 'exp_avg', 'exp_avg_sq']) and legacy.param_groups[0]['weight_decay'] == 0.0


class _ToyWrapper(torch.nn.Module):
    """what save_checkpoint reads of a ModelWrapper: config, current_epoch, state_dict(), optimizer, scheduler"""

    def __init__(self, build):
        from mindtheedge_amd.trainers.data_parallel import FlatParameters
        super().__init__()
        torch.manual_seed(0)
        self.net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.GroupNorm(1, 5), torch.nn.Conv2d(5, 2, 1))
        self.config, self.current_epoch = {'arch': {'seed': 42}}, 2
        self.optimizer = build(FlatParameters(self.net.parameters()))
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=2, gamma=0.5)


@pytest.mark.parametrize("kind", ["sgd_momentum", "sgd_plain", "adamw"])
def test_checkpoint_file_round_trip_for_every_optimizer(tmp_path, kind):
    """save_checkpoint writes whatever state the optimizer keeps (SGD: momentum_buffer, no step; plain SGD: none; Adam / AdamW: step and two
    moments) as host tensors; load_checkpoint + load_state_dict of a fresh optimizer restore it (state filled by hand: the step needs the GPU)"""
    from mindtheedge_amd.models.model_checkpoint import save_checkpoint, load_checkpoint
    from mindtheedge_amd.trainers.data_parallel import FusedAdam, FusedSGD
    build = {"sgd_momentum": lambda f: FusedSGD(f, lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=1e-3),
             "sgd_plain": lambda f: FusedSGD(f, lr=1e-2, weight_decay=1e-3),
             "adamw": lambda f: FusedAdam(f, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)}[kind]
    keys = {"sgd_momentum": ['momentum_buffer'], "sgd_plain": [], "adamw": ['step', 'exp_avg', 'exp_avg_sq']}[kind]
    w = _ToyWrapper(build)
    g = torch.Generator().manual_seed(4)
    for _, b in w.optimizer.state_buffers():
        b.copy_(torch.rand(b.shape, generator=g))
    w.optimizer.steps = 3
    path = save_checkpoint(str(tmp_path / "epoch=2.ckpt"), w)
    ckpt = load_checkpoint(path)
    assert ckpt['epoch'] == 2 and set(ckpt['state_dict']) == set(w.state_dict())
    state = ckpt['optimizer']['state']
    assert len(state) == (6 if keys else 0)
    assert all(set(st) == set(keys) and all(st[k].device.type == 'cpu' for k in keys) for st in state.values())
    fresh = _ToyWrapper({"adamw": lambda f: FusedAdam(f)}.get(kind, lambda f: FusedSGD(f, lr=0.5)))
    fresh.optimizer.load_state_dict(ckpt['optimizer'])
    fresh.scheduler.load_state_dict(ckpt['scheduler'])
    assert _same_state(fresh.optimizer, w.optimizer, keys) if keys else fresh.optimizer.state_dict()['state'] == {}
    assert fresh.optimizer.steps == {"sgd_momentum": 1, "sgd_plain": 0, "adamw": 3}[kind]
    live, want = fresh.optimizer.param_groups[0], w.optimizer.param_groups[0]
    assert all(live[k] == want[k] for k in want if k != 'params')


def test_flat_legacy_layout_is_adam_only():
    """the flat {'steps', 'exp_avg', 'exp_avg_sq'} layout was written by builds that had Adam only: FusedSGD refuses it"""
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedSGD
    opt = FusedSGD(FlatParameters([torch.nn.Parameter(torch.zeros(5))]), momentum=0.9)
    with pytest.raises(ValueError, match="torch's optimizer layout"):
        opt.load_state_dict({'steps': 3, 'momentum_buffer': torch.zeros(64)})


def test_fused_sgd_forms_its_coefficients_like_the_entry_point():
    """hyper = what optim_ref.sgd_hyper (and mte_sgd_step) form from the float32 dampening, also where the double's 1 - dampening
    rounds to another float32"""
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedSGD
    for damp in (0.6, 0.65, 0.8, 0.1, 0.0):
        opt = FusedSGD(FlatParameters([torch.nn.Parameter(torch.zeros(5))]), lr=3e-2, momentum=0.9, dampening=damp)
        for step in (1, 2, 3):
            opt.advance()
            assert opt.steps == step and torch.equal(opt.hyper, R.sgd_hyper(3e-2, 0.9, damp, step)), (damp, step)
    assert _f(1.0 - 0.6) != _f(1.0 - _f(0.6))                  # 0.6 is such a value
