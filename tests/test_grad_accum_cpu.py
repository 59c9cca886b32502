"""CPU: gradient accumulation over micro-batches (FusedFlatOptimizer(accumulate_grad_batches=k), Trainer, arch.accumulate_grad_batches).
1. trainers/trainer.py::accumulation_groups and the trainer's group ends, with and without a loader length.
2. Configuration routing: the default is 1 and builds an optimizer without a second gradient buffer; a YAML value reaches the optimizer.
3. Misuse raises.
4. World 2 over gloo on host buffers, in the pattern of tests/test_data_parallel_cpu.py: nothing is reduced under no_sync(), the last
   micro-batch's buckets each take the accumulated gradient once and are reduced once, and the result is the exact integer sum.
5. tests/accum_ref.py (the reference of the GPU tests) checks itself on hand-computed elements."""
import os
import socket

import pytest
import torch

import accum_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. grouping ---------------------------------------------------------------------------------------------------------------------------------------
def test_accumulation_groups():
    from mindtheedge_amd.trainers.trainer import accumulation_groups
    assert accumulation_groups(5, 2) == [2, 2, 1]
    assert accumulation_groups(4, 4) == [4]
    assert accumulation_groups(3, 8) == [3]
    assert accumulation_groups(0, 2) == []
    for n in (0, 1, 7):
        assert accumulation_groups(n, 1) == [1] * n
    for n in range(0, 20):
        for k in range(1, 7):
            sizes = accumulation_groups(n, k)
            assert sum(sizes) == n and all(s == k for s in sizes[:-1]) and all(1 <= s <= k for s in sizes)
    with pytest.raises(ValueError):
        accumulation_groups(5, 0)


@pytest.mark.parametrize("n,k", [(5, 2), (4, 4), (3, 8), (0, 2), (6, 1), (7, 3)])
def test_the_trainers_group_ends_are_those_groups_with_and_without_a_length(n, k):
    from mindtheedge_amd.trainers.trainer import _with_group_end, accumulation_groups
    want = [j == size - 1 for size in accumulation_groups(n, k) for j in range(size)]
    assert [last for _, last in _with_group_end(list(range(n)), k)] == want
    assert [last for _, last in _with_group_end((i for i in range(n)), k)] == want          # a generator has no len(): read one ahead
    assert [b for b, _ in _with_group_end((i for i in range(n)), k)] == list(range(n))


# ---- 2. configuration routing ------------------------------------------------------------------------------------------------------------------------
def _wrapper(arch=None):
    """a CPU ModelWrapper as tests/test_optimizer_family_cpu.py builds one"""
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.utils.config import load_config
    cfg = {"model": {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                              "edges_depth_edge_loss_all_scales": True, "flip_lr_prob": 0.0},
                     "depth_net": {"dropout": 0.0}, "optimizer": {"name": "AdamW", "depth": {"lr": 1e-4}}}}
    if arch is not None:
        cfg["arch"] = arch
    return ModelWrapper(load_config(None, cfg))


def test_the_config_default_is_one_and_builds_no_second_buffer():
    from mindtheedge_amd.utils.config import default_config, load_config
    for cfg in (default_config(), load_config(None, {"arch": {"max_epochs": 3}})):
        assert cfg.arch.accumulate_grad_batches == 1
    opt, _ = _wrapper().configure_optimizers()
    assert opt.accumulate_grad_batches == 1 and opt.flatp.accum is None
    assert not any("accum" in k for k in opt.state_dict()["param_groups"][0])


def test_a_yaml_value_reaches_the_optimizer_and_the_trainer():
    from mindtheedge_amd.trainers.trainer import Trainer
    from mindtheedge_amd.utils.config import load_config
    w = _wrapper({"accumulate_grad_batches": 4})
    opt, _ = w.configure_optimizers()
    assert opt.accumulate_grad_batches == 4
    assert opt.flatp.accum.shape == opt.flatp.grad.shape and opt.flatp.accum.dtype == torch.float32
    assert opt.flatp.accum.data_ptr() != opt.flatp.grad.data_ptr()
    assert not any("accum" in k for k in opt.state_dict()["param_groups"][0]) and "accum" not in opt.state_dict()
    assert Trainer(**w.config.arch).accumulate_grad_batches == 4 and Trainer().accumulate_grad_batches is None
    cfg = load_config(os.path.join(ROOT, "configs", "train_packnet_san_kitti_with_edges_accum.yaml"))
    assert cfg.arch.accumulate_grad_batches == 8
    assert cfg.model.optimizer.clip_grad_norm == 10.0 and cfg.model.optimizer.skip_nonfinite_steps is True and cfg.model.optimizer.name == "AdamW"


def test_a_trainers_own_value_reaches_the_optimizer():
    """Trainer.fit attaches itself to the module before it asks for the optimizer"""
    from mindtheedge_amd.trainers.trainer import Trainer
    w = _wrapper()
    w.trainer = Trainer(accumulate_grad_batches=2)
    opt, _ = w.configure_optimizers()
    assert opt.accumulate_grad_batches == 2 and opt.flatp.accum is not None


# ---- 3. misuse -------------------------------------------------------------------------------------------------------------------------------------------
def _small(cls, **kw):
    from mindtheedge_amd.trainers.data_parallel import FlatParameters
    params = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3, 4))]
    return params, cls(FlatParameters(params), **kw)


@pytest.mark.parametrize("bad", [0, -1, 1.5])
def test_a_group_size_below_one_raises(bad):
    from mindtheedge_amd.trainers.data_parallel import FusedAdam, FusedSGD
    from mindtheedge_amd.trainers.trainer import Trainer
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            _small(cls, accumulate_grad_batches=bad)
    if bad < 1:
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            Trainer(accumulate_grad_batches=bad)


def test_accumulate_misuse_raises_and_counts_no_step():
    from mindtheedge_amd.trainers.data_parallel import FusedAdam, FusedSGD
    for cls in (FusedAdam, FusedSGD):
        _, opt = _small(cls)
        assert opt.flatp.accum is None
        with pytest.raises(RuntimeError, match="accumulate_grad_batches"):
            opt.accumulate()
        params, opt = _small(cls, accumulate_grad_batches=3)
        before = opt.flatp.flat.clone()
        for i in range(2):
            opt.zero_grad()
            for p in params:
                p.grad.fill_(float(i + 1))
            with opt.no_sync():
                pass
            opt.accumulate()
        used = torch.cat([opt.flatp.accum[o:o + p.numel()] for p, o in zip(opt.flatp.params, opt.flatp.offsets)])
        assert bool((used == 3.0).all()) and float(opt.flatp.accum.sum()) == 3.0 * 17
        with pytest.raises(RuntimeError, match="already accumulated"):
            opt.accumulate()
        assert opt.steps == 0 and torch.equal(opt.flatp.flat, before) and opt._pending == 2


# ---- 4. two ranks over gloo ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _int_grads(flat, rank, micro):
    """integer-valued gradients per tensor: every sum below is exact in fp32 whatever its order"""
    g = torch.Generator().manual_seed(1000 + 10 * micro + rank)
    return [torch.randint(-8, 9, p.shape, generator=g).float() for p in flat.params]


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mindtheedge_amd.trainers.data_parallel import FlatParameters, BucketedAllReduce, FusedAdam
        params = [torch.nn.Parameter(torch.zeros(s)) for s in [(5,), (64,), (13, 10), (200,), (7,), (3, 3)]]
        flat = FlatParameters(params)
        red = BucketedAllReduce(flat, bucket_bytes=4 * 100)
        assert red.active and red.world == 2 and len(red.buckets) >= 3
        opt = FusedAdam(flat, reducer=red, accumulate_grad_batches=2)
        scales = []
        opt._host_step = lambda K, g, gscale: scales.append(gscale)     # (host buffers have no step kernel: keep what step() hands it)
        silent = flat.params[-1]                                          # never announced: finish() launches its bucket late
        micro = 0
        for group, size in enumerate((2, 2, 1)):                          # two full groups, then a short one
            want = torch.zeros_like(flat.grad)
            for j in range(size):
                opt.zero_grad()
                for r in range(world):
                    for p, o, g in zip(flat.params, flat.offsets, _int_grads(flat, r, micro)):
                        want[o:o + p.numel()] += g.flatten()
                for p, g in zip(flat.params, _int_grads(flat, rank, micro)):
                    p.grad.copy_(g)
                micro += 1
                if j + 1 < size:
                    with opt.no_sync():
                        for p in flat.params:
                            red._on_grad_ready(p)
                    assert red.launch_log == [] and red._works == [] and red._ready == [0] * len(red.buckets) and not red._seen
                    local = flat.grad.clone()
                    opt.accumulate()
                    assert torch.equal(flat.accum, local) and opt._pending == 1 and opt.steps == group
                else:
                    for p in flat.params:
                        if p is not silent:
                            red._on_grad_ready(p)
                    early = [b for b, _, _, _ in red.launch_log]
                    assert early == sorted(set(early)) and len(early) == len(red.buckets) - 1, early
                    opt.step()
                    launched = [b for b, _, _, _ in red.last_launches]
                    assert sorted(launched) == list(range(len(red.buckets))), launched        # every bucket once
            assert torch.equal(flat.grad, want), (group, float((flat.grad - want).abs().max()))
            assert scales[-1] == 1.0 / (world * size) and opt._pending == 0 and opt.steps == group + 1 and red._fold is None
        assert scales == [0.25, 0.25, 0.5]
        # forgetting no_sync(): the collectives went out on a partial sum, accumulate() refuses
        opt.zero_grad()
        for p in flat.params:
            red._on_grad_ready(p)
        try:
            opt.accumulate()
            raise AssertionError("accumulate() after a reduced backward must raise")
        except RuntimeError as e:
            assert "no_sync" in str(e)
        red.finish()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_accumulated_buckets_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in procs]
    for p in procs:
        p.join(30)
    assert all(r[1] == "ok" for r in res), res


# ---- 5. the reference ----------------------------------------------------------------------------------------------------------------------------------
def test_accum_ref_checks_itself():
    assert A.self_check()
    g = [torch.randn(1000, generator=torch.Generator().manual_seed(s)) for s in range(3)]
    assert torch.equal(A.sequential_sum(g), (g[0] + g[1]) + g[2])
    assert torch.equal(A.sequential_sum(g[:1]), g[0])
