"""GPU (-m gpu): MTE_OPT_HANDOFF_FENCES changes no bit of any result.

The four users of csrc/handoff.hpp (fused edge loss, edge-loss kinds, supervised loss, GroupNorm statistics) run their forward pass once with the
option at 0 and once at 1 -- the agent-scope release before each ticket and the acquire in the last arriver -- on shapes with several workgroups
per ticket and, where a kernel has two levels of tickets, several tickets.  Every output must be bit-identical: the fences order memory
operations, they take part in no arithmetic."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _both(run):
    """run() with the fences off and on -> the two tuples of outputs; the option is put back whatever happens"""
    from mindtheedge_amd import kernels as K
    # the C ABI has no getter: _lib.py records every set_option call in lib._options (to re-apply them to another build), and 0 is the
    # library's own initial value -- this read relies on that record
    before = K.lib._options.get(2, 0)
    out = []
    try:
        for fences in (0, 1):
            K.lib.set_option(2, fences)
            out.append(run())
            torch.cuda.synchronize()
    finally:
        K.lib.set_option(2, before)
    return out


def _assert_same(off, on):
    assert len(off) == len(on)
    for i, (a, b) in enumerate(zip(off, on)):
        assert bool(torch.isfinite(a.double()).all()), i
        assert torch.equal(a, b), i


def _edge_maps(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    inv = (0.02 + torch.rand(B, 1, H, W, generator=g)).to(DEV)
    edge = (torch.rand(B, 1, H, W, generator=g) < 0.2).float().to(DEV)
    normal = ((torch.rand(B, 1, H, W, generator=g) * 2 - 1) * 3.1).to(DEV)
    return inv, edge, normal


def test_fused_edge_loss():
    """B = 2, four scales from 72 x 136 with normals and silog depth: 3 x 3 tiles, three workgroups per image at scale 0, 8 image tickets"""
    from mindtheedge_amd import kernels as K
    B, S = 2, 4
    maps = [_edge_maps(B, 72 >> s, 136 >> s, seed=40 + s) for s in range(S)]
    g = torch.Generator().manual_seed(44)
    depth = torch.rand(B, 1, 72, 136, generator=g)
    gt = torch.where(depth < 0.4, torch.zeros(()), 1.0 + 50.0 * depth).to(DEV)          # metric depth, 0 = no measurement
    arr = (K._EdgeScale * S)()
    for o, (p, e, n) in zip(arr, maps):
        o.pred, o.edge, o.normal, o.mask, o.gmap, o.dpred = p.data_ptr(), e.data_ptr(), n.data_ptr(), None, None, None
        o.H, o.W = p.shape[-2], p.shape[-1]
    nwork = K.lib.mte_edge_loss_work_elems(ctypes.addressof(arr), S, B)

    def run():
        work = torch.zeros((nwork,), dtype=torch.float64, device=DEV)
        losses = torch.empty((S + 1,), dtype=torch.float32, device=DEV)
        coef = torch.empty((S * (2 * B + 1),), dtype=torch.float32, device=DEV)
        aux = torch.empty((2,), dtype=torch.float32, device=DEV)
        K.lib.mte_edge_loss_multi_fwd(ctypes.addressof(arr), S, B, 1, 1, 1, 4.0, 10.0, 1.0, gt.data_ptr(), work.data_ptr(), losses.data_ptr(),
                                      coef.data_ptr(), losses.data_ptr() + 4 * S, aux.data_ptr(), K._stream())
        return losses, coef, aux

    _assert_same(*_both(run))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_edge_loss_kinds(kind):
    """kinds 0, 1, 2 with dice, B = 2, 33 x 65: 2 x 2 ragged tiles per sample, two sample tickets"""
    from mindtheedge_amd import kernels as K
    B, H, W = 2, 33, 65
    inv, edge, normal = _edge_maps(B, H, W, seed=50 + kind)
    nwork = K.lib.mte_edge_loss_kind_work_elems(B, H, W)

    def run():
        work = torch.empty((nwork,), dtype=torch.float64, device=DEV)
        loss = torch.empty((), dtype=torch.float32, device=DEV)
        coef = torch.empty((2 * B + 5,), dtype=torch.float32, device=DEV)
        K.lib.mte_edge_loss_kind_fwd(inv.data_ptr(), edge.data_ptr(), normal.data_ptr(), None, None, B, H, W, kind, 1, 1, 1, 1, 4.0, 10.0, 1.0,
                                     work.data_ptr(), loss.data_ptr(), coef.data_ptr(), K._stream())
        # kind 0 fills every coefficient; kinds 1, 2 only the four leading ones
        return loss, (coef if kind == 0 else coef[:4].clone())

    _assert_same(*_both(run))


SUP_CHUNK = 256 * 4 * 4          # pixels per workgroup of sup_fwd_kernel: NT threads x 4 pixels x PASSES (supervised_loss.hip)


@pytest.mark.parametrize("method", ["berhu", "silog"])
def test_supervised_loss(method):
    """sparse-berhu (two launches, one ticket each) and sparse-silog over two scales of 3 and 2 workgroups, the last of each ragged: 5 workgroups
    draw each ticket, and the last arriver's per-scale sums read records of other workgroups at both scales"""
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.kernels_loss import SUPERVISED_METHODS
    B, sizes = 2, [(48, 96), (40, 72)]
    per_scale_blocks = [-(-B * h * w // SUP_CHUNK) for h, w in sizes]
    blocks = sum(per_scale_blocks)
    assert blocks >= 4 and min(per_scale_blocks) >= 2
    g = torch.Generator().manual_seed(60)
    preds = [(0.02 + torch.rand(B, 1, h, w, generator=g)).to(DEV) for h, w in sizes]
    depth = torch.rand(B, 1, 48, 96, generator=g)
    depth = torch.where(depth < 0.3, torch.zeros(()), 1.0 + 50.0 * depth).to(DEV)
    arr = K.SupervisedLossFn._scales(preds, None)
    nwork = K.lib.mte_supervised_loss_work_elems(ctypes.addressof(arr), len(preds), B)
    assert nwork == 2 + 16 + 4 * blocks          # two tickets, the BerHu hand-over, one 4-double record per workgroup: SUP_CHUNK is the kernel's

    def run():
        work = torch.empty((nwork,), dtype=torch.float64, device=DEV)
        loss = torch.empty((), dtype=torch.float32, device=DEV)
        per_scale = torch.empty((len(preds),), dtype=torch.float32, device=DEV)
        coef = torch.zeros((16,), dtype=torch.float32, device=DEV)
        K.lib.mte_supervised_loss_fwd(ctypes.addressof(arr), len(preds), B, depth.data_ptr(), 48, 96, SUPERVISED_METHODS.index(method), 1,
                                      work.data_ptr(), loss.data_ptr(), per_scale.data_ptr(), coef.data_ptr(), K._stream())
        return loss, per_scale, coef

    _assert_same(*_both(run))


# workgroups per sample of the statistics passes: ceil(HW / (16 rows x 1024 threads / (C / channels per 16 bytes))), i.e. at C = 64
# ceil(HW / 1024) in fp32 and ceil(HW / 2048) in bf16.  37 x 52 gives 2 and 1 -- in bf16 the fence arm runs but no record crosses
# workgroups -- so bf16 also runs 74 x 104, which gives 4.
@pytest.mark.parametrize("dtype,H,W", [("fp32", 37, 52), ("bf16", 37, 52), ("bf16", 74, 104)])
def test_groupnorm_statistics(dtype, H, W):
    """(3, 64, H, W) through the plain statistics pass and through the residual-tail pass (which never releases, and honours the acquire)"""
    from mindtheedge_amd import kernels as K
    B, C = 3, 64
    K.set_compute_dtype(dtype)
    try:
        tdt = K.compute_dtype()
        g = torch.Generator().manual_seed(70)
        y1 = K.as_act((torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3).to(DEV), tdt)
        s = K.as_act(torch.randn(B, C, H, W, generator=g).to(DEV), tdt)
        g1, b1, gt, bt = [(1.0 + 0.25 * torch.randn(C, generator=g)).to(DEV) for _ in range(4)]
        dt_, st = K._dt(y1), K._stream()

        def run():
            stats1, stats_t = K.gn_stats_buffer(B, y1.device), K.gn_stats_buffer(B, y1.device)
            K.lib.mte_gn_stats(K._pl(y1)[0], K._pl(y1)[1], 0, 0, 0, stats1.data_ptr(), B, H * W, C, dt_, st)
            t, z = K.new_act(B, C, H, W, y1.dtype), K.new_act(B, C, H, W, y1.dtype)
            K.lib.mte_gn_tail_fwd(K._pl(y1)[0], K._pl(y1)[1], stats1.data_ptr(), g1.data_ptr(), b1.data_ptr(), K._pl(s)[0], K._pl(s)[1], 0,
                                  K._pl(t)[0], K._pl(t)[1], stats_t.data_ptr(), gt.data_ptr(), bt.data_ptr(), K._pl(z)[0], K._pl(z)[1],
                                  B, H * W, C, 1e-5, dt_, st)
            return stats1[:B * 32].clone(), stats_t[:B * 32].clone(), t.float(), z.float()

        _assert_same(*_both(run))
    finally:
        K.set_compute_dtype("bf16")
