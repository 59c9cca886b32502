"""The cases of the GroupNorm(16)+ELU layout tests: ONE table for tests/test_gn_layout_cases_cpu.py (no GPU: the plan of every case is the intended one,
and the table reaches every kernel instance csrc/gn_plan.hpp can return) and tests/test_gpu_groupnorm_layout.py (every case on contiguous and on strided
operands).  Default knobs throughout.

A case is (dtype, B, C, H, W, second) with the kernel instance its forward and its backward pass are meant to reach:
    ("slab", NCH, cps_shift)                  one workgroup of 1024 threads per (sample, group), NCH 16-byte chunks per thread
    ("cluster", NCH, CL, cps_shift, launches) CL workgroups of 256 threads per (sample, group); 8 samples per launch, so B = 9 is two launches, the second
                                              with ONE live sample
    ("stream", statistics blocks, apply blocks) forward: no single pass, so mte_gn_stats + mte_gn_elu_fwd(stats_ready = 1)
    ("stream", blocks)                        backward: reduce + apply, the same number of blocks per sample in both
Pixel counts are odd wherever the form allows it, so the last thread row of a slab and the last workgroup of a cluster hold a short range; the exceptions are
the two sizes that fill a slab kernel to the last chunk (2048 and 4096 chunks: the thresholds NCH 2 -> 4 and slab -> cluster, with 4097 on the other side).
H and W are both above 1 (kernels._pl's fast path)."""
import collections

import torch

NONE, INPUT, SCALED = 0, 1, 2          # `second`: one input; v = y1 + scale2 * y2; one input whose gradient also leaves as d2 = scale2 * d1 (backward only)

_Case = collections.namedtuple("Case", "dtype B C H W second fwd bwd dbias rerun off4")


def Case(dtype, B, C, H, W, second, fwd, bwd, dbias=True, rerun=False, off4=False):
    """dbias: the backward call asks for the bias gradient; rerun: the single-pass forward runs twice on one statistics buffer that is not cleared in between;
    off4 (fp32): channel offsets and pads of 4 elements -- 16-byte but not 32-byte aligned pixels"""
    return _Case(dtype, B, C, H, W, second, fwd, bwd, dbias, rerun, off4)


CASES = [
    # ---- bf16: slab, NCH 2 and 4 at cps_shift 0 / 1 / 2 (128 / 256 / 512 channels)
    Case("bf16", 3, 128, 5, 13, NONE, fwd=("slab", 2, 0), bwd=("slab", 2, 0), rerun=True),          # 3 of a set of 8 samples: idle workgroups b >= B
    Case("bf16", 3, 128, 5, 13, NONE, fwd=("slab", 2, 0), bwd=("slab", 2, 0), dbias=False),
    Case("bf16", 3, 128, 5, 13, INPUT, fwd=("slab", 2, 0), bwd=("slab", 2, 0)),
    Case("bf16", 3, 128, 5, 13, SCALED, fwd=("slab", 2, 0), bwd=("stream", 1)),                      # (a scaled second output never takes a slab)
    Case("bf16", 9, 256, 5, 7, NONE, fwd=("slab", 2, 1), bwd=("slab", 2, 1)),                        # two sets of 8 samples
    Case("bf16", 9, 256, 5, 7, INPUT, fwd=("slab", 2, 1), bwd=("slab", 2, 1)),
    Case("bf16", 2, 512, 5, 7, NONE, fwd=("slab", 2, 2), bwd=("slab", 2, 2)),
    Case("bf16", 2, 512, 5, 7, INPUT, fwd=("slab", 2, 2), bwd=("slab", 2, 2), dbias=False),
    Case("bf16", 1, 128, 32, 64, NONE, fwd=("slab", 2, 0), bwd=("slab", 2, 0)),                      # 2048 chunks: every thread holds both of its chunks
    Case("bf16", 2, 128, 35, 59, NONE, fwd=("slab", 4, 0), bwd=("slab", 4, 0)),
    Case("bf16", 2, 128, 35, 59, INPUT, fwd=("slab", 4, 0), bwd=("slab", 4, 0)),
    Case("bf16", 2, 256, 15, 69, NONE, fwd=("slab", 4, 1), bwd=("slab", 4, 1)),
    Case("bf16", 2, 256, 15, 69, INPUT, fwd=("slab", 4, 1), bwd=("slab", 4, 1)),
    Case("bf16", 2, 512, 23, 31, NONE, fwd=("slab", 4, 2), bwd=("slab", 4, 2)),
    Case("bf16", 2, 512, 23, 31, INPUT, fwd=("slab", 4, 2), bwd=("slab", 4, 2)),
    Case("bf16", 2, 512, 23, 31, SCALED, fwd=("slab", 4, 2), bwd=("stream", 6)),
    Case("bf16", 1, 128, 64, 64, INPUT, fwd=("slab", 4, 0), bwd=("slab", 4, 0)),                     # 4096 chunks: the largest slab
    # ---- bf16: cluster
    Case("bf16", 2, 128, 53, 79, NONE, fwd=("cluster", 8, 4, 0, 1), bwd=("cluster", 4, 8, 0, 1), rerun=True),
    Case("bf16", 2, 128, 53, 79, INPUT, fwd=("cluster", 4, 8, 0, 1), bwd=("cluster", 4, 8, 0, 1)),
    Case("bf16", 2, 128, 53, 79, SCALED, fwd=("cluster", 8, 4, 0, 1), bwd=("cluster", 4, 8, 0, 1)),
    Case("bf16", 2, 128, 53, 79, SCALED, fwd=("cluster", 8, 4, 0, 1), bwd=("cluster", 4, 8, 0, 1), dbias=False),
    Case("bf16", 9, 128, 53, 79, NONE, fwd=("cluster", 8, 4, 0, 2), bwd=("cluster", 4, 8, 0, 2)),    # second launch: nb = 1
    Case("bf16", 9, 128, 53, 79, INPUT, fwd=("cluster", 4, 8, 0, 2), bwd=("cluster", 4, 8, 0, 2)),
    Case("bf16", 2, 256, 15, 137, NONE, fwd=("cluster", 8, 4, 1, 1), bwd=("cluster", 4, 8, 1, 1)),
    Case("bf16", 2, 256, 15, 137, SCALED, fwd=("cluster", 8, 4, 1, 1), bwd=("cluster", 4, 8, 1, 1)),
    Case("bf16", 2, 128, 59, 139, NONE, fwd=("cluster", 8, 8, 0, 1), bwd=("stream", 17)),
    Case("bf16", 2, 128, 59, 139, INPUT, fwd=("stream", 9, 33), bwd=("stream", 17)),                 # eight chunks and a second input: no such instance
    Case("bf16", 2, 128, 59, 139, SCALED, fwd=("cluster", 8, 8, 0, 1), bwd=("stream", 17)),
    # ---- bf16: stream (32 / 64 channels: a group is no whole 16-byte chunk)
    Case("bf16", 3, 32, 9, 13, NONE, fwd=("stream", 1, 1), bwd=("stream", 1)),
    Case("bf16", 3, 32, 9, 13, INPUT, fwd=("stream", 1, 1), bwd=("stream", 1)),
    Case("bf16", 3, 32, 9, 13, SCALED, fwd=("stream", 1, 1), bwd=("stream", 1)),
    Case("bf16", 3, 32, 9, 13, NONE, fwd=("stream", 1, 1), bwd=("stream", 1), dbias=False),
    Case("bf16", 3, 32, 9, 13, INPUT, fwd=("stream", 1, 1), bwd=("stream", 1), dbias=False),
    Case("bf16", 3, 32, 9, 13, SCALED, fwd=("stream", 1, 1), bwd=("stream", 1), dbias=False),
    Case("bf16", 2, 64, 63, 65, NONE, fwd=("stream", 2, 8), bwd=("stream", 4)),
    Case("bf16", 2, 64, 63, 65, INPUT, fwd=("stream", 2, 8), bwd=("stream", 4)),
    Case("bf16", 2, 64, 63, 65, SCALED, fwd=("stream", 2, 8), bwd=("stream", 4)),
    # ---- fp32: slab, NCH 2 and 4 at cps_shift 0 / 1 / 2 / 3 (64 / 128 / 256 / 512 channels)
    Case("fp32", 3, 64, 5, 13, NONE, fwd=("slab", 2, 0), bwd=("slab", 2, 0)),
    Case("fp32", 3, 64, 5, 13, INPUT, fwd=("slab", 2, 0), bwd=("slab", 2, 0), off4=True),
    Case("fp32", 2, 128, 5, 13, NONE, fwd=("slab", 2, 1), bwd=("slab", 2, 1)),
    Case("fp32", 9, 256, 5, 7, NONE, fwd=("slab", 2, 2), bwd=("slab", 2, 2)),
    Case("fp32", 9, 256, 5, 7, INPUT, fwd=("slab", 2, 2), bwd=("slab", 2, 2)),
    Case("fp32", 2, 512, 5, 7, INPUT, fwd=("slab", 2, 3), bwd=("slab", 2, 3)),
    Case("fp32", 2, 64, 35, 59, NONE, fwd=("slab", 4, 0), bwd=("slab", 4, 0), rerun=True),
    Case("fp32", 2, 64, 35, 59, INPUT, fwd=("slab", 4, 0), bwd=("slab", 4, 0)),
    Case("fp32", 2, 128, 15, 69, NONE, fwd=("slab", 4, 1), bwd=("slab", 4, 1)),
    Case("fp32", 2, 256, 9, 57, INPUT, fwd=("slab", 4, 2), bwd=("slab", 4, 2)),
    Case("fp32", 2, 512, 7, 37, NONE, fwd=("slab", 4, 3), bwd=("slab", 4, 3), dbias=False),
    Case("fp32", 2, 512, 7, 37, INPUT, fwd=("slab", 4, 3), bwd=("slab", 4, 3)),
    # ---- fp32: cluster (4097 pixels of 64 channels: one chunk more than the largest slab)
    Case("fp32", 2, 64, 17, 241, NONE, fwd=("cluster", 8, 4, 0, 1), bwd=("cluster", 4, 8, 0, 1)),
    Case("fp32", 2, 64, 17, 241, INPUT, fwd=("cluster", 4, 8, 0, 1), bwd=("cluster", 4, 8, 0, 1), off4=True),
    Case("fp32", 2, 64, 17, 241, SCALED, fwd=("cluster", 8, 4, 0, 1), bwd=("cluster", 4, 8, 0, 1)),
    Case("fp32", 9, 64, 17, 241, NONE, fwd=("cluster", 8, 4, 0, 2), bwd=("cluster", 4, 8, 0, 2)),     # second launch: nb = 1
    Case("fp32", 9, 64, 17, 241, INPUT, fwd=("cluster", 4, 8, 0, 2), bwd=("cluster", 4, 8, 0, 2)),
    Case("fp32", 2, 512, 19, 27, NONE, fwd=("cluster", 8, 4, 3, 1), bwd=("cluster", 4, 8, 3, 1), rerun=True),
    Case("fp32", 2, 512, 19, 27, SCALED, fwd=("cluster", 8, 4, 3, 1), bwd=("cluster", 4, 8, 3, 1)),
    Case("fp32", 2, 128, 17, 241, NONE, fwd=("cluster", 8, 8, 1, 1), bwd=("stream", 17)),
    Case("fp32", 2, 128, 17, 241, INPUT, fwd=("stream", 9, 33), bwd=("stream", 17)),
    # ---- fp32: stream
    Case("fp32", 2, 32, 37, 53, NONE, fwd=("stream", 1, 4), bwd=("stream", 2)),
    Case("fp32", 2, 32, 37, 53, INPUT, fwd=("stream", 1, 4), bwd=("stream", 2)),
    Case("fp32", 2, 32, 37, 53, SCALED, fwd=("stream", 1, 4), bwd=("stream", 2), off4=True),
    Case("fp32", 2, 32, 37, 53, NONE, fwd=("stream", 1, 4), bwd=("stream", 2), dbias=False),
    Case("fp32", 2, 32, 37, 53, INPUT, fwd=("stream", 1, 4), bwd=("stream", 2), dbias=False),
    Case("fp32", 2, 32, 37, 53, SCALED, fwd=("stream", 1, 4), bwd=("stream", 2), dbias=False),
]

# mte_gn_tail_fwd: (dtype, B, C, H, W, dropout, blocks per sample of its first launch (inner apply + statistics of the sum), of its second (the outer apply))
TailCase = collections.namedtuple("TailCase", "dtype B C H W dropout stats_blocks apply_blocks")
TAIL_CASES = [
    TailCase("bf16", 3, 32, 9, 13, True, 1, 1),
    TailCase("bf16", 3, 32, 9, 13, False, 1, 1),
    TailCase("bf16", 2, 64, 63, 65, True, 2, 8),
    TailCase("bf16", 2, 512, 23, 31, False, 3, 12),
    TailCase("fp32", 2, 32, 37, 53, False, 1, 4),
    TailCase("fp32", 2, 64, 17, 241, True, 5, 17),
    TailCase("fp32", 9, 256, 5, 7, True, 1, 1),
]


def case_id(c):
    if isinstance(c, TailCase):
        return "%s-%dx%dx%dx%d-%s" % (c.dtype, c.B, c.C, c.H, c.W, "dropout" if c.dropout else "plain")
    return "%s-%dx%dx%dx%d-%s%s%s%s" % (c.dtype, c.B, c.C, c.H, c.W, ("one", "two", "scaled")[c.second], "" if c.dbias else "-nodbias",
                                         "-rerun" if c.rerun else "", "-off4" if c.off4 else "")


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def make_inputs(c):
    """the operands of a case as fp32 CPU tensors [B, C, H, W], rounded to the compute dtype FIRST so that the kernels and the fp64 reference see identical
    values; the value distribution of tests/test_gpu_groupnorm.py (_run).  scale2 is Dropout2d's: 0 or 2 per (sample, channel), so it contains zeros."""
    tdt = torch_dtype(c)
    g = torch.Generator().manual_seed(c.B * 1000 + c.C + c.H + 7 * c.second)
    rnd = lambda *s: torch.randn(*s, generator=g)
    shape = (c.B, c.C, c.H, c.W)
    y1 = (rnd(*shape) * 1.5 + 0.3).to(tdt).float()
    y2 = rnd(*shape).to(tdt).float() if c.second == INPUT else None
    scale2 = ((torch.rand(c.B, c.C, generator=g) >= 0.5).float() * 2.0) if c.second != NONE else None
    gamma, beta = 1.0 + 0.25 * rnd(c.C), 0.1 * rnd(c.C)
    dz = rnd(*shape).to(tdt).float()
    if scale2 is not None:
        assert bool((scale2 == 0).any()) and bool((scale2 != 0).any())
    return {"y1": y1, "y2": y2, "scale2": scale2, "gamma": gamma, "beta": beta, "dz": dz}


def make_tail_inputs(c):
    """the operands of a tail case: the distribution of tests/test_gpu_groupnorm.py (test_residual_tail_in_two_launches)"""
    tdt = torch_dtype(c)
    g = torch.Generator().manual_seed(c.B * 77 + c.C + c.W)
    rnd = lambda *s: torch.randn(*s, generator=g)
    shape = (c.B, c.C, c.H, c.W)
    y1 = (rnd(*shape) * 1.5 + 0.3).to(tdt).float()
    s = rnd(*shape).to(tdt).float()
    scale = ((torch.rand(c.B, c.C, generator=g) >= 0.5).float() * 2.0) if c.dropout else None
    g1, b1, gt, bt = 1.0 + 0.25 * rnd(c.C), 0.1 * rnd(c.C), 1.0 + 0.25 * rnd(c.C), 0.1 * rnd(c.C)
    dz = rnd(*shape).to(tdt).float()
    return {"y1": y1, "s": s, "scale": scale, "g1": g1, "b1": b1, "gt": gt, "bt": bt, "dz": dz}
