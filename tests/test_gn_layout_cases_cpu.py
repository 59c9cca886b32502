"""The case table of the GroupNorm layout tests (tests/gn_layout_cases.py), checked without a GPU.

csrc/gn_plan.hpp is compiled ALONE with g++ (the harness of tests/test_gn_launch_table_cpu.py) and asked for the plan of every case: it must be the instance the
table names -- form, NCH, CL, cps_shift, blocks per sample, number of launches.  The table must reach every instance the plan can return: those the
comment above plan_gn names, and, independently, whatever a scan of the plan over a grid of shapes turns up.  The last test shows, for the fp64 reference alone,
that the per-slab error measure of the GPU test divides by numbers of one order: every (sample, group) slab's largest |want| is at least a tenth of the tensor's."""
import subprocess

import pytest
import torch

import conv_launch_recorder as R
import gn_layout_cases as T
import gn_ref
from test_gn_launch_table_cpu import HARNESS, STREAM, SLAB, CLUSTER

FIELDS = "rc form NT NCH CL cps_shift blocks_per_sample per_launch launches kernels".split()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("gn_layout_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", R.CSRC, "-o", str(exe), str(src)])

    def ask(queries):
        """queries: (entry, dtype name, B, HW, C, second, dbias, ready) -> one list of plans (dicts) per query; the tail has two"""
        lines = ["%s %d %d %d %d %d %d %d 0 -" % (e, 0 if dt == "bf16" else 1, B, HW, C, sec, db, rdy) for e, dt, B, HW, C, sec, db, rdy in queries]
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = [[dict(zip(FIELDS, (int(x) for x in p.split()[:len(FIELDS)]))) for p in ln.split(" | ")] for ln in out.stdout.splitlines()]
        assert len(got) == len(queries)
        return got
    return ask


def _single(p):
    """the instance a single-pass or backward plan stands for, in the table's words"""
    if p["rc"] != 0:
        return None
    if p["form"] == SLAB:
        assert (p["NT"], p["launches"], p["kernels"], p["blocks_per_sample"]) == (1024, 1, 1, 0)
        return ("slab", p["NCH"], p["cps_shift"])
    if p["form"] == CLUSTER:
        assert (p["NT"], p["kernels"], p["per_launch"]) == (256, 1, 8)
        return ("cluster", p["NCH"], p["CL"], p["cps_shift"], p["launches"])
    assert p["form"] == STREAM and (p["NT"], p["launches"]) == (256, 1)
    return ("stream", p["blocks_per_sample"])


def _case_plans(plan, c):
    h2 = 1 if c.second == T.INPUT else 0
    q = [("fwd", c.dtype, c.B, c.H * c.W, c.C, h2, 0, 0), ("stats", c.dtype, c.B, c.H * c.W, c.C, h2, 0, 0), ("fwd", c.dtype, c.B, c.H * c.W, c.C, h2, 0, 1),
         ("bwd", c.dtype, c.B, c.H * c.W, c.C, c.second, int(c.dbias), 0)]
    single, stats, apply_, bwd = (r[0] for r in plan(q))
    fwd = _single(single)
    if fwd is None:                                          # no single pass: the statistics pass and the stream apply
        assert (stats["rc"], stats["NT"], stats["kernels"], apply_["rc"], apply_["form"], apply_["kernels"]) == (0, 1024, 1, 0, STREAM, 1)
        fwd = ("stream", stats["blocks_per_sample"], apply_["blocks_per_sample"])
    b = _single(bwd)
    if b[0] == "stream":
        assert bwd["kernels"] == 2                            # reduce, then apply
    return fwd, b


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_every_case_reaches_its_instance(plan, c):
    assert c.H > 1 and c.W > 1
    assert not c.off4 or c.dtype == "fp32"
    assert not c.rerun or c.fwd[0] in ("slab", "cluster")
    assert _case_plans(plan, c) == (c.fwd, c.bwd)


@pytest.mark.parametrize("c", T.TAIL_CASES, ids=T.case_id)
def test_every_tail_case_has_its_two_launches(plan, c):
    tail, inner = plan([("tail", c.dtype, c.B, c.H * c.W, c.C, 1, 0, 0), ("stats", c.dtype, c.B, c.H * c.W, c.C, 0, 0, 0)])
    assert len(tail) == 2 and inner[0]["rc"] == 0
    first, second = tail
    assert (first["rc"], first["NT"], first["kernels"], first["launches"], first["blocks_per_sample"]) == (0, 1024, 1, 1, c.stats_blocks)
    assert (second["rc"], second["form"], second["NT"], second["kernels"], second["launches"], second["blocks_per_sample"]) == (0, STREAM, 256, 1, 1, c.apply_blocks)


def _reached():
    """the instances the table's cases name: (pass, dtype, second / has2, form, NCH, CL) -- what norm_act.hip instantiates a kernel for; cps_shift, the
    blocks per sample and the number of launches are arguments of those kernels"""
    out = set()
    for c in T.CASES:
        h2 = int(c.second == T.INPUT)
        f, b = c.fwd, c.bwd
        if f[0] == "stream":
            out |= {("stats", c.dtype, h2), ("apply", c.dtype, h2)}
        else:
            out.add(("fwd", c.dtype, h2, f[0], f[1], f[2] if f[0] == "cluster" else 0))
        if b[0] == "stream":
            out.add(("bwd", c.dtype, c.second, "stream", int(c.dbias)))
        else:
            out.add(("bwd", c.dtype, c.second, b[0], b[1], b[2] if b[0] == "cluster" else 0))
    return out


def test_the_table_reaches_every_instance_the_plan_comment_names():
    reached = _reached()
    shifts = {"bf16": (0, 1, 2), "fp32": (0, 1, 2, 3)}
    for dt in ("bf16", "fp32"):
        for nch in (2, 4):
            # slab forward and backward at every cps_shift the type allows, and with and without a second input
            assert {c.fwd[2] for c in T.CASES if c.dtype == dt and c.fwd[:2] == ("slab", nch)} == set(shifts[dt]), (dt, nch)
            assert {c.bwd[2] for c in T.CASES if c.dtype == dt and c.bwd[:2] == ("slab", nch)} == set(shifts[dt]), (dt, nch)
            for sec in (T.NONE, T.INPUT):
                assert ("fwd", dt, sec, "slab", nch, 0) in reached and ("bwd", dt, sec, "slab", nch, 0) in reached, (dt, nch, sec)
        assert {("fwd", dt, 0, "cluster", 8, 4), ("fwd", dt, 0, "cluster", 8, 8), ("fwd", dt, 1, "cluster", 4, 8)} <= reached, dt
        for sec in (T.NONE, T.INPUT, T.SCALED):
            assert ("bwd", dt, sec, "cluster", 4, 8) in reached, (dt, sec)
            for db in (0, 1):
                assert ("bwd", dt, sec, "stream", db) in reached, (dt, sec, db)
        for h2 in (0, 1):
            assert ("stats", dt, h2) in reached and ("apply", dt, h2) in reached, (dt, h2)
        assert {c.dropout for c in T.TAIL_CASES if c.dtype == dt} == {True, False}, dt
        for form in ("slab", "cluster"):                     # the single-pass forward twice on one statistics buffer
            assert any(c.rerun and c.dtype == dt and c.fwd[0] == form for c in T.CASES), (dt, form)
    assert {c.bwd[0] for c in T.CASES if c.off4} == {"slab", "cluster", "stream"}
    # the stream backward with one and with several blocks per sample; a cluster batch in two launches, forward (both sizes) and backward
    assert {c.bwd[1] == 1 for c in T.CASES if c.bwd[0] == "stream"} == {True, False}
    assert {c.fwd[1:3] for c in T.CASES if c.fwd[0] == "cluster" and c.fwd[4] == 2 and c.B % 8 == 1} == {(8, 4), (4, 8)}
    assert any(c.bwd[0] == "cluster" and c.bwd[4] == 2 and c.B % 8 == 1 for c in T.CASES)
    # scale2 with zeros in a slab case and in a stream case with a second input (the inputs' generator asserts the zeros)
    assert any(c.second == T.INPUT and c.bwd[0] == "slab" for c in T.CASES) and any(c.second == T.INPUT and c.bwd[0] == "stream" for c in T.CASES)


def test_the_table_reaches_every_instance_a_scan_of_the_plan_finds(plan):
    """the plan of every pass over a grid of shapes -- batches on both sides of a set of 8, every channel count the kernels take, pixel counts from 1 to past
    the largest cluster with the thresholds on both sides: no slab or cluster instance turns up that the table does not run"""
    hws = sorted(set(range(1, 20000, 41)) | {v + d for v in (256, 512, 1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)})
    queries = []
    for dt in ("bf16", "fp32"):
        for B in (1, 2, 3, 8, 9, 16, 32, 33):
            for C in (16, 32, 64, 128, 256, 512, 1024):
                for HW in hws:
                    queries += [("fwd", dt, B, HW, C, h2, 0, 0) for h2 in (0, 1)] + [("bwd", dt, B, HW, C, sec, 1, 0) for sec in (0, 1, 2)]
    found = set()
    for q, (p,) in zip(queries, plan(queries)):
        if p["rc"] == 0 and p["form"] in (SLAB, CLUSTER):
            found.add((q[0], q[1], q[5], "slab" if p["form"] == SLAB else "cluster", p["NCH"], p["CL"]))
    assert len(found) >= 28                                   # (the scan is not empty: 2 types x (4 + 3 forward, 4 + 3 backward))
    assert found <= _reached(), sorted(found - _reached())


@pytest.mark.parametrize("c", sorted({c._replace(dbias=True, rerun=False, off4=False) for c in T.CASES}), ids=T.case_id)
def test_every_slab_of_the_reference_is_of_order_one(c):
    """what the GPU test divides by: max |want| over a (sample, group) slab is at least a tenth of the tensor's for z, d1 and d2.  (d2 = scale2 * d1: a slab
    whose channels Dropout2d removed altogether is zero and is compared exactly instead; every other slab keeps a channel of the full size.)"""
    x = T.make_inputs(c)
    z, d1, d2 = gn_ref.layout_reference(c.second, x["y1"], x["y2"], x["scale2"], x["gamma"], x["beta"], x["dz"])[:3]
    for name, t in (("z", z), ("d1", d1), ("d2", d2)):
        if t is None:
            continue
        m = gn_ref.slab_max(t)
        if name == "d2":
            kept = x["scale2"].reshape(c.B, 16, -1).amax(dim=2) > 0
            assert bool((m[~kept] == 0).all()) and bool(kept.any())
            m = m[kept]
        assert float(m.min()) >= 0.1 * float(m.max()), (name, float(m.min()), float(m.max()))


@pytest.mark.parametrize("c", T.TAIL_CASES, ids=T.case_id)
def test_every_slab_of_the_tail_reference_is_of_order_one(c):
    x = T.make_tail_inputs(c)
    want = gn_ref._tail_reference(x["y1"], x["s"], x["scale"], x["g1"], x["b1"], x["gt"], x["bt"], x["dz"])
    for name in ("t", "z"):
        m = gn_ref.slab_max(want[name])
        assert float(m.min()) >= 0.1 * float(m.max()), (name, float(m.min()), float(m.max()))
    assert torch.isfinite(want["z"]).all()
