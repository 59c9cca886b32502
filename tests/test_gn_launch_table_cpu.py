"""Which kernels every GroupNorm pass gets, checked without a GPU (tests/conv_launch_recorder.py --gn).

tests/gn_launch_table.json was recorded from the commit BEFORE csrc/gn_plan.hpp existed (its run_stats / run_fwd / run_bwd / run_tail and launch ladders), through
the four C entry points and the two queries.  The working tree must reproduce every line -- clears, kernel instance, grid, block, dynamic LDS, the GnArgs fields
the host chose, return code, the queries' answers -- in the development build and, for the cases that set no knob, in the product build.  The second test compiles
csrc/gn_plan.hpp ALONE with g++ and requires the plan of every case to say what the recorder saw launched.  The third requires the queries Python asks to agree
with the forward launch, the fourth runs the plan under the host sanitizers at the extremes.  A rule changed on purpose: regenerate the table (tools/README.md) and review its diff."""
import itertools
import json
import os
import re
import subprocess

import pytest

import conv_launch_recorder as R


@pytest.fixture(scope="module")
def table():
    return R.load_table(R.GN_TABLE)


def test_the_table_holds_the_recorders_cases(table):
    assert [json.loads(ln)["case"] for ln in table] == R.gn_cases()
    assert os.path.getsize(R.GN_TABLE) <= os.path.getsize(R.TABLE)


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_launches_reproduce_the_table(table, tmp_path, dev):
    want = table if dev else [ln for ln in table if json.loads(ln)["case"].endswith(" -")]
    got = R.run(R.build(str(tmp_path), dev, gn=True), [json.loads(ln)["case"] for ln in want])
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(want), bad[0][0], bad[0][1])


HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "gn_plan.hpp"
static void print(const GnPlan& pl) {
    std::printf("%d %d %d %d %d %d %d %d %d %d %u", pl.rc, (int)pl.form, pl.NT, pl.NCH, pl.CL, pl.cps_shift, pl.blocks_per_sample, pl.per_launch, pl.launches, pl.kernels, pl.clears);
    for (int i = 0; i < 2; ++i) std::printf(" %u %u %d %ld %d", pl.launch[i].grid_x, pl.launch[i].grid_y, pl.launch[i].block, pl.launch[i].lds, pl.launch[i].reverse);
}
// one case per line, as the recorder's driver reads it; prints the plan of every pass of the case (the tail has two), " | " between them
int main() {
    char line[1024], entry[32], knobs[512];
    while (std::fgets(line, sizeof line, stdin)) {
        int dtype, B, HW, C, second, dbias, ready, prezeroed;
        if (std::sscanf(line, "%31s %d %d %d %d %d %d %d %d %511s", entry, &dtype, &B, &HW, &C, &second, &dbias, &ready, &prezeroed, knobs) != 10) return 2;
        GnKnobs k;
        if (std::strcmp(knobs, "-") != 0)
            for (char* tok = std::strtok(knobs, ","); tok; tok = std::strtok(nullptr, ",")) {
                int key, value;
                if (std::sscanf(tok, "%d=%d", &key, &value) != 2 || gn_knob_set(k, key, value) != MTE_OK) return 2;
            }
        const int es = dtype == 0 ? 2 : 4;
        const GnSecond sec = second == 1 ? GnSecond::Input : second == 2 ? GnSecond::ScaledOutput : GnSecond::None;
        if (!std::strcmp(entry, "stats")) print(plan_gn({es, B, HW, C, GnPass::Stats, sec, false, false}, k));
        else if (!std::strcmp(entry, "fwd")) print(plan_gn({es, B, HW, C, ready ? GnPass::FwdApply : GnPass::FwdSingle, sec, false, false}, k));
        else if (!std::strcmp(entry, "bwd")) print(plan_gn({es, B, HW, C, GnPass::Bwd, sec, dbias != 0, false}, k));
        else if (!std::strcmp(entry, "tail")) {
            print(plan_gn({es, B, HW, C, GnPass::TailStats, GnSecond::Input, false, false}, k));
            std::printf(" | ");
            print(plan_gn({es, B, HW, C, GnPass::FwdApply, GnSecond::None, false, true}, k));
        } else return 2;
        std::printf("\n");
    }
    return 0;
}
"""
STREAM, SLAB, CLUSTER = 0, 1, 2
CLEAR_RED, CLEAR_DBIAS, CLEAR_DGAMMA_DBETA, CLEAR_TICKETS, CLEAR_RECORDS = 1, 2, 4, 8, 16


def _case(row):
    entry, dtype, B, HW, C, second, dbias, ready, pz, knobs = row["case"].split()
    return (entry,) + tuple(int(v) for v in (dtype, B, HW, C, second, dbias, ready, pz)) + (knobs,)


def _expected_clears(bits, B, C):
    r16 = (B + 15) & ~15
    slots = 64 if B >= 8 else 512 // B
    out = []
    if bits & CLEAR_RED: out.append({"clear": "red", "bytes": 4 * B * C * 2})
    if bits & CLEAR_DBIAS: out.append({"clear": "dbias", "bytes": 4 * C})
    if bits & CLEAR_DGAMMA_DBETA: out += [{"clear": "dgamma", "bytes": 4 * C}, {"clear": "dbeta", "bytes": 4 * C}]
    if bits & CLEAR_TICKETS: out.append({"clear": "stats+%d" % (8 * 32 * B), "bytes": 8 * r16})
    if bits & CLEAR_RECORDS: out.append({"clear": "stats+%d" % (8 * (32 * B + r16)), "bytes": 8 * B * slots * 32})
    return out


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/gn_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, clears, form, template parameters, number of launches, grid,
    block, dynamic LDS and the fields it sets in GnArgs are what the recorder saw (the one case the entry point turns away before it plans is left out)."""
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", R.CSRC, "-o", str(exe), str(src)])
    rows = [json.loads(ln) for ln in table]
    rows = [r for r in rows if not (_case(r)[0] == "bwd" and _case(r)[5] == 3)]
    out = subprocess.run([str(exe)], input="\n".join(r["case"] for r in rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    forms = set()
    for r, line in zip(rows, lines):
        entry, dtype, B, HW, C, second, dbias, ready, pz, knobs = _case(r)
        want = []                                                           # the launch record the plans stand for
        rc = 0
        for plan in line.split(" | "):
            v = [int(x) for x in plan.split()]
            rc, form, NT, NCH, CL, cps_shift, bps, per_launch, launches, kernels, clears = v[:11]
            if rc != 0:
                break
            if not pz:
                want += _expected_clears(clears, B, C)
            forms.add((entry, form, NCH, CL))
            for i in range(kernels):
                gx, gy, block, lds, reverse = v[11 + 5 * i:16 + 5 * i]
                assert block == NT, r
                for j in range(launches):
                    ln = {"grid": gx, "grid_y": gy, "block": block, "lds": lds, "blocks_per_sample": bps, "reverse": reverse, "cps_shift": cps_shift, "ppl": per_launch,
                          "b0": j * per_launch, "nb": min(B - j * per_launch, per_launch), "form": form, "tail": (NCH, CL if form == CLUSTER else NT) if form != STREAM else None}
                    want.append(ln)
        assert rc == r["rc"], r
        if rc != 0:
            assert r["launches"] == [], r
            continue
        assert len(want) == len(r["launches"]), r
        for w, g in zip(want, r["launches"]):
            if "clear" in w:
                assert w == g, r
                continue
            name = g["k"]
            assert w["form"] == (SLAB if "_slab_" in name else CLUSTER if "_cluster_" in name else STREAM), r
            if w["tail"]:
                assert tuple(int(x) for x in re.findall(r"-?\d+", name)[-2:]) == w["tail"], r
            for key, dflt in (("grid", None), ("grid_y", 1), ("block", None), ("lds", None), ("blocks_per_sample", 0), ("reverse", 0), ("cps_shift", 0), ("ppl", 0), ("b0", 0), ("nb", 0)):
                assert g.get(key, dflt) == w[key], (key, r)
    # the table reaches every form plan_gn can return (gn_plan.hpp says why the other cluster sizes cannot be reached)
    assert {(f, nch, cl) for e, f, nch, cl in forms if e == "fwd" and f != STREAM} == {(SLAB, 2, 0), (SLAB, 4, 0), (CLUSTER, 8, 4), (CLUSTER, 8, 8), (CLUSTER, 4, 8)}
    assert {(f, nch, cl) for e, f, nch, cl in forms if e == "bwd"} == {(STREAM, 0, 0), (SLAB, 2, 0), (SLAB, 4, 0), (CLUSTER, 4, 8)}


def test_the_queries_agree_with_the_forward_launch(table):
    """mte_gn_fwd_is_single_pass_b (what kernels.conv_forward and kernels._gn_forward ask before they skip the statistics pass) is 1 exactly where the forward
    without ready statistics took a slab or cluster kernel, and mte_gn_fwd_is_single_pass exactly where it took a slab kernel: in every case of the table."""
    rows = [json.loads(ln) for ln in table]
    fwd = {}
    for r in rows:
        entry, dtype, B, HW, C, second, dbias, ready, pz, knobs = _case(r)
        if entry == "fwd" and not ready:
            names = [l["k"] for l in r["launches"] if "k" in l]
            assert (r["rc"] == 0) == bool(names), r
            fwd[(dtype, B, HW, C, second, pz, knobs)] = ("_slab_" in names[0], "_slab_" in names[0] or "_cluster_" in names[0]) if names else (False, False)
    assert any(v == (True, True) for v in fwd.values()) and any(v == (False, True) for v in fwd.values()) and any(v == (False, False) for v in fwd.values())
    for r in rows:
        entry, dtype, B, HW, C, second, dbias, ready, pz, knobs = _case(r)
        slab, single = fwd[(dtype, B, HW, C, 1 if second == 1 else 0, pz, knobs)]
        assert (r.get("q", 0), r.get("qb", 0)) == (int(slab), int(single)), r


def test_plan_is_sound_at_the_extremes(table, tmp_path):
    """plan_gn runs on every GroupNorm launch with whatever sizes the caller passes: a stand-alone host program built with -fsanitize=address,undefined plans
    every case of the table and B, HW, C of 0, 1, -1 and INT_MAX scale (with the smallest min_rows and the largest target too) and must end clean -- no division
    by zero, no shift or signed overflow in the cluster and chunk loops."""
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", R.CSRC, "-o", str(exe), str(src)])
    cases = [json.loads(ln)["case"] for ln in table]
    big = 2 ** 31 - 1
    for entry, dtype, B, HW, C, second in itertools.product(("stats", "fwd", "bwd", "tail"), (0, 1), (0, 1, -1, big), (0, 1, -1, big, big - 7),
                                                             (0, 1, -1, 16, 512, 2048, big, big - 15), (0, 1, 2)):
        for knobs in ("-", "2=1,3=%d" % big):
            cases.append("%s %d %d %d %d %d 1 0 0 %s" % (entry, dtype, B, HW, C, second, knobs))
    out = subprocess.run([str(exe)], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    assert len(out.stdout.splitlines()) == len(cases)
