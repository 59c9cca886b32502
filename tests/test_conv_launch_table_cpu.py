"""Which kernel every implicit-GEMM convolution gets, checked without a GPU (tests/conv_launch_recorder.py).

tests/conv_launch_table.json was recorded from the commit BEFORE csrc/conv_plan.hpp existed (its dispatch_igemm / launch_igemm / igemm8_launch), through the C entry
points.  The working tree must reproduce every line -- kernel instance, grid, block, dynamic LDS, LDS grant, split count, K order, return code -- in the development
build and, for the cases that set no knob, in the product build.  The second test compiles csrc/conv_plan.hpp ALONE with g++ and requires the plan of every case
to say what the recorder saw launched.  A rule changed on purpose: regenerate the table (tools/README.md) and review its diff."""
import json
import os
import subprocess

import pytest

import conv_launch_recorder as R


@pytest.fixture(scope="module")
def table():
    return R.load_table()


def test_the_table_holds_the_recorders_cases(table):
    from mindtheedge_amd import kernels as K
    assert R.SPLITK_SLABS == K.SPLITK_SLABS
    assert [json.loads(ln)["case"] for ln in table] == R.cases()


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_launches_reproduce_the_table(table, tmp_path, dev):
    want = table if dev else [ln for ln in table if json.loads(ln)["case"].endswith(" -")]
    got = R.run(R.build(str(tmp_path), dev), [json.loads(ln)["case"] for ln in want])
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(want), bad[0][0], bad[0][1])


HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "conv_plan.hpp"
// one case per line, as the recorder's driver reads it; prints rc grid threads lds splits kslice finish finish_grid optin
int main() {
    char line[1024], entry[32], knobs[512];
    while (std::fgets(line, sizeof line, stdin)) {
        int dtype, B, H, W, Cin_p, N, KH, KW, out_f32, has_ws, accumulate;
        long ldx, ws_elems;
        if (std::sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld %d %d %ld %d %511s", entry, &dtype, &B, &H, &W, &Cin_p, &N, &KH, &KW, &ldx, &out_f32, &has_ws, &ws_elems,
                        &accumulate, knobs) != 15) return 2;
        IgemmKnobs k;
        if (std::strcmp(knobs, "-") != 0)
            for (char* tok = std::strtok(knobs, ","); tok; tok = std::strtok(nullptr, ",")) {
                int key, value;
                if (std::sscanf(tok, "%d=%d", &key, &value) != 2 || !igemm_knob_set(k, key, value)) return 2;
            }
        const bool unshuffle = !std::strcmp(entry, "unshuffle"), sparse = !std::strcmp(entry, "sparse"), plain = !unshuffle && !sparse;
        const IgemmProblem p{dtype == 0 ? 2 : dtype == 1 ? 4 : 0, (long)B * H * W, N, Cin_p, KH, KW, ldx, plain ? out_f32 : 0, sparse, unshuffle ? N / 4 : 0,
                             unshuffle ? 0 : (accumulate >> 1) & 1, plain && has_ws, plain ? ws_elems : 0};
        const IgemmPlan pl = plan_igemm(p, k, DEV_BUILD);
        std::printf("%d %u %d %d %d %d %d %u %d\n", pl.rc, pl.grid, pl.threads, pl.lds_bytes, pl.splits, pl.kslice, (int)pl.finish, pl.finish_grid, (int)pl.lds_optin);
    }
    return 0;
}
"""


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/conv_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, grid, threads, LDS bytes, LDS opt-in, splits, K order and
    finish launch are what the recorder saw (cases the entry points turn away as bad arguments before they plan are left out)."""
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DDEV_BUILD=true", "-I", R.CSRC, "-o", str(exe), str(src)])
    rows = [json.loads(ln) for ln in table]
    rows = [r for r in rows if r["rc"] != -1]
    out = subprocess.run([str(exe)], input="\n".join(r["case"] for r in rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    plans = [[int(v) for v in ln.split()] for ln in out.stdout.splitlines()]
    assert len(plans) == len(rows)
    for r, (rc, grid, threads, lds, splits, kslice, finish, finish_grid, optin) in zip(rows, plans):
        assert rc == r["rc"], r
        if rc != 0:
            assert r["launches"] == []
            continue
        main = r["launches"][0]
        assert (grid, threads, lds) == (main["grid"], main["block"], main["lds"]), r
        assert (splits, kslice) == (main.get("splits", 1), main.get("kslice", 0)), r
        assert (lds if optin else 0) == main.get("granted", 0), r
        assert finish == (len(r["launches"]) == 2), r
        if finish:
            assert r["launches"][1]["k"].startswith("splitk_finish_kernel") and (r["launches"][1]["grid"], r["launches"][1]["block"]) == (finish_grid, 256), r
