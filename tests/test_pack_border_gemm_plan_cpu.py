"""CPU: the launch plan of the grouped forward ring GEMMs (plan_pack_border_gemm, csrc/pack_border_plan.hpp) compiled alone with g++, under the host
sanitizers.  For the three folded pack layers of the T8 training step and the small shapes of tests/test_gpu_pack_border_gemm.py (plain and with forced slice
counts): every group's K range is covered exactly once by its slices and no slice is empty; the workgroups of the grid map one to one onto (group, slice,
tile) and the tiles cover every row and column of every group; every workspace element a tile addresses lies inside the workspace, no two (group, slice, row,
column) share one, and the last element of the workspace is addressed -- so the size query is exactly what the plan addresses; the T8 layers fill a 256-CU chip."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mindtheedge_amd", "csrc")

# (C, Co, k, B, H, W) of the un-packed input, as in tests/test_gpu_pack_border.py: C16 = 16 C channels per ring line, H2 x W2 = H/2 x W/2
T8 = [(32, 32, 5, 8, 384, 1280), (64, 64, 3, 8, 192, 640), (128, 128, 3, 8, 96, 320)]            # pack1, pack2, pack3 at B = 8, 384 x 1280
SMALL = [(8, 8, 3, 1, 8, 12), (8, 8, 5, 3, 22, 24), (32, 16, 5, 2, 24, 64), (24, 24, 3, 2, 20, 260)]
FORCED = (0, 2, 3, 5, 1000)
CUS = 256

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pack_border_plan.hpp"
// one case per line: B H2 W2 C16 Co k bf16 cus force_splits; prints the plan, then what a walk over the whole grid found
int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        int B, H2, W2, C16, Co, k, bf16, cus, force;
        if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d", &B, &H2, &W2, &C16, &Co, &k, &bf16, &cus, &force) != 9) return 2;
        const PbGemmPlan p = plan_pack_border_gemm(B, H2, W2, C16, Co, k, bf16 != 0, cus, force);
        std::printf("plan %d %d %d %d %d %d %d %d %d %d %d %d %d %ld", p.rc, p.bm, p.bn, p.ksteps, p.per_split, p.splits[0], p.splits[1], p.splits[2], p.splits[3],
                    p.grid, p.threads, p.lds_bytes, p.tiles_n, p.ws_elems);
        for (int g = 0; g < 4; ++g) std::printf(" %d %d %d", p.M[g], p.n[g], p.tiles_m[g]);
        std::printf("\n");
        if (p.rc != 0) { std::printf("walk 0 0 0 0 0 0\n"); continue; }
        // slices: K-steps covered per group
        long bad_slices = 0;
        for (int g = 0; g < 4; ++g) {
            std::vector<int> seen(p.ksteps, 0);
            for (int s = 0; s < p.splits[g]; ++s) {
                int s0, s1;
                pb_gemm_slice(p.ksteps, p.per_split, s, &s0, &s1);
                if (s0 >= s1 || s0 < 0 || s1 > p.ksteps) { ++bad_slices; continue; }
                for (int q = s0; q < s1; ++q) ++seen[q];
            }
            for (int q = 0; q < p.ksteps; ++q) bad_slices += seen[q] != 1;
        }
        // workgroups: (group, slice, tile) once each; their rows x columns mark the workspace
        std::vector<unsigned char> ws((size_t)p.ws_elems, 0);
        long bad_blocks = 0, outside = 0, twice = 0, marked = 0, expect = 0;
        for (int g = 0; g < 4; ++g) expect += (long)p.splits[g] * p.M[g] * p.Ng;
        std::vector<int> hit((size_t)p.grid, 0);
        for (int b = 0; b < p.grid; ++b) {
            int g, s, tm, tn;
            pb_gemm_block(p, b, &g, &s, &tm, &tn);
            if (g < 0 || g > 3 || s < 0 || s >= p.splits[g] || tm < 0 || tm >= p.tiles_m[g] || tn < 0 || tn >= p.tiles_n) { ++bad_blocks; continue; }
            const int id = p.block0[g] + (s * p.tiles_m[g] + tm) * p.tiles_n + tn;
            if (id != b || hit[id]++) ++bad_blocks;
            for (int m = tm * p.bm; m < (tm + 1) * p.bm && m < p.M[g]; ++m)
                for (int c = tn * p.bn; c < (tn + 1) * p.bn && c < p.Ng; ++c) {
                    const long at = pb_gemm_ws_index(p, g, s, m, c);
                    if (at < 0 || at >= p.ws_elems) { ++outside; continue; }
                    if (ws[(size_t)at]++) ++twice; else ++marked;
                }
        }
        std::printf("walk %ld %ld %ld %ld %ld %d\n", bad_slices, bad_blocks, outside, twice, expect - marked, (int)ws[(size_t)p.ws_elems - 1]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("pbg_plan")
    src = d / "plan.cpp"
    src.write_text(HARNESS)
    exe = str(d / "plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, cases):
    """cases: (C, Co, k, B, H, W, bf16, cus, force) -> [(plan fields, walk fields)]"""
    text = "".join("%d %d %d %d %d %d %d %d %d\n" % (B, H // 2, W // 2, 16 * C, Co, k, bf16, cus, force) for C, Co, k, B, H, W, bf16, cus, force in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == 2 * len(cases)
    res = []
    for pl, wk in zip(rows[0::2], rows[1::2]):
        assert pl[0] == "plan" and wk[0] == "walk"
        v = [int(x) for x in pl[1:]]
        keys = ("rc", "bm", "bn", "ksteps", "per_split", "s0", "s1", "s2", "s3", "grid", "threads", "lds", "tiles_n", "ws_elems")
        plan = dict(zip(keys, v))
        plan["groups"] = [tuple(v[len(keys) + 3 * g:len(keys) + 3 * g + 3]) for g in range(4)]           # (M, n, tiles_m)
        res.append((plan, [int(x) for x in wk[1:]]))
    return res


def _sound(case, plan, walk):
    C, Co, k, B, H, W = case[:6]
    H2, W2, pad = H // 2, W // 2, k // 2
    assert plan["rc"] == 0, case
    splits = plan["s0"]
    assert plan["s1"] == plan["s2"] == plan["s3"] == splits >= 1
    assert plan["ksteps"] == k * 16 * C // 32
    assert (splits - 1) * plan["per_split"] < plan["ksteps"] <= splits * plan["per_split"]            # no empty slice, nothing left over
    assert [g[:2] for g in plan["groups"]] == [(B * (W2 + 2), W2 + 2)] * 2 + [(B * H2, H2)] * 2
    tiles = sum(g[2] for g in plan["groups"]) * plan["tiles_n"]
    assert plan["grid"] == tiles * splits
    assert plan["tiles_n"] * plan["bn"] >= pad * Co and all(g[2] * plan["bm"] >= g[0] for g in plan["groups"])
    assert 2 * plan["lds"] <= 160 * 1024 and plan["threads"] == 256                                 # two workgroups per CU
    assert plan["ws_elems"] == splits * 2 * B * (W2 + 2 + H2) * 2 * pad * Co                       # [splits][2B][n][N] per family
    bad_slices, bad_blocks, outside, twice, unmarked, last = walk
    assert (bad_slices, bad_blocks, outside, twice, unmarked) == (0, 0, 0, 0, 0), (case, walk)
    assert last == 1                                                                                # the query is not larger than what is addressed
    return splits


def test_t8_layers_fill_the_chip(harness):
    cases = [c + (1, CUS, 0) for c in T8]
    for case, (plan, walk) in zip(cases, _run(harness, cases)):
        splits = _sound(case, plan, walk)
        assert plan["grid"] >= CUS, (case, plan["grid"])
        assert splits > 1 and plan["per_split"] % 2 == 0
        assert plan["grid"] < 2 * CUS                      # and not more slabs than the chip needs


def test_small_shapes_and_forced_slices(harness):
    cases = [c + (1, CUS, f) for c in SMALL + T8[1:] for f in FORCED]
    seen = {}
    for case, (plan, walk) in zip(cases, _run(harness, cases)):
        seen[case[:6] + (case[8],)] = _sound(case, plan, walk)
    assert seen[SMALL[0] + (0,)] == 1                       # K = 384: too short to split
    assert all(seen[c + (0,)] == 1 for c in SMALL[:2])
    assert seen[SMALL[0] + (1000,)] == 6                    # 12 K-steps: a slice is never shorter than one stage of two
    assert seen[SMALL[3] + (5,)] == 5 and (3 * 16 * 24 // 32) % 5 != 0          # K-steps the slice count does not divide
    assert all(seen[c + (2,)] == 2 for c in SMALL)


def test_what_the_plan_refuses(harness):
    C, Co, k, B, H, W = SMALL[1]
    cases = [(C, Co, k, B, H, W, 0, CUS, 0),                # fp32
             (C, Co + 4, k, B, H, W, 1, CUS, 0),            # Co % 8
             (C, Co, 7, B, H, W, 1, CUS, 0), (C, Co, 4, B, H, W, 1, CUS, 0), (C, Co, k, 0, H, W, 1, CUS, 0), (C, Co, k, B, 6, W, 1, CUS, 0),
             (C, Co, k, -1, H, W, 1, CUS, 0), (C, Co, k, 1 << 12, 1 << 12, 1 << 12, 1, CUS, 0), (0, Co, k, B, H, W, 1, CUS, 0)]
    for case, (plan, _) in zip(cases, _run(harness, cases)):
        assert plan["rc"] == -3, case
    ok = [(C, Co, k, B, H, W, 1, 0, 0), (C, Co, k, B, H, W, 1, 1 << 20, 0), (C, Co, k, B, H, W, 1, CUS, -5)]      # odd CU counts and knobs still plan
    for case, (plan, walk) in zip(ok, _run(harness, ok)):
        _sound(case, plan, walk)
