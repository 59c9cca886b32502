"""Which kernel every LDS-patch convolution call gets, checked without a GPU (tests/conv_launch_recorder.py --patch).

tests/patch_launch_table.json was recorded from the commit BEFORE csrc/patch_plan.hpp existed (dispatch_fwd / launch_fwd / launch_form, launch_plus1x1 and
dispatch_wgrad / launch_wgrad / launch_wgrad_sl in conv_patch.hip, unchanged: their launches already named template instances).  The working tree must reproduce
every line -- the clear, kernel instance, grid, block, dynamic LDS, LDS grant, the PatchArgs / PatchWgradArgs fields the host chose, which pointers are passed,
return code or query answer, *parts_out, *tiles_per_sample_out -- in the development build and, for the cases that set no knob, in the product build.  The third
test requires mte_debug_set(33, 0) to undo a knob soup; the fourth compiles csrc/patch_plan.hpp ALONE with g++ and requires the plan of every case to say what the
recorder saw launched; the fifth runs that program under the host sanitizers at the extremes; the sixth requires every instance launch_patch_plan names to be
reached by the table, and says which of them the product build cannot reach.  A rule changed on purpose: regenerate the table (tools/README.md) and review its diff."""
import itertools
import json
import os
import re
import subprocess

import pytest

import conv_launch_recorder as R


@pytest.fixture(scope="module")
def table():
    return R.load_table(R.PATCH_TABLE)


@pytest.fixture(scope="module")
def dev_recorder(tmp_path_factory):
    return R.build(str(tmp_path_factory.mktemp("patch_dev")), True, patch=True)


def test_the_table_holds_the_recorders_cases(table):
    assert [json.loads(ln)["case"] for ln in table] == R.patch_cases()
    assert os.path.getsize(R.PATCH_TABLE) <= os.path.getsize(R.TABLE)
    with open(os.path.join(R.CSRC, "patch_plan.hpp")) as f:
        src = f.read()
    assert re.search(r"#define MTE_PATCH_WGRAD_WGS (\d+)", src).group(1) == str(R.PATCH_WGRAD_WGS)
    assert re.search(r"#define MTE_PATCH_WGRAD_WIDE_WGS (\d+)", src).group(1) == str(R.PATCH_WGRAD_WIDE_WGS)


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_launches_reproduce_the_table(table, tmp_path, dev_recorder, dev):
    want = table if dev else [ln for ln in table if json.loads(ln)["case"].endswith(" -")]
    got = R.run(dev_recorder if dev else R.build(str(tmp_path), False, patch=True), [json.loads(ln)["case"] for ln in want])
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(want), bad[0][0], bad[0][1])


def test_the_reset_key_undoes_a_knob_soup(dev_recorder):
    """mte_debug_set(33, 0) puts the eight LDS-patch knobs back too: after it every entry point launches what the case without knobs launches"""
    soup = "11=0,11=128,11=200,11=300,11=400,11=500,11=600,11=700"
    for plain, k in (("fwd 8 192 640 32 32 5 5 32 0 0 0 0 1 ", "conv_patch_fwd2_kernel<5, 1, true, false, false, false, true>"),
                     ("wgrad 8 192 640 96 64 3 3 96 0 0 0 512 1 ", "conv_patch_wgrad_kernel<3, 2, 3, 8, 1, 4>"),
                     ("wgrad 8 96 320 128 128 3 3 128 0 0 0 512 1 ", "conv_patch_wgrad_kernel<3, 2, 2, 8, 2, 4>"),
                     ("plus1x1 8 192 640 64 32 3 3 64 0 0 32 0 1 ", "conv_patch_fwd2_kernel<3, 1, true, false, false, true, true>")):
        s, a, b = (json.loads(ln) for ln in R.run(dev_recorder, [plain + soup, plain + soup + ",33=0", plain + "-"]))
        assert a == dict(b, case=a["case"]) and a["launches"][-1]["k"] == k
        assert s["launches"] != b["launches"]                                # (the soup itself changes the launch, or refuses it)


HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "patch_plan.hpp"
// one case per line, as the recorder's driver reads it; prints the plan (the queries: the plan of the problem their entry point asks about)
int main() {
    char line[1024], op[32], knobs[512];
    while (std::fgets(line, sizeof line, stdin)) {
        int B, H, W, C, N, KH, KW, acc, bias, C2, cap, shared;
        long ldx;
        if (std::sscanf(line, "%31s %d %d %d %d %d %d %d %ld %d %d %d %d %d %511s", op, &B, &H, &W, &C, &N, &KH, &KW, &ldx, &acc, &bias, &C2, &cap, &shared, knobs) != 15) return 2;
        PatchKnobs k;
        if (std::strcmp(knobs, "-") != 0)
            for (char* tok = std::strtok(knobs, ","); tok; tok = std::strtok(nullptr, ",")) {
                int key, value;
                if (std::sscanf(tok, "%d=%d", &key, &value) != 2 || (key != 11 && key != 33) || patch_knob_set(k, key == 33 ? PATCH_KNOB_RESET : value) != MTE_OK) return 2;
            }
        const bool aligned = bias < 0 || bias % 16 == 0;
        PatchProblem p{PatchOp::Fwd, B, H, W, C, N, KH, KW, ldx, acc != 0, aligned, 0, 0, false};
        if (!std::strcmp(op, "fwd_gn")) p.op = PatchOp::FwdGn;
        else if (!std::strcmp(op, "rank1") || !std::strcmp(op, "rank1_ok")) { p.op = PatchOp::FwdRank1; p.KH = p.KW = 3; p.accumulate = false; }
        else if (!std::strcmp(op, "plus1x1")) { p.op = PatchOp::FwdPlus1x1; p.KH = p.KW = 3; p.accumulate = false; p.C2 = C2; }
        else if (!std::strcmp(op, "wgrad")) { p.op = PatchOp::Wgrad; p.accumulate = false; p.bias_aligned = true; p.parts_cap = cap; p.wgrad_shares_chip = shared != 0; }
        else if (!std::strcmp(op, "supported")) p = {PatchOp::Fwd, 1, 1, W, C, N, KH, KW, C, false, true, 0, 0, false};
        else if (!std::strcmp(op, "wgrad_supported")) p = {PatchOp::Wgrad, 1, 1, W, C, N, KH, KW, C, false, true, 0, 1, false};
        else if (std::strcmp(op, "fwd")) return 2;
        const PatchPlan pl = plan_patch(p, k);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld %zu %u %u %d %zu\n", pl.rc, (int)pl.wgrad, (int)pl.second, pl.K, pl.NT, (int)pl.TALL,
                    (int)pl.R1, (int)pl.ACC, (int)pl.EXTRA, (int)pl.M16, pl.rows, pl.tiles_per_sample, pl.SL, pl.NW, pl.NH, pl.THW, pl.nslices, pl.groups, pl.parts_out,
                    pl.part_stride, pl.clear_bytes, pl.grid_x, pl.grid_y, pl.block, pl.lds);
    }
    return 0;
}
"""
PLANNED = ("fwd", "fwd_gn", "rank1", "rank1_ok", "plus1x1", "wgrad", "supported", "wgrad_supported")      # (repack, pack_elems, gn_elems: no choice to plan)


def _tf(*flags):
    return ", ".join("true" if f else "false" for f in flags)


def _build_plan(tmp_path, flags, name):
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags + ["-I", R.CSRC, "-o", str(exe), str(src)])
    return str(exe)


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/patch_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, clear and its bytes, instance, grid, block, dynamic LDS,
    grant, groups, part_stride, *parts_out and tiles per sample are what the recorder saw; a query's answer is the plan's"""
    exe = _build_plan(tmp_path, ["-Wall", "-Wextra", "-Werror"], "plan")
    rows = [r for r in (json.loads(ln) for ln in table) if r["case"].split()[0] in PLANNED]
    out = subprocess.run([exe], input="\n".join(r["case"] for r in rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows) > 1500
    for r, line in zip(rows, lines):
        op = r["case"].split()[0]
        (rc, wgrad, second, K, NT, TALL, R1, ACC, EXTRA, M16, rows_, tps, SL, NW, NH, THW, nslices, groups, parts, part_stride, clear_bytes, gx, gy, block,
         lds) = (int(x) for x in line.split())
        if op in ("supported", "wgrad_supported", "rank1_ok"):
            assert r["rc"] == (1 if rc == 0 else 0) and r["launches"] == [], r
            continue
        assert rc == r["rc"], r
        launches = list(r["launches"])
        if op == "wgrad":
            assert parts == r["parts"], r
        if rc != 0:
            assert launches == [] and r.get("tiles", -1) == -1, r
            continue
        if clear_bytes:
            assert launches.pop(0) == {"clear": "dw", "bytes": clear_bytes}, r
        assert len(launches) == 1, r
        g = launches[0]
        if wgrad:
            want = {"k": "conv_patch_wgrad_kernel<%d, %d, %d, %d, %d, %d>" % (K, NT, SL, NW, NH, THW), "grid": groups, "grid_y": nslices, "lds": lds, "granted": lds,
                    "groups": groups, "part_stride": part_stride}
            assert (gx, gy, block) == (groups, nslices, 64 * NW), r
        else:
            name = "conv_patch_fwd2_kernel<%d, %d, %s>" % (K, NT, _tf(TALL, R1, ACC, EXTRA, M16)) if second else "conv_patch_fwd_kernel<%d, %d, %s>" % (K, NT, _tf(TALL, ACC, EXTRA, M16))
            want = {"k": name, "grid": gx, "grid_y": gy, "lds": 0, "granted": 0}
            assert rows_ == (16 if TALL else 8) and gx == tps * int(r["case"].split()[1]), r
            if op == "fwd_gn":
                assert r["tiles"] == tps, r
        want["block"] = block
        for key, val in want.items():
            assert g.get(key, 1 if key == "grid_y" else 0) == val, (key, r)


def test_plan_is_sound_at_the_extremes(table, tmp_path):
    """plan_patch runs on every LDS-patch launch with whatever sizes the caller passes: a stand-alone host program built with -fsanitize=address,undefined plans
    every case of the table and B, H, W of 0, 1, -1 and up to 2^10 samples of 2^16 x 2^16 pixels with strides up to 2^16 (the pixel count times the stride stays
    inside a long, which the entry points' arithmetic has always needed), every class of Cin_p and N, every K, parts_cap of -1, 0, 1 and INT_MAX and the knobs at 0
    and at their largest, and must end clean -- no division by zero, no signed overflow; a tile count beyond a grid's x is refused."""
    exe = _build_plan(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "plan_san")
    cases = [c for c in (json.loads(ln)["case"] for ln in table) if c.split()[0] in PLANNED]
    n_table = len(cases)
    chans = (0, -8, 8, 24, 64, 96, 128, 2 ** 31 - 1)
    knob_sets = ("-", "11=0,11=200,11=300,11=400,11=500,11=600,11=700,11=100", "11=99,11=209,11=309,11=409,11=509,11=609,11=709,11=%d" % (2 ** 31 - 1))
    for (op, (KH, KW)), B, H, W in itertools.product(((o, kk) for o in ("fwd", "fwd_gn", "rank1", "plus1x1", "wgrad", "wgrad_supported")
                                                      for kk in ((1, 1), (3, 3), (5, 5), (7, 7), (2, 2), (3, 5)) if o in ("fwd", "wgrad") or kk == (3, 3)),
                                                     (0, 1, -1, 1 << 10), (0, 1, -1, 16, 1 << 16), (0, 32, -1, -32, 1 << 16)):
        for i, (cin_p, n) in enumerate(itertools.product(chans, chans)):
            cap = (-1, 0, 1, 2 ** 31 - 1)[i % 4]
            cases.append("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % (op, B, H, W, cin_p, n, KH, KW, (cin_p, 1 << 16, 8)[i % 3], i & 1, (0, 4, -1)[i % 3], (16, 0, 12)[i % 3], cap,
                                                                          i & 1, knob_sets[i % 3]))
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for rc in ("-1 ", "-3 ", "0 "):
        assert any(ln.startswith(rc) for ln in lines[n_table:])


# What the product build (no knob: tall tiles, the second form, 16x16x32 MFMAs, eight waves, the wide variant, 192 / 128 groups) cannot reach.  The kernels stay:
# the development build's variant tests (tests/test_gpu_conv_variants.py) and tools compare against them.  (The first form with 16x16x32 MFMAs is reached
# wherever the second form is not taken: one or two slices at 64 outputs, 1x1, a bias off a 16-byte boundary, an input beyond the descriptor bound.)
UNREACHABLE_IN_PRODUCT = {
    # the 32x32x16 MFMA forms (knobs 500 / 600 / 700 at 0; the product library does not have them): every forward instance with M16 = false
    "conv_patch_fwd_kernel<%s, false>" % a for a in (
        "1, 1, true, true, false", "1, 1, true, false, false", "1, 1, false, true, false", "1, 1, false, false, false", "3, 1, true, true, false",
        "3, 1, true, false, false", "3, 1, false, true, false", "3, 1, false, false, false", "5, 1, true, true, false", "5, 1, true, false, false",
        "5, 1, false, true, false", "5, 1, false, false, false", "7, 1, true, true, false", "7, 1, true, false, false", "7, 1, false, true, false",
        "7, 1, false, false, false", "1, 2, false, true, false", "1, 2, false, false, false", "3, 2, false, true, false", "3, 2, false, false, false",
        "5, 2, false, true, false", "5, 2, false, false, false", "3, 1, true, false, true", "3, 1, false, false, true", "3, 2, false, false, true")
} | {
    "conv_patch_fwd2_kernel<%s, false>" % a for a in (
        "3, 1, true, false, true, false", "3, 1, true, false, false, false", "3, 1, false, false, true, false", "3, 1, false, false, false, false",
        "5, 1, true, false, true, false", "5, 1, true, false, false, false", "5, 1, false, false, true, false", "5, 1, false, false, false, false",
        "7, 1, true, false, true, false", "7, 1, true, false, false, false", "7, 1, false, false, true, false", "7, 1, false, false, false, false",
        "3, 2, false, false, true, false", "3, 2, false, false, false, false", "5, 2, false, false, true, false", "5, 2, false, false, false, false",
        "3, 1, true, true, false, false", "3, 1, false, true, false, false", "3, 2, false, true, false, false", "3, 1, true, false, false, true",
        "3, 1, false, false, false, true", "3, 2, false, false, false, true")
} | {
    # the four-wave weight gradients that eight waves displace (knob 200 at 0)
    "conv_patch_wgrad_kernel<3, 2, 2, 4, 1, 8>", "conv_patch_wgrad_kernel<5, 1, 2, 4, 1, 8>", "conv_patch_wgrad_kernel<5, 2, 1, 4, 1, 8>",
    "conv_patch_wgrad_kernel<7, 1, 1, 4, 1, 8>",
}


def test_every_instance_of_the_launch_switch_is_reached_or_listed(table):
    """the instances the two launch_patch_plan switches name (csrc/conv_patch.hip), the instances the table's cases launched, and of those the ones a case
    without knobs launched: the switches name nothing the table does not reach, and exactly UNREACHABLE_IN_PRODUCT is reached with knobs only"""
    with open(os.path.join(R.CSRC, "conv_patch.hip")) as f:
        src = f.read()
    body = src[src.index("int launch_patch_plan("):src.index("#undef PATCH_FWD")]
    kernel = {"FWD": "conv_patch_fwd_kernel", "FWD2": "conv_patch_fwd2_kernel", "WGRAD": "conv_patch_wgrad_kernel"}
    named = ["%s<%s%s>" % (kernel[m], a, ", false" if x else "") for m, x, a in re.findall(r"\bPATCH_(FWD2?|WGRAD)(_32)?\(([^)]*)\)", body)]
    assert len(named) == len(set(named)) == 113 and len(UNREACHABLE_IN_PRODUCT) == 51      # each instance once
    rows = [json.loads(ln) for ln in table]
    reached = {l["k"] for r in rows for l in r["launches"] if "k" in l} - {"repack_patch_kernel"}
    product = {l["k"] for r in rows if r["case"].endswith(" -") for l in r["launches"] if "k" in l}
    assert reached == set(named)
    assert reached - product == UNREACHABLE_IN_PRODUCT
    assert {k for k in named if "wgrad" not in k and k.endswith("false>")} == {k for k in UNREACHABLE_IN_PRODUCT if "wgrad" not in k}
