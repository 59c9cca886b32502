"""Which kernel every conv3d pack / unpack call gets, checked without a GPU (tests/conv_launch_recorder.py --p3).

tests/p3_launch_table.json was recorded from the commit BEFORE csrc/p3_plan.hpp existed (the ladders inside the six entry points of pack3d.hip; its launch_p3 taking
the kernels as template arguments, which the recorder needs and which changes no code object).  The working tree must reproduce every line -- the clear, kernel
instance, grid, block, dynamic LDS, LDS grant, the P3Args / P3LArgs fields the host chose, which pointers are passed, return code -- in the development build and,
for the cases that set no knob, in the product build.  The third test compiles csrc/p3_plan.hpp ALONE with g++ and requires the plan of every case to say what the
recorder saw launched; the fourth runs that program under the host sanitizers at the extremes; the fifth requires every instance launch_p3plan names to be reached
by the table, and says which of them the product build cannot reach.  A rule changed on purpose: regenerate the table (tools/README.md) and review its diff."""
import itertools
import json
import os
import re
import subprocess

import pytest

import conv_launch_recorder as R


@pytest.fixture(scope="module")
def table():
    return R.load_table(R.P3_TABLE)


def test_the_table_holds_the_recorders_cases(table):
    assert [json.loads(ln)["case"] for ln in table] == R.p3_cases()
    assert os.path.getsize(R.P3_TABLE) <= os.path.getsize(R.TABLE)
    with open(os.path.join(R.CSRC, "p3_plan.hpp")) as f:
        assert re.search(r"#define MTE_P3W_WGS (\d+)", f.read()).group(1) == str(R.P3W_WGS)


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_launches_reproduce_the_table(table, tmp_path, dev):
    want = table if dev else [ln for ln in table if json.loads(ln)["case"].endswith(" -")]
    got = R.run(R.build(str(tmp_path), dev, p3=True), [json.loads(ln)["case"] for ln in want])
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(want), bad[0][0], bad[0][1])
    if dev:                                                             # mte_debug_set(33, 0) puts the conv3d knobs back too: the launch of the case without knobs
        plain = "unpack_bwd_data 0 8 192 640 32 32 32 "
        exe = os.path.join(str(tmp_path), "p3_recorder_dev")
        a, b = (json.loads(ln)["launches"] for ln in R.run(exe, [plain + "1=0,1=100,1=200,1=300,1=1256,1=2008,1=3001,33=0", plain + "-"]))
        assert a == b and a[0]["k"] == "unpack3d_bwd_data_dma32_kernel<4, true>"


HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "p3_plan.hpp"
// one case per line, as the recorder's driver reads it; prints the plan
int main() {
    static const char* const ops[6] = {"pack_fwd", "pack_bwd_data", "pack_bwd_weight", "unpack_fwd", "unpack_bwd_data", "unpack_bwd_weight"};
    char line[1024], op[32], knobs[512];
    while (std::fgets(line, sizeof line, stdin)) {
        int dtype, B, H, W, C;
        long ldx, ldo;
        if (std::sscanf(line, "%31s %d %d %d %d %d %ld %ld %511s", op, &dtype, &B, &H, &W, &C, &ldx, &ldo, knobs) != 9) return 2;
        P3Knobs k;
        if (std::strcmp(knobs, "-") != 0)
            for (char* tok = std::strtok(knobs, ","); tok; tok = std::strtok(nullptr, ",")) {
                int key, value;
                if (std::sscanf(tok, "%d=%d", &key, &value) != 2 || key != 1 || p3_knob_set(k, value) != MTE_OK) return 2;
            }
        int o = 0;
        while (o < 6 && std::strcmp(op, ops[o])) ++o;
        if (o == 6) return 2;
        const P3Plan pl = plan_p3({(P3Op)o, dtype, B, H, W, C, ldx, ldo}, k);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld %u %u %d %zu %d\n", pl.rc, (int)pl.form, (int)pl.f32, pl.CPT, pl.C, pl.HILO, pl.WAVES, pl.NH, pl.TH, pl.TW,
                    pl.tiles_h, pl.tiles_w, pl.ntiles, pl.dshift, pl.tshift, pl.total, pl.grid_x, pl.grid_y, pl.block, pl.lds, (int)pl.clear_dwb);
    }
    return 0;
}
"""
GATHER, LDS, LDS4, MFMA, DMA32, TAPS_K, WEIGHT_MFMA, WEIGHT_LDS = range(8)


def _instance(op, form, f32, CPT, C, HILO, WAVES, NH, TH):
    """the kernel instance a plan stands for, as the recorder prints it"""
    pack, T = op.startswith("pack"), "float" if f32 else "bf16"
    hilo = "true" if HILO else "false"
    if form == GATHER:
        return "%s_kernel<%s, %d>" % (op.replace("pack", "pack3d"), T, CPT) if pack else "%s_kernel<%s>" % (op.replace("unpack", "unpack3d"), T)
    if form == LDS:
        return op.replace("pack", "pack3d") + "_lds_kernel"
    if form == LDS4:
        return "unpack3d_bwd_data_lds4_kernel"
    if form == MFMA:
        return "pack3d_bwd_data_mfma_kernel<%s>" % hilo if pack else "%s_mfma_kernel<%d, %s>" % (op.replace("unpack", "unpack3d"), C, hilo)
    if form == DMA32:
        return "unpack3d_bwd_data_dma32_kernel<%d, %s>" % (WAVES, hilo)
    if form == TAPS_K:
        return "pack3d_fwd_tr_kernel<%d, %d>" % (TH, NH) if pack else "unpack3d_fwd_tr_kernel<%d, %d, %d>" % (C, TH, NH)
    if form == WEIGHT_MFMA:
        return "conv3d_bwd_weight_mfma_kernel<%s>" % ("false" if pack else "true")
    assert form == WEIGHT_LDS
    return op.replace("pack", "pack3d").replace("_bwd_weight", "_bwd_weight_lds_kernel")


def _build_plan(tmp_path, flags, name):
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags + ["-I", R.CSRC, "-o", str(exe), str(src)])
    return str(exe)


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/p3_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, clear, instance, grid, block, dynamic LDS and the fields it
    sets in P3Args / P3LArgs are what the recorder saw"""
    exe = _build_plan(tmp_path, ["-Wall", "-Wextra", "-Werror"], "plan")
    rows = [json.loads(ln) for ln in table]
    out = subprocess.run([exe], input="\n".join(r["case"] for r in rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        op = r["case"].split()[0]
        v = [int(x) for x in line.split()]
        rc, form, f32, CPT, C, HILO, WAVES, NH, TH, TW, tiles_h, tiles_w, ntiles, dshift, tshift, total, gx, gy, block, lds, clear = v
        assert rc == r["rc"], r
        launches = list(r["launches"])
        if clear:
            assert launches.pop(0) == {"clear": "dwb", "bytes": 448}, r
        if rc != 0:
            assert launches == [], r
            continue
        assert len(launches) == 1, r
        g = launches[0]
        assert g["k"] == _instance(op, form, f32, CPT, C, HILO, WAVES, NH, TH), r
        want = {"grid": gx, "grid_y": gy, "block": block, "lds": lds}
        if form == GATHER:
            want.update(total=total, granted=0)
        else:
            want.update(TH=TH, TW=TW, tiles_h=tiles_h, tiles_w=tiles_w, ntiles=ntiles, dshift=dshift, tshift=tshift, granted=112 * 1024)
        for key, val in want.items():
            assert g.get(key, 1 if key == "grid_y" else 0) == val, (key, r)


def test_plan_is_sound_at_the_extremes(table, tmp_path):
    """plan_p3 runs on every conv3d launch with whatever sizes the caller passes: a stand-alone host program built with -fsanitize=address,undefined plans every
    case of the table and B, H, W of 0, 1, -1 and up to 2^10 samples of 2^16 x (2^16 + 1) pixels with strides up to 2^16 (the pixel count times the stride stays
    inside a long, which the entry points' arithmetic has always needed), every C class and the knobs at 0 and at their largest, and must end clean -- no
    division by zero, no shift or signed overflow; a tile count beyond an int is refused."""
    exe = _build_plan(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "plan_san")
    cases = [json.loads(ln)["case"] for ln in table]
    for op, dtype, B, H, W, C in itertools.product(R.P3_OPS, (0, 1, 2), (0, 1, -1, 1 << 10), (0, 1, -1, 2, 1 << 16), (0, 1, -1, 2, (1 << 16) + 1),
                                                   (0, -8, 8, 24, 32, 64, 256, 512, 1024, 2 ** 31 - 1)):
        for ld, knobs in ((C, "-"), (1 << 16, "1=0"), (8, "1=555,1=100,1=200,1=1000,1=2000,1=3001"), (8, "1=315,1=2999,1=1999")):
            cases.append("%s %d %d %d %d %d %d %d %s" % (op, dtype, B, H, W, C, ld, ld, knobs))
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    assert any(ln.startswith("-1 ") for ln in lines[len(table):]) and any(ln.startswith("0 ") for ln in lines[len(table):])


# What the product build (no knob: lds 2, small tiles, matrix-core weight gradients, mfma_data 239) cannot reach.  The kernels stay: the development build's
# variant tests (tests/test_gpu_pack3d_variants.py) and tools compare against them.
UNREACHABLE_IN_PRODUCT = {
    "pack3d_bwd_data_mfma_kernel<false>", "unpack3d_bwd_data_mfma_kernel<32, false>", "unpack3d_bwd_data_mfma_kernel<64, false>",     # one-value weights (bit 4)
    "unpack3d_bwd_data_dma32_kernel<4, false>",
    "unpack3d_bwd_data_dma32_kernel<2, true>",                                                                                       # two waves (bit 2 clear)
    "unpack3d_fwd_mfma_kernel<32, false>", "unpack3d_fwd_mfma_kernel<64, false>", "unpack3d_fwd_mfma_kernel<32, true>", "unpack3d_fwd_mfma_kernel<64, true>",
    # (the banded forward: the taps-in-K form stands before it and takes every C it accepts)
    "unpack3d_fwd_tr_kernel<32, 8, 1>", "unpack3d_fwd_tr_kernel<64, 4, 1>", "unpack3d_fwd_tr_kernel<128, 2, 1>", "unpack3d_fwd_tr_kernel<256, 1, 1>",   # 1 or 2 passes
    "unpack3d_fwd_tr_kernel<32, 8, 2>", "unpack3d_fwd_tr_kernel<64, 4, 2>", "unpack3d_fwd_tr_kernel<128, 2, 2>", "unpack3d_fwd_tr_kernel<256, 1, 2>",
    "pack3d_bwd_weight_lds_kernel", "unpack3d_bwd_weight_lds_kernel",                                                               # VALU weight gradients
    # the pack layers' bf16 gather kernels: every C the library takes is <= 512, so bf16 always gets an LDS or matrix-core form (unpack: C = 8, 16 still gather)
    "pack3d_fwd_kernel<bf16, 4>", "pack3d_fwd_kernel<bf16, 8>", "pack3d_bwd_data_kernel<bf16, 4>", "pack3d_bwd_data_kernel<bf16, 8>",
    "pack3d_bwd_weight_kernel<bf16, 4>", "pack3d_bwd_weight_kernel<bf16, 8>",
}


def test_every_instance_of_the_launch_switch_is_reached_or_listed(table):
    """the instances launch_p3plan names (csrc/pack3d.hip), the instances the table's cases launched, and of those the ones a case without knobs launched: the
    switch names nothing the table does not reach, and exactly UNREACHABLE_IN_PRODUCT is reached with knobs only"""
    with open(os.path.join(R.CSRC, "pack3d.hip")) as f:
        src = f.read()
    body = src[src.index("int launch_p3plan("):src.index("#ifdef MTE_DEV", src.index("int launch_p3plan("))]
    named = [re.sub(r"\bbf16_t\b", "bf16", m) for m in re.findall(r"launch_(?:tiled|gather)<(\w+(?:<[^>]*>)?)>\(pl, a, st\)", body)]
    assert len(named) == len(set(named)) == body.count("case p3_key(") == 52                 # each instance once, one per case label
    rows = [json.loads(ln) for ln in table]
    reached = {l["k"] for r in rows for l in r["launches"] if "k" in l}
    product = {l["k"] for r in rows if r["case"].endswith(" -") for l in r["launches"] if "k" in l}
    assert reached == set(named)
    assert reached - product == UNREACHABLE_IN_PRODUCT
