"""Which kernel, how many pixel splits and how many slabs every mte_conv2d_wgrad call gets, checked without a GPU (tests/conv_launch_recorder.py --wgrad).

tests/wgrad_launch_table.json was recorded from the commit BEFORE csrc/wgrad_plan.hpp existed (wgrad9_launch in conv_wgrad9.hip, dispatch_wgrad / launch_wgrad_dma /
launch_wgrad in conv_igemm.hip, unchanged: their launches already named template instances).  The working tree must reproduce every line -- the clear and its
bytes, kernel instance, grid, block, dynamic LDS, LDS grant, the WgradArgs / Wgrad9Args fields the host chose, return code or query answer, *parts_out -- in the
development build and, for the cases that set no knob, in the product build.  The third test requires mte_debug_set(33, 0) to undo a knob soup; the fourth compiles
csrc/wgrad_plan.hpp ALONE with g++ and requires the plan of every case to say what the recorder saw launched; the fifth runs that program under the host sanitizers
at the extremes; the sixth requires every instance launch_wgrad_plan names to be reached by the table, and says which of them the product build cannot reach.  One
more drives the sizes the earlier launchers did not survive (below 1) through the entry point: refused, nothing launched, *parts_out untouched.  A
rule changed on purpose: regenerate the table (tools/README.md) and review its diff."""
import inspect
import itertools
import json
import os
import re
import subprocess

import pytest

import conv_launch_recorder as R


@pytest.fixture(scope="module")
def table():
    return R.load_table(R.WGRAD_TABLE)


@pytest.fixture(scope="module")
def dev_recorder(tmp_path_factory):
    return R.build(str(tmp_path_factory.mktemp("wgrad_dev")), True, wgrad=True)


def test_the_table_holds_the_recorders_cases(table):
    from mindtheedge_amd import kernels as K
    assert [json.loads(ln)["case"] for ln in table] == R.wgrad_cases()
    assert os.path.getsize(R.WGRAD_TABLE) <= os.path.getsize(R.TABLE)
    with open(os.path.join(R.CSRC, "wgrad_plan.hpp")) as f:
        src = f.read()
    assert re.search(r"#define MTE_WGRAD_WGS (\d+)", src).group(1) == str(R.WGRAD_WGS)
    assert re.search(r"#define MTE_W9_WGS (\d+)", src).group(1) == str(R.W9_WGS)
    assert "WGRAD_DESC_BOUND = 0x%xL" % R.DESC_BOUND in src
    # the stage size the recorder restates is the one kernels._conv_wgrad computes
    host = inspect.getsource(K._conv_wgrad)
    assert "wide = 256 if per <= (1 << 18) else (64 if per <= (1 << 19) else 32)" in host and "max(1, min(wide, (96 << 20) // (4 * per)))" in host
    assert "per = cout * kh * kw * Cp" in host


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "product"])
def test_launches_reproduce_the_table(table, tmp_path, dev_recorder, dev):
    want = table if dev else [ln for ln in table if json.loads(ln)["case"].endswith(" -")]
    got = R.run(dev_recorder if dev else R.build(str(tmp_path), False, wgrad=True), [json.loads(ln)["case"] for ln in want])
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(want), bad[0][0], bad[0][1])


def test_the_reset_key_undoes_a_knob_soup(dev_recorder):
    """mte_debug_set(33, 0) puts the five weight-gradient knobs back too: after it the entry point launches what the case without knobs launches"""
    soup = "4=0,8=0,9=64,26=0,27=16"
    for plain, k in (("wgrad 0 8 48 160 256 256 3 3 256 256 32 1 1 256 ", "conv_wgrad9_kernel<1>"),
                     ("wgrad 0 8 48 160 256 256 1 1 256 256 256 1 0 256 ", "conv_wgrad_dma_kernel<4, 4, 2, 2, true>"),
                     ("wgrad 0 8 48 160 512 128 5 5 512 128 14 1 1 256 ", "conv_wgrad_dma_kernel<2, 4, 2, 2, true>")):
        s, a, b = (json.loads(ln) for ln in R.run(dev_recorder, [plain + soup, plain + soup + ",33=0", plain + "-"]))
        assert a == dict(b, case=a["case"]) and a["launches"][-1]["k"] == k
        assert s["launches"] != b["launches"]                                # (the soup itself changes the launch)
    for kn in ("26=0", "8=0", "9=64", "27=16", "4=0"):                       # each key alone reaches its member
        plain = "wgrad 0 8 48 160 256 256 %s 256 256 32 1 1 256 " % ("3 3" if kn[:2] in ("26", "27") else "1 1")
        s, b = (json.loads(ln) for ln in R.run(dev_recorder, [plain + kn, plain + "-"]))
        assert s["launches"] != b["launches"], kn


HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "wgrad_plan.hpp"
// one case per line, as the recorder's driver reads it; prints the plan (the query: the rule the plan asks)
int main() {
    char line[1024], op[32], knobs[512];
    while (std::fgets(line, sizeof line, stdin)) {
        int dtype, B, H, W, C, N, KH, KW, cap, has_parts, shared, cus;
        long ldx, ldy;
        if (std::sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld %ld %d %d %d %d %511s", op, &dtype, &B, &H, &W, &C, &N, &KH, &KW, &ldx, &ldy, &cap, &has_parts, &shared, &cus,
                        knobs) != 16) return 2;
        WgradKnobs k;
        if (std::strcmp(knobs, "-") != 0)
            for (char* tok = std::strtok(knobs, ","); tok; tok = std::strtok(nullptr, ",")) {
                int key, value;
                if (std::sscanf(tok, "%d=%d", &key, &value) != 2 || !wgrad_knob_set(k, key, value)) return 2;
            }
        const int es = dtype == 0 ? 2 : dtype == 1 ? 4 : 0;
        if (!std::strcmp(op, "nine_tap")) { std::printf("%d\n", wgrad_nine_tap_rk(k, es, H, W, C, N, KH, KW) ? 1 : 0); continue; }
        if (std::strcmp(op, "wgrad")) return 2;
        const WgradPlan pl = plan_wgrad({es, B, H, W, C, N, KH, KW, ldx, ldy, cap, has_parts != 0, shared != 0, cus}, k);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld %d %zu %u %d %zu %d\n", pl.rc, (int)pl.family, pl.rk, pl.WNO, pl.WC, pl.TNO, pl.TC, (int)pl.row_aligned,
                    pl.tiles_n, pl.tiles_c, pl.splits, pl.blocks_per_split, pl.base, pl.units, pl.units_per_split, pl.part_stride, pl.parts_out, pl.clear_bytes, pl.grid,
                    pl.threads, pl.lds, (int)pl.lds_optin);
    }
    return 0;
}
"""
NINE_TAP, DMA, REG = 0, 1, 2                 # WgradFamily


def _build_plan(tmp_path, flags, name):
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags + ["-I", R.CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _plan(line):
    return [int(x) for x in line.split()]


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/wgrad_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, clear and its bytes, instance, grid, block, dynamic LDS,
    grant, every argument field the host chooses and *parts_out are what the recorder saw; the query's answer is the plan's rule"""
    exe = _build_plan(tmp_path, ["-Wall", "-Wextra", "-Werror"], "plan")
    rows = [json.loads(ln) for ln in table]
    out = subprocess.run([exe], input="\n".join(r["case"] for r in rows) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows) > 1000
    for r, line in zip(rows, lines):
        f = r["case"].split()
        if f[0] == "nine_tap":
            assert r["rc"] == int(line) and r["launches"] == [], r
            continue
        (rc, family, rk, WNO, WC, TNO, TC, fl, tiles_n, tiles_c, splits, bps, base, units, ups, part_stride, parts, clear_bytes, grid, threads, lds, optin) = _plan(line)
        assert rc == r["rc"], r
        launches = list(r["launches"])
        if rc != 0:
            assert launches == [] and r["parts"] == -1, r
            continue
        assert r["parts"] == (parts if f[12] == "1" else -1), r
        if clear_bytes:
            assert launches.pop(0) == {"clear": "dw", "bytes": clear_bytes}, r
            assert family == REG and splits > 1 and clear_bytes == 4 * int(f[5]) * int(f[6]) * int(f[7]) * int(f[8]), r
        assert len(launches) == 1, r
        tf = "true" if fl else "false"
        if family == NINE_TAP:
            want = {"k": "conv_wgrad9_kernel<%d>" % rk, "tiles_c": tiles_c, "base": base, "units": units, "units_per_split": ups, "part_stride": part_stride, "granted": lds}
            assert optin and parts == splits and grid == base * splits and base == tiles_n * tiles_c, r
        elif family == DMA:
            want = {"k": "conv_wgrad_dma_kernel<%d, %d, %d, %d, %s>" % (WNO, WC, TNO, TC, tf), "tiles_n": tiles_n, "tiles_c": tiles_c, "splits": splits,
                    "blocks_per_split": bps, "part_stride": part_stride, "granted": 0}
            assert not optin and threads == 64 * WNO * WC and parts == splits and (part_stride > 0) == (splits > 1), r
        else:
            want = {"k": "conv_wgrad_kernel<%s, %d, %d, %d, %d, %s>" % ("bf16" if f[1] == "0" else "float", WNO, WC, TNO, TC, tf), "tiles_n": tiles_n, "tiles_c": tiles_c,
                    "splits": splits, "blocks_per_split": bps, "part_stride": 0, "granted": 0}
            assert not optin and threads == 256 and parts == 1 and part_stride == 0, r
        want.update(grid=grid, block=threads, lds=lds)
        g = launches[0]
        for key, val in want.items():
            assert g.get(key, 1 if key == "splits" else 0) == val, (key, r)
        assert set(g) <= set(want), r


def test_plan_is_sound_at_the_extremes(table, tmp_path):
    """plan_wgrad runs on every mte_conv2d_wgrad call with whatever sizes the caller passes: a stand-alone host program built with -fsanitize=address,undefined
    plans every case of the table and a sweep, and must end clean -- no division by zero, no signed overflow; every return code is seen.  The sweep is the full
    product of seven kernel sizes (0, 1, 2, 3, 5, 7 and 3 x 5), B of 0, 1, -1, 2^10, H of 0, 1, -1, 16, 2^16, W of 0, 1, -1, 32, 40, 2^16 and the 81 pairs of
    channel counts 0, -8, 8, 24, 64, 96, 128, 256 and 2^31 - 1 (the pixel count times a stride stays inside a long, which the kernels' addressing has always
    needed).  It is NOT a product over the rest: element type, strides (the channel count, 8, 2^16), parts_cap (-1, 0, 1, INT_MAX), parts_out, shared, cus (0, 1,
    256, 2^20) and the knobs (defaults, all 0, all INT_MAX, 26 = 2 with 9 = 1) are dealt round-robin by the case's running number, so every size meets every value
    of each of them, not every combination of them.  Within the sweep a clear occurs only for the register-staged family, and only with more than one split."""
    exe = _build_plan(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "plan_san")
    cases = [json.loads(ln)["case"] for ln in table]
    n_table = len(cases)
    chans = (0, -8, 8, 24, 64, 96, 128, 256, 2 ** 31 - 1)
    big = 2 ** 31 - 1
    knob_sets = ("-", "4=0,8=0,9=0,26=0,27=0", "4=%d,8=%d,9=%d,26=%d,27=%d" % (big, big, big, big, big), "26=2,9=1")
    sizes = itertools.product(((0, 0), (1, 1), (2, 2), (3, 3), (5, 5), (7, 7), (3, 5)), (0, 1, -1, 1 << 10), (0, 1, -1, 16, 1 << 16), (0, 1, -1, 32, 40, 1 << 16))
    for j, ((KH, KW), B, H, W) in enumerate(sizes):
        for i, (cin_p, n) in enumerate(itertools.product(chans, chans), j):
            cases.append("wgrad %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % ((0, 1, 0, 2)[i % 4], B, H, W, cin_p, n, KH, KW, (cin_p, 1 << 16, 8)[i % 3], (n, 8, 1 << 16)[i % 3],
                                                                             (-1, 0, 1, big)[(i // 3) % 4], (1, 1, 0)[(i // 4) % 3], i & 1, (0, 1, 1 << 20, 256)[(i // 2) % 4], knob_sets[(i // 5) % 4]))
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) == n_table + 7 * 4 * 5 * 6 * 81
    sweep = [_plan(ln) for ln, c in zip(lines[n_table:], cases[n_table:])]
    for rc in (-1, -3, 0):
        assert any(p[0] == rc for p in sweep)
    launched = [p for p in sweep if p[0] == 0]
    assert {p[1] for p in launched} == {NINE_TAP, DMA, REG}
    cleared = [p for p in launched if p[17] > 0]
    assert cleared and all(p[1] == REG and p[10] > 1 for p in cleared)
    assert all(p[17] > 0 for p in launched if p[1] == REG and p[10] > 1)


def test_sizes_below_one_are_refused_before_any_launch(dev_recorder):
    """The refusals the plan adds, driven through mte_conv2d_wgrad itself (the commit before the plan divided by zero on these, so they are not in the recorded
    table): MTE_ERR_ARG, nothing launched or cleared, *parts_out untouched.  A pixel-block count beyond an int likewise; the query says 0 without channels."""
    base = dict(B=8, H=48, W=160, C=256, N=256, KH=3, KW=3)
    cases = []
    for dtype in (R.BF16, R.F32):
        for name in base:
            for bad in (0, -1):
                v = dict(base, **{name: bad})
                cases.append(R.wgrad_case("wgrad", dtype, v["B"], v["H"], v["W"], v["C"], v["N"], v["KH"], v["KW"], cap=8))
    cases.append(R.wgrad_case("wgrad", R.BF16, 1 << 10, 1 << 16, 1 << 16, 256, 256, 7, cap=8))      # 2^37 pixel blocks over six splits
    for r in (json.loads(ln) for ln in R.run(dev_recorder, cases)):
        assert (r["rc"], r["parts"], r["launches"]) == (-1, -1, []), r
    for c, n in ((0, 256), (256, 0), (-64, 128)):
        (r,) = (json.loads(ln) for ln in R.run(dev_recorder, [R.wgrad_case("nine_tap", R.BF16, 8, 48, 160, c, n, 3, cap=8)]))
        assert (r["rc"], r["launches"]) == (0, []), r


# What the product build (no knob: the LDS-DMA forms with their large tiles, the nine-tap kernel, 512 / 128 workgroups) cannot reach: nothing.  The register-staged
# bf16 instances are what a launch gets with at most 32 input or output channels or an operand beyond a buffer descriptor.
UNREACHABLE_IN_PRODUCT = set()


def test_every_instance_of_the_launch_switch_is_reached_or_listed(table):
    """the instances the switch of launch_wgrad_plan names (csrc/conv_igemm.hip; wgrad9_launch in csrc/conv_wgrad9.hip for the nine-tap pair), the instances the
    table's cases launched, and of those the ones a case without knobs launched: the switch names nothing the table does not reach, and exactly
    UNREACHABLE_IN_PRODUCT is reached with knobs only"""
    with open(os.path.join(R.CSRC, "conv_igemm.hip")) as f:
        src = f.read()
    body = src[src.index("int launch_wgrad_plan("):src.index("#undef WGRAD_REG")]
    named = []
    for m, a in re.findall(r"\bWGRAD_(DMA|REG)\(([^)]*)\)", body):
        for fl in ("true", "false"):
            named += ["conv_wgrad_dma_kernel<%s, %s>" % (a, fl)] if m == "DMA" else ["conv_wgrad_kernel<%s, %s, %s>" % (t, a, fl) for t in ("bf16", "float")]
    named += ["conv_wgrad9_kernel<%s>" % rk for rk in re.findall(r"case wgrad_key\(WgradFamily::NineTap, 2, (\d), 0, 0, 0\)", body)]
    with open(os.path.join(R.CSRC, "conv_wgrad9.hip")) as f:
        nine = f.read()
    assert set(re.findall(r"hipLaunchKernelGGL\((conv_wgrad9_kernel<\d>)", nine[nine.index("int wgrad9_launch("):])) == {k for k in named if "wgrad9" in k}
    assert len(named) == len(set(named)) == 24                               # each instance once
    rows = [json.loads(ln) for ln in table]
    reached = {l["k"] for r in rows for l in r["launches"] if "k" in l}
    product = {l["k"] for r in rows if r["case"].endswith(" -") for l in r["launches"] if "k" in l}
    assert reached == set(named)
    assert reached - product == UNREACHABLE_IN_PRODUCT
