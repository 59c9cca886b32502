"""What the optimizer family's entry points decide on the host, checked without a GPU (tests/conv_launch_recorder.py --optim).

tests/optim_launch_table.json was recorded from the commit BEFORE csrc/optim_plan.hpp existed, through the 16 launching entry points of csrc/optim.hip and its
three work-buffer queries.  The working tree must reproduce every line -- kernel instance, grid, block, the fields and plain arguments the host chose, return code,
the queries' answers.  The third test compiles csrc/optim_plan.hpp ALONE with g++ and requires the plan of every case to say what the recorder saw launched; the
fourth enumerates the chunk cut on the host for the tensor tables the GPU tests use (the cut fixes the summation order of mte_tensor_stats and of LAMB's trust
ratios); the fifth runs the same harness under the host sanitizers at the extremes.  A rule changed on purpose: regenerate the table (tools/README.md) and review
its diff."""
import json
import os
import re
import subprocess

import pytest

import conv_launch_recorder as R

CHUNK, CAP, MAX_T = R.STAT_CHUNK, R.STAT_CAP, R.STAT_MAX_T
LONG_MAX = 2 ** 63 - 1


@pytest.fixture(scope="module")
def table():
    return R.load_table(R.OPTIM_TABLE)


def test_the_table_holds_the_recorders_cases(table):
    assert [json.loads(ln)["case"] for ln in table] == R.optim_cases()
    assert os.path.getsize(R.OPTIM_TABLE) <= os.path.getsize(R.TABLE)


def test_launches_reproduce_the_table(table, tmp_path):
    got = R.run(R.build(str(tmp_path), True, optim=True), [json.loads(ln)["case"] for ln in table])
    bad = [(w, g) for w, g in zip(table, got) if w != g]
    assert not bad, "%d of %d cases differ; the first:\n  table: %s\n  now:   %s" % (len(bad), len(table), bad[0][0], bad[0][1])


# plan: one case per line, as the recorder's driver reads it (with its fake pointers and its errors); prints what the plan says.
# cut: one table per line, "n T b0 m0 b1 m1 ..."; prints "total max_chunks", then one line per chunk of the host enumeration (cut_sum: only the vectors they hold).
HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "optim_plan.hpp"
using namespace optim_plan;

static int plan_case(const char* line) {
    char entry[32], wd_s[32], mom_s[32], damp_s[32], trust_s[32], norm_s[32], err[32];
    long n;
    int T, decoupled, nesterov, step, n_classes, flag;
    if (std::sscanf(line, "%31s %ld %d %31s %d %31s %d %31s %d %d %31s %31s %d %31s", entry, &n, &T, wd_s, &decoupled, mom_s, &nesterov, damp_s, &step, &n_classes,
                    trust_s, norm_s, &flag, err) != 14) return 2;
    const float wd = std::strtof(wd_s, nullptr), mom = std::strtof(mom_s, nullptr), damp = std::strtof(damp_s, nullptr), max_trust = std::strtof(trust_s, nullptr),
                max_norm = std::strtof(norm_s, nullptr);
    const char* names[] = {"p", "g", "m", "v", "buf", "hyper", "ctl", "cls", "scales", "begin", "numel", "table", "work", "trust", "sums", "out", "scal", "b"};
    std::map<std::string, uintptr_t> P;
    int k = 0;
    for (const char* name : names) P[name] = (uintptr_t)(++k) << 32;
    const std::string e = entry;
    const bool seg = e.size() > 8 && e.compare(e.size() - 8, 8, "_seg_dev") == 0;
    if ((e == "ema_update_dev" || seg || e.compare(0, 5, "lamb_") == 0) && !flag) P["ctl"] = 0;
    if (e == "tensor_stats" && !flag) P["p"] = 0;
    if (!std::strncmp(err, "null:", 5)) P[err + 5] = 0;
    else if (!std::strncmp(err, "mis:", 4)) P[err + 4] += 4;
    else if (!std::strcmp(err, "eq")) P["b"] = P["p"];
    else if (!std::strcmp(err, "overlap")) P["b"] = P["p"] + 16;
    auto ptr = [&](const char* name) { return (const void*)P[name]; };
    if (e == "grad_norm_work_bytes") { std::printf("q %ld\n", grad_norm_work_bytes(n)); return 0; }
    if (e == "tensor_stats_work_bytes") { std::printf("q %ld\n", tensor_stats_work_bytes(n, T)); return 0; }
    if (e == "lamb_work_bytes") { std::printf("q %ld\n", lamb_work_bytes(n, T)); return 0; }
    if (e == "ema_update" || e == "ema_update_dev" || e == "flat_swap" || e == "grad_accumulate") {
        const PairPlan pl = plan_pair(ptr("p"), ptr("b"), n, e != "ema_update_dev" || ptr("scal") != nullptr);
        std::printf("pair %d %d %d %d\n", pl.rc, (int)pl.launch, pl.grid, pl.block);
        return 0;
    }
    if (e == "grad_norm_clip") {
        const NormPlan pl = plan_norm(ptr("g"), n, max_norm, ptr("work"), ptr("ctl"));
        std::printf("norm %d %d %d %ld %ld %ld\n", pl.rc, pl.grid, pl.block, pl.work.sum, pl.work.ticket, pl.work.records);
        return 0;
    }
    const StepForm form = e == "adamw_step" || e == "sgd_step" ? STEP_HOST : seg ? STEP_SEG : e.find("_ctl_") != std::string::npos ? STEP_CTL : STEP_DEV;
    if (e.compare(0, 5, "adamw") == 0 || e.compare(0, 3, "sgd") == 0) {
        const bool adam = e[0] == 'a';
        const StepCall c = {ptr("p"), ptr("g"), {adam ? ptr("m") : ptr("buf"), adam ? ptr("v") : nullptr}, n, ptr("hyper"), ptr("ctl"), step, wd, mom, damp, decoupled,
                            nesterov, ptr("cls"), ptr("scales"), n_classes};
        const StepPlan pl = adam ? plan_adam(c, form) : plan_sgd(c, form);
        std::printf("%s %d %d %d %d %d\n", adam ? "adam" : "sgd", pl.rc, pl.wd, pl.mom, pl.grid, pl.block);
        return 0;
    }
    const ChunkCall c = {ptr("p"), e == "lamb_apply" ? nullptr : ptr("g"), ptr("m"), ptr("v"), ptr("hyper"), ptr("begin"), ptr("numel"), ptr("table"),
                         e == "lamb_apply" ? nullptr : ptr("work"), ptr("trust"), ptr("sums"), ptr("out"), n, T, wd, max_trust};
    ChunkPlan pl;
    if (e == "tensor_stats") pl = plan_chunks(c, WITH_G | WITH_WORK | WITH_OUT, STAT_VALUES);
    else if (e == "lamb_moments") pl = plan_chunks(c, WITH_P | WITH_G | WITH_MV | WITH_HYPER | WITH_WORK | WITH_TRUST | WITH_SUMS, LAMB_VALUES);
    else if (e == "lamb_apply") pl = plan_chunks(c, WITH_P | WITH_MV | WITH_HYPER | WITH_TRUST, LAMB_VALUES);
    else return 2;
    std::printf("chunk %d %ld %d %d %ld %ld %d\n", pl.rc, pl.max_chunks, pl.grid, pl.block, pl.work.tickets, pl.work.records, (int)pl.has_p);
    return 0;
}

static int cut_case(char* line, bool quiet) {
    std::vector<long> v;
    for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) v.push_back(std::strtol(tok, nullptr, 10));
    if (v.size() < 2 || v[1] < 1 || v[1] > STAT_MAX_T || v.size() != 2 + 2 * (size_t)v[1]) return 2;
    const long n = v[0];
    const int T = (int)v[1];
    std::vector<long> begin(T), numel(T);
    for (int t = 0; t < T; ++t) { begin[t] = v[2 + 2 * t]; numel[t] = v[3 + 2 * t]; }
    std::vector<int> first(T + 1);
    long total = chunk_table_host(begin.data(), numel.data(), T, n, first.data());
    std::printf("%ld %ld\n", total, stat_max_chunks(n, T));
    if (total > stat_max_chunks(n, T)) total = stat_max_chunks(n, T);           // as the kernels: nothing past the records
    long vectors = 0;
    for (long c = 0; c < total; ++c) {
        const Chunk ch = chunk_at(c, first.data(), begin.data(), numel.data(), T, n);
        vectors += ch.nvec;
        if (!quiet) std::printf("%d %d %ld %ld %ld %ld %ld %d\n", ch.t, ch.chunks, ch.b, ch.m, ch.e0, ch.e1, ch.nvec, (int)ch.has_tail());
    }
    if (quiet) std::printf("%ld\n", vectors);
    return 0;
}

int main(int argc, char** argv) {
    static char line[1 << 20];
    const bool quiet = argc > 1 && !std::strcmp(argv[1], "cut_sum"), cut = quiet || (argc > 1 && !std::strcmp(argv[1], "cut"));
    while (std::fgets(line, sizeof line, stdin)) {
        const int rc = cut ? cut_case(line, quiet) : plan_case(line);
        if (rc) return rc;
    }
    return 0;
}
"""


def _build(tmp_path, sanitize=False):
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / ("plan_san" if sanitize else "plan")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-Wall", "-Wextra", "-Werror"]
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags + ["-I", R.CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(exe, mode, lines):
    out = subprocess.run([exe, mode], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def _bool(v):
    return "true" if v else "false"


def test_plan_header_alone_says_what_was_launched(table, tmp_path):
    """csrc/optim_plan.hpp with plain g++, no HIP include path: for every case the plan's return code, instance, grid, block, work-buffer offsets and chunk bound
    (or the query's answer) are what the recorder saw."""
    rows = [json.loads(ln) for ln in table]
    lines = _run(_build(tmp_path), "plan", [r["case"] for r in rows])
    assert len(lines) == len(rows)
    seen = set()
    for r, line in zip(rows, lines):
        kind, *v = line.split()
        v = [int(x) for x in v]
        entry, flag = r["case"].split()[0], int(r["case"].split()[12])
        if kind == "q":
            assert r == {"case": r["case"], "q": v[0]}, r
            continue
        assert v[0] == r["rc"], (r, line)
        if v[0] != 0 or (kind == "pair" and not v[1]):
            assert r["launches"] == [], r
            continue
        (ln,) = r["launches"]
        if kind == "pair":
            name = {"ema_update": "ema_update_kernel<false>", "ema_update_dev": "ema_update_kernel<true>", "flat_swap": "flat_swap_kernel",
                    "grad_accumulate": "grad_accumulate_kernel<%s>" % _bool(flag)}[entry]
            grid, block = v[2], v[3]
        elif kind == "norm":
            name, grid, block = "grad_norm_kernel", v[1], v[2]
            off = 4 if r["case"].endswith("mis:work") else 0                # (an alignment the norm launch does not test)
            assert ln["ptrs"].split()[1:4] == ["work" + ("+%d" % (o + off) if o + off else "") for o in v[3:6]], r
        elif kind in ("adam", "sgd"):
            wd, mom, grid, block = v[1:]
            dev, ctl, seg = not entry.endswith("_step"), "_ctl_" in entry, entry.endswith("_seg_dev")      # the form is the entry point's, a template argument
            if kind == "adam":
                name = "adamw_seg_kernel<%d>" % wd if seg else "adamw_kernel<%d, %s, %s>" % (wd, _bool(dev), _bool(ctl))
            else:
                name = "sgd_seg_kernel<%d, %s>" % (mom, _bool(wd)) if seg else "sgd_kernel<%d, %s, %s, %s>" % (mom, _bool(wd), _bool(dev), _bool(ctl))
        else:
            max_chunks, grid, block, tickets, records, has_p = v[1:]
            name = {"tensor_stats": "tensor_stats_kernel<%s>" % _bool(has_p), "lamb_moments": "lamb_moments_kernel", "lamb_apply": "lamb_apply_kernel"}[entry]
            assert ln["max_chunks"] == max_chunks, r
            if entry != "lamb_apply":
                at = 4 if entry == "tensor_stats" else 9
                assert ln["ptrs"].split()[at:at + 2] == ["work" + ("+%d" % o if o else "") for o in (tickets, records)], r
        assert (ln["k"], ln["grid"], ln["block"], ln["lds"]) == (name, grid, block, 0), (r, line)
        seen.add(name)
    assert len(seen) == 46                                                 # every instance optim.hip has is reached by some case


def _gpu_test_constant(module, name):
    """a list the GPU tests define (they import torch and the library at import, so the line is read, not the module)"""
    with open(os.path.join(R.TESTS, module)) as f:
        (expr,) = re.findall(r"^%s = ([^#\n]*)" % name, f.read(), re.M)
    return eval(expr, {"CHUNK": CHUNK})


def _aligned_layout(numels):
    """(n, begins) as FlatParameters lays tensors out: every begin a multiple of 64"""
    begins, n = [], 0
    for m in numels:
        begins.append(n)
        n += (m + 63) // 64 * 64
    return n, begins


def _cut_tables():
    """name -> (n, begins, numels, disjoint and 64-aligned)"""
    out = {}
    for name, numels in (("stats", _gpu_test_constant("test_gpu_tensor_scales.py", "STAT_NUMELS")), ("lamb_a", _gpu_test_constant("test_gpu_lamb.py", "A_NUMELS")),
                         ("lamb_b", _gpu_test_constant("test_gpu_lamb.py", "B_NUMELS")), ("t4096", [1 + (37 * t) % (2 * CHUNK + 9) for t in range(MAX_T)]),
                         ("one_chunk_more", [CHUNK, CHUNK + 1, CHUNK - 1, 4 * CHUNK])):
        n, begins = _aligned_layout(numels)
        out[name] = (n, begins, list(numels), True)
    assert len(out["lamb_b"][2]) == 1100 > CAP and out["stats"][2][-1] == 3 * CHUNK + 1003
    n, begins = _aligned_layout([100, 5, 2 * CHUNK + 1, 64, 7, 9])
    # an empty tensor, a range that leaves [0, n), a misaligned begin, a negative begin and a negative count between valid ones
    out["invalid"] = (n, [begins[0], begins[1], begins[2], n - 32, begins[4] + 2, -64, begins[5]], [100, 0, 2 * CHUNK + 1, 64, 7, 9, -1], False)
    return out


@pytest.mark.parametrize("name", sorted(_cut_tables()))
def test_the_chunk_cut_covers_every_tensor_once_in_order(tmp_path, name):
    n, begins, numels, disjoint = _cut_tables()[name]
    T = len(numels)
    lines = _run(_build(tmp_path), "cut", ["%d %d " % (n, T) + " ".join("%d %d" % bm for bm in zip(begins, numels))])
    total, max_chunks = (int(x) for x in lines[0].split())
    chunks = [tuple(int(x) for x in ln.split()) for ln in lines[1:]]
    assert max_chunks == n // CHUNK + T
    if disjoint:
        assert total <= max_chunks                                         # sum ceil(m_t / C) <= floor(n / C) + T: what the record buffer's size rests on
    assert len(chunks) == min(total, max_chunks)
    at = 0                                                                 # global index of the next chunk
    for t, (b, m) in enumerate(zip(begins, numels)):
        valid = b >= 0 and m > 0 and b % 4 == 0 and b + m <= n
        count = -(-m // CHUNK) if valid else 1
        mine = chunks[at:at + count]
        assert len(mine) == count and all(c[0] == t and c[1] == count for c in mine), (t, mine[:2])    # consecutive global indices, in the table's order
        if not valid:
            assert mine == [(t, 1, 0, 0, 0, 0, 0, 0)], (t, mine)
        else:
            edge = 0
            for k, (_, _, cb, cm, e0, e1, nvec, tail) in enumerate(mine):
                assert (cb, cm, e0) == (b, m, edge) and e0 == k * CHUNK and e0 < e1 <= m and e1 - e0 <= CHUNK, (t, k)
                assert nvec == (e1 - e0) // 4 and tail == (e1 == m), (t, k)                    # whole vectors; the m & 3 trailing elements go to the last chunk,
                assert (e1 - e0) % 4 == 0 or e1 == m, (t, k)                                   # the only one that can be ragged
                edge = e1
            assert edge == m, t                                            # [0, numel) exactly once
        at += count
    assert at == total


def test_plan_is_sound_at_the_extremes(table, tmp_path):
    """The same harness as a stand-alone program built with -fsanitize=address,undefined: every case of the table, n and T at their extremes, and chunk tables
    with n = 2^40, T = 4096 and begins near LONG_MAX -- no signed overflow in the grid, layout and chunk arithmetic, no read outside first[0 .. T]."""
    exe = _build(tmp_path, sanitize=True)
    cases = [json.loads(ln)["case"] for ln in table]
    for entry in list(R.OPT_PTRS) + list(R.OPT_QUERIES):
        for n in (2 ** 40, 2 ** 62, LONG_MAX, -LONG_MAX - 1, 2 ** 31 * CHUNK):
            for T in (1, MAX_T, 2 ** 31 - 1, -2 ** 31):
                cases.append(R.optim_case(entry, n, T))
    assert len(_run(exe, "plan", cases)) == len(cases)
    n = 2 ** 40
    tables = []
    numels = [n // MAX_T // 64 * 64 - 61] * MAX_T                          # T = 4096 tensors that fill 2^40 elements: 2^25 chunks
    tables.append((n, _aligned_layout(numels)[1], numels))
    tables.append((n, [LONG_MAX, LONG_MAX - 3, LONG_MAX // 4 * 4, -LONG_MAX - 1, 0, n - 64], [64, LONG_MAX, 8, 64, LONG_MAX, 64]))
    tables.append((n, [0] * MAX_T, [CHUNK * 3 + 1] * MAX_T))                # a table that overlaps itself: more chunks than max_chunks
    tables.append((LONG_MAX, [0, 2 ** 62], [2 ** 40, 2 ** 40]))
    for n, begins, numels in tables:
        lines = _run(exe, "cut_sum", ["%d %d " % (n, len(numels)) + " ".join("%d %d" % bm for bm in zip(begins, numels))])
        assert len(lines) == 2
    assert int(lines[1]) == 2 * 2 ** 40 // 4                                # the last table: both tensors whole, as vectors
