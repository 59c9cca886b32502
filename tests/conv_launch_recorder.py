"""Launch recorder of the implicit-GEMM convolution and of GroupNorm: which kernel instance, grid, block and dynamic LDS every case gets, found on the CPU.

conv_igemm.hip and conv_igemm8.hip are compiled for the host alone (hipcc --cuda-host-only) with tests/conv_launch_shim.hpp in front, which turns every launch
into a line of text, and linked with tests/conv_launch_driver.cpp, which calls the three C entry points.  tests/conv_launch_table.json holds one line per case:
the case (the driver's input line) and what was launched.  tests/test_conv_launch_table_cpu.py requires the working tree to reproduce every line.
--gn: the same for norm_act.hip with tests/gn_launch_driver.cpp (four entry points, two queries, the clears) and tests/gn_launch_table.json
(tests/test_gn_launch_table_cpu.py).  --p3: the same for pack3d.hip with tests/p3_launch_driver.cpp (the six conv3d pack / unpack entry points) and
tests/p3_launch_table.json (tests/test_p3_launch_table_cpu.py).  --patch: the same for conv_patch.hip with tests/patch_launch_driver.cpp (the LDS-patch convolution's
six launching entry points and its queries) and tests/patch_launch_table.json (tests/test_patch_launch_table_cpu.py).  --wgrad: the same for mte_conv2d_wgrad and its
query (conv_igemm.hip, conv_wgrad9.hip) with tests/wgrad_launch_driver.cpp and tests/wgrad_launch_table.json (tests/test_wgrad_launch_table_cpu.py); the shim answers
the device query with the CU count of the case.  --optim: the same for optim.hip with tests/optim_launch_driver.cpp (the optimizer family's 16 launching entry points
and three work-buffer queries; the kernels' plain arguments are recorded too) and tests/optim_launch_table.json (tests/test_optim_launch_table_cpu.py).

    python tests/conv_launch_recorder.py [--gn | --p3 | --patch | --wgrad | --optim] --write            regenerate the table from the working tree (after a dispatch rule was changed ON PURPOSE)
    python tests/conv_launch_recorder.py [--gn | --p3 | --patch | --wgrad | --optim] --csrc DIR --out F  record another checkout's csrc/ (the parent's, to compare)
"""
import argparse
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "mindtheedge_amd", "csrc")
TABLE = os.path.join(TESTS, "conv_launch_table.json")
GN_TABLE = os.path.join(TESTS, "gn_launch_table.json")
P3_TABLE = os.path.join(TESTS, "p3_launch_table.json")
PATCH_TABLE = os.path.join(TESTS, "patch_launch_table.json")
WGRAD_TABLE = os.path.join(TESTS, "wgrad_launch_table.json")
OPTIM_TABLE = os.path.join(TESTS, "optim_launch_table.json")
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
SPLITK_SLABS = 8                    # kernels.SPLITK_SLABS (the test checks that they agree)
BF16, F32 = 0, 1
SOLO = 2                            # MTE_CONV_SOLO bit of `accumulate`


def build(out_dir, dev, csrc=CSRC, extra=(), gn=False, p3=False, patch=False, wgrad=False, optim=False):
    """-> path of the recorder program built from `csrc` (dev: with -DMTE_DEV, the build that has the knobs; gn: the GroupNorm driver and norm_act.hip with it;
    p3: the conv3d pack / unpack driver and pack3d.hip; patch: the LDS-patch convolution driver and conv_patch.hip; wgrad: the weight-gradient driver;
    optim: the optimizer driver and optim.hip, with the kernels' plain arguments recorded too.
    conv_wgrad9.hip is linked into all of them: conv_igemm.hip launches through it)"""
    exe = os.path.join(out_dir, ("gn_" if gn else "p3_" if p3 else "patch_" if patch else "wgrad_" if wgrad else "optim_" if optim else "") + ("recorder_dev" if dev else "recorder"))
    cmd = [HIPCC, "--cuda-host-only", "-fuse-cuid=none", "-Wl,--allow-multiple-definition", "-std=c++17", "-O1", "-Wno-unused-value", "-I", csrc, "-I", TESTS, "-include", os.path.join(TESTS, "conv_launch_shim.hpp")]
    cmd += ["-DMTE_DEV"] if dev else []
    cmd += list(extra) + [os.path.join(csrc, "conv_igemm.hip"), os.path.join(csrc, "conv_igemm8.hip"), os.path.join(csrc, "conv_wgrad9.hip")]
    if gn:
        cmd += [os.path.join(csrc, "norm_act.hip"), os.path.join(TESTS, "gn_launch_driver.cpp")]
    elif p3:
        cmd += [os.path.join(csrc, "pack3d.hip"), os.path.join(TESTS, "p3_launch_driver.cpp")]
    elif patch:
        cmd += [os.path.join(csrc, "conv_patch.hip"), os.path.join(TESTS, "patch_launch_driver.cpp")]
    elif wgrad:
        cmd += [os.path.join(TESTS, "wgrad_launch_driver.cpp")]
    elif optim:
        cmd += ["-DMTE_REC_PLAIN_ARGS", os.path.join(csrc, "optim.hip"), os.path.join(TESTS, "optim_launch_driver.cpp")]
    else:
        cmd += [os.path.join(TESTS, "conv_launch_driver.cpp")]
    cmd += ["-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, case_lines):
    """-> the driver's output lines, one per case"""
    out = subprocess.run([exe], input="\n".join(case_lines) + "\n", capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("recorder failed: " + out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(case_lines)
    return lines


def splitk_workspace_elems(M, N):
    """what kernels._splitk_workspace offers for an [M][N] output"""
    return 0 if ((M + 127) // 128) * ((N + 127) // 128) >= 384 else SPLITK_SLABS * M * N


def round8(c):
    return (c + 7) // 8 * 8


def case(entry, dtype, B, H, W, cin_p, N, k, ldx=None, out_f32=0, ws=None, accumulate=0, knobs=None):
    """ws: None = no workspace, else the element count offered with a non-null pointer"""
    ks = ",".join("%d=%d" % kv for kv in knobs) if knobs else "-"
    return "%s %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % (entry, dtype, B, H, W, cin_p, N, k, k, cin_p if ldx is None else ldx, out_f32,
                                                             0 if ws is None else 1, ws or 0, accumulate, ks)


def training_shapes():
    """every mte_conv2d_igemm / mte_conv2d_igemm_unshuffle shape of the T8 training step (profiles/r06_v7_conv_table.txt)"""
    seen = []
    with open(os.path.join(ROOT, "profiles", "r06_v7_conv_table.txt")) as f:
        for line in f:
            m = re.search(r"(mte_conv2d_igemm(?:_unshuffle)?)\s+B,H,W,Cin_p,N,KH,KW=\((.*)\)", line)
            if m:
                key = (m.group(1),) + tuple(int(v) for v in m.group(2).split(","))
                if key not in seen:
                    seen.append(key)
    return seen


# ---- the shapes and knob settings of tests/test_gpu_conv_variants.py and tools/igemm_ablate.py, igemm8_check.py, igemm_race_stress.py (cin, cout, k, B, H, W[, ldx])
T_256 = [(64, 128, 3, 2, 24, 40), (96, 256, 3, 3, 10, 52), (32, 128, 5, 1, 30, 33), (128, 384, 1, 2, 16, 48)]
T_PP = [(256, 256, 3, 8, 48, 160), (64, 256, 5, 2, 96, 320), (96, 512, 3, 3, 10, 52), (128, 256, 1, 8, 48, 160), (32, 256, 1, 2, 16, 48), (64, 512, 1, 1, 24, 40),
        (96, 256, 1, 2, 10, 52)]
T_SPLIT = [(512, 256, 3, 4, 32, 40), (1024, 512, 3, 2, 40, 64)]
T_192 = [(32, 72, 3, 2, 24, 40), (64, 88, 3, 1, 30, 33), (96, 96, 1, 2, 16, 48), (32, 72, 3, 1, 17, 31)]
T_IGEMM8 = [(64, 256, 3, 2, 24, 40, None), (96, 256, 3, 3, 10, 52, None), (32, 384, 5, 1, 17, 33, None), (128, 384, 1, 2, 16, 48, None),
            (256, 256, 3, 2, 48, 80, None), (64, 200, 3, 2, 40, 64, 96), (128, 128, 3, 2, 48, 96, None), (96, 128, 3, 1, 33, 47, None),
            (512, 104, 3, 1, 24, 80, None), (160, 136, 3, 1, 31, 45, 200), (32, 128, 7, 1, 64, 96, None), (1024, 512, 3, 1, 12, 40, None)]
TOOL_ABLATE = [(512, 512, 3, 8, 24, 80), (256, 256, 3, 8, 48, 160), (128, 128, 3, 8, 96, 320), (512, 128, 5, 8, 48, 160)]
TOOL_CHECK = T_IGEMM8 + [(32, 256, 3, 1, 30, 33, None), (256, 256, 3, 8, 48, 160, None), (64, 256, 5, 4, 96, 320, None), (384, 256, 3, 2, 48, 160, None),
                         (128, 512, 3, 8, 24, 80, None), (256, 256, 1, 8, 48, 160, None), (128, 128, 3, 2, 96, 320, None), (2048, 256, 3, 2, 12, 40, None)]
TOOL_BENCH = [(32, 128, 7, 192, 640), (4096, 256, 3, 24, 80), (8192, 512, 3, 12, 40), (256, 4096, 3, 24, 80), (512, 8192, 3, 12, 40), (512, 128, 5, 48, 160),
              (64, 256, 5, 96, 320), (128, 512, 5, 48, 160), (64, 104, 3, 192, 640), (512, 768, 3, 24, 80), (128, 200, 3, 96, 320), (768, 512, 3, 24, 80),
              (256, 384, 3, 48, 160), (128, 128, 3, 96, 320), (512, 512, 3, 24, 80), (384, 256, 3, 48, 160), (256, 256, 3, 48, 160), (512, 256, 3, 24, 80),
              (64, 128, 3, 96, 320), (256, 128, 3, 48, 160), (128, 256, 3, 48, 160), (256, 512, 3, 24, 80), (512, 512, 3, 12, 40), (128, 128, 1, 96, 320),
              (256, 256, 1, 48, 160), (512, 512, 1, 24, 80), (192, 128, 3, 96, 320), (128, 192, 3, 96, 320)]
TOOL_RACE = T_256 + [(256, 256, 3, 8, 48, 160), (64, 256, 5, 4, 96, 320), (384, 256, 3, 2, 48, 160), (128, 512, 3, 8, 24, 80), (256, 256, 1, 8, 48, 160)]


def cases():
    out = []

    def add(*a, **kw):
        c = case(*a, **kw)
        if c not in out:
            out.append(c)

    # ---- the training step: with the workspace kernels._splitk_workspace passes and with none, solo or not, bf16 and fp32
    for entry, B, H, W, cin_p, N, kh, kw in training_shapes():
        M = B * H * W
        if entry == "mte_conv2d_igemm_unshuffle":
            for dtype in (BF16, F32):
                for acc in (0, 1):
                    add("unshuffle", dtype, B, H, W, cin_p, N, kh, accumulate=acc)
            continue
        for dtype in (BF16, F32):
            for ws in (splitk_workspace_elems(M, N) or None, None):
                for acc in (0, SOLO):
                    add("igemm", dtype, B, H, W, cin_p, N, kh, ws=ws, accumulate=acc)

    for entry in ("igemm", "sparse", "unshuffle"):                      # an element type the library does not have
        add(entry, 2, 8, 48, 160, 256, 256, 3)

    # ---- tests/test_gpu_conv_variants.py (K.conv_forward: solo launches; with and without accumulation the choice is the same, one of the two is recorded)
    for cin, cout, k, B, H, W in T_256:
        for big in (0, 1, 2):
            kn = [(6, big), (23, 0), (7, 1)]
            add("igemm", BF16, B, H, W, round8(cin), cout, k, accumulate=SOLO, knobs=kn)
            if round8(cin) % 128 == 0:
                add("igemm", BF16, B, H, W, cout, round8(cin), k, accumulate=SOLO, knobs=kn)
    for cin, cout, k, B, H, W in T_PP:
        for big, pp in ((0, 0), (2, 1), (2, 0)):
            add("igemm", BF16, B, H, W, round8(cin), cout, k, accumulate=SOLO, knobs=[(6, big), (23, 0), (7, 1), (21, pp)])
    for cin, cout, k, B, H, W in T_SPLIT:
        for big in (2, 0):
            add("igemm", BF16, B, H, W, cin, cout, k, ws=splitk_workspace_elems(B * H * W, cout) or None, accumulate=SOLO, knobs=[(6, big), (23, 0)])
    for cin, cout, k, B, H, W in T_192:
        for big in (0, 3):
            add("igemm", BF16, B, H, W, round8(cin), cout, k, accumulate=SOLO, knobs=[(6, big), (23, 0), (7, 1)])
    for cin, cout, k, B, H, W, ldx in T_IGEMM8:
        M = B * H * W
        for v8 in (0, 39, 7):
            for split in (False, True):
                add("igemm", BF16, B, H, W, round8(cin), cout, k, ldx=ldx, ws=8 * M * cout if split else None, accumulate=SOLO,
                    knobs=[(23, v8), (24, 1000000 if split else 1), (6, 0)])
        if round8(cin) % 64 == 0:
            for one in (1, 0):
                for split in (False, True):
                    add("igemm", BF16, B, H, W, round8(cin), cout, k, ldx=ldx, ws=8 * M * cout if split else None, accumulate=SOLO,
                        knobs=[(23, 39), (6, 0), (28, one), (24, 1000000 if split else 1)])

    # ---- tools/igemm_ablate.py, igemm8_check.py, igemm_race_stress.py
    for big in (2, 1, 0):
        for cin, cout, k, B, H, W in TOOL_ABLATE:
            for abl in (0, 1, 2, 4, 3, 5, 6, 7):
                add("igemm", BF16, B, H, W, cin, cout, k, accumulate=SOLO, knobs=[(15, 4), (6, big), (7, 100 if big == 2 else 224), (17, abl)])
    for cin, cout, k, B, H, W, ldx in TOOL_CHECK:
        M = B * H * W
        for split in (False, True):
            for v8 in (0, 39, 7):
                add("igemm", BF16, B, H, W, round8(cin), cout, k, ldx=ldx, ws=8 * M * cout if split else None, accumulate=SOLO,
                    knobs=[(23, v8), (24, 1000000 if split else 1), (6, 0)])
    for cin, cout, k, H, W in TOOL_BENCH:
        for v8 in (0, 3, 7, 35):
            add("igemm", BF16, 8, H, W, cin, cout, k, ws=splitk_workspace_elems(8 * H * W, cout) or None, accumulate=SOLO, knobs=[(23, v8)])
    for cin, cout, k, B, H, W in TOOL_RACE:
        for big, pp, v8 in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (0, 0, 39), (0, 0, 7)):
            add("igemm", BF16, B, H, W, round8(cin), cout, k, accumulate=SOLO, knobs=[(6, big), (7, 1), (21, pp), (23, v8), (24, 1)])

    # ---- boundaries, one group at a time around three base shapes (B, H, W, Cin_p, N, k); fp32 beside bf16 on the first
    bases = [(8, 48, 160, 256, 256, 3), (8, 24, 80, 512, 512, 3), (8, 96, 320, 128, 128, 3)]
    for i, (B, H, W, cin_p, N0, k) in enumerate(bases):
        M = B * H * W
        for dtype in (BF16, F32) if i == 0 else (BF16,):
            wss = (None, 8 * M) if dtype == BF16 else (None,)              # (slabs per output element)
            for n in (32, 33, 64, 65, 68, 96, 97, 128, 129, 200, 256, 328, 384, 456):
                for ws in wss:
                    add("igemm", dtype, B, H, W, cin_p, n, k, ws=ws and ws * n)
            for c in (8, 24, 32, 40, 64, 72, 512, 8192):
                for ws in wss:
                    add("igemm", dtype, B, H, W, c, N0, k, ws=ws and ws * N0)
            for kk in (1, 3, 5, 7):
                for ws in wss:
                    add("igemm", dtype, B, H, W, cin_p, N0, kk, ws=ws and ws * N0)
            for ws in (0, M * N0, 2 * M * N0, 8 * M * N0):
                for acc in (0, SOLO):
                    add("igemm", dtype, B, H, W, cin_p, N0, k, ws=ws, accumulate=acc)
            for n in (32, 96, 128, 256):
                add("igemm", dtype, B, H, W, cin_p, n, k, out_f32=1, ws=8 * M * n)
                add("sparse", dtype, B, H, W, cin_p, n, k, accumulate=SOLO)
            for n in (32, 128, 256, 512, 100):
                for c in (cin_p, 40):
                    add("unshuffle", dtype, B, H, W, c, n, k)
    # every knob away from its default, on the first base shape (and where it steers the split-K rule, on two few-tile shapes)
    knob_sets = [[(23, 0)], [(23, 0), (6, 0)], [(23, 0), (6, 1)], [(23, 0), (6, 2)], [(23, 0), (21, 0)], [(23, 19)], [(23, 23)], [(23, 55)], [(23, 50)], [(23, 49)],
                 [(0, 0)], [(0, 2)], [(32, 0)], [(15, 1), (23, 0)], [(15, 3), (23, 0)], [(15, 4), (23, 0)], [(19, 0), (23, 0)], [(19, 1000), (23, 0)], [(29, 0)],
                 [(29, 1000)], [(28, 0)], [(24, 1)], [(24, 1000000)], [(7, 1)], [(7, 1000000)], [(7, 1), (23, 0)], [(7, 1000000), (23, 0)]]
    B, H, W, cin_p, N0, k = bases[0]
    M = B * H * W
    for kn in knob_sets:
        for n in (32, 128, 256):
            for ws in (None, 8 * M * n):
                add("igemm", BF16, B, H, W, cin_p, n, k, ws=ws, accumulate=SOLO if kn[0][0] in (15, 19) and ws is None else 0, knobs=kn)
        for b2, h2, w2 in ((8, 24, 80), (8, 12, 40)):
            add("igemm", BF16, b2, h2, w2, 512, 512, 3, ws=8 * b2 * h2 * w2 * 512, knobs=kn)
        if kn[0][0] in (0, 32):                                            # the loader knobs: every form that has another loader, and the forms that need one
            for dtype, c, n in ((F32, cin_p, 32), (F32, cin_p, 64), (F32, cin_p, 128), (BF16, cin_p, 64), (BF16, 40, 64), (BF16, cin_p, 96)):
                add("igemm", dtype, B, H, W, c, n, k, knobs=kn)
            add("unshuffle", BF16, B, H, W, cin_p, 128, k, knobs=kn)
            add("sparse", BF16, B, H, W, cin_p, N0, k, knobs=kn)
    # tile counts on both sides of every threshold, for each tile height (one image row of M pixels; 384: where choose_splits stops splitting four-wave tiles)
    for height, ns, ts in ((128, (128,), (96, 128, 200, 224, 256, 384, 512)), (192, (96,), (96, 128, 200, 224, 256, 512)), (256, (128, 256), (96, 128, 200, 224, 256, 512))):
        for t in ts:
            for M in (height * (t - 1), height * (t - 1) + 1):
                for n in ns:
                    for ws in (None, 8 * M * n):
                        for kn in (None, [(23, 0)]):
                            add("igemm", BF16, 1, 1, M, 256, n, 3, ws=ws, knobs=kn)
                if height == 256:
                    add("igemm", BF16, 1, 1, M, 64, 256, 1, ws=8 * M * 256)                  # (two K-steps: too short a reduction to split)
                    add("igemm", BF16, 1, 1, M, 64, 128, 3, knobs=[(23, 0)])               # (18 K-steps: the two-workgroup ring of the 256 x 128 tile)
    # one ldx on each side of the activation bound, one Cin_p on each side of the weight bound (both 0x7ff00000 bytes), for every form that asks
    for dtype, es in ((BF16, 2), (F32, 4)):
        for B, H, W, cin_p, n, k in ((8, 48, 160, 256, 256, 3), (8, 48, 160, 256, 32, 3), (8, 48, 160, 256, 96, 3)):
            M = B * H * W
            edge = ((0x7ff00000 - 1) // es - cin_p) // (M - 1)                          # largest ldx inside the bound
            for ldx in (edge // 8 * 8, edge // 8 * 8 + 8):
                for kn in (None, [(23, 0)]):
                    add("igemm", dtype, B, H, W, cin_p, n, k, ldx=ldx, knobs=kn)
                add("unshuffle", dtype, B, H, W, cin_p, n, k, ldx=ldx)
        for n, k in ((512, 7), (32, 7)):
            edge = (0x7ff00000 - 1) // es // (n * k * k)
            for c in (edge // 64 * 64, edge // 64 * 64 + 64):
                for kn in (None, [(23, 0)]):
                    add("igemm", dtype, 1, 16, 32, c, n, k, knobs=kn)
    return out


# ---- GroupNorm (--gn): (B, C, H, W) of tests/test_gpu_groupnorm.py and tests/test_gpu_handoff_fences.py
GN_TEST = [(2, 512, 24, 80), (3, 512, 12, 40), (2, 256, 24, 40), (1, 128, 16, 24), (9, 256, 8, 16), (2, 64, 32, 64), (3, 32, 64, 64), (2, 128, 96, 320), (8, 512, 24, 80),
           (8, 256, 48, 160), (5, 128, 48, 160), (3, 256, 23, 79), (12, 512, 24, 80)]
GN_TEST_TAIL = [(2, 32, 64, 64), (8, 64, 96, 160), (3, 64, 37, 52), (3, 64, 74, 104)]            # (the tail tests' other shapes are in GN_TEST)


def gn_training_shapes():
    """(B, HW, C) of every GroupNorm of the T8 training step, bench.py's size (PackNetSAN01: ni, n1 .. n5 = 32, 32, 64, 128, 256, 512 at 384 x 1280 and the five
    halvings below it; these are also the layer classes of tools/gn_bench.py, overlap_probe.py and inloop_clock.py)"""
    H, W = 384, 1280
    return [(8, H * W, 32)] + [(8, (H >> i) * (W >> i), c) for i, cs in ((1, (32, 64)), (2, (64, 128)), (3, (128, 256)), (4, (256, 512)), (5, (512,))) for c in cs]


def gn_case(entry, dtype, B, HW, C, second=0, dbias=0, ready=0, prezeroed=0, knobs=None):
    return "%s %d %d %d %d %d %d %d %d %s" % (entry, dtype, B, HW, C, second, dbias, ready, prezeroed, ",".join("%d=%d" % kv for kv in knobs) if knobs else "-")


def gn_cases():
    out = []

    def add(B, HW, C, knobs=None, full=False, single=False, dtypes=(BF16, F32)):
        """one shape through the entry points.  full: all four, in every combination of the flags each takes.  Otherwise in every combination of what the form and
        the geometry can depend on -- element type, second tensor, ready statistics -- with the bias gradient on and the buffers not pre-zeroed, i.e. with every
        clear and the larger dynamic LDS (the whole product over every shape would be four times the convolution table).  single: only the two passes that can
        take a slab or a cluster, the forward without ready statistics and the backward."""
        for dtype in dtypes:
            for pz in (0, 1) if full else (0,):
                for second in (0, 1):
                    out.append(gn_case("fwd", dtype, B, HW, C, second, ready=0, prezeroed=pz, knobs=knobs))
                    if full or (second == 0 and not single):
                        out.append(gn_case("fwd", dtype, B, HW, C, second, ready=1, prezeroed=pz, knobs=knobs))
                        out.append(gn_case("stats", dtype, B, HW, C, second, prezeroed=pz, knobs=knobs))
                    if full or (second == 1 and not single):
                        out.append(gn_case("tail", dtype, B, HW, C, second, prezeroed=pz, knobs=knobs))
                for m2 in (0, 1, 2):
                    for dbias in (0, 1) if full else (1,):
                        out.append(gn_case("bwd", dtype, B, HW, C, m2, dbias=dbias, prezeroed=pz, knobs=knobs))

    for B, HW, C in gn_training_shapes():                                  # the whole product on one shape of each form: stream, cluster, slab
        add(B, HW, C, full=(HW, C) in ((96 * 320, 128), (24 * 80, 512), (12 * 40, 512)))
    for B, C, H, W in GN_TEST:                                             # each with the slab kernels on (the default) and off
        add(B, H * W, C)
        add(B, H * W, C, [(13, 0)], single=True)
    for B, C, H, W in GN_TEST_TAIL:
        add(B, H * W, C)
    for B, C, H, W in ((8, 512, 24, 80), (8, 256, 48, 160)):               # test_cluster_route_is_taken_and_is_bit_reproducible
        add(B, H * W, C, [(25, 0)], single=True, dtypes=(BF16,))
    add(8, 24 * 80, 512, [(25, 1000)], single=True, dtypes=(BF16,))                        # the spin limit: changes no launch
    # ---- thresholds.  A slab is HW * cps chunks, cps = chunks per pixel of one group: at C = 512 4 in bf16 and 8 in fp32, at C = 128 1 and 2.
    for hw in (256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097):    # C = 512: the slab kernels' NCH step (2048 chunks), GN_SLAB_MAX, the clusters' 4 -> 8
        add(8, hw, 512, single=True)                                       # and where the cluster rule gives up (256 * nmax chunks per workgroup, nmax = 8 or 4)
    for hw in (8192, 8193, 16384, 16385):                                  # C = 128: the same steps at one and two chunks per pixel
        add(8, hw, 128, single=True)
    for B in (1, 7, 9, 32, 33):                                            # samples per launch: 8; four launches at the most
        add(B, 24 * 80, 512, single=True)
    for C in (64, 128, 256, 1024):                                         # group sizes 4 .. 64 channels: cps 1, 2, 4, 8 and no slab (with 8 x 480 x 512 of the step)
        add(8, 12 * 40, C, single=True)
    add(8, 24 * 80, 1024, single=True)
    for C in (24, 48, 2048, 4096):                                         # refused, or refused in fp32 only (2048)
        add(8, 12 * 40, C)
    for B in (1, 7, 33):                                                   # the statistics grid: capped by MTE_GN_SLOTS (512, 73 against the 74 wanted, 64)
        add(B, 20000, 512, dtypes=(BF16,))
    add(3, 20000, 512, [(3, 1000000)], dtypes=(BF16,))                                     # ... and by 170 slots with a target that asks for more than the rows give
    for kn in ([(2, 16)], [(2, 17)], [(2, 64)], [(3, 512)], [(3, 8192)], [(14, 0)]):      # min_rows (forward: capped at 16), target, zigzag
        add(8, 96 * 320, 128, kn, dtypes=(BF16,))
    seen = set()
    return [c for c in out if not (c in seen or seen.add(c))]

# ---- conv3d pack / unpack (--p3).  (C, B, H, W) of tests/test_gpu_pack3d_variants.py, H and W of the un-packed side
P3_OPS = ("pack_fwd", "pack_bwd_data", "pack_bwd_weight", "unpack_fwd", "unpack_bwd_data", "unpack_bwd_weight")
P3_T_PACK = [(32, 2, 16, 32), (32, 1, 20, 36), (64, 1, 12, 40), (128, 1, 8, 16), (256, 1, 4, 16), (512, 1, 4, 8), (16, 2, 8, 12)]
P3_T_UNPACK = [(32, 2, 12, 20), (32, 1, 17, 33), (64, 1, 9, 40), (128, 1, 8, 16), (256, 1, 5, 16), (512, 1, 4, 8)]
P3_T_UNPACK_BWD = [(32, 2, 16, 32), (32, 1, 17, 33), (32, 3, 8, 16), (32, 1, 1, 1), (32, 1, 9, 47), (64, 1, 12, 48), (64, 2, 5, 19), (64, 1, 4, 16), (32, 2, 96, 160)]
P3_T_UNPACK_FWD = P3_T_UNPACK_BWD + [(128, 1, 7, 21), (128, 2, 8, 16), (256, 1, 5, 16), (256, 2, 3, 33)]
P3_T_PACK_FWD = [(32, 2, 16, 32), (32, 1, 6, 70), (64, 1, 12, 40), (64, 2, 10, 6), (128, 1, 8, 36), (256, 1, 4, 34), (512, 1, 4, 8), (64, 16, 6, 64)]
P3_T_PACK_BWD = [(32, 2, 16, 32), (32, 1, 18, 34), (32, 3, 8, 64), (32, 1, 2, 2), (32, 1, 10, 94), (64, 1, 12, 48), (64, 2, 10, 38), (128, 1, 8, 36), (256, 1, 4, 34),
                 (512, 1, 4, 8), (32, 2, 96, 160), (64, 16, 6, 64)]
# tools/conv3d_bench.py (B = 8), p3_wgrad_bench.py (B = 8: (kind, C, H, W)) and loss_conv3d_race_stress.py
P3_TOOL_BENCH = [("unpack_bwd_data", 32, 192, 640), ("unpack_bwd_data", 64, 96, 320), ("unpack_bwd_data", 128, 48, 160), ("unpack_fwd", 32, 192, 640),
                 ("unpack_fwd", 64, 96, 320), ("unpack_fwd", 128, 48, 160), ("unpack_fwd", 256, 24, 80), ("pack_bwd_data", 32, 192, 640), ("pack_bwd_data", 64, 96, 320),
                 ("pack_bwd_data", 128, 48, 160), ("pack_bwd_data", 256, 48, 160), ("pack_bwd_data", 512, 24, 80), ("pack_fwd", 256, 48, 160), ("pack_fwd", 512, 24, 80)]
P3_TOOL_WGRAD = [("pack", 64, 384, 1280), ("pack", 64, 192, 640), ("pack", 128, 96, 320), ("pack", 256, 48, 160), ("pack", 512, 24, 80), ("unpack", 512, 12, 40),
                 ("unpack", 256, 24, 80), ("unpack", 128, 48, 160), ("unpack", 64, 96, 320), ("unpack", 64, 192, 640)]
P3_TOOL_RACE = [(32, 8, 192, 640), (64, 8, 96, 320), (32, 2, 50, 70)]
P3W_WGS = 512                       # MTE_P3W_WGS (csrc/p3_plan.hpp)


def p3_training_shapes():
    """(op, B, H, W, C, ldx, ldo) of every conv3d pack / unpack call of the T8 training step, bench.py's size (PackNetSAN01 at 8 x 384 x 1280, n1 .. n5 = 32, 64,
    128, 256, 512).  pack1 .. pack3 are folded into their convolution (kernels.PackFoldedConvGnEluFn) and run the conv3d kernels on the exact border bands only,
    top + bottom and left + right as one batch of 16; pack4 and pack5 run them whole.  unpack5 .. unpack1 write their result into the decoder's concat buffers
    (pixel stride: their own channels + the skip's), and their gradient arrives as a slice of such a buffer or as a tensor of its own."""
    out = []
    for C, H, W, k in ((32, 384, 1280, 5), (64, 192, 640, 3), (128, 96, 320, 3)):
        hb = 2 * (k // 2) + 1
        for h, w in ((2 * hb, W), (H, 2 * hb)):
            out += [(op, 16, h, w, C, C, 16 * C) for op in P3_OPS[:3]]
    for C, H, W in ((256, 48, 160), (512, 24, 80)):
        out += [(op, 8, H, W, C, C, 16 * C) for op in P3_OPS[:3]]
    for C, H, W, skip in ((512, 12, 40, 256), (256, 24, 80, 128), (128, 48, 160, 64), (64, 96, 320, 32), (32, 192, 640, 32)):
        for ldo in (C + skip, C):
            out += [(op, 8, H, W, C, C, ldo) for op in P3_OPS[3:]]
    return out


def p3_case(op, dtype, B, H, W, C, ldx=None, ldo=None, knobs=None):
    """ldx, ldo: None = the dense tensors' (C, and 16 C for the pack layers' feature side); knobs: values of mte_debug_set(1, .)"""
    return "%s %d %d %d %d %d %d %d %s" % (op, dtype, B, H, W, C, C if ldx is None else ldx, (16 * C if op.startswith("pack") else C) if ldo is None else ldo,
                                           ",".join("1=%d" % v for v in knobs) if knobs else "-")


def p3_cases():
    out = []

    def add(*a, **kw):
        c = p3_case(*a, **kw)
        if c not in out:
            out.append(c)

    for op, B, H, W, C, ldx, ldo in p3_training_shapes():
        for dtype in (BF16, F32):
            add(op, dtype, B, H, W, C, ldx, ldo)
    for op in P3_OPS:                                                      # an element type the library does not have
        add(op, 2, 8, 48, 160, 256)

    # ---- tests/test_gpu_pack3d_variants.py
    for C, B, H, W in P3_T_PACK:
        for lds in (1, 0):
            for op in P3_OPS[:3]:
                add(op, BF16, B, H, W, C, knobs=[lds])
    for C, B, H, W in P3_T_UNPACK:
        for lds in (0, 1, 2):
            for op in P3_OPS[3:]:
                add(op, BF16, B, H, W, C, knobs=[lds])
    for C, B, H, W in P3_T_UNPACK_BWD:
        for knob in (300, 301, 303, 307):
            add("unpack_bwd_data", BF16, B, H, W, C, knobs=[knob])
    for C, B, H, W in P3_T_UNPACK_FWD:
        for knob in (307, 539) + ((315,) if C <= 64 else ()):
            add("unpack_fwd", BF16, B, H, W, C, knobs=[knob, 2000 + 1024])
        if C <= 64:
            for wgs in (8, 24):
                add("unpack_fwd", BF16, B, H, W, C, knobs=[315, 2000 + wgs])
    for C, B, H, W in P3_T_PACK_FWD:
        for knob in (539, 347):
            add("pack_fwd", BF16, B, H, W, C, knobs=[knob])
    for C, B, H, W in P3_T_PACK_BWD:
        for knob in (411, 539, 555):
            add("pack_bwd_data", BF16, B, H, W, C, knobs=[knob])

    # ---- tools/conv3d_bench.py (its default variants, those its README row names, the output passes), p3_wgrad_bench.py, loss_conv3d_race_stress.py
    seen_ops = set()
    for op, C, H, W in P3_TOOL_BENCH:
        for knob in (300, 411, 539) + ((315, 331, 347) if op not in seen_ops else ()):       # (the other variants on the first shape of each op)
            add(op, BF16, 8, H, W, C, knobs=[knob])
        seen_ops.add(op)
        if op == "unpack_fwd":
            for passes in (1, 2, 4):
                add(op, BF16, 8, H, W, C, knobs=[539, 3000 + passes])
    for kind, C, H, W in P3_TOOL_WGRAD:
        for mfma, small in ((0, 1), (1, 0), (1, 1)):
            add(kind + "_bwd_weight", BF16, 8, H, W, C, knobs=[200 + mfma, 100 + small])
    for C, B, H, W in P3_TOOL_RACE:
        for op in ("unpack_fwd", "unpack_bwd_data"):
            add(op, BF16, B, H, W, C)

    # ---- thresholds, one group at a time
    for C in (8, 16, 24, 32, 64, 128, 256, 512, 1024):                     # every C the library takes, one between and one above (refused)
        for op in P3_OPS:
            for dtype in (BF16, F32):
                add(op, dtype, 2, 24, 40, C)
            for knobs in ([0], [1]) + (([300], [555]) if op.endswith("_data") else ([300], [331]) if op.endswith("_fwd") else ()):
                add(op, BF16, 2, 24, 40, C, knobs=knobs)
    for H, W in ((23, 40), (24, 39), (1, 1), (2, 2)):                      # odd H or W: refused by the pack forward alone
        for op in P3_OPS:
            add(op, BF16, 2, H, W, 64)
            add(op, F32, 2, H, W, 64)
    # tile counts on both sides of a whole tile: every tile is 1 .. 16 rows of 2 .. 32 pixels, so a 32 x 64 volume is whole tiles of every shape and 33 x 65 one
    # row and one column more (pack: the packed side, half of H and W).  Tiles: p3_tile small and large, 2 x 16 (taps in K), 4 x 16 (banded) for pack; up_tile
    # whole and halved, up4_tile, 256 / C x 16 (taps in K), 8 or 4 x 16 (banded) for unpack
    per_op = {"pack_fwd": ([347], [100]), "pack_bwd_data": ([411], [100]), "pack_bwd_weight": ([100], [100, 200], [200]),          # (what steers each op's tiles)
              "unpack_fwd": ([315], [300]), "unpack_bwd_data": ([301], [300], [1]), "unpack_bwd_weight": ([100], [100, 200], [200])}
    for C in (32, 64, 128, 256, 512):
        for d in (0, 1):
            for op in P3_OPS:
                for knobs in (None,) + per_op[op]:
                    if op.startswith("pack"):
                        add(op, BF16, 3, 2 * (32 + d), 2 * (64 + d), C, knobs=knobs)
                    else:
                        add(op, BF16, 3, 32 + d, 64 + d, C, knobs=knobs)
    # ntiles on both sides of every workgroup cap: the weight gradients' 512 (LDS kernels; unpack: 1024 with the small tiles), MTE_P3W_WGS, persist_wgs
    for cap in sorted({512, 1024, P3W_WGS}):
        for n in (cap - 1, cap, cap + 1):
            for knobs in (None, [200], [200, 100], [100]):
                add("pack_bwd_weight", BF16, n, 8, 32, 32, knobs=knobs)                      # (one 4 x 16 or 8 x 16 tile per sample)
                add("unpack_bwd_weight", BF16, n, 8, 32, 32, knobs=knobs)                   # (one 8 x 32 or 16 x 32 tile per sample)
    for wgs in (8, 24, 1024):
        for n in (wgs - 1, wgs, wgs + 1):
            add("unpack_fwd", BF16, n, 8, 16, 32, knobs=[315, 2000 + wgs])                   # (one 8 x 16 tile per sample)
    for threads in (256, 512, 1024):                                       # threads of the matrix-core weight gradient
        add("pack_bwd_weight", BF16, 8, 48, 160, 256, knobs=[1000 + threads])
        add("unpack_bwd_weight", BF16, 8, 24, 80, 256, knobs=[1000 + threads])
    # the gather weight gradients' thread caps: 256 * 1024 (pack) and 256 * 2048 (unpack) threads with work
    for W in (2 * 4096 - 2, 2 * 4096, 2 * 4096 + 2):                       # 64 channels: 16 threads per packed pixel
        add("pack_bwd_weight", F32, 4, 2, W, 64)
    for W in (8192 - 1, 8192, 8192 + 1):                                   # 512 channels: 64 threads per pixel
        add("unpack_bwd_weight", F32, 1, 1, W, 512)
    # ldx / ldo one step inside and one step outside each 1 << 30 element bound
    lim = 1 << 30
    for B, H, W, C in ((8, 48, 160, 256), (8, 48, 160, 32)):                                  # pack backward data: (pixels - 1) * ldo + 16 C < lim
        edge = (lim - 1 - 16 * C) // (B * (H // 2) * (W // 2) - 1)
        for ldo in (edge, edge + 1):
            add("pack_bwd_data", BF16, B, H, W, C, ldo=ldo)
    for C in (32, 64):                                                     # banded unpack forward: (pixels - 1) * ldx + C < lim
        edge = (lim - 1 - C) // (8 * 96 * 320 - 1)
        for ldx in (edge, edge + 1):
            add("unpack_fwd", BF16, 8, 96, 320, C, ldx=ldx, knobs=[315])
    edge = (lim - 1 - 32) // (8 * 4 * 192 * 640 - 1)                        # LDS-DMA unpack backward data: (4 pixels - 1) * ldo + 32 < lim
    for ldo in (edge, edge + 1):
        for knobs in (None, [303], [331]):
            add("unpack_bwd_data", BF16, 8, 192, 640, 32, ldo=ldo, knobs=knobs)
    # the grid < 1 << 30 test of the two depth-slab forms: tiles x (4 C / 128) slabs, at C = 512 (16 slabs) with one packed pixel per sample
    for B in (lim // 16 - 1, lim // 16):
        add("pack_fwd", BF16, B, 2, 2, 512)
        add("pack_bwd_data", BF16, B, 2, 2, 512, ldo=8)
    return out


# ---- LDS-patch convolution (--patch).  (cin, cout, k, B, H, W) of tests/test_gpu_conv_variants.py: SHAPES (those that reach the family) and PATCH_M16_SHAPES
PATCH_T_SHAPES = [(32, 32, 7, 2, 16, 64), (512, 32, 5, 1, 12, 32), (3, 32, 5, 2, 20, 64), (65, 32, 3, 1, 9, 96), (64, 64, 3, 2, 16, 32), (32, 64, 1, 2, 8, 64),
                  (97, 64, 3, 1, 24, 32), (1024, 64, 3, 1, 8, 32), (64, 32, 3, 2, 10, 32), (16, 16, 3, 1, 8, 32), (32, 64, 3, 1, 7, 64), (3, 32, 5, 1, 37, 96),
                  (3, 16, 3, 2, 9, 32), (3, 32, 7, 1, 16, 32), (8, 24, 5, 2, 16, 64), (128, 128, 3, 2, 16, 64), (200, 128, 3, 1, 12, 32), (64, 128, 3, 2, 8, 64),
                  (256, 128, 3, 1, 13, 32), (72, 96, 3, 2, 9, 32), (64, 72, 3, 1, 6, 96), (32, 32, 3, 1, 24, 64), (72, 32, 3, 1, 20, 32), (32, 32, 5, 1, 40, 64),
                  (40, 32, 5, 1, 20, 32), (32, 24, 7, 1, 21, 32), (136, 64, 3, 1, 11, 64), (256, 64, 5, 1, 12, 64), (48, 56, 5, 2, 9, 32), (128, 32, 7, 1, 18, 32)]
PATCH_T_M16 = [(32, 32, 7, 2, 16, 64), (128, 32, 7, 1, 18, 32), (256, 64, 5, 1, 12, 64), (48, 56, 5, 2, 9, 32), (64, 64, 3, 2, 16, 32), (32, 64, 1, 2, 8, 64),
               (72, 32, 3, 1, 20, 32), (136, 64, 3, 1, 11, 64), (65, 32, 3, 1, 9, 96), (64, 32, 3, 2, 10, 32)]
# tests/test_gpu_layers.py: (cm, cout, B, H, W) of the rank-1 test, (c1, cp, c2, B, H, W) of the plus-1x1 test
PATCH_T_RANK1 = [(64, 32, 2, 32, 64), (64, 32, 1, 24, 32), (64, 32, 1, 8, 64), (96, 64, 2, 16, 64), (96, 64, 1, 20, 32), (32, 32, 1, 16, 32)]
PATCH_T_PLUS = [(64, 64, 64, 2, 16, 64), (64, 32, 64, 1, 24, 32), (64, 32, 64, 2, 8, 32), (32, 64, 32, 1, 20, 64), (96, 64, 40, 1, 8, 32)]
# tools/inloop_clock.py (cin, cout, k, H, W, pass, knob values), rank1_bench.py (cm, N, H, W), shortcut_fold_bench.py (c1, cp, c2, H, W); B = 8
PATCH_TOOL_CLOCK = [(32, 32, 7, 384, 1280, "fwd", (500, 501)), (64, 32, 3, 192, 640, "fwd", ()), (64, 64, 3, 192, 640, "fwd", ()), (256, 64, 5, 96, 320, "fwd", (500, 501)),
                    (64, 64, 3, 192, 640, "wgrad", ()), (32, 32, 7, 384, 1280, "wgrad", ())]
PATCH_TOOL_RANK1 = [(64, 32, 384, 1280), (96, 64, 192, 640)]
PATCH_TOOL_FOLD = [(64, 32, 64, 192, 640), (64, 64, 64, 192, 640)]
PATCH_WGRAD_WGS, PATCH_WGRAD_WIDE_WGS = 192, 128      # MTE_PATCH_WGRAD_WGS, MTE_PATCH_WGRAD_WIDE_WGS (csrc/patch_plan.hpp)


def patch_training_shapes():
    """(entry, B, H, W, Cin_p, N, k) of every LDS-patch call of the T8 training step, bench.py's size (profiles/r06_v7_conv_table.txt)"""
    seen = []
    with open(os.path.join(ROOT, "profiles", "r06_v7_conv_table.txt")) as f:
        for line in f:
            m = re.search(r"mte_conv2d_patch_(\w+)\s+B,H,W,Cin_p,N,KH,KW=\((.*)\)", line)
            if m:
                key = (m.group(1).replace("fwd_rank1", "rank1").replace("fwd_plus1x1", "plus1x1"),) + tuple(int(v) for v in m.group(2).split(","))[:6]
                if key not in seen:
                    seen.append(key)
    return seen


def patch_wgrad_cap(cin_p, n, k, slabs=True):
    """the slabs kernels.conv_wgrad makes room for"""
    per = n * k * k * cin_p
    wide = 256 if per <= (1 << 18) else (64 if per <= (1 << 19) else 32)
    return max(1, min(512, (192 << 20) // (4 * per))) if slabs else max(1, min(wide, (96 << 20) // (4 * per)))


def patch_wgrad_sl(cin_p, n, k):
    """32-channel input slices a workgroup of the weight gradient takes, with the knobs at their defaults (plan_patch, csrc/patch_plan.hpp)"""
    if k == 3 and n <= 64 and 64 < cin_p <= 96:
        return 3
    return 2 if n > 64 or (k <= 3 or k == 5 and n <= 32) and cin_p > 32 else 1


def patch_case(entry, B, H, W, cin_p, N, kh, kw=None, ldx=None, acc=0, bias=0, C2=0, cap=0, shared=1, knobs=None):
    """bias: -1 = none, else its offset from a 16-byte boundary; knobs: values of mte_debug_set(11, .), or (key, value) pairs"""
    ks = ",".join("%d=%d" % (kv if isinstance(kv, tuple) else (11, kv)) for kv in knobs) if knobs else "-"
    return "%s %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % (entry, B, H, W, cin_p, N, kh, kh if kw is None else kw, cin_p if ldx is None else ldx, acc, bias, C2, cap,
                                                             shared, ks)


def patch_cases():
    out = []

    def add(*a, **kw):
        c = patch_case(*a, **kw)
        if c not in out:
            out.append(c)

    def layer(cin_p, n, k, B, H, W, knobs=None):
        """what K.ConvFn runs for one layer: forward, data gradient (the transposed layer, no bias), weight gradient -- each only where the library's query
        sends it to this family"""
        add("fwd", B, H, W, cin_p, n, k, knobs=knobs)
        add("fwd", B, H, W, n, cin_p, k, bias=-1, knobs=knobs)
        add("wgrad", B, H, W, cin_p, n, k, cap=patch_wgrad_cap(cin_p, n, k), knobs=knobs)

    # ---- the training step
    for entry, B, H, W, cin_p, N, k in patch_training_shapes():
        add("supported", B, H, W, cin_p, N, k)
        add("wgrad_supported", B, H, W, cin_p, N, k)
        if entry == "fwd":
            for acc in (0, 1):
                for bias in (0, -1):
                    add("fwd", B, H, W, cin_p, N, k, acc=acc, bias=bias)
        elif entry == "fwd_gn":
            for acc in (0, 1):
                add("fwd_gn", B, H, W, cin_p, N, k, acc=acc)
            add("gn_elems", B, H, W, cin_p, N, k)
        elif entry == "rank1":
            add("rank1_ok", B, H, W, cin_p, N, k)
            add("rank1", B, H, W, cin_p, N, k)
        elif entry == "plus1x1":
            for c2 in (32, 64):
                add("plus1x1", B, H, W, cin_p, N, k, bias=-1, C2=c2)
        else:
            for shared in (1, 0):
                for slabs in (True, False):
                    add("wgrad", B, H, W, cin_p, N, k, cap=patch_wgrad_cap(cin_p, N, k, slabs), shared=shared)
        if entry == "fwd":
            add("repack", B, H, W, cin_p, N, k)
            add("pack_elems", B, H, W, cin_p, N, k)

    # ---- tests/test_gpu_conv_variants.py, tests/test_gpu_layers.py
    for cin, cout, k, B, H, W in PATCH_T_SHAPES:
        layer(round8(cin), cout, k, B, H, W)
    for cin, cout, k, B, H, W in PATCH_T_M16:
        layer(round8(cin), cout, k, B, H, W, knobs=[500, 600, 700])         # (the test's other half sets the defaults: the lines above)
    for cm, cout, B, H, W in PATCH_T_RANK1:
        add("rank1_ok", B, H, W, cm, cout, 3)
        add("rank1", B, H, W, cm, cout, 3)
        add("fwd", B, H, W, cm, cout, 3, acc=1)
    for c1, cp, c2, B, H, W in PATCH_T_PLUS:
        add("fwd", B, H, W, c2, cp, 1, bias=-1)
        add("fwd", B, H, W, c1, cp, 3, acc=1, bias=-1)
        add("plus1x1", B, H, W, c1, cp, 3, bias=-1, C2=c2)
    # ---- tools/inloop_clock.py, rank1_bench.py, shortcut_fold_bench.py
    for cin, cout, k, H, W, what, values in PATCH_TOOL_CLOCK:
        for v in values or (None,):
            add(what, 8, H, W, cin, cout, k, cap=patch_wgrad_cap(cin, cout, k) if what == "wgrad" else 0, knobs=v and [v])
    for cm, N, H, W in PATCH_TOOL_RANK1:
        add("rank1", 8, H, W, cm, N, 3)
        add("fwd", 8, H, W, cm, N, 3, acc=1)
    for c1, cp, c2, H, W in PATCH_TOOL_FOLD:
        add("fwd", 8, H, W, c2, cp, 1, bias=-1)
        add("fwd", 8, H, W, c1, cp, 3, acc=1, bias=-1)
        add("plus1x1", 8, H, W, c1, cp, 3, bias=-1, C2=c2)

    # ---- thresholds, one group at a time (B = 2, W = 64 unless the group is about them)
    for cin_p in (8, 32, 40, 64, 72, 96, 104):                            # every class of Cin_p x N x K; every knob at 0 where it is asked
        for n in (8, 32, 40, 64, 72, 128, 136):
            if (cin_p == 8) != (n == 8) and not (cin_p == 8 and n == 32):
                continue
            for k in (1, 3, 5, 7):
                if cin_p in (8, 32, 64):
                    add("supported", 2, 24, 64, cin_p, n, k)
                    for knobs in (None, [300]) if n > 64 and k == 3 else (None,):
                        add("wgrad_supported", 2, 24, 64, cin_p, n, k, knobs=knobs)
                if n <= 64:
                    for knobs in (None, [400]) + (([0], [500], [600], [700]) if cin_p in (32, 72) else ()):
                        add("fwd", 2, 24, 64, cin_p, n, k, knobs=knobs)
                if n <= 64 or n <= 128 and k == 3:                         # (beyond: refused whatever the knobs, as the queries' lines say)
                    for knobs in (None, [200]) + (([300],) if n > 64 else ()):
                        add("wgrad", 2, 24, 64, cin_p, n, k, cap=64, knobs=knobs)
            if n <= 64:
                for entry, k0 in (("rank1_ok", ([400],)), ("rank1", ([0], [400], [700])), ("plus1x1", ([0], [400], [600], [700])), ("fwd_gn", ([0], [400]))):
                    for knobs in (None,) + (k0 if cin_p in (32, 72) else k0[:1]):
                        add(entry, 2, 24, 64, cin_p, n, 3, C2=32 if entry == "plus1x1" else 0, knobs=knobs)
    for H in (15, 16):                                                     # tall tiles from 16 rows on (one output tile only); 14 / 16 for the rank-1 term, which wants H even
        for cin_p, n, k in ((32, 32, 3), (32, 32, 5), (40, 32, 5), (40, 32, 3), (32, 64, 3), (72, 64, 3), (32, 32, 1), (32, 32, 7), (40, 32, 7)):
            for acc in (0, 1):
                add("fwd", 2, H, 64, cin_p, n, k, acc=acc)
                add("fwd_gn", 2, H, 64, cin_p, n, k, acc=acc)
            add("fwd", 2, H, 64, cin_p, n, k, knobs=[0])
            add("wgrad", 2, H, 64, cin_p, n, k, cap=64)
            if k == 3:
                for h in (H, H - 1):
                    add("rank1_ok", 2, h, 64, cin_p, n, 3)
                    add("rank1", 2, h, 64, cin_p, n, 3)
                add("plus1x1", 2, H, 64, cin_p, n, 3, C2=16)
    for n in (16, 24, 40, 48):                                             # GroupNorm records want whole groups of N / 16 channels
        add("fwd_gn", 2, 24, 64, 32, n, 3)
    for kh, kw in ((2, 2), (4, 4), (3, 5), (3, 1), (9, 9)):          # even, mixed and other kernel sizes: refused
        for entry in ("supported", "wgrad_supported", "fwd", "fwd_gn", "wgrad"):
            for n in (32, 128) if "supported" in entry or entry == "wgrad" else (32,):
                add(entry, 2, 24, 64, 64, n, kh, kw, cap=64)
    for W in (32, 33, 48):                                             # W % 32
        for entry in ("supported", "wgrad_supported", "fwd", "fwd_gn", "rank1_ok", "rank1", "plus1x1", "wgrad"):
            add(entry, 2, 24, W, 64, 32, 3, C2=16, cap=64)
        add("wgrad", 2, 24, W, 64, 128, 3, cap=64)
    for cin_p, n in ((12, 32), (32, 12), (0, 32), (32, 0)):                # channel counts that are no multiple of 8, or none
        for entry in ("supported", "wgrad_supported", "fwd", "wgrad"):
            if "wgrad" not in entry or cin_p:                              # (no input channels, no slices to deal the groups over: the parent's query said yes and its launch divided by zero; now refused)
                add(entry, 2, 24, 64, cin_p, n, 3, cap=64)
    for B, H, W in ((0, 24, 64), (2, 0, 64), (2, 24, 0), (1, 1, 32)):      # empty tensors are refused nowhere: an empty grid
        for entry in ("fwd", "fwd_gn", "gn_elems", "rank1", "plus1x1", "wgrad"):
            add(entry, B, H, W, 32, 32, 3, C2=16, cap=64)
    for c2 in (0, 4, 8, 12, 16, 72):                                       # channels of the 1x1 term
        add("plus1x1", 2, 24, 64, 64, 32, 3, C2=c2)
    for bias in (-1, 0, 4):                                            # the second form reads the bias in 16-byte groups
        for entry, cin_p, n, k in (("fwd", 32, 32, 5), ("fwd", 72, 64, 3), ("fwd", 32, 64, 3), ("fwd_gn", 32, 32, 3), ("rank1_ok", 64, 32, 3), ("rank1", 64, 32, 3),
                                   ("plus1x1", 64, 32, 3)):
            add(entry, 2, 24, 64, cin_p, n, k, bias=bias, C2=16)
    # one ldx on each side of the second form's 0x7ff00000-byte bound
    for B, H, W, cin_p, n, k in ((8, 384, 1280, 32, 32, 7), (8, 192, 640, 96, 64, 3), (8, 192, 640, 64, 32, 3)):
        edge = ((0x7ff00000 - 1) // 2 - cin_p) // (B * H * W - 1)
        for ldx in (edge // 8 * 8, edge // 8 * 8 + 8):
            for entry in ("fwd", "fwd_gn") + (("rank1_ok", "rank1", "plus1x1") if k == 3 else ()):
                add(entry, B, H, W, cin_p, n, k, ldx=ldx, C2=16)
            add("wgrad", B, H, W, cin_p, n, k, ldx=ldx, cap=512)
    # the weight gradient's groups: want = wgs (x 2 alone on the chip) over the slices, capped by the tiles and by the slabs there is room for
    for i, (cin_p, n, k) in enumerate(((64, 32, 3), (128, 128, 3), (96, 64, 3), (32, 32, 7), (256, 64, 5), (256, 32, 5))):
        for shared in (1, 0):
            for knobs in (None, [128], [384]) if i < 2 else (None,):
                wgs = PATCH_WGRAD_WIDE_WGS if n > 64 else knobs[0] if knobs else PATCH_WGRAD_WGS
                g = -(-wgs * (1 if shared else 2) // -(-cin_p // (32 * patch_wgrad_sl(cin_p, n, k))))
                for cap in (0, 1, g - 1, g, g + 1):
                    add("wgrad", 8, 192, 640, cin_p, n, k, cap=cap, shared=shared, knobs=knobs)
        for B, H, W in ((1, 8, 32), (1, 9, 32), (2, 16, 64)):           # fewer tiles than groups
            add("wgrad", B, H, W, cin_p, n, k, cap=512)
    # the instances few calls reach: the first form where the second would be taken (a bias 4 bytes off a 16-byte boundary; knob 400), the 32x32x16 MFMA forms
    # (500 / 600 / 700), each with and without accumulation, in 8-row and in 16-row tiles (one output tile only)
    for k in (1, 3, 5, 7):
        for n, H, cin_p in ((32, 8, 32), (32, 16, 32), (64, 8, 32), (64, 8, 72)):
            if n == 64 and (k == 7 or cin_p == 72 and k != 3):
                continue
            for bias, knobs in ((4, None), (0, [500, 600, 700]), (0, [400, 600])):
                for acc in (0, 1):
                    add("fwd", 2, H, 64, cin_p, n, k, acc=acc, bias=bias, knobs=knobs)
                if k == 3 and cin_p == 32:
                    add("plus1x1", 2, H, 64, cin_p, n, 3, bias=bias, C2=16, knobs=knobs)
            if k == 3:
                add("rank1", 2, H, 64, cin_p, n, 3, knobs=[700])
    # a knob soup and the reset: what mte_debug_set(33, 0) has to undo
    for entry, cin_p, n, k in (("fwd", 32, 32, 5), ("wgrad", 96, 64, 3), ("plus1x1", 64, 32, 3)):
        add(entry, 8, 192, 640, cin_p, n, k, C2=32, cap=512, knobs=[0, 128, 200, 300, 400, 500, 600, 700])
    return out


# ---- weight gradient (--wgrad): mte_conv2d_wgrad and its query.  (cin, cout, k, B, H, W) of tests/test_gpu_conv_variants.py: WGRAD_SHAPES, the launch-width test,
# the stage test (with its element type); WGRAD9_SHAPES: (cin, cout, B, H, W, input as a slice of a buffer 64 channels wider)
WGRAD_T_SHAPES = [(128, 128, 3, 2, 16, 64), (72, 96, 3, 2, 9, 40), (256, 64, 3, 1, 12, 32), (64, 128, 1, 3, 7, 24), (40, 256, 5, 1, 6, 168), (512, 512, 3, 1, 8, 20),
                  (136, 264, 3, 2, 5, 80), (64, 64, 7, 1, 9, 48), (256, 256, 3, 2, 12, 32), (128, 256, 3, 2, 9, 40), (256, 128, 3, 1, 6, 168), (512, 256, 1, 2, 10, 24)]
WGRAD_T_NINE = [(128, 128, 2, 16, 64, False), (256, 256, 2, 12, 32, False), (128, 256, 2, 8, 80, False), (512, 512, 1, 8, 48, False), (192, 128, 1, 6, 160, True),
                (64, 384, 3, 10, 32, False), (256, 128, 1, 5, 64, True), (64, 128, 8, 24, 80, False), (2048, 128, 16, 3, 160, False), (128, 128, 1, 1, 32, False)]
WGRAD_T_WIDTH = [(256, 256, 3, 2, 24, 64), (64, 64, 3, 1, 32, 64), (32, 32, 7, 1, 16, 64), (128, 128, 3, 1, 16, 96)]
WGRAD_T_STAGE = [(128, 128, 3, BF16, 1, 24, 32), (64, 64, 5, BF16, 1, 48, 32), (256, 256, 1, BF16, 1, 48, 32), (32, 32, 3, BF16, 1, 48, 32), (64, 64, 3, F32, 1, 48, 32)]
WGRAD_WGS, W9_WGS = 512, 128        # MTE_WGRAD_WGS, MTE_W9_WGS (csrc/wgrad_plan.hpp)
DESC_BOUND = 0x7ff00000             # bytes a buffer descriptor addresses


def wgrad_training_shapes():
    """(B, H, W, Cin_p, N, KH, KW) of every mte_conv2d_wgrad call of the T8 training step, bench.py's size (profiles/r06_v7_conv_table.txt)"""
    seen = []
    with open(os.path.join(ROOT, "profiles", "r06_v7_conv_table.txt")) as f:
        for line in f:
            m = re.search(r"mte_conv2d_wgrad\s+B,H,W,Cin_p,N,KH,KW=\((.*)\)", line)
            if m:
                key = tuple(int(v) for v in m.group(1).split(","))
                if key not in seen:
                    seen.append(key)
    return seen


def wgrad_stage_cap(cin_p, n, kh, kw):
    """the slabs kernels._conv_wgrad makes room for in front of mte_conv2d_wgrad"""
    per = n * kh * kw * cin_p
    wide = 256 if per <= (1 << 18) else (64 if per <= (1 << 19) else 32)
    return max(1, min(wide, (96 << 20) // (4 * per)))


def wgrad_case(entry, dtype, B, H, W, cin_p, N, kh, kw=None, ldx=None, ldy=None, cap=None, parts_out=1, shared=1, cus=256, knobs=None):
    """cap: None = what kernels._conv_wgrad passes"""
    kw = kh if kw is None else kw
    return "%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % (entry, dtype, B, H, W, cin_p, N, kh, kw, cin_p if ldx is None else ldx, N if ldy is None else ldy,
                                                               wgrad_stage_cap(cin_p, N, kh, kw) if cap is None else cap, parts_out, shared, cus,
                                                               ",".join("%d=%d" % kv for kv in knobs) if knobs else "-")


def wgrad_cases():
    out = []

    def add(*a, **kw):
        c = wgrad_case(*a, **kw)
        if c not in out:
            out.append(c)

    # ---- the training step: bf16 and fp32, beside the data-gradient chain and alone (there with a second CU count), the stage of kernels._conv_wgrad and 0, 1, 2 slabs
    for B, H, W, cin_p, N, kh, kw in wgrad_training_shapes():
        add("nine_tap", BF16, B, H, W, cin_p, N, kh, kw)
        for dtype in (BF16, F32):
            for shared in (1, 0):
                for cap in (None, 0, 1, 2):
                    add("wgrad", dtype, B, H, W, cin_p, N, kh, kw, cap=cap, shared=shared)
            add("wgrad", dtype, B, H, W, cin_p, N, kh, kw, shared=0, cus=64)
    add("wgrad", 2, 8, 48, 160, 256, 256, 3)                              # an element type the library does not have
    add("nine_tap", F32, 8, 48, 160, 256, 256, 3)

    # ---- tests/test_gpu_conv_variants.py (K.use_wgrad_side_stream is on unless the test turns it off)
    for cin, cout, k, B, H, W in WGRAD_T_SHAPES:
        for kn in (None, [(8, 0)], [(8, 0), (4, 0)]):
            add("wgrad", BF16, B, H, W, round8(cin), cout, k, knobs=kn)
    for cin, cout, B, H, W, sliced in WGRAD_T_NINE:
        for kn in ([(26, 1)], [(26, 0)], [(26, 2)], None):
            add("wgrad", BF16, B, H, W, cin, cout, 3, ldx=cin + 64 if sliced else None, knobs=kn)
        add("nine_tap", BF16, B, H, W, cin, cout, 3)
    for cin, cout, k, B, H, W in WGRAD_T_WIDTH:
        for shared in (1, 0):
            add("wgrad", BF16, B, H, W, cin, cout, k, shared=shared)
    for cin, cout, k, dtype, B, H, W in WGRAD_T_STAGE:
        for shared in (1, 0):
            for cap in (1, 2, 3):
                add("wgrad", dtype, B, H, W, cin, cout, k, cap=cap, shared=shared)

    # ---- both sides of every rule, one group at a time
    for n in (32, 40, 64, 72, 128, 256, 264):                              # the tile ladders and the nine-tap kernel's whole tiles
        for c in (32, 40, 64, 128, 136, 256):
            for k in (3, 5):
                add("wgrad", BF16, 8, 48, 160, c, n, k)
            add("wgrad", F32, 8, 48, 160, c, n, 3)
            add("nine_tap", BF16, 8, 48, 160, c, n, 3)
            if n in (64, 128, 256) and c in (64, 128, 256):
                for kn in ([(8, 0)], [(8, 2)], [(4, 0)], [(26, 0)], [(26, 2)]):
                    add("wgrad", BF16, 8, 48, 160, c, n, 3, knobs=kn)
                add("nine_tap", BF16, 8, 48, 160, c, n, 3, knobs=[(26, 0)])
    for W in (24, 32, 40, 160, 168):                                       # row-aligned pixel blocks: W % 32 == 0 or W >= 160; the nine-tap forms: W % 32, W % 16 with H even
        for H in (5, 6):
            for dtype, c, n, k in ((BF16, 128, 128, 5), (F32, 128, 128, 5), (BF16, 32, 32, 3), (BF16, 32, 64, 3), (BF16, 128, 128, 3)):
                add("wgrad", dtype, 2, H, W, c, n, k, cap=8)
            for kn in (None, [(26, 2)]):
                add("nine_tap", BF16, 2, H, W, 128, 128, 3, knobs=kn)
            add("wgrad", BF16, 2, H, W, 128, 128, 3, cap=8, knobs=[(26, 2)])
    for H in (11, 12, 23, 24, 25, 36, 49, 50, 100):                        # nine-tap, one K-step per row: at least 12 K-steps per split, rounded up to the four ring slots
        for cus in (256, 64):
            for cap in (2, 8):
                add("wgrad", BF16, 1, H, 32, 128, 128, 3, cap=cap, shared=0, cus=cus)
    for H in (15, 16, 17, 31, 32, 33, 48, 49):                             # one pixel block per row: at least 16 per split
        for dtype, c, n, k in ((BF16, 64, 64, 5), (F32, 64, 64, 5), (BF16, 32, 32, 3)):
            add("wgrad", dtype, 1, H, 32, c, n, k, cap=8)
    for k, kw in ((1, 1), (7, 7), (2, 2), (4, 4), (3, 5), (5, 3), (1, 3)):  # even and mixed kernel sizes are not refused
        for dtype in (BF16, F32):
            add("wgrad", dtype, 2, 24, 64, 128, 128, k, kw)
        add("nine_tap", BF16, 2, 24, 64, 128, 128, k, kw)
    for c, n in ((12, 32), (32, 12), (128, 132), (68, 128)):               # channel counts that are no multiple of 8
        add("wgrad", BF16, 2, 24, 64, c, n, 3)
    # a stride that puts each descriptor bound just inside and just outside: the nine-tap kernel's x, the generic kernels' x, dy (both element types)
    for B, H, W, c, n in ((8, 48, 160, 256, 256), (8, 96, 320, 128, 128)):
        M = B * H * W
        for dtype, es in ((BF16, 2), (F32, 4)):
            edges = [((DESC_BOUND - 1) // es - c) // (M + 3)] + ([(DESC_BOUND - 1) // 2 // (M + 2 * W + 16)] if dtype == BF16 else [])
            for edge in edges:
                for ldx in (edge // 8 * 8, edge // 8 * 8 + 8):
                    add("wgrad", dtype, B, H, W, c, n, 3, ldx=ldx)
            edge = ((DESC_BOUND - 1) // es - n) // (M - 1)
            for ldy in (edge // 8 * 8, edge // 8 * 8 + 8):
                add("wgrad", dtype, B, H, W, c, n, 3, ldy=ldy)
    for dtype, c, n, k in ((BF16, 256, 256, 3), (BF16, 512, 128, 5), (BF16, 32, 32, 3), (F32, 128, 128, 3)):      # no parts_out: no nine-tap kernel
        for shared in (1, 0):
            add("wgrad", dtype, 8, 48, 160, c, n, k, parts_out=0, shared=shared)
    # the width knobs, and the whole-rounds search with several CU counts
    for c, n, k in ((256, 256, 3), (512, 128, 5), (128, 128, 1), (4096, 256, 3)):
        for shared in (1, 0):
            for kn in ([(9, 256)], [(9, 1024)], [(27, 0)], [(27, 64)], [(27, 256)], [(26, 0), (9, 256)], [(26, 0), (8, 0)]):
                add("wgrad", BF16, 8, 48, 160, c, n, k, shared=shared, knobs=kn)
        for cus in (64, 128, 304):
            add("wgrad", BF16, 8, 48, 160, c, n, k, shared=0, cus=cus)
            add("wgrad", BF16, 8, 48, 160, c, n, k, shared=0, cus=cus, knobs=[(26, 0)])
    return out

# ---- the optimizer family (--optim): the 16 launching entry points of optim.hip and its three work-buffer queries
OPT_EDGE = 4 * 256 * 8192           # elements at which opt_grid reaches its cap of 8192 workgroups
OPT_REAL = 76993280                 # about the real layout's size (a multiple of 64)
OPT_NS = (0, 1, 3, 4, 5, 64, 1023, 1024, OPT_EDGE - 4, OPT_EDGE, OPT_EDGE + 4, OPT_REAL)
OPT_NS_64 = (0, 64, 128, 960, 1024, 1088, OPT_EDGE - 64, OPT_EDGE, OPT_EDGE + 64, OPT_REAL)      # the SEG forms want n % 64 == 0
STAT_CHUNK, STAT_CAP, STAT_MAX_T = 32768, 1024, 4096                    # csrc/optim_plan.hpp
OPT_PTRS = {                                                             # the pointer arguments of each entry point, by the driver's names
    "ema_update": "p b", "ema_update_dev": "p b scal ctl", "flat_swap": "p b", "grad_accumulate": "p b", "grad_norm_clip": "g work ctl",
    "adamw_step": "p g m v", "adamw_step_dev": "p g m v hyper", "adamw_step_ctl_dev": "p g m v hyper ctl", "adamw_step_seg_dev": "p g m v hyper cls scales ctl",
    "sgd_step": "p g buf", "sgd_step_dev": "p g buf hyper", "sgd_step_ctl_dev": "p g buf hyper ctl", "sgd_step_seg_dev": "p g buf hyper cls scales ctl",
    "tensor_stats": "g p begin numel work out", "lamb_moments": "p g m v hyper begin numel table work trust sums ctl",
    "lamb_apply": "p m v hyper begin numel table trust ctl"}
OPT_PAIR = ("ema_update", "ema_update_dev", "flat_swap", "grad_accumulate")
OPT_ADAM = ("adamw_step", "adamw_step_dev", "adamw_step_ctl_dev", "adamw_step_seg_dev")
OPT_SGD = ("sgd_step", "sgd_step_dev", "sgd_step_ctl_dev", "sgd_step_seg_dev")
OPT_CHUNK = ("tensor_stats", "lamb_moments", "lamb_apply")
OPT_QUERIES = ("grad_norm_work_bytes", "tensor_stats_work_bytes", "lamb_work_bytes")


def optim_case(entry, n=1024, T=2, wd="0.01", dec=1, mom="0.9", nest=0, damp="0", step=2, ncls=2, trust="10", norm="1", flag=None, err="-"):
    """flag: None = the usual one (grad_accumulate: add; everything else: 1 -- with ctl, with p, skip_nonfinite)"""
    flag = (0 if entry == "grad_accumulate" else 1) if flag is None else flag
    return "%s %d %d %s %d %s %d %s %d %d %s %s %d %s" % (entry, n, T, wd, dec, mom, nest, damp, step, ncls, trust, norm, flag, err)


def optim_cases():
    out = []

    def add(*a, **kw):
        c = optim_case(*a, **kw)
        if c not in out:
            out.append(c)

    # ---- every entry point over n: the tails, one workgroup and two, the grid cap's edge, the real size; n < 0
    for entry in OPT_PTRS:
        for n in (OPT_NS_64 if entry.endswith("_seg_dev") else OPT_NS) + (-1, -64):
            add(entry, n)
    # ---- every instance selector
    for entry in OPT_ADAM:
        for wd in ("0", "0.01"):
            for dec in (0, 1):
                add(entry, wd=wd, dec=dec)
    for entry in OPT_SGD:
        for mom, nest in (("0", 0), ("0.9", 0), ("0.9", 1)):
            for wd in ("0", "0.01"):
                add(entry, mom=mom, nest=nest, wd=wd)
        add(entry, mom="0", err="null:buf")                                # without momentum `buf` may be null
        add(entry, damp="0.5")
        add(entry, step=1)
    for entry in ("adamw_step_seg_dev", "sgd_step_seg_dev"):
        for ncls in (1, 16):
            for flag in (0, 1):
                add(entry, ncls=ncls, flag=flag)
    for entry in ("ema_update_dev", "tensor_stats", "grad_accumulate", "grad_norm_clip", "lamb_moments", "lamb_apply"):
        for flag in (0, 1):
            add(entry, flag=flag)
    add("lamb_moments", trust="0")
    add("lamb_moments", wd="0")
    add("lamb_apply", wd="0")
    add("grad_norm_clip", norm="inf")
    # ---- the chunk launches: T, and n / STAT_CHUNK + T below, at and above STAT_CAP, and on both sides of the largest int
    for entry in OPT_CHUNK:
        for T in (1, 2, STAT_MAX_T):
            for n in (1024, STAT_CHUNK * (STAT_CAP - 1 - T), STAT_CHUNK * (STAT_CAP - T), STAT_CHUNK * (STAT_CAP + 1 - T), STAT_CHUNK * (2 ** 31 - 1 - T),
                      STAT_CHUNK * (2 ** 31 - T)):
                if n > 0:
                    add(entry, n, T)
    # ---- every argument error, one case per rule (a pointer the entry point does not test is recorded too: it is launched)
    for entry, ptrs in OPT_PTRS.items():
        n = 1024
        for name in ptrs.split():
            add(entry, n, err="null:" + name)
            add(entry, n, err="mis:" + name)
        if entry in OPT_PAIR:
            for n2 in (0, 4, 5, 1024):                                     # 16 bytes apart: disjoint up to four elements
                add(entry, n2, err="eq")
                add(entry, n2, err="overlap")
        if entry in OPT_ADAM + OPT_SGD + ("lamb_moments", "lamb_apply"):
            for wd in ("-1", "nan", "-0"):
                add(entry, n, wd=wd)
        if entry in OPT_ADAM[:1] + OPT_SGD[:1]:
            for step in (0, -1):
                add(entry, n, step=step)
        if entry in OPT_SGD:
            for mom in ("-1", "nan"):
                add(entry, n, mom=mom)
            add(entry, n, mom="0", nest=1)                                 # Nesterov without momentum
            add(entry, n, nest=1, damp="0.5")                              # ... and with dampening (the host form's rule)
        if entry.endswith("_seg_dev"):
            for n2 in (1000, 1028):
                add(entry, n2)
            for ncls in (0, 17, -1):
                add(entry, n, ncls=ncls)
        if entry in OPT_CHUNK:
            for T in (0, STAT_MAX_T + 1, -1):
                add(entry, n, T)
        if entry == "lamb_moments":
            for trust in ("-1", "nan"):
                add(entry, n, trust=trust)
        if entry == "grad_norm_clip":
            for norm in ("0", "nan", "-1"):
                add(entry, n, norm=norm)
    # ---- the three queries over the same n and T
    for n in OPT_NS + (-1, STAT_CHUNK * (STAT_CAP - 2)):
        add("grad_norm_work_bytes", n)
        for T in (0, 1, 2, STAT_MAX_T, STAT_MAX_T + 1):
            add("tensor_stats_work_bytes", n, T)
            add("lamb_work_bytes", n, T)
    for n in (256 * 4 * 255, 256 * 4 * 255 + 4, 256 * 4 * 256, 256 * 4 * 256 + 4):      # the norm grid's cap
        add("grad_norm_work_bytes", n)
        add("grad_norm_clip", n)
    return out


def record(csrc=CSRC, dev=True, extra=(), gn=False, p3=False, patch=False, wgrad=False, optim=False):
    with tempfile.TemporaryDirectory() as tmp:
        cs = gn_cases() if gn else p3_cases() if p3 else patch_cases() if patch else wgrad_cases() if wgrad else optim_cases() if optim else cases()
        if optim:                                                          # no knobs: one build, and a case's last word is its error, not a knob list
            return run(build(tmp, dev, csrc, extra, optim=True), cs)
        return run(build(tmp, dev, csrc, extra, gn, p3, patch, wgrad), cs if dev else [c for c in cs if c.endswith(" -")])


def load_table(path=TABLE):
    """-> the table's lines (the file is a JSON array with one case per line)"""
    with open(path) as f:
        return [line.rstrip(",\n") for line in f if line.startswith("{")]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--out")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--product", action="store_true", help="the build without -DMTE_DEV: the cases that set no knob")
    ap.add_argument("--gn", action="store_true", help="GroupNorm (norm_act.hip, tests/gn_launch_table.json)")
    ap.add_argument("--p3", action="store_true", help="conv3d pack / unpack (pack3d.hip, tests/p3_launch_table.json)")
    ap.add_argument("--patch", action="store_true", help="LDS-patch convolution (conv_patch.hip, tests/patch_launch_table.json)")
    ap.add_argument("--wgrad", action="store_true", help="weight gradient (mte_conv2d_wgrad: conv_igemm.hip, conv_wgrad9.hip, tests/wgrad_launch_table.json)")
    ap.add_argument("--optim", action="store_true", help="the optimizer family (optim.hip, tests/optim_launch_table.json)")
    a = ap.parse_args()
    lines = record(a.csrc, dev=not a.product, gn=a.gn, p3=a.p3, patch=a.patch, wgrad=a.wgrad, optim=a.optim)
    for ln in lines:
        json.loads(ln)
    with open((GN_TABLE if a.gn else P3_TABLE if a.p3 else PATCH_TABLE if a.patch else WGRAD_TABLE if a.wgrad else OPTIM_TABLE if a.optim else TABLE) if a.write else a.out, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")
    print("%d cases" % len(lines))
