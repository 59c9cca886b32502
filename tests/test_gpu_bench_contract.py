"""GPU (-m gpu): bench.py prints exactly one JSON line on stdout with the keys the driver's contract names (a short run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                        "--full"], capture_output=True, text=True, timeout=580, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["unit"] == "images/sec" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert "synthetic" in d["data"] and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]          # whole-job images / max-over-ranks time
    assert 50 < d["value"] < 2000
    for name, bound, unit in (("roofline", "mfma", "TFLOP/s"), ("roofline_hbm", "hbm", "GB/s")):
        o = d[name]
        assert o["bound"] == bound and o["unit"] == unit and o["peak"] > 0
        assert abs(o["frac"] - o["achieved"] / o["peak"]) < 1e-9 and 0 < o["frac"] < 1
        assert o["traffic"] is None or o["traffic"] > 0
    # round 2: how the step was launched, the loss stencils as ONE forward + ONE backward launch, the all-reduce layout
    assert d["step_launch"].split(" ")[0] in ("hip_graph", "eager")
    loss = d["roofline_hbm"]["edge_loss_stencils"]
    assert loss["launches_per_step"] <= 4 and loss["achieved"] > 0
    ar = d["allreduce"]
    assert ar["rccl_ranks"] == 1 and ar["allreduce_exposed_ms"] == 0.0
    assert max(ar["buckets_mb"]) > 150 and ar["message_mb"] == 32.0            # the 151 MB pack5.conv weight rides in one bucket ...
    assert max(ar["messages_per_bucket"]) >= 5                                   # ... which goes out as <= 32 MB messages
    # round 3: per-rank step time (fastest / slowest rank, before the closing barrier) beside the max-over-ranks figure
    assert 0 < d["rank_ms_per_step_min"] <= d["rank_ms_per_step_max"] <= d["ms_per_step"] * 1.001


@pytest.mark.timeout(900)
def test_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path):
    """Without --full the run only times its steps: no per-kernel timing, CPU baseline or extra steps.  --dump-outputs writes
    what the last timed step computed (float32 .npy files, at most 64 MB in all); its loss is the one the line reports, and two
    runs with the same arguments write the same arrays."""
    import numpy as np
    runs = []
    for tag in ("a", "b"):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=400, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        runs.append((json.loads(lines[0]), out))
    d, out = runs[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "bf16" and d["higher_is_better"] is True
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("roofline", "roofline_hbm", "cpu_baseline", "parity", "host_enqueue_unthrottled_ms_per_step"):
        assert k not in d, k
    files = sorted(p.name for p in out.iterdir())
    assert {"loss.npy", "inv_depths_0.npy", "inv_depths_3.npy"} <= set(files), files
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 2**20
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert arrays["inv_depths_0"].shape == (8, 1, 384, 1280)
    assert abs(float(arrays["loss"].sum()) - d["final_loss"]) <= 1e-6 * abs(d["final_loss"])
    d2, out2 = runs[1]
    assert sorted(p.name for p in out2.iterdir()) == files and d2["final_loss"] == d["final_loss"]
    for f in files:
        assert np.array_equal(np.load(out2 / f), arrays[f[:-4]]), f


@pytest.mark.timeout(900)
def test_process_group_does_not_cost_the_overlap():
    """The launch the driver uses for N > 1 (torch.distributed.run, RCCL, bucketed all-reduce from grad-ready callbacks) with ONE rank against the plain
    N = 1 run on the same box: the streams RCCL brings must not push the main chain and the weight-gradient stream onto one hardware queue.  Round 3 found
    a third stream of the host side doing exactly that (25.4 -> 35.1 ms per step; profiles/r03_band_stream_ab.txt); the bound is loose -- it is a schedule
    check, not a benchmark."""
    def run(dist):
        env = dict(os.environ)
        cmd = [sys.executable]
        if dist:
            env["MTE_BENCH_DIST_SELFTEST"] = "1"
            cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29541"]
        cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "4", "--no-cpu-baseline", "--no-kernel-timing"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    plain, dist = run(False), run(True)
    assert dist["allreduce"]["rccl_ranks"] == 1 and dist["step_launch"].startswith("eager")
    assert dist["ms_per_step"] < 1.15 * plain["ms_per_step"], (plain["ms_per_step"], dist["ms_per_step"])
