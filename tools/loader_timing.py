"""T8 training-step time with the three loaders on real files (results: profiles/prefetch_loader.txt):

  A   SplitLoader              one sample at a time on the training stream, four host reads per sample
  B   PrefetchSplitLoader      decode threads + one batched preparation pass per batch (datasets/prefetch.py), num_workers 4 / 8 / 16
  C   SyntheticLoader          device-resident batches: the floor (what bench.py measures)

    python tools/loader_timing.py --series [--out profiles/prefetch_loader.txt] [--repeats 3]
        writes a seeded set of KITTI-size files into a temporary folder, then runs A B4 A B8 A B16 C ... , every configuration as a process
        of its own under its own `timeout`, alternating on one box; stops at the first run that fails.  Reports per configuration the median
        over its runs of ms per step (wall clock around one final synchronise) and images/s, the spread of A's runs, B - A and B - C.
    python tools/loader_timing.py --config B8 --data DIR        one run, one JSON line (what --series starts)
    python tools/loader_timing.py --write DIR                   only the files
    python tools/loader_timing.py --prep-only 5 --data DIR      a few batches of the prefetching loader alone, no model: the process to put behind
        `rocprofv3 --kernel-trace --stats --` for the launch count per batch of the preparation stage (a run of its own)

    python tools/loader_timing.py --lidar-series [--out profiles/prefetch_lidar.txt] [--repeats 3] [--parent DIR]
        the LiDAR column (results: profiles/prefetch_lidar.txt): the completion configuration (SemiSupEdgeCompletionModel, RGB+LiDAR network),
        the column on and perturbed, 8 workers.  Alternates  P (the prefetching loader of the built checkout DIR, e.g. the parent commit),
        L (this tree, batched column), S (this tree, batched_lidar=False: the per-sample column), then the same step without the column (B8)
        and on device-resident batches (C).  Reports medians, P's own spread, P - L, and what L leaves exposed against B8.
    --lidar                 adds the LiDAR column to --config / --prep-only / --write: the completion model, lidar_scale / lidar_add / drop 0.1
    --no-batched-lidar      with --lidar: DeviceStage(batched_lidar=False)
    --tree DIR              import mindtheedge_amd from another built checkout (a tree without the batched column takes no --no-batched-lidar)

The files are read from the page cache after the first pass: this times decoding and preparation, not a disk.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:                                           # before the package is imported
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")                          # as bench.py: main chain + weight-gradient stream

KITTI_SIZES = ((375, 1242), (370, 1226), (374, 1238), (376, 1241))
SHAPE, BATCH, RECORDS = (384, 1280), 8, 32
LIDAR_SCALE, LIDAR_ADD, LIDAR_DROP = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5)), 0.1      # the reference's augmentation block


def write_files(folder, seed=0):
    """RECORDS frames in the four KITTI sizes: RGB, 16-bit depth at ~5 % density, four edge and four normal scales at 384 x 1280 >> s"""
    import numpy as np
    from PIL import Image
    g = np.random.default_rng(seed)
    os.makedirs(os.path.join(folder, "normals"), exist_ok=True)
    for i in range(RECORDS):
        h, w = KITTI_SIZES[i % 4]
        coarse = g.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3))
        rgb = np.kron(coarse, np.ones((8, 8, 1), dtype=np.int64))[:h, :w] + g.integers(-12, 13, (h, w, 3))      # blocks + noise: compresses like a photograph, not like noise
        Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8)).save(os.path.join(folder, "rgb%02d.png" % i))
        raw = ((g.random((h, w)) < 0.05) * (256 + g.integers(0, 79 * 256, (h, w)))).astype(np.uint16)
        raw[0, 0] = 300
        Image.fromarray(raw).save(os.path.join(folder, "depth%02d.png" % i))
        sparse = ((g.random((h, w)) < 0.05) * (256 + g.integers(0, 79 * 256, (h, w)))).astype(np.uint16)      # ~23 k returns, a 64-beam sweep's share of the frame
        sparse[0, 0] = 300
        Image.fromarray(sparse).save(os.path.join(folder, "lidar%02d.png" % i))
        for s in range(4):
            eh, ew = SHAPE[0] >> s, SHAPE[1] >> s
            Image.fromarray(((g.random((eh, ew)) < 0.03) * 255).astype(np.uint8)).save(os.path.join(folder, "%08d_e_00%d.png" % (i, s)))
            smooth = np.kron(g.integers(0, 256, (eh // 4 + 1, ew // 4 + 1)), np.ones((4, 4), dtype=np.int64))[:eh, :ew]
            Image.fromarray(smooth.astype(np.uint8)).save(os.path.join(folder, "normals", "%08d_e_00%d.png" % (i, s)))


def write_split(folder, batches, lidar=False):
    path = os.path.join(folder, "split_%d%s.txt" % (batches, "_lidar" if lidar else ""))
    with open(path, "w") as f:
        for j in range(batches * BATCH):
            i = j % RECORDS
            f.write("rgb%02d.png depth%02d.png %08d_e_000.png %s None None None normals/%08d_e_000.png\n" % (i, i, i, "lidar%02d.png" % i if lidar else "None", i))
    return path


def make_loader(config, folder, batches, jitter, lidar=False, batched_lidar=True, synthetic_lidar=False):
    import torch
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, SplitLoader
    from mindtheedge_amd.datasets.prefetch import PrefetchSplitLoader
    from mindtheedge_amd.utils.synthetic import SyntheticLoader
    if config == "C":
        return SyntheticLoader(BATCH, SHAPE[0], SHAPE[1], batches, torch.device("cuda", 0), lidar=synthetic_lidar)
    kw = {"input_depth_type": ["velodyne"], "lidar_scale": LIDAR_SCALE, "lidar_add": LIDAR_ADD, "lidar_drop_rate": LIDAR_DROP} if lidar else {}
    ds = KittiEdgeSplitDataset(write_split(folder, batches, lidar), SHAPE, root=folder, jittering=(0.2, 0.2, 0.2, 0.05) if jitter else (), **kw)
    if config == "A":
        return SplitLoader(ds, BATCH, shuffle=True, seed=0)
    kw = {} if batched_lidar else {"batched_lidar": False}               # (a checkout without the batched column has no such argument)
    return PrefetchSplitLoader(ds, BATCH, shuffle=True, seed=0, num_workers=int(config[1:]), prefetch=2, **kw)


def run_config(args):
    """warm-up + timed T8 steps (bench.py's model and optimizer, bf16) fed by one loader -> one JSON line"""
    import random
    import torch
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, broadcast_parameters
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K.set_compute_dtype("bf16")
    torch.manual_seed(42)
    kind = SemiSupEdgeModel
    if args.lidar:                                                        # configs/train_packnet_san_completion_with_edges.yaml: the RGB+LiDAR network and its model
        from mindtheedge_amd.models.SemiSupEdgeCompletionModel import SemiSupEdgeCompletionModel as kind
    net = PackNetSAN01(dropout=0.5, version="1A", **({"with_san": True} if args.lidar else {})).to(dev)
    model = kind(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog",
                 supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.5)
    model.add_depth_net(net)
    model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
    model.train()
    flat = FlatParameters(net.parameters())
    broadcast_parameters(flat)
    opt = FusedAdam(flat, lr=1e-4)
    random.seed(100)
    torch.manual_seed(1000)
    with_column = args.lidar and not args.without_column
    loader = make_loader(args.config, args.data, args.warmup + args.steps, args.jitter, with_column, not args.no_batched_lidar, args.lidar)
    host = {"s": None}
    if with_column and not args.no_batched_lidar and args.config != "C":  # the consumer thread's time in the LiDAR draws and the survivor count
        from mindtheedge_amd.datasets import lidar_prep as lp
        if hasattr(lp, "draw_batch"):                                     # (a checkout without the batched column has none)
            inner, host["s"] = lp.draw_batch, 0.0

            def timed(*a, **kw):
                t = time.perf_counter()
                try:
                    return inner(*a, **kw)
                finally:
                    host["s"] += time.perf_counter() - t
            lp.draw_batch = timed
    if args.lidar and not with_column and args.config != "C":             # the completion step without the column's preparation: the same map for every step
        fixed = torch.zeros((BATCH, 1) + SHAPE, device=dev)
        fixed[:, :, ::4, ::5] = 10.0
    t0 = None
    n = 0
    for batch in loader:
        if n == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if args.lidar and not with_column and args.config != "C":
            batch["lidar"], batch["input_depth"] = fixed, fixed
        opt.zero_grad()
        out = model(batch)
        out["loss"].backward()
        opt.step()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert n == args.warmup + args.steps, n
    host_ms = host["s"]
    print(json.dumps({"config": args.config, "lidar": bool(with_column), "batched_lidar": bool(with_column and not args.no_batched_lidar),
                      "lidar_host_ms_per_batch": None if host_ms is None else host_ms / n * 1e3, "ms_per_step": dt / args.steps * 1e3, "images_per_s": BATCH * args.steps / dt, "steps": args.steps,
                      "warmup": args.warmup, "jitter": bool(args.jitter), "final_loss": float(out["loss"].detach().float().sum()),
                      "device": torch.cuda.get_device_name(0)}))


def prep_only(args):
    import torch
    loader = make_loader("B4", args.data, args.prep_only, args.jitter, args.lidar, not args.no_batched_lidar)
    for batch in loader:
        pass
    torch.cuda.synchronize()
    print("prepared %d batches of %d" % (args.prep_only, BATCH))


def series(args):
    order = []
    for _ in range(args.repeats):
        order += ["A", "B4", "A", "B8", "A", "B16", "C"]
    runs, lines = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        write_files(tmp)
        for config in order:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--config", config, "--data", tmp,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--jitter"] if args.jitter else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                         # nothing more is started on the card after a run that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("configuration %s ended with status %d: the series stops here" % (config, r.returncode))
            res = json.loads(r.stdout.strip().splitlines()[-1])
            runs.setdefault(config, []).append(res)
            print("%-4s %8.3f ms/step %8.1f images/s" % (config, res["ms_per_step"], res["images_per_s"]), flush=True)
    device = runs["A"][0]["device"]
    lines.append("T8 training step (SemiSupEdgeModel, bf16, batch %d, %d x %d) fed from KITTI-size files, %s" % (BATCH, SHAPE[0], SHAPE[1], device))
    lines.append("%d warm-up + %d timed steps per run, wall clock around one final synchronise; every run a process of its own, order: %s"
                 % (args.warmup, args.steps, " ".join(order)))
    lines.append("colour jitter %s; files in the page cache" % ("on" if args.jitter else "off"))
    med = {}
    for config in ("A", "B4", "B8", "B16", "C"):
        ms = [r["ms_per_step"] for r in runs[config]]
        med[config] = statistics.median(ms)
        name = {"A": "A  SplitLoader", "C": "C  SyntheticLoader (floor)"}.get(config, "B  prefetching loader, num_workers %s" % config[1:])
        lines.append("%-42s median %8.3f ms/step %8.1f images/s   runs: %s" % (name, med[config], BATCH / med[config] * 1e3, " ".join("%.3f" % v for v in ms)))
    a = [r["ms_per_step"] for r in runs["A"]]
    spread = max(a) - min(a)
    lines.append("spread of A's own runs (max - min): %.3f ms" % spread)
    for config in ("B4", "B8", "B16"):
        gain = med["A"] - med[config]
        lines.append("A - %-3s = %7.3f ms (%s the spread of A)   %-3s - C = %7.3f ms still exposed"
                     % (config, gain, "more than" if gain > spread else "NOT more than", config, med[config] - med["C"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def lidar_series(args):
    """P L S .. B8 C, see the module docstring"""
    runs = {}
    names = {"P": "P  prefetching loader of the --parent checkout", "L": "L  this tree, batched LiDAR column",
             "S": "S  this tree, batched_lidar=False (per-sample column)", "B8": "B8 the same step without the column's preparation",
             "C": "C  SyntheticLoader with a LiDAR map (floor)"}
    flags = {"P": ["--config", "B8", "--tree", args.parent], "L": ["--config", "B8"], "S": ["--config", "B8", "--no-batched-lidar"],
             "B8": ["--config", "B8", "--without-column"], "C": ["--config", "C"]}
    order = []
    for _ in range(args.repeats):
        order += (["P"] if args.parent else []) + ["L", "S", "B8", "C"]
    with tempfile.TemporaryDirectory() as tmp:
        write_files(tmp)
        for config in order:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--lidar", "--data", tmp, "--steps", str(args.steps),
                   "--warmup", str(args.warmup)] + flags[config] + (["--jitter"] if args.jitter else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                         # nothing more is started on the card after a run that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("configuration %s ended with status %d: the series stops here" % (config, r.returncode))
            res = json.loads(r.stdout.strip().splitlines()[-1])
            runs.setdefault(config, []).append(res)
            print("%-4s %8.3f ms/step %8.1f images/s" % (config, res["ms_per_step"], res["images_per_s"]), flush=True)
    lines = ["T8 completion step (SemiSupEdgeCompletionModel, RGB+LiDAR network, bf16, batch %d, %d x %d) fed from KITTI-size files, LiDAR column on and"
             % (BATCH, SHAPE[0], SHAPE[1]), "perturbed (drop %.1f), 8 workers, %s" % (LIDAR_DROP, runs["L"][0]["device"]),
             "%d warm-up + %d timed steps per run, wall clock around one final synchronise; every run a process of its own, order: %s"
             % (args.warmup, args.steps, " ".join(order)), "colour jitter %s; files in the page cache" % ("on" if args.jitter else "off")]
    med = {}
    for config in [c for c in ("P", "L", "S", "B8", "C") if c in runs]:
        ms = [r["ms_per_step"] for r in runs[config]]
        med[config] = statistics.median(ms)
        lines.append("%-56s median %8.3f ms/step %8.1f images/s   runs: %s" % (names[config], med[config], BATCH / med[config] * 1e3, " ".join("%.3f" % v for v in ms)))
    host = [r["lidar_host_ms_per_batch"] for r in runs["L"]]
    lines.append("L: consumer-thread host time for the LiDAR draws and the survivor count: median %.3f ms per batch of %d" % (statistics.median(host), BATCH))
    base = "P" if "P" in runs else "S"
    p = [r["ms_per_step"] for r in runs[base]]
    spread = max(p) - min(p)
    lines.append("spread of %s's own runs (max - min): %.3f ms" % (base, spread))
    gain = med[base] - med["L"]
    lines.append("%s - L = %7.3f ms (%s the spread of %s)" % (base, gain, "more than" if gain > spread else "NOT more than", base))
    lines.append("L - B8 = %7.3f ms of the column still exposed;  L - C = %7.3f ms of the whole data path" % (med["L"] - med["B8"], med["L"] - med["C"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lidar-series", action="store_true")
    ap.add_argument("--lidar", action="store_true", help="the LiDAR column, perturbed, and the completion model")
    ap.add_argument("--no-batched-lidar", action="store_true", help="with --lidar: the per-sample column (DeviceStage(batched_lidar=False))")
    ap.add_argument("--without-column", action="store_true", help="with --lidar: the completion step on a fixed LiDAR map, no column in the loader")
    ap.add_argument("--tree", default="", help="import the package from this built checkout")
    ap.add_argument("--parent", default="", help="--lidar-series: a built checkout to alternate with (the parent commit)")
    ap.add_argument("--series", action="store_true")
    ap.add_argument("--config", choices=["A", "B4", "B8", "B16", "C"])
    ap.add_argument("--write", default="")
    ap.add_argument("--prep-only", type=int, default=0)
    ap.add_argument("--data", default="")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one run of --series")
    ap.add_argument("--jitter", action="store_true", help="colour jitter (0.2, 0.2, 0.2, 0.05), the reference's recipe")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 50 or args.warmup < 10:
        ap.error("at least 10 warm-up and 50 timed steps")
    if args.write:
        return write_files(args.write)
    if args.series:
        return series(args)
    if args.lidar_series:
        return lidar_series(args)
    if not args.data:
        ap.error("--config / --prep-only need --data DIR (see --write)")
    if args.prep_only:
        return prep_only(args)
    if not args.config:
        ap.error("one of --series, --lidar-series, --config, --write, --prep-only")
    return run_config(args)


if __name__ == "__main__":
    main()
