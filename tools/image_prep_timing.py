"""Timing of the training-image preparation on the GPU box (results: profiles/image_prep.txt):

  host path   what the dataset did before image_prep.py: PIL LANCZOS resize on the host + upload + torch /255, per frame and per batch of 8
  device path upload of the decoded frame + mte_image_resample_u8 (+ mte_color_jitter_u8_to_f32 over the batch, with rgb_original)
  kernels     HIP-event time of each launch group after warm-up, and the achieved share of HBM bandwidth from the algorithmic bytes
              (resample: source window + 3 H W out; jitter: 3 H W in per launch + 12 H W out, x 2 with rgb_original)

    python tools/image_prep_timing.py [--reps 200] [--out profiles/image_prep.txt]
    python tools/image_prep_timing.py --dataset-only --tree <checkout of the parent commit>      ds[i] end to end on another tree
    python tools/image_prep_timing.py --lidar [--out profiles/lidar_prep.txt]      ds[i] end to end with and without the LiDAR column
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

# --tree DIR: import the package from another checkout (the parent commit, for the ds[i] comparison)
_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _TREE)

HBM_PEAK = 8.0e12                      # bytes / s, spec
SRC, DST, B = (375, 1242), (384, 1280), 8


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def event_ms(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t)


def dataset_timing(args):
    """ds[i] end to end (PNG decode included) on KITTI-size files written to a temporary folder; works on the parent commit too"""
    import tempfile
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset
    g = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        lines = []
        for i in range(B):
            Image.fromarray(g.integers(0, 256, SRC + (3,), dtype=np.uint8)).save(os.path.join(tmp, "rgb%d.png" % i), compress_level=1)
            lines.append("rgb%d.png None None None None None None None\n" % i)
        split = os.path.join(tmp, "split.txt")
        open(split, "w").writelines(lines)
        ds = KittiEdgeSplitDataset(split, DST, root=tmp)
        med, best = host_ms(lambda: [ds[i] for i in range(B)], max(10, args.reps // 10))
        text = "ds[i] for a batch of 8 (rgb only, PNG decode included), tree %s: median %8.3f ms   min %8.3f ms" % (os.path.basename(os.path.abspath(_TREE)) or ".", med, best)
        decode = host_ms(lambda: [np.asarray(Image.open(os.path.join(tmp, "rgb%d.png" % i)).convert("RGB")) for i in range(B)], max(10, args.reps // 10))
        text += "\n   of which PNG decode of the 8 files: median %8.3f ms" % decode[0]
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


def lidar_timing(args):
    """ds[i] end to end on KITTI-size files without the LiDAR column, with it, and with its perturbation; then the device calls alone"""
    import tempfile
    from mindtheedge_amd.datasets.kitti_edges import KittiEdgeSplitDataset, resize_depth_preserve
    from mindtheedge_amd.datasets import lidar_prep as lp
    g = np.random.default_rng(0)
    scale, add = ((1, 1, 1), (1, 1, 1.1)), ((0, 0, 0), (1.5, 1.5, 0.5))
    reps = max(10, args.reps // 10)
    lines = ["LiDAR column, %d x %d -> %d x %d at 5 %% density, batch %d, %s" % (SRC + DST + (B, torch.cuda.get_device_name(0)))]
    with tempfile.TemporaryDirectory() as tmp:
        rows = []
        for i in range(B):
            Image.fromarray(g.integers(0, 256, SRC + (3,), dtype=np.uint8)).save(os.path.join(tmp, "rgb%d.png" % i), compress_level=1)
            raw = ((g.random(SRC) < 0.05) * (256 + g.integers(0, 79 * 256, SRC))).astype(np.uint16)
            raw[0, 0] = 300
            Image.fromarray(raw).save(os.path.join(tmp, "lidar%d.png" % i), compress_level=1)
            rows.append("rgb%d.png None None lidar%d.png None None None None\n" % (i, i))
        split = os.path.join(tmp, "split.txt")
        open(split, "w").writelines(rows)
        for name, kw in [("without the column", {}), ("with the column (read + resize_depth_preserve)", {"input_depth_type": ["velodyne"]}),
                         ("with the column, perturbed (two host reads per sample)", {"input_depth_type": ["velodyne"], "lidar_scale": scale,
                                                                                   "lidar_add": add, "lidar_drop_rate": 0.1})]:
            ds = KittiEdgeSplitDataset(split, DST, root=tmp, **kw)
            med, best = host_ms(lambda: [ds[i] for i in range(B)], reps)
            lines.append("ds[i] for a batch of 8, %-56s median %8.3f ms   min %8.3f ms   (host clock around a synchronise, %d reps)" % (name, med, best, reps))
    depth = torch.from_numpy(((g.random(DST) < 0.05) * (1 + 79 * g.random(DST))).astype(np.float32)).cuda()
    med, best = host_ms(lambda: lp.augment_depth_values(depth, scale, add, 0.1), args.reps)
    lines.append("augment_depth_values alone, %d returns (draws, uploads, 10 launches, two host reads)   median %8.3f ms   min %8.3f ms" % (int((depth > 0).sum()), med, best))
    med, best = event_ms(lambda: resize_depth_preserve(depth, DST), args.reps)
    lines.append("resize_depth_preserve alone (HIP events)   median %7.4f ms  min %7.4f ms" % (med, best))
    pts = np.stack([g.uniform(-30, 30, 100000), g.uniform(-8, 8, 100000), g.uniform(0.5, 80, 100000)])
    med, best = host_ms(lambda: lp.project_lidar(pts, lp.GTA_INTRINSICS), args.reps)
    lines.append("project_lidar, 100000 points into 1080 x 1920 (upload included)   median %8.3f ms   min %8.3f ms" % (med, best))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--tree", default="")
    ap.add_argument("--dataset-only", action="store_true")
    ap.add_argument("--lidar", action="store_true", help="time the dataset's LiDAR column instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken without one says nothing")
    if args.dataset_only:
        return dataset_timing(args)
    if args.lidar:
        return lidar_timing(args)
    from mindtheedge_amd.datasets import image_prep as ip
    g = np.random.default_rng(0)
    frames = [g.integers(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(B)]
    pil = [Image.fromarray(f) for f in frames]
    H, W = DST
    lines = ["image preparation, %d x %d -> %d x %d, batch %d, %s, torch threads %d" % (SRC + DST + (B, torch.cuda.get_device_name(0), torch.get_num_threads()))]

    def host_frame(i=0):
        img = pil[i].resize((W, H), Image.LANCZOS)
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).cuda().permute(2, 0, 1).float() / 255.0

    def device_frame(i=0):
        return ip.color_jitter_to_tensor(ip.resize_image_u8(torch.from_numpy(frames[i]).cuda(), DST).unsqueeze(0))

    random.seed(0)
    params = [ip.draw_color_jitter((0.2, 0.2, 0.2, 0.05)) for _ in range(B)]

    def device_batch_jitter():
        resized = torch.stack([ip.resize_image_u8(torch.from_numpy(f).cuda(), DST) for f in frames])
        return ip.color_jitter_to_tensor(resized, params, want_original=True)

    n = max(20, args.reps // 4)
    for name, fn in [("host path, one frame (PIL resize + upload + /255)", host_frame),
                     ("host path, batch of 8", lambda: [host_frame(i) for i in range(B)]),
                     ("device path, one frame (upload + resample + to_tensor)", device_frame),
                     ("device path, batch of 8, no jitter", lambda: [device_frame(i) for i in range(B)]),
                     ("device path, batch of 8, resample + batched jitter + rgb_original", device_batch_jitter)]:
        med, best = host_ms(fn, n)
        lines.append("%-72s median %8.3f ms   min %8.3f ms   (host clock around a synchronise, %d reps)" % (name, med, best, n))

    # kernels alone, HIP events
    src = torch.from_numpy(frames[0]).cuda()
    med, best = event_ms(lambda: ip.resize_image_u8(src, DST), args.reps)
    nbytes = SRC[0] * SRC[1] * 3 + H * W * 3
    lines.append("resample call (one launch, LDS intermediate; HIP events, output allocation included)   median %7.4f ms  min %7.4f ms   %6.1f GB/s of algorithmic bytes = %4.1f %% of 8 TB/s"
                 % (med, best, nbytes / best / 1e6, 100 * nbytes / (best * 1e-3) / HBM_PEAK))
    med, best = event_ms(lambda: ip.resize_image_u8(src, DST, two_pass=True), args.reps)
    lines.append("resample call, two-launch form (HBM intermediate)     median %7.4f ms  min %7.4f ms" % (med, best))
    batch = torch.stack([ip.resize_image_u8(torch.from_numpy(f).cuda(), DST) for f in frames])
    for name, p, orig, launches in [("to_tensor only", None, False, 1), ("jitter, 8 orders", params, False, 2), ("jitter + rgb_original", params, True, 2)]:
        med, best = event_ms(lambda: ip.color_jitter_to_tensor(batch, p, want_original=orig), args.reps)
        nbytes = B * H * W * (3 * launches + 12 * (2 if orig else 1))
        lines.append("colour jitter batch of 8: %-22s median %7.4f ms  min %7.4f ms   %6.1f GB/s of algorithmic bytes = %4.1f %% of 8 TB/s "
                     "(includes the parameter upload and the zero fill of the sums)" % (name, med, best, nbytes / best / 1e6, 100 * nbytes / (best * 1e-3) / HBM_PEAK))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dataset_timing(args)


if __name__ == "__main__":
    main()
