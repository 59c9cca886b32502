"""Timing of the depth visualisation of one KITTI-size frame (384 x 1280) on the GPU box (results: profiles/depth_viz.txt):

  device route  utils/depth.py::viz_inv_depth / depth_log_color on the frame where it lies (on the device), then the uint8 image to the host
  host route    the frame to the host as float32, then the reference's arithmetic there: np.percentile + matplotlib's plasma for the
                visualisation, np.log + min / max + matplotlib's Spectral for the log colouring (needs matplotlib; skipped without it)
  kernels       HIP-event time of mte_order_stats_f32 and mte_colormap_u8 (both modes) alone, with their share of HBM bandwidth

    python tools/viz_timing.py [--reps 100] [--out profiles/depth_viz.txt]

Nothing rests on these numbers: the frame is 2 MB and either route takes a fraction of a forward pass."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from image_prep_timing import event_ms, host_ms           # noqa: E402

SHAPE = (384, 1280)
HBM_GBS = 8000.0                                          # MI355X peak, for the share only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken without one says nothing")
    from mindtheedge_amd.utils import depth as D
    g = np.random.default_rng(0)
    inv = (g.random(SHAPE) * 0.4).astype(np.float32)
    depth = np.exp(g.random(SHAPE) * np.log(80.0)).astype(np.float32)
    inv_d, depth_d = torch.from_numpy(inv).cuda(), torch.from_numpy(depth).cuda()
    H, W = SHAPE
    lines = ["one frame %d x %d, %s" % (H, W, torch.cuda.get_device_name(0))]
    routes = [("viz_inv_depth: device route (kernels + uint8 copy)", lambda: D.viz_inv_depth(inv_d).cpu()),
              ("log colouring: device route (kernels + uint8 copy)", lambda: D.depth_log_color(depth_d).cpu())]
    try:
        import matplotlib
        plasma, spectral = matplotlib.colormaps["plasma"], matplotlib.colormaps["Spectral"]

        def host_viz():
            a = inv_d.cpu().numpy()
            a = a / (np.percentile(a, 95) + 1e-6)
            return plasma(np.clip(a, 0., 1.))[:, :, :3] * 255

        def host_log():
            a = np.log(depth_d.cpu().numpy())
            a = a - a.min()
            a = a / a.max()
            return (spectral(a)[:, :, :3] * 255).astype(np.uint8)
        routes.insert(1, ("viz_inv_depth: host route (float32 copy + numpy + matplotlib)", host_viz))
        routes.append(("log colouring: host route (float32 copy + numpy + matplotlib)", host_log))
    except ImportError:
        lines.append("host route: not measured (matplotlib is not installed)")
    n = max(10, args.reps // 4)
    for name, fn in routes:
        med, best = host_ms(fn, n)
        lines.append("%-68s median %8.3f ms   min %8.3f ms   (host clock around a synchronise, %d reps)" % (name, med, best, n))
    table = D.color_table("plasma", "rint", inv_d.device)
    div = torch.tensor([0.38], dtype=torch.float32, device=inv_d.device)
    lo_hi = torch.tensor([[0.0, float(np.log(80.0))]], dtype=torch.float32, device=inv_d.device)
    hw = H * W
    kernels = [("mte_order_stats_f32 (k, k + 1 of %d values; 4 passes)" % hw, lambda: D.order_stats(inv_d.reshape(-1), [int(0.95 * (hw - 1))]), 4 * 4 * hw),
               ("mte_colormap_u8, division mode", lambda: D.colormap_u8(inv_d.unsqueeze(0), table, divisor=div), 7 * hw),
               ("mte_colormap_u8, log mode", lambda: D.colormap_u8(depth_d.unsqueeze(0), table, lo_hi=lo_hi), 7 * hw)]
    for name, fn, nbytes in kernels:
        med, best = event_ms(fn, args.reps)
        gbs = nbytes / best / 1e6
        lines.append("%-68s median %7.4f ms  min %7.4f ms   (HIP events, allocations included; %.1f GB/s of touched bytes = %.1f %% of HBM peak)"
                     % (name, med, best, gbs, 100 * gbs / HBM_GBS))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
