"""Timing of one validation sample at a KITTI-size frame on the GPU box (results: profiles/eval_prep.txt):

  device route  eval_prep.validation_sample on the decoded arrays: upload + LANCZOS resize + resize_depth_preserve + the uint8 bilinear
                resizes of edge, edge_1..3 and rgb_edge + ToTensor
  host route    the same transform with PIL (LANCZOS) and NumPy (tests/eval_prep_ref.py), then the upload of its results
  kernels       HIP-event time of mte_resize_linear_u8 and mte_resize_nearest_f32 alone

    python tools/eval_prep_timing.py [--reps 100] [--out profiles/eval_prep.txt]

File decoding is the same on both routes and is left out."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from image_prep_timing import event_ms, host_ms           # noqa: E402

SRC = (375, 1242)                                          # -> 352 x 1216, the frame rounded down to multiples of 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken without one says nothing")
    import eval_prep_ref as R
    from mindtheedge_amd.datasets import eval_prep as ep
    g = np.random.default_rng(0)
    h, w = SRC
    host = {"rgb": g.integers(0, 256, SRC + (3,), dtype=np.uint8),
            "depth": ((g.random(SRC) < 0.2) * (1 + 79 * g.random(SRC))).astype(np.float32),
            "input_depth": ((g.random(SRC) < 0.05) * (1 + 79 * g.random(SRC))).astype(np.float32),
            "edge": ((g.random(SRC) < 0.1) * 255).astype(np.uint8), "rgb_edge": ((g.random(SRC) < 0.1) * 255).astype(np.uint8)}
    for s in range(1, 4):
        host["edge_%d" % s] = ((g.random((h // 2 ** s, w // 2 ** s)) < 0.1) * 255).astype(np.uint8)

    def device_route():
        return ep.validation_sample({k: torch.from_numpy(v).cuda() for k, v in host.items()})

    def host_route():
        return {k: torch.from_numpy(v).cuda() for k, v in R.validation_sample(host).items()}

    got, want = device_route(), host_route()
    for k, v in want.items():
        assert torch.equal(got[k], v), k                   # the two routes compute the same sample
    H, W = got["rgb"].shape[-2:]
    lines = ["one validation sample, %d x %d -> %d x %d (rgb, depth, input_depth, edge + 3 scales, rgb_edge), %s" % (SRC + (H, W, torch.cuda.get_device_name(0)))]
    n = max(10, args.reps // 4)
    for name, fn in [("device route (upload + eval_prep.validation_sample)", device_route), ("host route (PIL + NumPy, then upload)", host_route)]:
        med, best = host_ms(fn, n)
        lines.append("%-56s median %8.3f ms   min %8.3f ms   (host clock around a synchronise, %d reps)" % (name, med, best, n))
    edge = torch.from_numpy(host["edge"]).cuda()
    lidar = torch.from_numpy(host["input_depth"]).cuda()
    for name, fn, nbytes in [("mte_resize_linear_u8 %d x %d -> %d x %d" % (SRC + (H, W)), lambda: ep.resize_linear_u8(edge, (H, W)), 4 * H * W + H * W),
                             ("mte_resize_nearest_f32 %d x %d -> %d x %d" % (SRC + (H, W)), lambda: ep.resize_nearest_f32(lidar, (H, W)), 8 * H * W)]:
        med, best = event_ms(fn, args.reps)
        lines.append("%-56s median %7.4f ms  min %7.4f ms   (HIP events, output allocation included; %.1f GB/s of touched bytes)"
                     % (name, med, best, nbytes / best / 1e6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
