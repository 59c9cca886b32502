"""HIP-event times of the supervised losses (csrc/supervised_loss.hip: one forward launch -- two for BerHu -- and one backward launch for
all scales) and of the nearest upsample of upsample_depth_maps at the T8 loss shapes: B = 8, inverse depth at 384 x 1280 and its three
halvings, metric depth at 384 x 1280 with 5 % valid pixels (the LiDAR density of utils/synthetic.py).

    python tools/supervised_loss_timing.py [--reps 50]

Prints one line per configuration: forward, backward and forward + backward per step in ms (median of `reps` timed steps after warm-up)
and the achieved HBM rate of the step at the nominal traffic (forward: prediction 4 B/pixel + ground truth gathered at 4 B/pixel;
backward: the same + 4 B/pixel gradient write; upsample: 4 B/output pixel written forward and read backward, plus the small maps)."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.kernels_loss import SUPERVISED_METHODS, _SupScale, _UpsampleMap
    lib = K.lib
    dev = torch.device("cuda")
    B, H, W = 8, 384, 1280
    sizes = [(H >> s, W >> s) for s in range(4)]
    gen = torch.Generator(device="cpu").manual_seed(0)
    depth = ((torch.rand(B, 1, H, W, generator=gen) < 0.05).float() * (1 + 79 * torch.rand(B, 1, H, W, generator=gen))).to(dev)
    inv = [(0.02 + torch.rand(B, 1, h, w, generator=gen)).to(dev) for h, w in sizes]
    dinv = [torch.empty_like(i) for i in inv]
    st = torch.cuda.current_stream().cuda_stream
    gout = torch.ones((1,), dtype=torch.float32, device=dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    rows = []
    loss = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty((16,), dtype=torch.float32, device=dev)
    for n in (1, 4):
        arr = (_SupScale * n)()
        for o, p, d in zip(arr, inv, dinv):
            o.pred, o.dpred, o.H, o.W = p.data_ptr(), d.data_ptr(), p.shape[2], p.shape[3]
        work = torch.empty((lib.mte_supervised_loss_work_elems(ctypes.addressof(arr), n, B),), dtype=torch.float64, device=dev)
        npix = sum(B * h * w for h, w in sizes[:n])
        for mid, name in enumerate(SUPERVISED_METHODS):
            for sparse in (1, 0):
                if name == "berhu" and not sparse:
                    continue

                def fwd():
                    lib.mte_supervised_loss_fwd(ctypes.addressof(arr), n, B, depth.data_ptr(), H, W, mid, sparse, work.data_ptr(),
                                                loss.data_ptr(), None, coef.data_ptr(), st)

                def bwd():
                    lib.mte_supervised_loss_bwd(ctypes.addressof(arr), n, B, depth.data_ptr(), H, W, mid, sparse, coef.data_ptr(),
                                                gout.data_ptr(), st)
                fwd()
                rows.append(("%s%s n=%d" % ("sparse-" if sparse else "", name, n), timed(fwd), timed(bwd), npix * 8.0, npix * 12.0))
    # upsample_depth_maps: scales 1-3 to 384 x 1280 in one launch, and the adjoint
    ups = [torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) for _ in range(3)]
    fa, ba = (_UpsampleMap * 3)(), (_UpsampleMap * 3)()
    for s in range(3):
        h, w = sizes[s + 1]
        fa[s].src, fa[s].dst, fa[s].h, fa[s].w = inv[s + 1].data_ptr(), ups[s].data_ptr(), h, w
        ba[s].src, ba[s].dst, ba[s].h, ba[s].w = ups[s].data_ptr(), dinv[s + 1].data_ptr(), h, w

    def ufwd():
        lib.mte_upsample_nearest_fwd(ctypes.addressof(fa), 3, B, H, W, st)

    def ubwd():
        lib.mte_upsample_nearest_bwd(ctypes.addressof(ba), 3, B, H, W, st)
    small = sum(B * h * w for h, w in sizes[1:])
    rows.append(("upsample scales 1-3", timed(ufwd), timed(ubwd), 3 * B * H * W * 4.0 + small * 4, 3 * B * H * W * 4.0 + small * 4))
    torch.cuda.synchronize()
    print("T8 loss shapes: B=%d, scales %s, depth %dx%d (5%% valid); median of %d steps" % (B, sizes, H, W, args.reps))
    print("%-26s %9s %9s %9s %9s" % ("config", "fwd ms", "bwd ms", "step ms", "TB/s"))
    for name, f, b, bf, bb in rows:
        print("%-26s %9.4f %9.4f %9.4f %9.2f" % (name, f, b, f + b, (bf + bb) / ((f + b) * 1e-3) / 1e12))


if __name__ == "__main__":
    main()
