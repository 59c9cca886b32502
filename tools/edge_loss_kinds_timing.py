"""HIP-event times of the edge-loss kinds (csrc/edge_loss_kinds.hip: one forward + one backward launch per scale) at the T8 loss
shapes -- B = 8, four scales from 384 x 1280, inverse depth in, Sobel + normals + sigmoid, no mask -- next to the four-scale
cross-entropy launches mte_edge_loss_multi_fwd / _bwd on the same inputs.

    python tools/edge_loss_kinds_timing.py [--reps 50]

Prints one line per configuration: forward, backward and forward + backward per step in ms (median of `reps` timed steps after
warm-up) and the achieved HBM rate of the step at the nominal traffic (forward: inverse depth, label, normal = 12 B/pixel, + 4 B/pixel
of box labels for the spatially adaptive kind; backward: + 4 B/pixel gradient write)."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = [("cross_entropy_dice", 0, 1), ("attention_loss", 1, 0), ("attention_loss_dice", 1, 1),
         ("spatially_adaptive", 2, 0), ("spatially_adaptive_dice", 2, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.kernels_loss import _EdgeScale
    lib = K.lib
    dev = torch.device("cuda")
    B = 8
    sizes = [(384 // 2 ** s, 1280 // 2 ** s) for s in range(4)]
    gen = torch.Generator(device="cpu").manual_seed(0)
    inv = [(0.05 + torch.rand(B, 1, h, w, generator=gen)).to(dev) for h, w in sizes]
    edge = [(torch.rand(B, 1, h, w, generator=gen) < 0.1).float().to(dev) for h, w in sizes]
    nrm = [((torch.rand(B, 1, h, w, generator=gen) * 2 - 1) * 3.14159).to(dev) for h, w in sizes]
    dpred = [torch.empty_like(i) for i in inv]
    npix = sum(B * h * w for h, w in sizes)
    st = torch.cuda.current_stream().cuda_stream
    gout = torch.ones((4,), dtype=torch.float32, device=dev)

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

    # ---- the four-scale cross-entropy launches of the training step
    arr = (_EdgeScale * 4)()
    for o, p, e, n, d in zip(arr, inv, edge, nrm, dpred):
        o.pred, o.edge, o.normal, o.mask, o.gmap, o.dpred = p.data_ptr(), e.data_ptr(), n.data_ptr(), None, None, d.data_ptr()
        o.H, o.W = p.shape[-2], p.shape[-1]
    work = torch.zeros((lib.mte_edge_loss_work_elems(ctypes.addressof(arr), 4, B),), dtype=torch.float64, device=dev)
    losses = torch.empty((4,), dtype=torch.float32, device=dev)
    coef = torch.empty((4 * (2 * B + 1),), dtype=torch.float32, device=dev)

    def multi_fwd():
        lib.mte_edge_loss_multi_fwd(ctypes.addressof(arr), 4, B, 1, 1, 1, 4.0, 10.0, 1.0, None, work.data_ptr(), losses.data_ptr(),
                                    coef.data_ptr(), None, None, st)

    def multi_bwd():
        lib.mte_edge_loss_multi_bwd(ctypes.addressof(arr), 4, B, 1, 1, 1, 4.0, coef.data_ptr(), gout.data_ptr(), None, None, None, st)

    multi_fwd()
    rows = [("cross_entropy (multi)", timed(multi_fwd), timed(multi_bwd), 12.0, 16.0)]

    # ---- the kinds: one launch per scale
    kw = [torch.empty((lib.mte_edge_loss_kind_work_elems(B, h, w),), dtype=torch.float64, device=dev) for h, w in sizes]
    kl = torch.empty((4,), dtype=torch.float32, device=dev)
    kc = [torch.empty((2 * B + 5,), dtype=torch.float32, device=dev) for _ in sizes]
    for name, kind, dice in KINDS:
        def fwd():
            for s, (h, w) in enumerate(sizes):
                lib.mte_edge_loss_kind_fwd(inv[s].data_ptr(), edge[s].data_ptr(), nrm[s].data_ptr(), None, None, B, h, w, kind, dice, 1, 1, 1,
                                           4.0, 10.0, 1.0, kw[s].data_ptr(), kl.data_ptr() + 4 * s, kc[s].data_ptr(), st)

        def bwd():
            for s, (h, w) in enumerate(sizes):
                lib.mte_edge_loss_kind_bwd(inv[s].data_ptr(), edge[s].data_ptr(), nrm[s].data_ptr(), None, kc[s].data_ptr(), gout.data_ptr(),
                                           dpred[s].data_ptr(), B, h, w, kind, dice, 1, 1, 1, 4.0, st)
        fwd()
        extra = 4.0 if kind == 2 else 0.0
        rows.append((name, timed(fwd), timed(bwd), 12.0 + extra, 16.0 + extra))
    torch.cuda.synchronize()
    print("T8 loss shapes: B=%d, scales %s, %.2f M pixels; median of %d steps" % (B, sizes, npix / 1e6, args.reps))
    print("%-26s %9s %9s %9s %9s" % ("config", "fwd ms", "bwd ms", "step ms", "TB/s"))
    for name, f, b, bf, bb in rows:
        tb = npix * (bf + bb) / ((f + b) * 1e-3) / 1e12
        print("%-26s %9.4f %9.4f %9.4f %9.2f" % (name, f, b, f + b, tb))


if __name__ == "__main__":
    main()
