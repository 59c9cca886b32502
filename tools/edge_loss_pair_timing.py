"""development aid: the two-branch loss launch against two single launches, from this tree's library and from another build of it.

    python tools/edge_loss_pair_timing.py [--other-lib PATH] [--shape B H W] [--out FILE.json]

Two series: pair = mte_edge_loss_pair_fwd + _bwd; single = two mte_edge_loss_multi_fwd + _bwd calls.  Each is run from this tree's library and,
with --other-lib (a build of another commit, e.g. the parent commit's; --single-lib is the same switch under its old name), from that library too.
Default shape: the T8 loss shapes (8 x 384x1280), always four scales with ground truth.  Device events around windows of 20 forward + backward
passes on zeroed workspaces (MTE_OPT_LOSS_PREZEROED on, as in the training step), the series alternating, order reversed every round.
Compares bit for bit every output -- losses, silog losses, coef, silog_aux and all eight gradient maps -- of like series of the two libraries,
and of pair against single within a library.  Results: profiles/edge_loss_pair.txt, profiles/edge_fast_template.txt."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mindtheedge_amd import kernels as K                       # noqa: E402
from mindtheedge_amd import _lib as L                          # noqa: E402
from mindtheedge_amd.kernels_loss import _EdgeScale, _EdgePairScale   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other-lib", "--single-lib", dest="other_lib", default="", help="a second library to run both series from")
ap.add_argument("--shape", type=int, nargs=3, default=[8, 384, 1280], metavar=("B", "H", "W"))
ap.add_argument("--out", default="", help="also write the result as JSON here")
args = ap.parse_args()
(B, H, W), S = args.shape, 4
ITERS, ROUNDS, WARM = 20, 40, 5
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(5)
r = lambda *s: torch.rand(*s, generator=g, device=dev)
preds = [[0.05 + 1.9 * r(B, 1, H >> s, W >> s) for s in range(S)] for _ in range(2)]
edges = [(r(B, 1, H >> s, W >> s) < 0.08).float() * r(B, 1, H >> s, W >> s) for s in range(S)]
normals = [(r(B, 1, H >> s, W >> s) * 2 - 1) * math.pi for s in range(S)]
gt = (r(B, 1, H, W) < 0.1).float() * (1.0 + 79.0 * r(B, 1, H, W))
st = K._stream()

libs = {"this": L.lib.load()}
if args.other_lib and os.path.abspath(args.other_lib) != os.path.abspath(L.LIB_PATH):
    other = ctypes.CDLL(args.other_lib)
    for name, proto in L.parse_header().items():
        if hasattr(other, name) and (name.startswith("mte_edge_loss_") or name == "mte_set_option"):
            fn = getattr(other, name)
            fn.argtypes = [t for t, _ in proto]
            fn.restype = L.RETURNS.get(name, ctypes.c_int)
    libs["other"] = other
for lib in libs.values():
    lib.mte_set_option(1, 1)                               # zeroed workspaces handed in, as the training step does


class Series:
    """one kind of launch from one library, with outputs of its own: losses [2][S], silog [2], coef [2][S][2B + 1], aux [2][2], 8 gradient maps"""

    def __init__(self, lib, kind):
        self.lib, self.kind, self.times = lib, kind, []
        self.dpreds = [[torch.full_like(p, float("nan")) for p in pr] for pr in preds]
        self.losses = torch.empty((2, S), device=dev); self.silog = torch.empty((2,), device=dev)
        self.coef = torch.empty((2, S * (2 * B + 1)), device=dev); self.aux = torch.empty((2, 2), device=dev)
        if kind == "single":
            self.scales = []
            for br in range(2):
                arr = (_EdgeScale * S)()
                for s, o in enumerate(arr):
                    o.pred, o.edge, o.normal, o.mask, o.gmap, o.dpred = preds[br][s].data_ptr(), edges[s].data_ptr(), normals[s].data_ptr(), None, None, self.dpreds[br][s].data_ptr()
                    o.H, o.W = H >> s, W >> s
                self.scales.append(arr)
            n, rows = lib.mte_edge_loss_work_elems(ctypes.addressof(self.scales[0]), S, B), 2 * ITERS
        else:
            self.scales = (_EdgePairScale * S)()
            for s, o in enumerate(self.scales):
                for br in range(2):
                    o.pred[br], o.dpred[br] = preds[br][s].data_ptr(), self.dpreds[br][s].data_ptr()
                o.edge, o.normal, o.H, o.W = edges[s].data_ptr(), normals[s].data_ptr(), H >> s, W >> s
            n, rows = lib.mte_edge_loss_pair_work_elems(ctypes.addressof(self.scales), S, B), ITERS
        assert n > 0
        self.pool = torch.zeros((rows, n), dtype=torch.float64, device=dev)

    def run(self, i):
        lib = self.lib
        if self.kind == "single":
            for br in range(2):
                a = ctypes.addressof(self.scales[br])
                rc = lib.mte_edge_loss_multi_fwd(a, S, B, 1, 1, 1, 4.0, 10.0, 1.0, gt.data_ptr(), self.pool[2 * i + br].data_ptr(), self.losses[br].data_ptr(),
                                                 self.coef[br].data_ptr(), self.silog[br:].data_ptr(), self.aux[br].data_ptr(), st)
                rc |= lib.mte_edge_loss_multi_bwd(a, S, B, 1, 1, 1, 4.0, self.coef[br].data_ptr(), None, gt.data_ptr(), self.aux[br].data_ptr(), None, st)
                assert rc == 0
        else:
            a = ctypes.addressof(self.scales)
            rc = lib.mte_edge_loss_pair_fwd(a, S, B, 4.0, 10.0, 1.0, gt.data_ptr(), self.pool[i].data_ptr(), self.losses.data_ptr(), self.coef.data_ptr(),
                                            self.silog.data_ptr(), self.aux.data_ptr(), st)
            rc |= lib.mte_edge_loss_pair_bwd(a, S, B, 4.0, self.coef.data_ptr(), None, gt.data_ptr(), self.aux.data_ptr(), None, st)
            assert rc == 0

    def window(self):
        self.pool.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            self.run(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / ITERS            # us per forward + backward

    def outputs(self):
        out = {"losses": self.losses, "silog": self.silog, "coef": self.coef, "silog_aux": self.aux}
        out.update({"dpred[%d][%d]" % (br, s): self.dpreds[br][s] for br in range(2) for s in range(S)})
        return out


def same_bits(x, y):
    """-> the names of the outputs that differ (none: every output is bit-equal)"""
    xo, yo = x.outputs(), y.outputs()
    return [k for k in xo if not torch.equal(xo[k], yo[k])]


series = {(name, kind): Series(lib, kind) for kind in ("single", "pair") for name, lib in libs.items()
          if kind == "single" or hasattr(lib, "mte_edge_loss_pair_fwd")}
order = list(series.values())
for _ in range(WARM):
    for x in order:
        x.window()
differ = {"%s %s" % (kind, "this == other"): same_bits(series["this", kind], series["other", kind])
          for kind in ("single", "pair") if ("other", kind) in series}
differ.update({"%s pair == singles" % name: same_bits(series[name, "pair"], series[name, "single"]) for name in libs if (name, "pair") in series})
for rnd in range(ROUNDS):
    for x in (order if rnd % 2 == 0 else order[::-1]):
        x.times.append(x.window())


def q(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "p10": v[len(v) // 10], "p90": v[-1 - len(v) // 10], "max": v[-1]}


res = {"shape": [B, H, W, S], "iters_per_window": ITERS, "windows": ROUNDS, "unit": "us per forward+backward",
       "other_lib": os.path.basename(os.path.dirname(os.path.abspath(args.other_lib))) + "/" + os.path.basename(args.other_lib) if "other" in libs else None,
       "times": {"%s %s" % k: q(x.times) for k, x in series.items()},
       "outputs_that_differ": differ, "all_bit_equal": not any(differ.values()),
       "losses_pair": series["this", "pair"].losses.tolist(), "silog_pair": series["this", "pair"].silog.tolist()}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
