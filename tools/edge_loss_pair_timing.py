"""development aid: the two-branch loss launch against two single launches at the T8 loss shapes (8 x 384x1280, four scales).

    python tools/edge_loss_pair_timing.py [--single-lib PATH] [--out FILE.json]

Pair = mte_edge_loss_pair_fwd + _bwd of this tree's library; single = two mte_edge_loss_multi_fwd + _bwd calls, taken from the library at
--single-lib (a build of another commit, e.g. the parent commit's; default: this tree's).  Device events around windows of 20 forward + backward
passes on zeroed workspaces (MTE_OPT_LOSS_PREZEROED on, as in the training step), the two series alternating, order swapped every round.
Also compares the two paths' outputs bit for bit.  Results: profiles/edge_loss_pair.txt."""
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

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("--single-lib", default=L.LIB_PATH, help="library the two single launches are taken from")
ap.add_argument("--out", default="", help="also write the result as JSON here")
args = ap.parse_args()
B, H, W, S = 8, 384, 1280, 4
ITERS, ROUNDS, WARM = 20, 40, 5
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(5)
r = lambda *s: torch.rand(*s, generator=g, device=dev)
preds = [[0.05 + 1.9 * r(B, 1, H >> s, W >> s) for s in range(S)] for _ in range(2)]
edges = [(r(B, 1, H >> s, W >> s) < 0.08).float() * r(B, 1, H >> s, W >> s) for s in range(S)]
normals = [(r(B, 1, H >> s, W >> s) * 2 - 1) * math.pi for s in range(S)]
gt = (r(B, 1, H, W) < 0.1).float() * (1.0 + 79.0 * r(B, 1, H, W))
dpreds = [[torch.empty_like(p) for p in pr] for pr in preds]
dpreds_pair = [[torch.empty_like(p) for p in pr] for pr in preds]

cur = L.lib.load()
slib = cur if os.path.abspath(args.single_lib) == os.path.abspath(L.LIB_PATH) else ctypes.CDLL(args.single_lib)
for name, proto in L.parse_header().items():
    if hasattr(slib, name) and name.startswith("mte_edge_loss_") and "pair" not in name or name == "mte_set_option":
        fn = getattr(slib, name)
        fn.argtypes = [t for t, _ in proto]
        fn.restype = L.RETURNS.get(name, ctypes.c_int)
cur.mte_set_option(1, 1)
slib.mte_set_option(1, 1)                                  # both: zeroed workspaces handed in, as the training step does
st = K._stream()

single = []
for br in range(2):
    arr = (_EdgeScale * S)()
    for s, o in enumerate(arr):
        o.pred, o.edge, o.normal, o.mask, o.gmap, o.dpred = preds[br][s].data_ptr(), edges[s].data_ptr(), normals[s].data_ptr(), None, None, dpreds[br][s].data_ptr()
        o.H, o.W = H >> s, W >> s
    single.append(arr)
pair = (_EdgePairScale * S)()
for s, o in enumerate(pair):
    for br in range(2):
        o.pred[br], o.dpred[br] = preds[br][s].data_ptr(), dpreds_pair[br][s].data_ptr()
    o.edge, o.normal, o.H, o.W = edges[s].data_ptr(), normals[s].data_ptr(), H >> s, W >> s
n1 = slib.mte_edge_loss_work_elems(ctypes.addressof(single[0]), S, B)
n2 = cur.mte_edge_loss_pair_work_elems(ctypes.addressof(pair), S, B)
pool1 = torch.zeros((2 * ITERS, n1), dtype=torch.float64, device=dev)
pool2 = torch.zeros((ITERS, n2), dtype=torch.float64, device=dev)
l1 = torch.empty((2, S + 1), device=dev); c1 = torch.empty((2, S * (2 * B + 1)), device=dev); a1 = torch.empty((2, 2), device=dev)
l2 = torch.empty((2, S), device=dev); c2 = torch.empty((2 * S * (2 * B + 1),), device=dev); s2 = torch.empty((2,), device=dev); a2 = torch.empty((4,), device=dev)


def run_single(i):
    for br in range(2):
        a = ctypes.addressof(single[br])
        rc = slib.mte_edge_loss_multi_fwd(a, S, B, 1, 1, 1, 4.0, 10.0, 1.0, gt.data_ptr(), pool1[2 * i + br].data_ptr(), l1[br].data_ptr(), c1[br].data_ptr(),
                                            l1[br].data_ptr() + 4 * S, a1[br].data_ptr(), st)
        rc |= slib.mte_edge_loss_multi_bwd(a, S, B, 1, 1, 1, 4.0, c1[br].data_ptr(), None, gt.data_ptr(), a1[br].data_ptr(), None, st)
        assert rc == 0


def run_pair(i):
    a = ctypes.addressof(pair)
    rc = cur.mte_edge_loss_pair_fwd(a, S, B, 4.0, 10.0, 1.0, gt.data_ptr(), pool2[i].data_ptr(), l2.data_ptr(), c2.data_ptr(), s2.data_ptr(), a2.data_ptr(), st)
    rc |= cur.mte_edge_loss_pair_bwd(a, S, B, 4.0, c2.data_ptr(), None, gt.data_ptr(), a2.data_ptr(), None, st)
    assert rc == 0


def window(fn):
    pool1.zero_(); pool2.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(ITERS):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ITERS                # us per forward + backward


for _ in range(WARM):
    window(run_single); window(run_pair)
# same numbers?
equal = bool(torch.equal(l1[:, :S], l2) and torch.equal(l1[:, S], s2)) and all(torch.equal(x, y) for br in range(2) for x, y in zip(dpreds[br], dpreds_pair[br]))
ts, tp = [], []
for rnd in range(ROUNDS):
    if rnd % 2 == 0:
        ts.append(window(run_single)); tp.append(window(run_pair))
    else:
        tp.append(window(run_pair)); ts.append(window(run_single))


def q(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "p10": v[len(v) // 10], "p90": v[-1 - len(v) // 10], "max": v[-1]}


res = {"shape": [B, H, W, S], "iters_per_window": ITERS, "windows": ROUNDS, "unit": "us per forward+backward",
       "single_lib": os.path.basename(os.path.dirname(os.path.abspath(args.single_lib))) + "/" + os.path.basename(args.single_lib), "two_single_launches": q(ts), "pair": q(tp), "pair_bit_equal_to_singles": equal,
       "losses_pair": l2.tolist(), "silog_pair": s2.tolist()}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
